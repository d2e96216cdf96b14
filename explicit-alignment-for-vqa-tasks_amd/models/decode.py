"""Generation for the prefix LM (``_generate_from_embeddings`` src/models/clipcap.py:387-471): the causal step sources of the pick
loop (:func:`~eavqa_amd.models.search.pick_loop`, which owns the token bookkeeping, the per-step rules and the early stop), the beam
search over a shared prompt cache, and candidate scoring.

Three sources produce the same logits for position t:
  * re-forward (``use_cache=False``) - the reference's algorithm verbatim: every step re-runs the whole, growing sequence
    (clipcap.py:414-419), on one row per prompt or on replicated rows (several draws per prompt);
  * per-row cache - prefill once, keep per-layer K/V in HBM ``[B, S_max, E]`` and run one token per step; a decode step is
    weight-streaming (HBM) bound.  An LM held in e4m3 streams half the bytes (``eavqa_lm_block_forward_fp8``; every Linear =
    row-quantised activations x e4m3 weights, as in the re-forward loop);
  * shared prompt (:class:`_SharedStep`) - B prompts prefilled once, G rows per prompt attend "shared prompt | own tail".
What is fed back is the RAW pick of the previous step (clipcap.py:423), not the emitted token (pad for a finished row).
:func:`greedy_decode` and :func:`group_sample_decode` choose a source and run the loop.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from .. import _lib, _lib_llama, ops
from . import search
from .constrained import CONSTRAINT_KWARGS, upload_constraint
from .lm import FrozenCausalLM, linear
from .search import mark as _mark

Tensor = torch.Tensor


def greedy_decode(lm: FrozenCausalLM, prefix_rows: Tensor, src: Tensor, mask: Tensor, pos: Tensor, B: int, S0: int,
                  max_length: int, pad_token_id: Optional[int], eos_token_id: Optional[int], use_cache: bool = True,
                  output_scores: bool = False, marks: Optional[list] = None, sampler=None, logits_plan=None, constraint=None):
    """``src/mask/pos``: int32 [B, S0 + max_length] for the whole horizon (appended positions have mask 1;
    their ``src`` entries are filled in as tokens are produced).  ``output_scores``: also return the float32
    [B, produced] log-probabilities of the raw greedy tokens (what HF's ``output_scores=True`` yields after
    ``log(softmax)``, few_shot_vqa_executor.py:301-314).  ``marks`` (bench instrumentation): a list that receives
    ``("prefill", event)`` and ``("decode", event)`` - HIP events recorded on the launch stream behind the prefill and behind the
    last decode step.  ``sampler`` (a :class:`~eavqa_amd.models.sampling.Sampler` with its seed set): the per-step pick is a draw
    (``eavqa_sample_pick``; the uniform of step t, row b is Philox(seed, t, b)) instead of the argmax; the scores are then the
    log-probabilities of the drawn tokens under the processed distribution.  ``logits_plan`` (a
    :class:`~eavqa_amd.models.logits_process.LogitsPlan`): HF's logits processors run on each step's logits before the pick
    (``eavqa_logits_process``).  The history is the emitted ``tokens[:, :t]``: with ``inputs_embeds`` HF's ``input_ids`` start empty, so
    the prompt length is 0; the scores are then log-probabilities under the processed distribution.  ``constraint`` (an
    :class:`~eavqa_amd.models.constrained.AnswerTrie`): the step's logits are then masked to the answer set (``eavqa_trie_constrain``),
    after the processors."""
    dev = lm.device
    proc = logits_plan.upload(lm.vocab, dev) if logits_plan is not None else None
    con = upload_constraint(constraint, eos_token_id, B, lm.vocab, dev)
    if use_cache:
        source = _cached_source(lm, prefix_rows, src, mask, pos, B, S0, S0 + max_length)
    else:
        source = _reforward_source(lm, prefix_rows, src, mask, pos, B, S0)
    _mark(marks, "prefill")
    seq, logp = search.pick_loop(source, B, lm.vocab, max_length, pad_token_id, eos_token_id, dev, sampler=sampler, proc=proc, con=con,
                                 scores="logp" if output_scores else None, marks=marks)
    ids = seq.numpy().astype(int).tolist()                     # clipcap.py:469
    return (ids, logp) if output_scores else ids


@torch.no_grad()
def ensemble_decode(lm: FrozenCausalLM, prefix_rows: Tensor, src: Tensor, mask: Tensor, pos: Tensor, B: int, n: int, S0: int,
                    max_length: int, pad_token_id: Optional[int], eos_token_id: Optional[int], combine: str = "product", weights=None,
                    use_cache: bool = True, output_scores: bool = False, sampler=None, logits_plan=None, constraint=None, ignored_ids=()):
    """One answer per question from its ``n`` ensemble members: ``src/mask/pos`` as for :func:`greedy_decode`, on B * n prompt rows
    ordered (question, member), prefilled as one batch.  ``combine`` "product" / "mixture": the loop of :func:`greedy_decode` on B rows
    over :func:`~eavqa_amd.models.search.ensemble_source` - the member source is :func:`_cached_source` (``use_cache=False``:
    :func:`_reforward_source`) on the B * n rows, and every member is fed the raw pick made from the combined scores.  Returns the ids
    (B lists), with ``output_scores`` also the float32 [B, produced] log-probabilities of the picks under the combined, processed
    distribution.  ``combine`` "select": the B * n rows are decoded independently in one loop and the first best member per question is
    kept (:func:`~eavqa_amd.models.search.select_members`; the sum of a row's picked log-probabilities skips ``ignored_ids``);
    ``output_scores`` is not built there."""
    if lm.fp8:
        raise NotImplementedError('lm_weight_format="fp8": ensemble decoding is built for fp32 and bf16 weights')
    dev, R = lm.device, B * n
    proc = logits_plan.upload(lm.vocab, dev) if logits_plan is not None else None
    con = upload_constraint(constraint, eos_token_id, B, lm.vocab, dev)
    if use_cache:
        member = _cached_source(lm, prefix_rows, src, mask, pos, R, S0, S0 + max_length)
    else:
        member = _reforward_source(lm, prefix_rows, src, mask, pos, R, S0)
    if combine == "select":
        if output_scores:
            raise NotImplementedError('output_scores together with ensemble="select" is not built')
        seq, logp = search.pick_loop(member, R, lm.vocab, max_length, pad_token_id, eos_token_id, dev, sampler=sampler, proc=proc, con=con,
                                     scores="logp")
        fill = pad_token_id if pad_token_id is not None else 0
        return search.select_members(seq, logp, B, n, 0, fill, eos_token_id, ignored_ids).numpy().astype(int).tolist()
    source = search.ensemble_source(member, B, n, lm.vocab, combine, dev, weights=weights)
    seq, logp = search.pick_loop(source, B, lm.vocab, max_length, pad_token_id, eos_token_id, dev, sampler=sampler, proc=proc, con=con,
                                 scores="logp" if output_scores else None)
    ids = seq.numpy().astype(int).tolist()
    return (ids, logp) if output_scores else ids


def _cached_source(lm, prefix_rows, src, mask, pos, B, S0, S_max):
    """Step source over a per-row :class:`_KVCache`: the prompt is prefilled here; position t > 0 feeds the previous step's raw pick."""
    cache = _KVCache(lm, B, S_max, B * S0)
    first = _prefill(lm, cache, prefix_rows, src[:, :S0].contiguous(), pos[:, :S0].contiguous(), mask, B, S0, S_max)

    def logits(t, seq, raw):
        if t == 0:
            return first
        src[:, S0 + t - 1] = raw                               # the RAW argmax (or draw) is what gets embedded (clipcap.py:423)
        return _decode_step(lm, cache, raw, pos[:, S0 + t - 1].contiguous(), mask, B, S0 + t - 1, S_max)
    return logits


def _reforward_source(lm, prefix_rows, src, mask, pos, R, S0):
    """Step source without a cache: ``lm.forward`` over [prompt | raw picks so far] on the R rows of ``src`` / ``mask`` / ``pos``."""
    def logits(t, seq, raw):
        if t:
            src[:, S0 + t - 1] = raw
        return _replicated_logits(lm, prefix_rows, src, pos, mask, R, S0 + t)
    return logits


def _shared_source(lm, prefix_rows, src, mask, pos, B, G, S0, max_length):
    """Step source over one shared prompt cache (:class:`_SharedStep`, one tail buffer: draws never change rows): B * G rows ordered
    (b, row); the raw pick of step t - 1 becomes tail position t - 1."""
    rep = lambda x: x.repeat_interleave(G, dim=0).contiguous()
    pos_r = rep(pos)
    drv = _SharedStep(lm, B, G, S0, max(max_length - 1, 1), 1)
    first = rep(drv.prefill(prefix_rows, src, pos, mask))

    def logits(t, seq, raw):
        return first if t == 0 else drv.step(raw, pos_r[:, S0 + t - 1].contiguous(), mask, t - 1)
    return logits


@torch.no_grad()
def score_decode(lm: FrozenCausalLM, prefix_rows: Tensor, src: Tensor, mask: Tensor, pos: Tensor, B: int, S0: int, candidates: Tensor,
                 share_prompt: bool = True) -> Tensor:
    """Token log-probabilities float32 [B, C, Tc] of ``candidates`` (int64 [B, C, Tc] on the device, right-padded with -100) as
    continuations of the B prompts.  ``src/mask/pos``: int32 [B, S0 + Tc] as for :func:`greedy_decode` (appended positions have mask 1).

    ``share_prompt``: the prompts are prefilled ONCE into a K/V cache (``S_max = S0``); the prefill's last-position logits give the first
    token's log-probability for all C candidates of a row.  The other Tc - 1 positions run as B * C * (Tc - 1) rows whose attention has two
    segments - the shared prompt (B batch entries of C * (Tc - 1) queries over the cache planes, not causal, the prompt's key mask) and
    the candidate's own tokens (B * C entries, causal; right-padded positions sit behind every scored query, so they need no mask) -
    merged by their log-sum-exps (``eavqa_attention_merge``): the attend step handed to ``lm.layer_loop``, the layer loop of
    ``lm.forward``, here without look-ahead hints.  False: ``lm.forward`` on B * C rows of [prompt | candidate] (``src`` names
    prefix rows by index, so the prefix rows themselves are not copied) - the slow route, kept to compare against.  An LM held in e4m3
    (``weight_format="fp8"``) always takes the replicated route: the shared route is built for fp32 and bf16 weights."""
    from . import scoring
    c, dev = lm.cfg, lm.device
    H, hd, V = c.n_head, c.head_dim, lm.vocab
    _, C, Tc = candidates.shape
    R = B * C
    ar = lambda n: torch.arange(n, device=dev)
    head = (lambda h, out: linear(h, lm.head_q, out=out)) if lm.fp8 else (lambda h, out: ops.gemm(h, lm.head, out=out))
    inputs = candidates[..., :-1].clamp_min(0).to(torch.int32)                       # [B, C, Tc - 1]: the tokens fed after the prompt
    if lm.fp8 or not share_prompt:
        S = S0 + Tc - 1
        rep = lambda x: x[:, :S].repeat_interleave(C, dim=0)
        src_r = rep(src)
        src_r[:, S0:] = inputs.reshape(R, Tc - 1)
        hid = lm.forward(prefix_rows, src_r.contiguous(), rep(pos).contiguous(), rep(mask).contiguous(), R, S, logits="none")["hidden"]
        idx = ((ar(B)[None, :, None] * C + ar(C)[:, None, None]) * S + (S0 - 1) + ar(Tc)[None, None, :]).reshape(C, B * Tc)
        return scoring.score_hidden(hid, idx.to(torch.int32).contiguous(), candidates, head, V, lm.vpad)
    tok = torch.empty((B, C, Tc), device=dev, dtype=torch.float32)
    cache = _KVCache(lm, B, S0, B * S0)
    logits0 = _prefill(lm, cache, prefix_rows, src[:, :S0].contiguous(), pos[:, :S0].contiguous(), mask, B, S0, S0)
    for c0 in range(0, C, 64):                                                        # eavqa_token_logprobs gathers up to 64 labels per row
        tok[:, c0:c0 + 64, 0] = ops.token_logprobs(logits0, V, candidates[:, c0:c0 + 64, 0].contiguous())
    Tq = Tc - 1
    if Tq == 0:
        return tok
    scale = hd ** -0.5
    p_rows = pos[:, S0:S0 + Tq].unsqueeze(1).expand(B, C, Tq).reshape(-1).contiguous()
    x = ops.embed_assemble(inputs.reshape(-1).contiguous(), p_rows, lm.wte, None, lm.wpe)

    def attend(li, q, k, v):
        """The shared prompt (layer li's cache planes, under the prompt's key mask) and the candidate's own tokens, merged."""
        o1, l1 = ops.attention_fwd(q, cache.k[li], cache.v[li], B, H, C * Tq, S0, hd, key_mask=mask, ld_mask=mask.stride(0), causal=False,
                                   scale=scale, save_lse=True, kv_batch_rows=S0)
        o2, l2 = ops.attention_fwd(q, k, v, R, H, Tq, Tq, hd, causal=True, scale=scale, save_lse=True)
        return ops.attention_merge(o1, l1, o2, l2, B, C, Tq, H, hd), None

    x, _ = lm.layer_loop(x, attend, save=False, hints=False)
    hid = lm.final_norm(x)
    idx = ((ar(B)[None, :, None] * C + ar(C)[:, None, None]) * Tq + ar(Tq)[None, None, :]).reshape(C, B * Tq)
    tok[:, :, 1:] = scoring.score_hidden(hid, idx.to(torch.int32).contiguous(), candidates[..., 1:].contiguous(), head, V, lm.vpad)
    return tok


class _KVCache:
    """Per-layer K/V ``[B, S_max, E]`` plus the host-side layer table and scratch of the block driver that serves the model:
    ``eavqa_lm_block_forward``; for an LM held in e4m3 (``weight_format="fp8"``) ``eavqa_lm_block_forward_fp8``, whose table points at the
    weight BYTES beside a second table of per-tensor scales; for the Llama family ``eavqa_llama_block_forward`` and its own layer struct."""

    def __init__(self, lm: FrozenCausalLM, B: int, S_max: int, max_rows: int):
        c, nl = lm.cfg, len(lm.layers)
        E, H, F, eps, dt = c.n_embd, c.n_head, c.ffn, float(c.eps), ops.dtype_id(lm.dtype)
        self.k = [torch.empty((B * S_max, E), device=lm.device, dtype=lm.dtype) for _ in lm.layers]
        self.v = [torch.empty((B * S_max, E), device=lm.device, dtype=lm.dtype) for _ in lm.layers]
        self.scales = None
        # The block driver that serves this model, chosen here and nowhere else: its layer struct (``names``: a field whose _Layer attribute
        # has another name), its workspace size as a function of the rows, and ``self.forward`` - the C call :func:`_block` makes, on the
        # cache it is handed (a closure over ``self`` would keep the K / V planes alive until the cycle collector runs).
        names = {}
        if c.arch == "llama":                    # eavqa_llama_block_forward and its own layer table (no biases)
            struct, names = _lib_llama.LlamaLayer, dict(w_gu="w_fc1", w_down="w_fc2")
            size = lambda rows: _lib_llama.load().eavqa_llama_block_workspace_bytes(dt, rows, E, F)
            self.forward = lambda s, B, Sq, row0, S_max, x, pos, mask: _lib_llama.call(
                "eavqa_llama_block_forward", dt, nl, s.table, E, H, F, eps, B, Sq, row0, S_max, x.data_ptr(), pos.data_ptr(),
                lm.rope_cos.data_ptr(), lm.rope_sin.data_ptr(), lm.rope_cos.shape[0], mask.data_ptr(), mask.stride(0), s.ws.data_ptr(),
                s.ws_bytes, ops._stream())
        elif lm.fp8:                             # the table points at the e4m3 bytes, a second table carries the per-tensor scales
            struct, self.scales = _lib.LMLayer, (_lib.LMLayerScales * nl)()
            size = lambda rows: _lib.load().eavqa_lm_block_fp8_workspace_bytes(rows, E, F)
            self.forward = lambda s, B, Sq, row0, S_max, x, pos, mask: _lib.call(
                "eavqa_lm_block_forward_fp8", nl, s.table, s.scales, E, H, F, _lib.ACT[c.act], eps, B, Sq, row0, S_max, x.data_ptr(),
                mask.data_ptr(), mask.stride(0), s.ws.data_ptr(), s.ws_bytes, ops._stream())
        else:
            struct = _lib.LMLayer
            size = lambda rows: _lib.load().eavqa_lm_block_workspace_bytes(dt, rows, E, F)
            self.forward = lambda s, B, Sq, row0, S_max, x, pos, mask: _lib.call(
                "eavqa_lm_block_forward", dt, nl, s.table, E, H, F, _lib.ACT[c.act], eps, B, Sq, row0, S_max, x.data_ptr(),
                mask.data_ptr(), mask.stride(0), s.ws.data_ptr(), s.ws_bytes, ops._stream())
        self.table = (struct * nl)()
        for i, L in enumerate(lm.layers):
            t = self.table[i]
            t.k_cache, t.v_cache = self.k[i].data_ptr(), self.v[i].data_ptr()
            for field in (f for f, _ in struct._fields_ if f not in ("k_cache", "v_cache")):
                w = getattr(L, names.get(field, field))
                if self.scales is not None and field.startswith("w_"):
                    setattr(self.scales[i], "s_" + field[2:], w.scale)
                    w = w.q
                setattr(t, field, w.data_ptr())
        # prefill (max_rows = B * S0 rows) and decode steps (B rows; their split-K partial sums) share one workspace
        self.ws_bytes = max(int(size(max_rows)), int(size(B)))
        self.ws = torch.empty(self.ws_bytes, device=lm.device, dtype=torch.uint8)


def _block(lm: FrozenCausalLM, cache: _KVCache, x: Tensor, mask: Tensor, B: int, Sq: int, row0: int, S_max: int,
           pos: Optional[Tensor] = None) -> Tensor:
    """All decoder layers for ``Sq`` new positions per row starting at sequence index ``row0`` (one C call): K/V of the
    new positions are appended to the cache and attention runs against rows [0, row0+Sq).  ``x`` is updated in place.  ``pos``: int32, the
    position of every new row (read by the Llama family's rotation only)."""
    cache.forward(cache, B, Sq, row0, S_max, x, pos, mask)
    return x


def _last_logits(lm: FrozenCausalLM, x: Tensor, B: int, Sq: int) -> Tensor:
    return lm._head(lm.final_norm(x.view(B, Sq, lm.cfg.n_embd)[:, -1]))


def _prefill(lm, cache, prefix_rows, src, pos, mask, B, S0, S_max) -> Tensor:
    x = ops.embed_assemble(src, pos, lm.wte, prefix_rows, lm.wpe)
    x = _block(lm, cache, x, mask, B, S0, 0, S_max, pos)
    return _last_logits(lm, x, B, S0)


def _decode_step(lm, cache, raw, pos_col, mask, B, row0, S_max) -> Tensor:
    x = ops.embed_assemble(raw, pos_col, lm.wte, None, lm.wpe)
    x = _block(lm, cache, x, mask, B, 1, row0, S_max, pos_col)
    return _last_logits(lm, x, B, 1)


# =========================================================================== k beams / n draws per prompt over ONE prompt cache
MAX_SHARED_TAIL = 256             # tail positions per row eavqa_attention_decode_shared takes


class _SharedStep:
    """The cached step of B prompts x G rows per prompt (``eavqa_lm_block_step_shared``): the prompt is prefilled ONCE into a
    :class:`_KVCache` of ``S_max = S0`` rows per prompt and never copied or reordered; each row's own tokens live in tail caches
    ``[2 * n_layer, B * G, t_max, E]`` - ``n_buffers`` of them (beam search gathers a ping into a pong by beam parent after each step)."""

    def __init__(self, lm: FrozenCausalLM, B: int, G: int, S0: int, t_max: int, n_buffers: int):
        if lm.fp8:
            raise NotImplementedError('weight_format="fp8": beams / several draws over a shared prompt cache are built for fp32 and bf16 '
                                      "weights")
        if lm.cfg.arch == "llama":
            raise NotImplementedError('arch="llama": the shared-prompt step (eavqa_lm_block_step_shared) is built for GPT-2 / OPT layers')
        if not 1 <= t_max <= MAX_SHARED_TAIL:
            raise NotImplementedError(f"max_length={t_max + 1}: at most {MAX_SHARED_TAIL + 1} new tokens per row over a shared prompt cache")
        c = lm.cfg
        self.lm, self.B, self.G, self.S0, self.t_max = lm, B, G, S0, t_max
        self.cache = _KVCache(lm, B, S0, B * S0)
        nl, E = len(lm.layers), c.n_embd
        self.planes = [torch.empty((2 * nl, B * G, t_max, E), device=lm.device, dtype=lm.dtype) for _ in range(n_buffers)]
        self.tails = []
        for p in self.planes:
            tab = (_lib.LMTail * nl)()
            for i in range(nl):
                tab[i].k_tail, tab[i].v_tail = p[2 * i].data_ptr(), p[2 * i + 1].data_ptr()
            self.tails.append(tab)
        self.ws_bytes = int(_lib.load().eavqa_lm_block_step_shared_workspace_bytes(ops.dtype_id(lm.dtype), B * G, E, c.ffn))
        self.ws = torch.empty(self.ws_bytes, device=lm.device, dtype=torch.uint8)

    def prefill(self, prefix_rows, src, pos, mask) -> Tensor:
        return _prefill(self.lm, self.cache, prefix_rows, src[:, :self.S0].contiguous(), pos[:, :self.S0].contiguous(), mask, self.B, self.S0,
                        self.S0)

    def step(self, tokens: Tensor, pos_col: Tensor, mask: Tensor, t: int, buf: int = 0) -> Tensor:
        """Logits [B * G, V_padded] after feeding ``tokens`` (int32 [B * G]) as tail position ``t`` of buffer ``buf``."""
        lm, c, R = self.lm, self.lm.cfg, self.B * self.G
        x = ops.embed_assemble(tokens, pos_col, lm.wte, None, lm.wpe)
        _lib.call("eavqa_lm_block_step_shared", ops.dtype_id(lm.dtype), len(lm.layers), self.cache.table, self.tails[buf], c.n_embd, c.n_head,
                  c.ffn, _lib.ACT[c.act], float(c.eps), self.B, self.G, self.S0, self.S0, int(t), self.t_max, x.data_ptr(), mask.data_ptr(),
                  mask.stride(0), self.ws.data_ptr(), self.ws_bytes, ops._stream())
        return _last_logits(lm, x, R, 1)


def _replicated_logits(lm, prefix_rows, src_r, pos_r, mask_r, R, S):
    return lm.forward(prefix_rows, src_r[:, :S].contiguous(), pos_r[:, :S].contiguous(), mask_r[:, :S].contiguous(), R, S, logits="last")["logits"]


@torch.no_grad()
def beam_decode(lm: FrozenCausalLM, prefix_rows: Tensor, src: Tensor, mask: Tensor, pos: Tensor, B: int, S0: int, max_length: int,
                num_beams: int, num_return_sequences: int = 1, length_penalty: float = 1.0, early_stopping=False,
                pad_token_id: Optional[int] = None, eos_token_id: Optional[int] = None, use_cache: bool = True, logits_plan=None,
                constraint=None, members=None):
    """HF ``GenerationMixin._beam_search`` (transformers 5.15) over ``inputs_embeds`` for the prefix LM: the causal counterpart of
    ``FrozenT5.beam_search``.  ``src/mask/pos`` as for :func:`greedy_decode`; ``max_length`` new tokens.  With ``inputs_embeds`` HF's
    ``input_ids`` start empty; ``eavqa_beam_step`` wants a first column, so the state has ``max_length + 1`` columns with a dummy first one
    holding pad, step t runs at ``cur_len = t + 1`` with ``prompt_len = 1`` (HF's ``(t + 1) ** length_penalty`` and its "hit at the last
    position" rule), and the dummy column is stripped from the result.  Logits processors see ``run_seq[:, 1:]`` (history length t, prompt
    length 0) and run on log-probabilities, as on the T5 path; so does ``constraint`` (the answer set, ``eavqa_trie_constrain``).
    ``use_cache``: the prompt is prefilled once for the B questions and the B * k rows attend "shared prompt | own tail" (:class:`_SharedStep`); the tails are gathered by beam parent (``eavqa_beam_reorder``).
    False: every step re-runs ``lm.forward`` over [prompt | running sequence] on B * k replicated rows.  The host reads ``st.cont`` every
    fourth step.  ``members`` (a :class:`~eavqa_amd.models.search.EnsembleMembers`; None: every launch is as described so far): beam
    search under an ensemble - ``src/mask/pos`` hold the B * n prompts ordered (question, member), prefilled as one batch; the LM runs on
    B * n * k rows ordered (question, member, beam), ``ops.ensemble_combine_groups`` folds each step's logits to the B * k rows the rules
    and ``eavqa_beam_step`` see, ``search.expand_beams`` carries the step's tokens and parents back to the member rows.
    Returns ``(sequences int64 [B * nrs, <= max_length], sequences_scores float32 [B * nrs])`` on the host; positions
    behind a hypothesis' end hold ``pad or eos``."""
    k, nrs, ML = int(num_beams), int(num_return_sequences), int(max_length)
    if not 1 <= k <= 8 or not 1 <= nrs <= k:
        raise ValueError(f"num_beams in 1..8 and num_return_sequences <= num_beams (got {num_beams}, {num_return_sequences})")
    if ML < 1:
        raise ValueError("beam search needs max_length >= 1 new token")
    if lm.fp8:
        raise NotImplementedError('weight_format="fp8": beam search on the causal path is built for fp32 and bf16 weights')
    n = members.n if members is not None else 1
    Bi = B * n                                                 # the prompts: (question, member) pairs
    dev, V, R = lm.device, lm.vocab, Bi * k
    fill = pad_token_id if pad_token_id is not None else eos_token_id
    eos = -1 if eos_token_id is None else int(eos_token_id)
    st = ops.BeamState(B, k, ML + 1, fill, fill, dev)
    proc = logits_plan.upload(V, dev) if logits_plan is not None else None
    con = upload_constraint(constraint, eos_token_id, B, V, dev)
    rep = lambda x: x.repeat_interleave(k, dim=0).contiguous()
    pos_r = rep(pos)
    cached = bool(use_cache)
    # what the decoder rows are fed and gathered by: the beam step's own buffers, or their copies on the member rows
    tokens, parents = st.next_tokens, st.parents
    if members is not None and use_cache:
        tokens, parents = members.expand_beams(st.next_tokens, st.parents, B, k)
    if cached:
        drv = _SharedStep(lm, Bi, k, S0, max(ML - 1, 1), 2)
        lg = rep(drv.prefill(prefix_rows, src, pos, mask))
        cur = 0
    else:
        src_r, mask_r = rep(src), rep(mask)
    for t in range(ML):
        if not cached:
            if t:
                run = st.run_seq[:, 1:t + 1]
                src_r[:, S0:S0 + t] = (run if members is None else members.expand_rows(run, B, k)).to(torch.int32)
            lg = _replicated_logits(lm, prefix_rows, src_r, pos_r, mask_r, R, S0 + t)
        if members is not None:
            lg = members.combine(lg, V, k)
        logprobs = search.apply_rules(proc, con, lg, V, st.run_seq[:, 1:], t, 0, logprobs=True)
        ops.beam_step(lg, V, st, t + 1, eos, length_penalty, early_stopping, prompt_len=1, logprobs=logprobs)
        if (t + 1) % 4 == 0 and int(st.cont[t + 1].item()) == 0:
            break
        if cached and t + 1 < ML:
            if members is not None:
                members.expand_beams(st.next_tokens, st.parents, B, k, tokens, parents)
            if t:                                              # tail positions 0..t-1 follow their beams; the prompt cache stays put
                ops.beam_reorder(drv.planes[cur], drv.planes[1 - cur], parents, t)
                cur = 1 - cur
            lg = drv.step(tokens.to(torch.int32), pos_r[:, S0 + t].contiguous(), mask, t, cur)
    return search.beam_result(st, nrs, first=1)


@torch.no_grad()
def group_sample_decode(lm: FrozenCausalLM, prefix_rows: Tensor, src: Tensor, mask: Tensor, pos: Tensor, B: int, S0: int, max_length: int,
                        num_return_sequences: int, sampler, pad_token_id: Optional[int] = None, eos_token_id: Optional[int] = None,
                        use_cache: bool = True, logits_plan=None, constraint=None, members=None):
    """n = ``num_return_sequences`` draws per prompt: the loop of :func:`greedy_decode` with ``eavqa_sample_pick`` on B * n rows ordered
    (b, draw) - the uniform of step t, row r = b * n + j is Philox(seed, t, r) - over the shared step of :func:`beam_decode` (draws never
    change rows: one tail buffer, nothing reordered).  ``use_cache=False`` re-runs ``lm.forward`` on the replicated rows.  ``members`` (a
    :class:`~eavqa_amd.models.search.EnsembleMembers`): the n draws per question are made under an ensemble - ``src/mask/pos`` hold the
    B * members.n prompts ordered (question, member), the step source runs n rows for each of them and
    :func:`~eavqa_amd.models.search.ensemble_group_source` folds its logits to the B * n rows of the loop.  Returns
    ``(ids List[List[int]] of B * n rows, float32 [B * n] sums of the drawn tokens' log-probabilities under the processed distribution)``;
    finished rows emit pad, whose steps add nothing to the sum."""
    n, ML = int(num_return_sequences), int(max_length)
    if not 1 <= n <= 8:
        raise ValueError(f"num_return_sequences in 1..8 (got {num_return_sequences})")
    if sampler is None or sampler.seed is None:
        raise ValueError("group_sample_decode needs a sampler with its seed set")
    if lm.fp8:
        raise NotImplementedError('weight_format="fp8": several draws per prompt on the causal path are built for fp32 and bf16 weights')
    dev, V, R = lm.device, lm.vocab, B * n
    items = B * members.n if members is not None else B        # the prompts: with members, (question, member) pairs
    proc = logits_plan.upload(V, dev) if logits_plan is not None else None
    con = upload_constraint(constraint, eos_token_id, B, V, dev)
    if use_cache:
        source = _shared_source(lm, prefix_rows, src, mask, pos, items, n, S0, ML)
    else:
        rep = lambda x: x.repeat_interleave(n, dim=0).contiguous()
        source = _reforward_source(lm, prefix_rows, rep(src), rep(mask), rep(pos), items * n, S0)
    if members is not None:
        source = search.ensemble_group_source(source, B, n, V, members, dev)
    seq, scores = search.pick_loop(source, R, V, ML, pad_token_id, eos_token_id, dev, sampler=sampler, proc=proc, con=con, scores="logp_sum")
    return seq.numpy().astype(int).tolist(), scores


_BEAM_KWARGS = ("num_beams", "num_return_sequences", "length_penalty", "early_stopping")
_DRAW_KWARGS = ("num_return_sequences", "temperature", "top_k", "top_p", "seed")
_COMMON_KWARGS = ("max_length", "pad_token_id", "eos_token_id", "use_cache")


def shared_search_plan(kind: str, kw: dict, *, config_eos_token_id: Optional[int] = None, config_pad_token_id: Optional[int] = None) -> dict:
    """The arguments of ``ClipCaptionModel.generate_beams`` (``kind="beams"``) / ``generate_draws`` (``"draws"``) by name (missing or None =
    the default), checked on the host before anything runs, with the rules and error types of ``vct0.generation_plan``: 1..8 beams
    (``NotImplementedError`` beyond), ``num_return_sequences`` in 1..num_beams (``ValueError``) or 1..8 draws, one eos id, ``early_stopping``
    False / True / "never"; an unknown name raises ``TypeError`` naming it; eos and pad fall back to the LM config's, and both missing
    raises ``ValueError``.  Returns the resolved dict; ``logits`` holds the :class:`~eavqa_amd.models.logits_process.LogitsPlan` or None,
    ``sampler`` (draws) the :class:`~eavqa_amd.models.sampling.Sampler`, its seed still None when the call named none, and - only when
    ``allowed_sequences`` was given - ``constraint`` the :class:`~eavqa_amd.models.constrained.AnswerTrie`."""
    from .logits_process import LOGITS_KWARGS
    from .sampling import sampling_plan
    if kind not in ("beams", "draws"):
        raise ValueError(f"kind={kind!r}: 'beams' or 'draws'")
    known = (_BEAM_KWARGS if kind == "beams" else _DRAW_KWARGS) + _COMMON_KWARGS + LOGITS_KWARGS + CONSTRAINT_KWARGS
    unknown = sorted(n for n in kw if n not in known)
    if unknown:
        raise TypeError(f"unexpected generation arguments: {unknown}")
    ml = kw.get("max_length")
    ml = 10 if ml is None else int(ml)
    if ml < 1:
        raise ValueError(f"max_length={ml}: at least one new token")
    # only the names the call gave: HF's default top_k of 50 holds when top_k is not named, None / 0 switch the filter off
    sampler = None if kind == "beams" else sampling_plan(dict({n: kw[n] for n in ("temperature", "top_k", "top_p", "seed") if n in kw}, do_sample=True))
    r = search.resolve_common(kw, sampler=sampler, max_length=ml, config_eos_token_id=config_eos_token_id,
                              config_pad_token_id=config_pad_token_id, need_fill=True, eos_needs_pad=kind == "draws")
    plan = dict(max_length=ml, pad_token_id=r["pad_token_id"], eos_token_id=r["eos_token_id"], num_return_sequences=r["num_return_sequences"],
                use_cache=True if kw.get("use_cache") is None else bool(kw["use_cache"]), logits=r["logits"])
    if kind == "beams":
        plan.update(num_beams=r["num_beams"], early_stopping=r["early_stopping"], length_penalty=r["length_penalty"])
    else:
        plan["sampler"] = sampler
    if r["constraint"] is not None:                            # the key exists only when the call named `allowed_sequences`
        plan["constraint"] = r["constraint"]
    return plan
