"""The full-sequence passes of the frozen LMs and the transformer mapper as a list of small cases, shared by the call-trace test
(tests/test_lm_pass_trace_cpu.py, tensors on the CPU, contents never read) and the bit-for-bit test (tests/test_lm_pass_gpu.py).
The ``*_cached`` cases are the cached generation route instead: a prefill and two one-token steps through the family's block driver.

A case builds a FRESH model (so no case sees what an earlier one prepared lazily: transposed weights, folded weights, a cast shadow), and
``run(model, dev)`` returns the tensors the GPU test compares.  Every shape is decided on the host: packed passes get ``lengths=``."""
import os
from typing import Callable, List, NamedTuple

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HF_DIRS = {"gpt2": "hf_gpt2_tiny", "opt": "hf_opt_tiny"}
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
L = 3                     # prefix positions per row


class Case(NamedTuple):
    name: str
    make: Callable            # (dev) -> model
    run: Callable             # (model, dev) -> {name: tensor}
    root: Callable            # (model) -> the object whose tensors the trace names by attribute path
    family: str               # "lm" (the frozen causal LM's own pass) | "t5" | "mapper"


# ----------------------------------------------------------------------------------------------------------------- models
def _hf_lm(arch, dtype):
    def make(dev):
        from eavqa_amd.models.lm import FrozenCausalLM, LMConfig, load_local_hf
        cfg, sd = load_local_hf(os.path.join(GOLDEN, HF_DIRS[arch]))
        return FrozenCausalLM(LMConfig.from_hf_dict(cfg), sd, dtype, dev)
    return make


def _fp8_lm(dev):
    from eavqa_amd.models.lm import FrozenCausalLM, LMConfig, random_init_state_dict
    cfg = LMConfig("gpt2", 2, 4, 128, 256, 320, 64)
    return FrozenCausalLM(cfg, random_init_state_dict(cfg, 5, "cpu"), torch.bfloat16, dev, weight_format="fp8")


def _llama_lm(dtype):
    """Two layers, grouped K/V heads (4 query heads over 2), an untied head, hd = 16, F % 4 == 0."""
    def make(dev):
        from eavqa_amd.models.lm import FrozenCausalLM, LMConfig, random_init_state_dict
        cfg = LMConfig.from_hf_dict(dict(model_type="llama", vocab_size=320, hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
                                         num_key_value_heads=2, intermediate_size=96, max_position_embeddings=64, rms_norm_eps=1e-5))
        return FrozenCausalLM(cfg, random_init_state_dict(cfg, 5, "cpu"), dtype, dev)
    return make


def _t5(dtype, gated):
    def make(dev):
        from eavqa_amd.models.t5 import FrozenT5, T5Config, random_init_t5_state_dict
        cfg = T5Config(64, 16, 4, 128, 2, 2, 320, gated=gated, tied=not gated)
        return FrozenT5(cfg, random_init_t5_state_dict(cfg, 7, "cpu"), dtype, dev)
    return make


def _mapper(dtype):
    def make(dev):
        from eavqa_amd.models.clipcap import TransformerMapper
        torch.manual_seed(11)                                 # the default nn init draws on the host
        return TransformerMapper(32, 64, L, 2, num_layers=2, device=dev, dtype=dtype)
    return make


# ----------------------------------------------------------------------------------------------------------------- inputs
def _prefix_batch(lm, dev, lengths, T, seed, horizon=0):
    """B rows of L prefix + T text positions, ``lengths[b]`` of them attended (right padding), labels on the attended text positions
    that have a text predecessor: a proper subset of the rows.  ``horizon`` appended, attended positions (scoring)."""
    from eavqa_amd import ops
    g = torch.Generator().manual_seed(seed)
    B, V, E = len(lengths), lm.vocab, lm.cfg.n_embd
    tok = torch.randint(3, V - 8, (B, T), generator=g)
    qm = torch.zeros(B, T, dtype=torch.int64)
    labels = torch.full((B, L + T), -100, dtype=torch.int64)
    for b, n in enumerate(lengths):
        qm[b, :n - L] = 1
        labels[b, L + 1:n] = tok[b, 1:n - L]
    rows = (0.5 * torch.randn(B * L, E, generator=g)).to(dev, lm.dtype)
    tok_ext = torch.cat([tok, torch.zeros(B, horizon, dtype=torch.int64)], 1)
    qm_ext = torch.cat([qm, torch.ones(B, horizon, dtype=torch.int64)], 1)
    src, mask, pos = ops.build_prefix_rows(tok_ext.to(dev), qm_ext.to(dev), L, lm.cfg.pos_mode)
    return rows, src, mask, pos, labels.to(dev), int((labels != -100).sum()), g


def _candidates(V, B, C, Tc, g):
    cand = torch.randint(3, V - 8, (B, C, Tc), generator=g)
    cand[0, 1, Tc - 1] = -100
    cand[B - 1, C - 1, 1:] = -100
    return cand


# ----------------------------------------------------------------------------------------------------------------- runs
def _train(pack, scored, lengths=(8, 6), T=5, **switches):
    def run(lm, dev):
        for k, v in switches.items():
            assert hasattr(lm, k)
            setattr(lm, k, v)
        B, S = len(lengths), L + T
        rows, src, mask, pos, labels, n_lab, _ = _prefix_batch(lm, dev, lengths, T, 3)
        M = sum(lengths) if pack else B * S
        assert not scored or 0 < n_lab < M
        out = lm.forward(rows, src, pos, mask, B, S, labels=labels, save=True, pack=pack, lengths=list(lengths) if pack else None,
                         n_scored=n_lab if scored else None)
        d = lm.backward(out["tape"], torch.ones(1, device=dev, dtype=torch.float32), rows.shape[0])
        return dict(loss=out["loss"], count=out["count"], logits=out["logits"][:, :lm.vocab], dprefix=d)
    return run


def _logits(mode, lengths=(8, 6), T=5, **switches):
    def run(lm, dev):
        for k, v in switches.items():
            assert hasattr(lm, k)
            setattr(lm, k, v)
        B, S = len(lengths), L + T
        rows, src, mask, pos, _, _, _ = _prefix_batch(lm, dev, lengths, T, 3)
        if switches:                                          # the folded route is a packed one (M rows, not B * S)
            out = lm.forward(rows, src, pos, mask, B, S, logits=mode, pack=True, lengths=list(lengths))
        else:
            out = lm.forward(rows, src, pos, mask, B, S, logits=mode)
        return dict(hidden=out["hidden"]) if mode == "none" else dict(logits=out["logits"][:, :lm.vocab])
    return run


def _score(share, C=3, Tc=3, T=5, lengths=(8, 6)):
    def run(lm, dev):
        from eavqa_amd.models.decode import score_decode
        B = len(lengths)
        rows, src, mask, pos, _, _, g = _prefix_batch(lm, dev, lengths, T, 4, horizon=Tc)
        cand = _candidates(lm.vocab, B, C, Tc, g).to(dev)
        return dict(token_logprobs=score_decode(lm, rows, src, mask, pos, B, L + T, cand, share_prompt=share))
    return run


def _cached(seed, lengths=(8, 6), T=5):
    """The cached generation route: prefill of the prompt, then two one-token steps teacher-forced from the horizon columns."""
    def run(lm, dev):
        from eavqa_amd.models import decode
        B, S0 = len(lengths), L + T
        rows, src, mask, pos, _, _, _ = _prefix_batch(lm, dev, lengths, T, seed, horizon=2)
        cache = decode._KVCache(lm, B, S0 + 2, B * S0)
        out = dict(prefill=decode._prefill(lm, cache, rows, src[:, :S0].contiguous(), pos[:, :S0].contiguous(), mask, B, S0, S0 + 2))
        for t in range(2):
            out[f"step{t}"] = decode._decode_step(lm, cache, src[:, S0 + t].contiguous(), pos[:, S0 + t].contiguous(), mask, B, S0 + t, S0 + 2)
        return {k: v[:, :lm.vocab] for k, v in out.items()}
    return run


def _t5_train(t5, dev):
    g = torch.Generator().manual_seed(6)
    B, S, Td, c = 2, 6, 4, t5.cfg
    enc_rows = (0.5 * torch.randn(B * S, c.d_model, generator=g)).to(dev, t5.dtype)
    labels = torch.randint(2, c.vocab, (B, Td), generator=g)
    labels[1, Td - 1] = -100
    out = t5.forward_train(enc_rows, B, S, labels.to(dev))
    d = t5.backward(out["tape"], torch.ones(1, device=dev, dtype=torch.float32))
    tape = out["tape"]                                        # (a dict at the commit the fixtures were recorded from: the cases run there too)
    return dict(loss=out["loss"], count=tape["count"] if isinstance(tape, dict) else tape.count, logits=out["logits"][:, :c.vocab], denc=d)


def _t5_score(t5, dev):
    g = torch.Generator().manual_seed(8)
    B, S, C, Tc, c = 2, 6, 3, 3, t5.cfg
    ids = torch.randint(2, c.vocab, (B, S), generator=g).to(dev)
    mask = torch.ones(B, S, dtype=torch.int32)
    mask[1, S - 2:] = 0
    mask = mask.to(dev)
    with torch.no_grad():
        enc_out, _ = t5.encode(t5.embed(ids), mask, B, S)
        cand = _candidates(c.vocab, B, C, Tc, g).to(dev)
        return dict(token_logprobs=t5.score(enc_out, mask, B, S, cand, share_prompt=True))


def mapper_grad_parts(mod):
    """The mapper's flat gradient as (everything but the LayerNorm affine gradients, dgamma of every layer, dbeta of every layer):
    ``ln_dparam_kernel`` sums dgamma / dbeta with float atomics, whose order is not fixed."""
    fl = mod.flat
    rest = fl.grad.clone()
    parts = {"weight": [], "bias": []}
    for i in range(mod.num_layers):
        for norm in ("norm1", "norm2"):
            for kind in parts:
                name = f"transformer.layers.{i}.{norm}.{kind}"
                parts[kind].append(fl.g(name).clone())
                fl.view(rest, name).zero_()
    return rest, torch.cat(parts["weight"]), torch.cat(parts["bias"])


def _mapper_run(mod, dev):
    g = torch.Generator().manual_seed(12)
    B, N, E = 2, mod.clip_length + mod.prefix_length, mod.E
    x = torch.randn(B, 32, generator=g).to(dev)
    y = mod(x)
    dout = torch.randn(B, N, E, generator=g)
    dout[:, :mod.clip_length] = 0                             # only the prefix rows of the stream are consumed
    y.backward(dout.to(dev, y.dtype))
    rest, dgamma, dbeta = mapper_grad_parts(mod)
    return dict(out=y.detach(), grad=rest, grad_ln_dgamma=dgamma, grad_ln_dbeta=dbeta)


# ----------------------------------------------------------------------------------------------------------------- the list
FOLD = dict(lengths=(20, 18, 17, 15), T=17)                   # B = 4, S = 20, M = 70 > 64: where fold_layernorm switches on


def _cases() -> List[Case]:
    same = lambda m: m
    out = []
    for arch in ("gpt2", "opt"):
        for dn, dt in DTYPES.items():
            lm = _hf_lm(arch, dt)
            p = f"{arch}_{dn}_"
            out += [Case(p + "train_packed_scored", lm, _train(True, True), same, "lm"),
                    Case(p + "train_packed", lm, _train(True, False), same, "lm"),
                    Case(p + "train_masked", lm, _train(False, False), same, "lm"),
                    Case(p + "logits_all", lm, _logits("all"), same, "lm"),
                    Case(p + "logits_last", lm, _logits("last"), same, "lm"),
                    Case(p + "logits_none", lm, _logits("none"), same, "lm"),
                    Case(p + "score_shared", lm, _score(True), same, "lm"),
                    Case(p + "score_replicated", lm, _score(False), same, "lm")]
        lm = _hf_lm(arch, torch.bfloat16)
        out += [Case(f"{arch}_bf16_train_no_prefetch", lm, _train(True, True, weight_prefetch=False), same, "lm"),
                Case(f"{arch}_bf16_train_fold", lm, _train(True, False, fold_layernorm=True, **FOLD), same, "lm"),
                Case(f"{arch}_bf16_hidden_fold", lm, _logits("none", fold_layernorm=True, **FOLD), same, "lm")]
    out += [Case("fp8_train_fused_quantizer", _fp8_lm, _train(True, True, fuse_quantizer=True), same, "lm"),
            Case("fp8_train_separate_quantizer", _fp8_lm, _train(True, True, fuse_quantizer=False), same, "lm"),
            Case("fp8_score", _fp8_lm, _score(True), same, "lm")]
    for dn, dt in DTYPES.items():
        out += [Case(f"t5_gated_{dn}_train", _t5(dt, True), _t5_train, same, "t5"),
                Case(f"t5_plain_{dn}_train", _t5(dt, False), _t5_train, same, "t5"),
                Case(f"t5_gated_{dn}_score_shared", _t5(dt, True), _t5_score, same, "t5"),
                Case(f"mapper_{dn}", _mapper(dt), _mapper_run, lambda m: m.flat, "mapper")]
    # appended behind the 49 cases above, whose order and names stay: the Llama family, then the cached generation route of every family
    for dn, dt in DTYPES.items():
        lm = _llama_lm(dt)
        p = f"llama_{dn}_"
        out += [Case(p + "train_packed_scored", lm, _train(True, True), same, "lm"),
                Case(p + "train_packed", lm, _train(True, False), same, "lm"),
                Case(p + "train_masked", lm, _train(False, False), same, "lm"),
                Case(p + "logits_all", lm, _logits("all"), same, "lm"),
                Case(p + "logits_last", lm, _logits("last"), same, "lm"),
                Case(p + "logits_none", lm, _logits("none"), same, "lm")]
    out += [Case("llama_bf16_train_no_prefetch", _llama_lm(torch.bfloat16), _train(True, True, weight_prefetch=False), same, "lm")]
    for arch, lm_of in (("gpt2", lambda dt: _hf_lm("gpt2", dt)), ("opt", lambda dt: _hf_lm("opt", dt)), ("llama", _llama_lm)):
        out += [Case(f"{arch}_{dn}_cached", lm_of(dt), _cached(5), same, "lm") for dn, dt in DTYPES.items()]
    out += [Case("fp8_cached", _fp8_lm, _cached(5), same, "lm")]
    return out


CASES = _cases()


# ----------------------------------------------------------------------------------------------------------------- recorded form
FULL_BYTES = 4096         # a quantity above this size is recorded as the SHA-256 of its bytes: equality is all the GPU test asks of it


def recorded(t):
    """A result tensor as the fixture holds it: a numpy array (bf16 widened to float32, which is exact), or - above ``FULL_BYTES`` -
    the 32 digest bytes of that array.  Returns (key suffix, array)."""
    import hashlib

    import numpy as np
    a = t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    if a.nbytes <= FULL_BYTES:
        return "", a
    return "@sha256", np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
