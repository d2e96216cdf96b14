"""Inputs and CPU replays of tests/test_ensemble_generate_gpu.py: B = 3 questions x n = 3 ensemble members on the tiny committed weights
(loaded as tests/_search_modes.py does), ``max_length`` = 6, fp32.

T5: the fixture's few-shot prompt (three images per row) is member 0; a further member permutes the images (what
``num_permutations_of_in_context_examples`` does to the shots) and redraws some of the prompt's text tokens by seed, so that the members
disagree.  :func:`t5_oracle_scores` replays a sequence teacher-forced through oracle/ref_cpu.py, member by member, and
:func:`oracle_greedy` decodes with the oracle alone - which is how MEMBER_SEED was chosen: on the CPU, so that every step's top-two
margin of the combined oracle scores is at least 2e-3 for both T5 tags and both modes (see :func:`margins`)."""
import functools

import torch

import _ensemble_ref as eref
from conftest import load_golden

B, N, MAX_LENGTH = 3, 3, 6
MEMBER_SEED = 2
PERMUTATIONS = ([0, 1, 2], [1, 0, 2], [2, 1, 0])
T = torch.from_numpy


@functools.lru_cache(maxsize=None)
def t5_members(tag, seed=MEMBER_SEED):
    """``dict(prefix [B, N, 3, D], question_tokens [B, N, T], question_mask [B, N, T], special_token_id)`` on the host."""
    z = load_golden(f"vct0_{tag}.npz")
    V = int(z["cfg"][0])
    tok, mask, pf = T(z["fs_tokens"]), T(z["fs_mask"]), T(z["fs_prefix"])[:, :, 0]
    assert tok.shape[0] == B and pf.shape[1] == 3
    g = torch.Generator().manual_seed(seed)
    toks = []
    for i in range(N):
        t = tok.clone()
        if i:
            free = (t < V - 3) & (t > 2) & (mask != 0)                      # neither a sentinel nor a special id nor padding
            redraw = free & (torch.rand(t.shape, generator=g) < 0.5)
            t[redraw] = torch.randint(3, V - 10, (int(redraw.sum()),), generator=g)
        toks.append(t)
    return dict(prefix=torch.stack([pf[:, p] for p in PERMUTATIONS], dim=1), question_tokens=torch.stack(toks, dim=1),
                question_mask=torch.stack([mask] * N, dim=1), special_token_id=V - 1)


def t5_member_call(tag, i, seed=MEMBER_SEED):
    """Member i alone, as the keywords of ``VCT0Model.generate``."""
    m = t5_members(tag, seed)
    return dict(prefix=m["prefix"][:, i], question_tokens=m["question_tokens"][:, i], question_mask=m["question_mask"][:, i],
                special_token_id=m["special_token_id"])


def repeated(call, n=N):
    """n copies of one prompt: the [B, ...] tensors of a plain call as [B, n, ...]."""
    return {k: torch.stack([v] * n, dim=1) if torch.is_tensor(v) else v for k, v in call.items()}


@functools.lru_cache(maxsize=None)
def _t5_oracle(tag):
    z = load_golden(f"vct0_{tag}.npz")
    V, E, DKV, H, F, NL, L, D, gated, tied = [int(v) for v in z["cfg"]]
    sd = {k[3:]: T(v) for k, v in z.items() if k.startswith("lm.")}
    mapper = {k[4:]: T(v) for k, v in z.items() if k.startswith("map.")}
    return sd, dict(n_layer=NL, n_head=H, d_kv=DKV, gated=bool(gated), tied=bool(tied)), mapper, L, E


@functools.lru_cache(maxsize=None)
def _t5_oracle_encoders(tag, seed):
    """Per member: (encoder output [B, S, E], mask [B, S]) of oracle/ref_cpu.py."""
    from oracle import ref_cpu as o
    sd, cfg, mapper, L, E = _t5_oracle(tag)
    m = t5_members(tag, seed)
    out = []
    with torch.no_grad():
        for i in range(N):
            tok, msk, pf = m["question_tokens"][:, i], m["question_mask"][:, i], m["prefix"][:, i]
            pp = o.mapper_project(pf.reshape(-1, pf.shape[-1]), mapper, "mlp", L, E, None, 8).view(B, -1, L, E)
            emb, emask = o.insert_prefix_into_input(L, pf.shape[1] - 1, tok, sd["shared.weight"][tok], pp, msk, m["special_token_id"])
            out.append((o.t5_encoder(sd, cfg, emb, emask), emask))
    return out


def t5_member_logits(tag, ids, seed=MEMBER_SEED):
    """The oracle's logits [steps, B * N, V] (rows ordered (question, member)) for the decoder teacher-forced on ``ids`` int64
    [B, 1 + steps] (the start token first): step k scores ``ids[:, k + 1]``."""
    from oracle import ref_cpu as o
    sd, cfg, _, _, _ = _t5_oracle(tag)
    per_member = []
    with torch.no_grad():
        for enc, emask in _t5_oracle_encoders(tag, seed):
            per_member.append(o.t5_lm_logits(sd, cfg, o.t5_decoder(sd, cfg, sd["shared.weight"][ids[:, :-1]], enc, emask)))      # [B, steps, V]
    lg = torch.stack(per_member, dim=1)                                     # [B, N, steps, V]
    return lg.permute(2, 0, 1, 3).reshape(lg.shape[2], B * N, lg.shape[3])


def t5_oracle_scores(tag, ids, mode, weights=None, seed=MEMBER_SEED):
    """float64 [steps, B, V]: the members' oracle logits combined by tests/_ensemble_ref.py."""
    return torch.stack([eref.combine(step, N, mode, weights) for step in t5_member_logits(tag, ids, seed)])


def ban(scores, banned):
    """``bad_words_ids`` of one id each on combined scores [..., V]: those columns become -inf."""
    s = scores.clone()
    s[..., list(banned)] = float("-inf")
    return s


def oracle_greedy(tag, mode, seed=MEMBER_SEED, max_length=MAX_LENGTH, banned=()):
    """Greedy ensemble decoding with the oracle alone (no eos handling: the tiny models never emit T5's eos; ``banned``: ids kept out,
    as ``bad_words_ids`` does - the tiny models prefer id 0, the pad): ``(ids [B, max_length], float64 scores [max_length - 1, B, V])``."""
    ids = torch.zeros((B, 1), dtype=torch.int64)
    while ids.shape[1] < max_length:
        last = ban(t5_oracle_scores(tag, torch.cat([ids, ids[:, :1]], dim=1), mode, None, seed)[-1], banned)
        ids = torch.cat([ids, last.argmax(-1)[:, None]], dim=1)
    return ids, ban(t5_oracle_scores(tag, ids, mode, None, seed), banned)


def margins(scores):
    """Top-two margin of every (step, question) of float64 ``scores`` [steps, B, V]."""
    top2 = scores.topk(2, dim=-1).values
    return top2[..., 0] - top2[..., 1]


def causal_members(plain, few, V, seed=MEMBER_SEED):
    """The plain and the few-shot call of ``_search_modes.causal_model`` as N members per question: member 0 is the call itself, the
    others carry redrawn CLIP embeddings and some redrawn text tokens.  ``(plain [B, N, ...], few [B, N, ...])``."""
    g = torch.Generator().manual_seed(seed)

    def members(call, sentinel_floor):
        toks, pfs = [], []
        for i in range(N):
            t, p = call["question_tokens"].clone(), call["prefix"].clone()
            if i:
                redraw = (t < sentinel_floor) & (call["question_mask"] != 0) & (torch.rand(t.shape, generator=g) < 0.5)
                t[redraw] = torch.randint(3, sentinel_floor, (int(redraw.sum()),), generator=g)
                p = p + 0.7 * torch.randn(p.shape, generator=g)
            toks.append(t)
            pfs.append(p)
        out = dict(call, question_tokens=torch.stack(toks, dim=1), prefix=torch.stack(pfs, dim=1),
                   question_mask=torch.stack([call["question_mask"]] * N, dim=1))
        return out
    return members(plain, V - 10), members(few, V - 10)


def member_of(call, i):
    """Member i of a [B, N, ...] call, as a plain [B, ...] call."""
    return {k: v[:, i] if torch.is_tensor(v) else v for k, v in call.items()}
