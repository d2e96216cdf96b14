"""GPU: beam search (``num_beams`` > 1) - ``eavqa_beam_step`` against a torch restatement of one step of HF's
``GenerationMixin._beam_search`` (transformers 5.15), ``eavqa_beam_reorder`` against ``index_select``, the decoder step whose B * k rows
share B encoder outputs against the plain step on k-fold repeated inputs, and ``VCT0Prefix.generate(num_beams=k)`` against what the
REFERENCE's ``VCT0Prefix.generate`` produced (tests/golden/vct0_beam.npz, written by tests/golden/make_golden_beam.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import load_golden

DEV = "cuda"
NEG = -1.0e9
MARGIN = 1e-3          # smallest ranking gap a case may have: the kernel's log-softmax differs from torch's by ~1e-6, never by 1e-3


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------ one step of HF's beam search, in torch
class Gaps:
    def __init__(self):
        self.min = float("inf")


def _top(x, n, gaps):
    """``torch.topk(x, n)`` with the tie rule spelled out (stable: the smaller index wins) and the ranking margin recorded: the smallest gap
    between adjacent values among the n selected and the first one not selected, -1e9 sentinels ignored."""
    v, i = torch.sort(x, dim=-1, descending=True, stable=True)
    w = v[..., :min(n + 1, v.shape[-1])]
    real = w > -1.0e8
    g = (w[..., :-1] - w[..., 1:])[real[..., :-1] & real[..., 1:]]
    if g.numel():
        gaps.min = min(gaps.min, float(g.min()))
    return v[..., :n], i[..., :n]


def _gather(t, idx):
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.take_along_dim(t, idx.expand(*idx.shape[:2], *t.shape[2:]), dim=1)


def init_state(B, k, max_length, start, fill):
    run_seq = torch.full((B, k, max_length), fill, dtype=torch.int64)
    run_seq[:, :, 0] = start
    run_scores = torch.full((B, k), NEG)
    run_scores[:, 0] = 0.0
    return dict(run_seq=run_seq, run_scores=run_scores, pool_seq=run_seq.clone(), pool_scores=torch.full((B, k), NEG),
                pool_len=torch.ones((B, k), dtype=torch.int64), pool_fin=torch.zeros((B, k), dtype=torch.bool), improve=torch.ones(B, dtype=torch.bool))


def ref_step(st, logits, V, k, cur_len, max_length, eos, lp, es, gaps, prompt_len=1):
    """Steps b - g of ``_beam_search`` (generation/utils.py:3384-3508) on the CPU: returns (new state, next tokens, flat parents, continue)."""
    B = st["run_scores"].shape[0]
    acc = torch.log_softmax(logits[:, :V].float(), dim=-1).view(B, k, V) + st["run_scores"][:, :, None]
    tv, ti = _top(acc.reshape(B, k * V), 2 * k, gaps)                                              # c. _get_top_k_continuations
    par, tok = ti // V, ti % V
    cand_seq = _gather(st["run_seq"], par).clone()
    cand_seq[:, :, cur_len] = tok
    hit = (tok == eos) | (cur_len + 1 == max_length)                                               # d. eos / max_length criteria
    rv = tv + hit.to(torch.float32) * NEG                                                          # e. _get_running_beams_for_next_iteration
    _, ni = _top(rv, k, gaps)
    new = dict(run_seq=_gather(cand_seq, ni), run_scores=_gather(rv, ni))
    next_tokens = _gather(tok, ni).reshape(-1)
    parents = (_gather(par, ni) + torch.arange(B)[:, None] * k).reshape(-1)
    did = hit & (torch.arange(2 * k) < k)[None, :]                                                 # f. _update_finished_beams
    s = tv / ((cur_len + 1 - prompt_len) ** lp)
    s = s + (st["pool_fin"].all(-1, keepdim=True) & (es is True)).to(torch.float32) * NEG
    s = s + (~st["improve"][:, None]).to(torch.float32) * NEG
    s = s + (~did) * NEG
    ms = torch.cat((st["pool_scores"], s), 1)
    _, mi = _top(ms, k, gaps)
    new["pool_seq"] = _gather(torch.cat((st["pool_seq"], cand_seq), 1), mi)
    new["pool_scores"] = _gather(ms, mi)
    new["pool_fin"] = _gather(torch.cat((st["pool_fin"], did), 1), mi)
    new["pool_len"] = _gather(torch.cat((st["pool_len"], torch.full((B, 2 * k), cur_len + 1)), 1), mi)
    cur = cur_len + 1                                                                              # g. _check_early_stop_heuristic
    L = (max_length - prompt_len) if (es == "never" and lp > 0.0) else (cur - prompt_len)
    best = new["run_scores"][:, :1] / (L ** lp)
    worst = torch.where(new["pool_fin"], new["pool_scores"].min(1, keepdim=True)[0], torch.tensor(NEG))
    new["improve"] = st["improve"] & (best > worst).any(-1)
    cont = bool(new["improve"].any()) and not (bool(new["pool_fin"].all()) and es is True) and not bool(hit.all())
    return new, next_tokens, parents, cont


def _close(got, want, what):
    """Scores: 2e-5 on real values; -1e9 sentinels (whose float32 spacing is 64) only have to be sentinels on both sides."""
    got, want = got.reshape(-1).cpu(), want.reshape(-1)
    real = want > -1.0e8
    assert torch.equal(got > -1.0e8, real), what
    assert (got[real] - want[real]).abs().max().item() <= 2e-5 if real.any() else True, (what, got, want)
    assert (got[~real] - want[~real]).abs().max().item() <= 256.0 if (~real).any() else True, what


def _step_logits(seed, step, B, k, V, ld):
    g = torch.Generator().manual_seed(1000 * seed + step)
    lg = torch.full((B * k, ld), 1.0e30)          # pad columns: a read beyond V would win every selection
    lg[:, :V] = torch.randn(B * k, V, generator=g) * 4
    return lg


MAX_LENGTH, N_STEPS = 7, 6


def _scenario(seed, B, k, V, ld, lp, es):
    """Six consecutive steps on the CPU restatement.  Per step the logits, the eos id and the states before and after:
      step 1 plain (beams 1.. still at -1e9);  2: eos = item 0's best candidate (enters the pool);  3: eos = a candidate of item 0 at rank
      k .. 2k - 1 that is in no rank < k (must NOT enter the pool);  4: every beam of item 1 has eos on top, so all of its top k hit and the
      next running beams come from ranks k .. 2k - 1;  5: item 2's improvement flag is already down and its best candidate is eos (masked
      with -1e9, the pool stays);  6: cur_len + 1 == max_length, every candidate hits."""
    gaps = Gaps()
    st = init_state(B, k, MAX_LENGTH, 0, 1)
    steps = []
    for step in range(1, N_STEPS + 1):
        lg = _step_logits(seed, step, B, k, V, ld)
        before = {n: v.clone() for n, v in st.items()}
        acc = torch.log_softmax(lg[:, :V], -1).view(B, k, V) + st["run_scores"][:, :, None]
        order = torch.sort(acc.reshape(B, k * V), dim=-1, descending=True, stable=True)[1][:, :2 * k] % V
        eos = -1                                   # no token is eos in the plain steps
        if step == 2:
            eos = int(order[0, 0])
        elif step == 3:
            late = [int(t) for t in order[0, k:] if int(t) not in order[0, :k].tolist()]
            assert late
            eos = late[0]
        elif step == 4:
            eos = 7
            lg[k:2 * k, eos] = lg[k:2 * k, :V].max(-1).values + 40.0
        elif step == 5:
            before["improve"][2] = False
            eos = int(order[2, 0])
        st, tokens, parents, cont = ref_step(before, lg, V, k, step, MAX_LENGTH, eos, lp, es, gaps)
        steps.append(dict(logits=lg, eos=eos, before=before, after=st, tokens=tokens, parents=parents, cont=cont))
    return steps, gaps.min


# seeds whose CPU restatement keeps the 1e-3 ranking margin in every row of every step (found by running _scenario over seeds 0, 1, ... on
# the CPU; the test asserts the margin again): 0 unless listed
SEEDS = {(8, 50): 11, (8, 96): 1, (8, 32128): 34}


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("V", [50, 96, 32128])
@pytest.mark.parametrize("k,lp,es", [(1, 1.0, False), (2, 1.0, True), (3, 2.0, False), (5, 1.0, "never"), (8, 0.5, True)])
def test_beam_step_is_one_step_of_hf_beam_search(ops, k, lp, es, V, pad):
    B = 3
    ld = (V + 32 + 3) // 4 * 4 if pad else V
    steps, gap = _scenario(SEEDS.get((k, V), 0), B, k, V, ld, lp, es)
    assert gap >= MARGIN, gap
    # the scenario is what its docstring says
    s2, s3, s4, s5, s6 = steps[1], steps[2], steps[3], steps[4], steps[5]
    assert s2["after"]["pool_fin"][0].any() and not s2["before"]["pool_fin"][0].any()
    assert torch.equal(s3["after"]["pool_fin"][0], s3["before"]["pool_fin"][0]) and torch.equal(s3["after"]["pool_seq"][0], s3["before"]["pool_seq"][0])
    assert (s4["tokens"][k:2 * k] != s4["eos"]).all() and s4["after"]["pool_fin"][1].sum() >= min(k, 2)
    assert torch.equal(s5["after"]["pool_seq"][2], s5["before"]["pool_seq"][2]) and not s5["after"]["improve"][2]
    assert s6["after"]["pool_fin"][:2].all() and not s6["cont"]            # (item 2's pool was frozen by the flag forced down in step 5)
    if k > 1:
        assert any(not torch.equal(s["parents"], torch.arange(B * k)) for s in steps[1:])

    st = ops.BeamState(B, k, MAX_LENGTH, 0, 1, DEV)
    for step, s in enumerate(steps, start=1):
        st.improve.copy_(s["before"]["improve"].to(torch.int32))          # (step 5 enters with item 2's flag down)
        ops.beam_step(s["logits"].to(DEV), V, st, step, s["eos"], lp, es)
        w = s["after"]
        what = f"step {step}"
        assert torch.equal(st.next_tokens.cpu(), s["tokens"]), what
        assert torch.equal(st.parents.cpu().long(), s["parents"]), what
        assert torch.equal(st.run_seq.cpu().view(B, k, -1), w["run_seq"]), what
        assert torch.equal(st.pool_seq.cpu().view(B, k, -1), w["pool_seq"]), what
        assert torch.equal(st.pool_len.cpu().long(), w["pool_len"]), what
        assert torch.equal(st.pool_fin.cpu().bool(), w["pool_fin"]), what
        assert torch.equal(st.improve.cpu().bool(), w["improve"]), what
        assert int(st.cont[step].item()) == int(s["cont"]), what
        _close(st.run_scores, w["run_scores"], what + " running scores")
        _close(st.pool_scores, w["pool_scores"], what + " pool scores")


# ------------------------------------------------------------------------------------------------ K / V cache reorder
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("inner", [64, 136, 2056])
@pytest.mark.parametrize("t", [1, 5])
def test_beam_reorder_is_index_select(ops, dtype, inner, t):
    rows, t_max, planes = 6, 7, 4                                            # 2 layers x (K, V)
    g = torch.Generator().manual_seed(3)
    src = torch.randn(planes, rows, t_max, inner, generator=g).to(dtype).to(DEV)
    keep = src.clone()
    for parents in ([0, 0, 2, 5, 4, 4], [5, 3, 1, 0, 2, 4]):                 # repeated / permuted
        dst = torch.full_like(src, 7.0)
        par = torch.tensor(parents, dtype=torch.int32, device=DEV)
        ops.beam_reorder(src, dst, par, t)
        assert torch.equal(dst[:, :, :t], src.index_select(1, par.long())[:, :, :t])
        assert (dst[:, :, t:] == 7.0).all()                                   # positions >= t are not touched
        assert torch.equal(src, keep)


# ------------------------------------------------------------------------------------------------ decoder step, B * k rows over B encoder outputs
def _model(tag, dtype):
    from eavqa_amd.models.t5 import FrozenT5, T5Config
    from eavqa_amd.models.vct0 import VCT0Prefix
    z = load_golden(f"vct0_{tag}.npz")
    T = lambda a: torch.from_numpy(a)
    V, E, DKV, H, F, NL, L, D, gated, tied = [int(v) for v in z["cfg"]]
    sd = {n[3:]: T(v) for n, v in z.items() if n.startswith("lm.")}
    lm = FrozenT5(T5Config(E, DKV, H, F, NL, NL, V, bool(gated), bool(tied)), sd, dtype, DEV)
    model = VCT0Prefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=dtype, device=DEV).eval()
    model.clip_project.load_state_dict({n[4:]: T(v) for n, v in z.items() if n.startswith("map.")})
    return model, V, D


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 6e-2)])
def test_beams_decoder_step_equals_the_plain_step_on_repeated_encoder_outputs(dtype, tol):
    """``eavqa_t5_decoder_step_beams`` (B = 2, k = 3: six decoder rows over two encoder outputs) against ``decode_step`` on six rows whose
    encoder K / V and mask are repeated k-fold; and its Python mirror ``decode_step(beams=k)`` bit for bit."""
    from eavqa_amd.models.t5 import _StepDriver
    model, V, D = _model("t0", dtype)
    lm, c = model.lm, model.lm.cfg
    B, k, S, t, t_max = 2, 3, 11, 4, 6
    R, I = B * k, c.inner
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(B * S, c.d_model, generator=g).to(dtype).to(DEV)
    mask = torch.ones(B, S, dtype=torch.int32)
    mask[1, S - 3:] = 0
    mask = mask.to(DEV)
    y = torch.randn(R, c.d_model, generator=g).to(DEV)
    kv = lm.cross_kv(enc)
    fill = [(torch.randn(R * t_max, I, generator=g).to(dtype).to(DEV), torch.randn(R * t_max, I, generator=g).to(dtype).to(DEV)) for _ in lm.dec]
    clone = lambda: [(a.clone(), b.clone()) for a, b in fill]
    rel = lm.rel_table(True, t_max)
    c_native, c_py, c_ref = clone(), clone(), clone()
    got = _StepDriver(lm, c_native, kv, B, t_max, beams=k).step(y.clone(), mask, t, S, rel).clone()
    mirror = lm.decode_step(y.clone(), c_py, mask, B, t, S, kv, t_max, rel, beams=k)
    assert torch.equal(got, mirror)
    for (a, b), (a2, b2) in zip(c_native, c_py):
        assert torch.equal(a, a2) and torch.equal(b, b2)
    rep = lambda x: x.view(B, S, -1).repeat_interleave(k, dim=0).reshape(R * S, -1).contiguous()
    lm.step_route = 1                                                       # the eavqa_gemm route on both sides
    try:
        want = lm.decode_step(y.clone(), c_ref, mask.repeat_interleave(k, dim=0).contiguous(), R, t, S, [rep(x) for x in kv], t_max, rel)
    finally:
        lm.step_route = 0
    err = (got.float() - want.float()).abs().max().item()
    print(f"[{dtype}] beams step vs repeated plain step: max |diff| {err:.2e}")
    # fp32: 1e-5 absolute; bf16: the bound of the cached-vs-uncached T5 test (test_t5_gpu.py), relative to the largest entry
    assert err <= (tol if dtype == torch.float32 else tol * max(1.0, want.float().abs().max().item()))
    for (a, b), (a2, b2) in zip(c_native, c_ref):
        assert torch.equal(a, a2) and torch.equal(b, b2)                     # the appended K / V rows do not depend on the cross-attention


# ------------------------------------------------------------------------------------------------ the reference's beam search
ES = {0: False, 1: True, 2: "never"}


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("tag", ["t0", "t5v10"])
def test_generate_with_beams_matches_the_reference(tag, native):
    """Every case of vct0_beam.npz in fp32: ``sequences`` equal to the reference's including shape and fill, ``sequences_scores`` within
    2e-4 (2e-5 logits parity x at most 7 accumulated steps, before the division by a length >= 1)."""
    z = load_golden("vct0_beam.npz")
    model, V, D = _model(tag, torch.float32)
    model.lm.native_step = native
    T = lambda a: torch.from_numpy(a)
    for name, path in zip(z["cases"].tolist(), z["paths"].tolist()):
        f = lambda field: z[f"{tag}.{name}.{field}"]
        k, nrs, es, eos, max_length = [int(v) for v in f("params")]
        assert float(f("min_gap")) >= MARGIN
        kw = dict(max_length=max_length, num_beams=k, num_return_sequences=nrs, length_penalty=float(f("length_penalty")), early_stopping=ES[es],
                  eos_token_id=eos, do_sample=False, output_scores=True, return_dict_in_generate=True, special_token_id=V - 1)
        if path == "prefix":
            o = model.generate(prefix=T(f("prefix")), **kw)
        else:
            o = model.generate(prefix=T(f("prefix")), question_tokens=T(f("tokens")), question_mask=T(f("mask")), no_prefix=path == "text", **kw)
        want, want_scores = T(f("sequences")), T(f("sequences_scores"))
        err = (o.sequences_scores - want_scores).abs().max().item()
        print(f"[{tag} {name} native={native}] sequences {tuple(o.sequences.shape)} max |score diff| {err:.2e}")
        assert o.sequences.shape == want.shape and torch.equal(o.sequences, want), (name, o.sequences, want)
        assert err <= 2e-4, name
        assert o.scores is None
        if path == "prefix":                                                # without return_dict_in_generate: the plain id tensor
            assert torch.equal(model.generate(prefix=T(f("prefix")), **{**kw, "return_dict_in_generate": False}), want)


def _prefix_run(model, D, B, **kw):
    prefix = 3.0 * torch.randn(B, D, generator=torch.Generator().manual_seed(B))
    return model.generate(prefix=prefix, output_scores=True, return_dict_in_generate=True, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,k", [(2, 4), (9, 8)])
def test_cached_beam_search_equals_the_reforward_loop(dtype, B, k):
    """``use_cache=True`` (K / V caches reordered by beam parent every step) and ``use_cache=False`` (the decoder re-run over the running
    sequences, no cache, no reorder) return the same ids; B = 9, k = 8 is 72 decoder rows, beyond the 64-row kernels."""
    model, V, D = _model("t0", dtype)
    kw = dict(max_length=12, num_beams=k, num_return_sequences=k, eos_token_id=18)
    a, b = _prefix_run(model, D, B, use_cache=True, **kw), _prefix_run(model, D, B, use_cache=False, **kw)
    print(f"[{dtype} B={B} k={k}] max |score diff| {(a.sequences_scores - b.sequences_scores).abs().max().item():.2e}")
    assert a.sequences.shape == (B * k, a.sequences.shape[1]) and torch.equal(a.sequences, b.sequences)


def test_num_beams_one_is_the_greedy_path():
    model, V, D = _model("t0", torch.float32)
    a = _prefix_run(model, D, 3, max_length=9)
    b = _prefix_run(model, D, 3, max_length=9, num_beams=1)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(torch.stack(list(a.scores)), torch.stack(list(b.scores)))
    assert a.sequences_scores is None and b.sequences_scores is None
    # the eos override reaches the greedy path: with the fixture's text-only inputs and its eos (a token the model emits early), every row
    # is the run without the override up to its first eos, pad afterwards, and the batch is cut where the last row ends
    z = load_golden("vct0_beam.npz")
    f = lambda field: torch.from_numpy(z[f"t0.text_k3.{field}"])
    kw = dict(prefix=f("prefix"), question_tokens=f("tokens"), question_mask=f("mask"), no_prefix=True, max_length=8)
    eos = int(f("params")[3])
    free, got = model.generate(**kw), model.generate(eos_token_id=eos, **kw)
    want = free.clone()
    ends = []
    for r in range(free.shape[0]):
        hits = (free[r, 1:] == eos).nonzero()
        end = int(hits[0]) + 2 if hits.numel() else free.shape[1]
        want[r, end:] = 0
        ends.append(end)
    assert min(ends) < free.shape[1]                                         # the override did end a row early
    assert torch.equal(got, want[:, :max(ends)])
