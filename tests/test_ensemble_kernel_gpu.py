"""GPU: ``eavqa_ensemble_combine`` against the float64 restatement of tests/_ensemble_ref.py (which tests/test_ensemble_ref_cpu.py pins
to torch).  As in tests/test_sample_gpu.py the input's pad columns hold 3e38 - one read of them and a member's maximum is wrong - and
the output buffer is pre-filled with a sentinel that must survive beyond column V.  Tolerance: 2e-5 * max(1, |want|), the bound
tests/test_sample_gpu.py holds ``eavqa_sample_pick``'s log-probabilities to."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _ensemble_ref as ref

DEV = "cuda"
PAD_FILL = 3.0e38
SENTINEL = 123.0
NEG_INF = float("-inf")
# V = 7: fewer columns than a wave; 1000 in 1001: scalar loads, V % 4 != 0; 32128 in 32192: 16-byte loads with padding; 50272: more than
# one stride pass per thread of the row statistics, 50 column chunks per question
SHAPES = [(1, 7, 7), (3, 64, 64), (2, 1000, 1001), (2, 32128, 32192), (1, 50272, 50272)]
MEMBERS = (1, 2, 3, 8)
MODES = ("product", "mixture")


@pytest.fixture(scope="module")
def ops():
    from eavqa_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def case(B, V, n):
    """float32 member logits [B * n, V] of a seeded draw, spread like an LM head's (members disagree about the best tokens)."""
    g = torch.Generator().manual_seed(1000 * n + V + B)
    return 4.0 * torch.randn(B * n, V, generator=g) + torch.randn(B * n, 1, generator=g)


@functools.lru_cache(maxsize=None)
def wanted(B, V, n, mode):
    return ref.combine(case(B, V, n), n, mode)


def run(ops, x, n, mode, ld=None, ld_out=None, weights=None, lse=False):
    """One call on float32 CPU ``x`` [B * n, V] placed in a [B * n, ld] device buffer: ``(out [B, ld_out] on the host, member_lse)``."""
    R, V = x.shape
    ld = V if ld is None else ld
    ld_out = ld if ld_out is None else ld_out
    buf = torch.full((R, ld), PAD_FILL, dtype=torch.float32)
    buf[:, :V] = x
    out = torch.full((R // n, ld_out), SENTINEL, dtype=torch.float32, device=DEV)
    w = torch.tensor(ref.normalise(weights, n), dtype=torch.float32, device=DEV) if weights is not None else None
    ml = torch.full((R,), 9.0, dtype=torch.float32, device=DEV) if lse else None
    got = ops.ensemble_combine(buf.to(DEV), V, n, mode, w, out=out, member_lse=ml)
    torch.cuda.synchronize()
    assert got is out
    return out.cpu(), (ml.cpu() if lse else None)


def check(got, want, V):
    """Columns < V within 2e-5 * max(1, |want|) of float64 ``want`` with the same -inf set and no NaN; the sentinel beyond."""
    g = got[:, :V].double()
    assert not torch.isnan(got).any()
    assert torch.equal(torch.isinf(g), torch.isinf(want)) and (g[torch.isinf(g)] == NEG_INF).all()
    fin = ~torch.isinf(want)
    err = (g[fin] - want[fin]).abs() / want[fin].abs().clamp_min(1.0)
    assert err.max().item() <= 2e-5, err.max().item()
    assert (got[:, V:] == SENTINEL).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", MEMBERS)
@pytest.mark.parametrize("B,V,ld", SHAPES, ids=[f"B{b}-V{v}-ld{l}" for b, v, l in SHAPES])
def test_combine_matches_the_float64_restatement(ops, B, V, ld, n, mode):
    x = case(B, V, n)
    got, lse = run(ops, x, n, mode, ld, lse=True)
    check(got, wanted(B, V, n, mode), V)
    want_lse = torch.logsumexp(x.double(), dim=-1)
    assert ((lse.double() - want_lse).abs() / want_lse.abs().clamp_min(1.0)).max().item() <= 2e-5
    if mode == "mixture":                                      # a normalised row
        assert torch.logsumexp(got[:, :V].double(), dim=-1).abs().max().item() <= 2e-5


@pytest.mark.parametrize("B,V,ld", SHAPES, ids=[f"B{b}-V{v}-ld{l}" for b, v, l in SHAPES])
def test_one_member_product_is_log_softmax(ops, B, V, ld):
    """n = 1, product: the member's log_softmax - the float64 one within the tolerance, and bit for bit the row
    ``eavqa_logits_process(to_logprobs=1)`` leaves (both take M and lse from csrc/row_lse.h)."""
    x = case(B, V, 1)
    got, _ = run(ops, x, 1, "product", ld)
    check(got, torch.log_softmax(x.double(), dim=-1), V)
    rows = torch.full((B, ld), PAD_FILL, dtype=torch.float32)
    rows[:, :V] = x
    rows = rows.to(DEV)
    ops.logits_process(rows, V, None, 0, to_logprobs=True)
    assert torch.equal(got[:, :V], rows[:, :V].cpu())


@pytest.mark.parametrize("B,V,ld", [(2, 1000, 1001), (2, 32128, 32192)])
def test_minus_infinity_in_one_member_and_in_all(ops, B, V, ld):
    n = 3
    x = case(B, V, n).clone()
    one, every = [5, 6, 7, 8, V - 1], [0, 13, 14, 15, 16, V - 2]          # whole 4-column groups and single columns
    x[1::n, one] = NEG_INF
    x[:, every] = NEG_INF
    prod, _ = run(ops, x, n, "product", ld)
    mix, _ = run(ops, x, n, "mixture", ld)
    assert (prod[:, one] == NEG_INF).all() and torch.isfinite(mix[:, one]).all()
    assert (prod[:, every] == NEG_INF).all() and (mix[:, every] == NEG_INF).all()
    check(prod, ref.combine(x, n, "product"), V)
    check(mix, ref.combine(x, n, "mixture"), V)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hot", [0, 1, 2])
def test_one_hot_weights_give_that_members_log_softmax(ops, mode, hot):
    """The zero-weight members hold -inf everywhere and logits of +-1e4: none of it may reach the result."""
    B, V, n = 2, 1000, 3
    x = case(B, V, n).clone()
    others = [i for i in range(n) if i != hot]
    x[others[0]::n] = NEG_INF
    x[others[1]::n] = 1e4 * torch.sign(x[others[1]::n])
    w = [0.0] * n
    w[hot] = 2.5                                               # normalised to 1 on the host
    got, _ = run(ops, x, n, mode, 1001, weights=w)
    check(got, torch.log_softmax(x[hot::n].double(), dim=-1), V)


@pytest.mark.parametrize("mode", MODES)
def test_logits_of_magnitude_1e4_do_not_overflow(ops, mode):
    B, V, n = 2, 32128, 3
    x = case(B, V, n) * 2500.0
    assert x.abs().max().item() > 1e4
    got, lse = run(ops, x, n, mode, 32192, lse=True)
    assert torch.isfinite(lse).all()
    check(got, ref.combine(x, n, mode), V)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ld,ld_out", [(1000, 1003), (1001, 1004), (1024, 1000), (1004, 1024)])
def test_out_may_have_another_leading_dimension(ops, mode, ld, ld_out):
    """Vector loads with scalar stores, and the other way round."""
    B, V, n = 2, 1000, 2
    got, _ = run(ops, case(B, V, n), n, mode, ld, ld_out)
    assert got.shape == (B, ld_out)
    check(got, wanted(B, V, n, mode), V)


def test_weights_enter_as_given(ops):
    B, V, n = 3, 64, 3
    for mode in MODES:
        got, _ = run(ops, case(B, V, n), n, mode, weights=[1.0, 2.0, 5.0])
        check(got, ref.combine(case(B, V, n), n, mode, [1.0, 2.0, 5.0]), V)


def test_bad_calls_are_rejected_without_a_launch(ops):
    from eavqa_amd import _lib
    x = torch.zeros((9, 64), dtype=torch.float32, device=DEV)
    out = torch.full((1, 64), SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.EavqaError, match="code -1"):      # n = 9
        ops.ensemble_combine(x, 64, 9, "product", out=out)
    with pytest.raises(_lib.EavqaError, match="code -1"):      # out == logits
        ops.ensemble_combine(x, 64, 1, "product", out=x)
    with pytest.raises(_lib.EavqaError):                       # ld < V
        ops.ensemble_combine(x, 65, 3, "product")
    stats = torch.empty(18, dtype=torch.float32, device=DEV)
    assert _lib.load().eavqa_ensemble_combine(3, 3, 65, x.data_ptr(), 64, 0, None, out.data_ptr(), 65, stats.data_ptr(), None, None) == -1
    with pytest.raises(ValueError):
        ops.ensemble_combine(x, 64, 3, "average")
    with pytest.raises(_lib.EavqaError):
        ops.ensemble_combine(x.cpu(), 64, 3, "product")
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
