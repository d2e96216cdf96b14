"""CPU: the host side of gradient-norm clipping - the config key ``train.additional.gradient_clipping`` reaches ``FusedAdamW`` through the
executor, what is not built is refused by name, bad values are rejected, and the device table of AdamW's bias corrections holds the very
floats ``eavqa_adamw`` computes on the host.  No kernel runs here: ``FusedAdamW(max_grad_norm=...)`` constructs on CPU tensors."""
import math
import struct
import types

import pytest
import torch


def f32(x):
    return struct.unpack("f", struct.pack("f", float(x)))[0]


@pytest.fixture(scope="module", autouse=True)
def lib():
    from eavqa_amd import build, _lib
    build.build()
    return _lib.load()


def cpu_flat():
    from eavqa_amd.models.clipcap import FlatParams
    return FlatParams([("model.0.weight", (6, 5)), ("model.0.bias", (6,))], "cpu", torch.float32)


def executor(additional, cls="ClipCapExecutor"):
    from eavqa_amd.trainers import clipcap_executor, vct0_executor
    from eavqa_amd.utils.attrdict import AttrDict
    cfg = AttrDict({"train": {"lr": 1e-3, "scheduler": "none", "epochs": 1, "additional": additional}})
    model = types.SimpleNamespace(clip_project=types.SimpleNamespace(flat=cpu_flat()))
    Executor = getattr(clipcap_executor, cls, None) or getattr(vct0_executor, cls)
    return Executor(cfg, None, model=model, dtype=torch.float32, device="cpu")


@pytest.mark.parametrize("cls", ["ClipCapExecutor", "VCT0Executor"])
@pytest.mark.parametrize("additional,want", [
    ({"warmup_steps": 0, "gradient_clipping": 0.5}, 0.5),
    ({"warmup_steps": 0, "gradient_clipping": 0}, None),
    ({"warmup_steps": 0}, None),
    ({"gradient_clipping": 2, "gradient_clip_algorithm": "norm"}, 2.0),
])
def test_the_config_key_reaches_the_optimiser(cls, additional, want):
    ex = executor(additional, cls)
    ex.configure_optimizers()
    assert ex.optimizer.max_grad_norm == want
    if want is not None:
        assert ex.optimizer.grad_norm.device.type == "cpu" and int(ex.optimizer.applied_steps) == 0 and int(ex.optimizer.skipped_steps) == 0


def test_clipping_by_value_is_refused_by_name():
    with pytest.raises(NotImplementedError, match="gradient_clip_algorithm"):
        executor({"gradient_clipping": 0.5, "gradient_clip_algorithm": "value"}).configure_optimizers()
    with pytest.raises(NotImplementedError, match="gradient_clip_algorithm"):
        executor({"gradient_clip_algorithm": "value"}).configure_optimizers()


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("-inf")])
def test_bad_max_grad_norm_raises(bad):
    from eavqa_amd.trainers.optim import FusedAdamW
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdamW(cpu_flat(), max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        executor({"gradient_clipping": bad}).configure_optimizers()


def test_off_and_measure_only_values():
    from eavqa_amd.trainers.optim import FusedAdamW
    assert FusedAdamW(cpu_flat()).max_grad_norm is None and FusedAdamW(cpu_flat(), max_grad_norm=0).max_grad_norm is None
    assert FusedAdamW(cpu_flat(), max_grad_norm=float("inf")).max_grad_norm == float("inf")
    with pytest.raises(AttributeError, match="max_grad_norm"):
        FusedAdamW(cpu_flat()).grad_norm


def test_the_sharded_optimiser_refuses_the_argument_before_anything_else():
    from eavqa_amd.trainers.optim import ShardedAdamW
    with pytest.raises(NotImplementedError, match="max_grad_norm"):
        ShardedAdamW(None, max_grad_norm=1.0)            # (no flat buffer is touched: the refusal comes first)


def test_state_dict_carries_the_applied_count_and_load_writes_it_back():
    from eavqa_amd.trainers.optim import FusedAdamW
    opt = FusedAdamW(cpu_flat(), max_grad_norm=1.0)
    opt._state[4], opt._state[5] = 7, 2
    sd = opt.state_dict()
    assert (sd["step"], sd["skipped_steps"]) == (7, 2)
    fresh = FusedAdamW(cpu_flat(), max_grad_norm=1.0)
    fresh.load_state_dict(sd)
    assert (int(fresh.applied_steps), int(fresh.skipped_steps)) == (7, 2)


def host_corrections(beta1, beta2, t):
    """(inv_bc1, inv_sqrt_bc2) as csrc/optim.hip computes them in eavqa_adamw: double arithmetic on the float32 betas."""
    b1, b2 = f32(beta1), f32(beta2)
    return f32(1.0 / (1.0 - math.pow(b1, t))), f32(1.0 / math.sqrt(1.0 - math.pow(b2, t)))


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.95)])
def test_bias_correction_table_holds_the_host_expressions(betas):
    """Early rows, two in the range where inv_bc1 of beta1 = 0.9 has just become 1.0f while inv_sqrt_bc2 is still far from it, and the
    last row: the first at which both corrections are 1.0f (the row before it is not), after which the host expressions stay 1.0f.
    Length for beta2 = 0.999: 1 / sqrt(1 - x) ~ 1 + x / 2 rounds to 1.0f once x / 2 < 2^-24, i.e. t > ln(2^-23) / ln(0.999f) = 15 934.6."""
    from eavqa_amd.trainers.optim import bias_correction_table
    table = bias_correction_table(*betas)
    assert table.dtype == torch.float32 and table.dim() == 2 and table.shape[1] == 2
    n = table.shape[0]
    for t in (1, 2, 165, 166, n):
        if t <= n:
            assert tuple(table[t - 1].tolist()) == host_corrections(*betas, t), t
    assert tuple(table[-1].tolist()) == (1.0, 1.0) and tuple(table[-2].tolist()) != (1.0, 1.0)
    assert host_corrections(*betas, n + 1) == (1.0, 1.0) and host_corrections(*betas, 100 * n) == (1.0, 1.0)
    if betas == (0.9, 0.999):
        assert n == 15935


def test_the_table_follows_the_betas():
    from eavqa_amd.trainers.optim import FusedAdamW, bias_correction_table
    opt = FusedAdamW(cpu_flat(), max_grad_norm=1.0)
    assert torch.equal(opt._bias_table(), bias_correction_table(0.9, 0.999))
    opt.param_groups[0]["betas"] = (0.8, 0.95)
    assert torch.equal(opt._bias_table(), bias_correction_table(0.8, 0.95))
    with pytest.raises(ValueError, match="betas"):
        bias_correction_table(1.0, 0.999)
