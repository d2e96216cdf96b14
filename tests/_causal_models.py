"""The tiny GPT-2 / OPT prefix LMs of clipcap_gpt2_mlp.npz / clipcap_opt_mlp.npz on the GPU, and the few-shot inputs the causal tests
share (as tests/test_score_causal_gpu.py builds them)."""
import functools

import torch

from conftest import load_golden

DEV = "cuda"
ARCHS = {"gpt2": "clipcap_gpt2_mlp.npz", "opt": "clipcap_opt_mlp.npz"}
T = torch.from_numpy


@functools.lru_cache(maxsize=None)
def model(arch, dtype):
    """(fixture arrays, ClipCaptionPrefix on the GPU) - one instance per (arch, dtype) for the whole session."""
    from eavqa_amd.models.clipcap import ClipCaptionPrefix
    from eavqa_amd.models.lm import FrozenCausalLM, LMConfig
    z = load_golden(ARCHS[arch])
    sub = lambda p: {k[len(p):]: T(v) for k, v in z.items() if k.startswith(p)}
    if arch == "gpt2":
        V, E, NLAY, NH, NPOS, L, D, CL, NL = [int(v) for v in z["cfg"]]
        cfg = LMConfig("gpt2", NLAY, NH, E, 4 * E, V, NPOS, 1e-5, "gelu_new", V - 1, None)
    else:
        V, E, NLAY, NH, NPOS, L, D, FFN = [int(v) for v in z["cfg"]]
        cfg = LMConfig("opt", NLAY, NH, E, FFN, V, NPOS, 1e-5, "relu", 2, 1)
    lm = FrozenCausalLM(cfg, sub("lm."), dtype, DEV)
    m = ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", lm=lm, dtype=dtype, device=DEV).eval()
    m.clip_project.load_state_dict(sub("map."), strict=True)
    return z, m


def drawn_inputs(z, B, seed, T_q=6):
    """(tokens [B, T_q], mask with right padding on every third row, prefix [B, D]) drawn by seed."""
    V, D = int(z["cfg"][0]), int(z["cfg"][6])
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(3, V - 8, (B, T_q), generator=g)
    mask = torch.ones(B, T_q, dtype=torch.long)
    mask[1::3, T_q - 2:] = 0
    return tok, mask, 3.0 * torch.randn(B, D, generator=g)


def fewshot_inputs(z, seed=9):
    """Three images per row, sentinel positions that differ between rows, right padding on one row."""
    V, D = int(z["cfg"][0]), int(z["cfg"][6])
    g = torch.Generator().manual_seed(seed)
    B, n_img, seg = 3, 3, 4
    special = V - 5
    width = n_img * (1 + seg) + 2
    tok = torch.randint(3, special - n_img - 1, (B, width), generator=g)
    for b in range(B):
        for i in range(n_img):
            tok[b, i * (1 + seg) + (b % 2)] = special - i
    mask = torch.ones(B, width, dtype=torch.long)
    mask[1, -2:] = 0
    return tok, mask, torch.randn(B, n_img, D, generator=g), n_img, special
