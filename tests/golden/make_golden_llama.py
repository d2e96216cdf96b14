#!/usr/bin/env python3
"""Generate tests/golden/clipcap_llama_mlp.npz by RUNNING THE REFERENCE on a tiny HF ``LlamaForCausalLM``.

Run where make_golden.py runs (it needs the reference checkout that file imports from, and transformers):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_llama.py

Written as the OPT section of make_golden.py is: the reference hard-wires GPT-2, so its ``ClipCaptionPrefix`` is built on
the tiny GPT-2, ``model.gpt`` is swapped for the Llama model and ``.transformer.wte`` aliased to its ``embed_tokens``; the reference's own
``forward`` (concat, labels, loss) and ``generate`` (greedy loop over the growing sequence) then run unchanged.  Nothing from the
reference is copied: the file holds inputs, seeded random-init weights and the reference's outputs, under the keys of
clipcap_opt_mlp.npz.  V, E, the layer count and the FFN width are the OPT fixture's, so every GEMM shape is one the suite already runs;
4 heads over 2 key / value heads.

"Generated ids exact" must not hinge on a tie: every generated step's top-2 logit margin has to be >= 1e-3 in every row, otherwise the
LM is re-drawn from the next seed.  The archive is written with fixed zip timestamps, so a re-run reproduces the file byte for byte.
"""
import importlib.util
import io
import os
import sys
import tempfile
import types
import zipfile

sys.dont_write_bytecode = True
os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "clipcap_llama_mlp.npz"
MIN_MARGIN = 1e-3
NKV, NPOS, EPS, THETA = 2, 64, 1e-5, 10000.0


def _base():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def save_deterministic(path, arrays):
    """numpy's .npz layout (one .npy per key, deflated) with a constant timestamp in every zip entry."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    base = _base()
    clipcap, _ = base._import_reference()
    from transformers import GPT2Config, GPT2LMHeadModel, LlamaConfig, LlamaForCausalLM

    with np.load(os.path.join(HERE, "clipcap_opt_mlp.npz")) as z:
        V, E, NLAY, NH, _, L, D, FFN = [int(v) for v in z["cfg"]]
    tmp = tempfile.mkdtemp(prefix="eavqa_golden_llama_")
    # the tiny GPT-2 the reference class is constructed on (its LM is replaced below; E equal, so the MLP mapper has the same shapes)
    torch.manual_seed(2021)
    gcfg = GPT2Config(vocab_size=V, n_embd=E, n_layer=1, n_head=NH, n_positions=NPOS, bos_token_id=V - 1, eos_token_id=V - 1,
                      attn_implementation="eager", resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0)
    d_gpt2 = os.path.join(tmp, "gpt2")
    GPT2LMHeadModel(gcfg).save_pretrained(d_gpt2)

    pad_id = 0
    for seed in range(17, 117):
        gen = torch.Generator().manual_seed(seed)
        torch.manual_seed(seed)
        lcfg = LlamaConfig(vocab_size=V, hidden_size=E, intermediate_size=FFN, num_hidden_layers=NLAY, num_attention_heads=NH,
                           num_key_value_heads=NKV, max_position_embeddings=NPOS, rms_norm_eps=EPS, rope_theta=THETA,
                           tie_word_embeddings=False, attention_bias=False, mlp_bias=False, attn_implementation="eager",
                           pad_token_id=pad_id, bos_token_id=1, eos_token_id=2)
        llama = LlamaForCausalLM(lcfg).eval()
        torch.manual_seed(seed + 1000)
        model = clipcap.ClipCaptionPrefix(prefix_length=L, prefix_size=D, mapping_type="mlp", model_version=d_gpt2)
        llama.transformer = types.SimpleNamespace(wte=llama.model.embed_tokens)
        model.gpt = llama
        model.train()
        B, T = 4, 9
        ids, mask = base.ragged_batch(gen, B, T, V, pad_id, 3)
        ids = ids.clamp(min=3)
        ids = ids * mask + pad_id * (1 - mask)
        labels = ids.clone()
        labels[mask == 0] = -100
        prefix = torch.randn(B, D, generator=gen)
        out = model(question_tokens=ids, prefix=prefix, question_mask=mask, labels=labels, pad_token_id=pad_id)
        out.loss.backward()
        grads = {"g." + n: p.grad.numpy() for n, p in model.clip_project.named_parameters()}
        model.eval()
        gids, gmask = base.ragged_batch(gen, B, 6, V, pad_id, 2)
        gids = (gids.clamp(min=3)) * gmask + pad_id * (1 - gmask)
        margins = []

        def watch(_module, _args, output):
            top = output.logits[:, -1, :].float().topk(2, dim=-1).values
            margins.append((top[:, 0] - top[:, 1]).min().item())

        hook = llama.register_forward_hook(watch)
        with torch.no_grad():
            free = model.generate(question_tokens=gids, prefix=prefix, question_mask=gmask, max_length=5, pad_token_id=pad_id,
                                  eos_token_id=None)
            forced_eos = int(free[2][1])
            forced = model.generate(question_tokens=gids, prefix=prefix, question_mask=gmask, max_length=5, pad_token_id=pad_id,
                                    eos_token_id=forced_eos)
        hook.remove()
        if min(margins) >= MIN_MARGIN:
            break
        print(f"seed {seed}: smallest top-2 margin {min(margins):.2e} < {MIN_MARGIN}: next seed")
    else:
        raise RuntimeError("no seed gave tie-free generation")
    assert len(margins) >= 6 and min(margins) >= MIN_MARGIN
    arrays = dict(cfg=np.array([V, E, NLAY, NH, NPOS, L, D, FFN, NKV]), rms_norm_eps=np.array(EPS), rope_theta=np.array(THETA),
                  seed=np.array(seed), min_margin=np.array(min(margins)),
                  ids=ids.numpy(), mask=mask.numpy(), labels=labels.numpy(), prefix=prefix.numpy(), pad_id=np.array(pad_id),
                  loss=out.loss.detach().numpy(), logits=out.logits.detach().numpy(),
                  gen_ids=gids.numpy(), gen_mask=gmask.numpy(), gen_free=np.array(free), gen_forced=np.array(forced),
                  gen_forced_eos=np.array(forced_eos),
                  **base._np(llama.state_dict(), "lm."), **base._np(model.clip_project.state_dict(), "map."), **grads)
    path = os.path.join(HERE, NAME)
    save_deterministic(path, arrays)
    print(f"wrote {NAME}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays, seed {seed}, smallest top-2 margin {min(margins):.3e}")


if __name__ == "__main__":
    main()
