"""Generates tests/golden/incontext.npz: the training step on interleaved image-text rows, computed by the REFERENCE's code and HF.

Run in the build container only (needs /root/reference and transformers):

    python tests/golden/make_golden_incontext.py

What it executes: the reference's ``MLP`` mapper (src/models/clipcap.py) on every image, the reference's own
``VCT0Model.insert_prefix_into_input`` (src/models/vct0.py:494-533) on the token embeddings and the mapper's output, and HF
``lm(inputs_embeds=joint_embeddings, attention_mask=joint_attention_masks, labels=labels)`` - the generate branch's call of
``insert_prefix_into_input`` (:446-456) composed with the training call (:390-393) - on the tiny GPT-2 / OPT / T0-style T5 whose weights
tests/golden/clipcap_gpt2_mlp.npz, clipcap_opt_mlp.npz and vct0_t0.npz already hold (they are read from there, not stored again).  For
the causal LMs the labels go through the same ``insert_prefix_into_input`` as 1-wide "embeddings" with a -100 "prefix", which is the
layout ``ops.build_fewshot_labels`` builds; for T5 the labels are the decoder targets.

Cases per model: 3 images per row, sentinel positions that differ between rows, right padding on row 1; the causal LMs with labels on
the last segment only (``last``) and on the two closing tokens of every segment (``all``), T5 with two sets of decoder targets.
Inputs are drawn as tests/_incontext_ref.py ``episode`` draws them.  The file holds data only: inputs, loss, logits, mapper gradients
and (causal) the expanded labels."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from make_golden import _import_reference  # noqa: E402

N_IMG = 3


def ref_insert(vct0, L, E, toks, text, pp, masks, special):
    self_ = types.SimpleNamespace(prefix_length=L, lm_embedding_size=E)
    return vct0.VCT0Model.insert_prefix_into_input(self_, toks.shape[0], N_IMG - 1, toks, text, pp, masks, special_token_id=special)


def load_mapper(clipcap, z, D, E, L):
    mlp = clipcap.MLP((D, (E * L) // 2, E * L))
    mlp.load_state_dict({k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("map.")}, strict=True)
    return mlp


def step(mlp, lm, call):
    mlp.zero_grad(set_to_none=True)
    out = call()
    out.loss.backward()
    return out.loss.detach().numpy(), out.logits.detach().numpy(), {n: p.grad.numpy().copy() for n, p in mlp.named_parameters()}


def causal(clipcap, vct0, arch, out):
    from make_golden_causal_beam import build
    from _incontext_ref import episode
    lm, _, V, L, D, pad, z = build(arch)
    E = lm.get_input_embeddings().weight.shape[1]
    for p in lm.parameters():
        p.requires_grad_(False)
    mlp = load_mapper(clipcap, z, D, E, L)
    special = V - 5
    tok, mask, last, every = episode(V, special, n_img=N_IMG)
    B = tok.shape[0]
    prefix = torch.randn(B, N_IMG, D, generator=torch.Generator().manual_seed(5))
    out.update({f"{arch}.tokens": tok.numpy(), f"{arch}.mask": mask.numpy(), f"{arch}.prefix": prefix.numpy(),
                f"{arch}.special": np.array(special), f"{arch}.L": np.array(L)})
    for name, labels in (("last", last), ("all", every)):
        full, _ = ref_insert(vct0, L, 1, tok, labels[..., None].float(), torch.full((B, N_IMG, L, 1), -100.0), mask, special)
        full = full[..., 0].long()

        def call():
            pp = mlp(prefix).view(B, -1, L, E)
            emb, am = ref_insert(vct0, L, E, tok, lm.get_input_embeddings()(tok), pp, mask, special)
            return lm(inputs_embeds=emb, attention_mask=am, labels=full)

        loss, logits, grads = step(mlp, lm, call)
        print(f"{arch:5s} {name:5s} loss {float(loss):.6f} logits {logits.shape} labels scored {(full != -100).sum().item()}")
        out.update({f"{arch}.{name}.labels": labels.numpy(), f"{arch}.{name}.labels_out": full.numpy(), f"{arch}.{name}.loss": loss})
        out.update({f"{arch}.{name}.gmap.{n}": g for n, g in grads.items()})
        out[f"{arch}.logits"] = logits                                       # the same for both label sets


def t5(clipcap, vct0, out):
    from transformers import T5Config, T5ForConditionalGeneration
    from _incontext_ref import episode
    z = np.load(os.path.join(HERE, "vct0_t0.npz"))
    V, E, DKV, H, F, NL, L, D, gated, tied = [int(v) for v in z["cfg"]]
    cfg = T5Config(vocab_size=V, d_model=E, d_kv=DKV, num_heads=H, d_ff=F, num_layers=NL, num_decoder_layers=NL, dropout_rate=0.0,
                   feed_forward_proj="gated-gelu" if gated else "relu", tie_word_embeddings=bool(tied), decoder_start_token_id=0, pad_token_id=0,
                   eos_token_id=1, relative_attention_num_buckets=32, relative_attention_max_distance=128)
    cfg._attn_implementation = "eager"
    lm = T5ForConditionalGeneration(cfg).eval()
    missing, unexpected = lm.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("lm.")}, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    for p in lm.parameters():
        p.requires_grad_(False)
    mlp = load_mapper(clipcap, z, D, E, L)
    special = V - 1
    tok, mask, _, _ = episode(V, special, n_img=N_IMG)
    B = tok.shape[0]
    g = torch.Generator().manual_seed(6)
    prefix = torch.randn(B, N_IMG, D, generator=g)
    short = torch.randint(2, V - 8, (B, 3), generator=g)
    short[:, -1] = 1                                                         # answer, eos
    ragged = torch.randint(2, V - 8, (B, 7), generator=g)
    ragged[1, 5:] = -100
    ragged[2, 3:] = -100
    out.update({"t0.tokens": tok.numpy(), "t0.mask": mask.numpy(), "t0.prefix": prefix.numpy(), "t0.special": np.array(special),
                "t0.L": np.array(L)})
    for name, labels in (("short", short), ("ragged", ragged)):
        def call():
            pp = mlp(prefix).view(B, -1, L, E)
            emb, am = ref_insert(vct0, L, E, tok, lm.shared(tok), pp, mask, special)
            return lm(inputs_embeds=emb, attention_mask=am, labels=labels)

        loss, logits, grads = step(mlp, lm, call)
        print(f"t0    {name:6s} loss {float(loss):.6f} logits {logits.shape}")
        out.update({f"t0.{name}.labels": labels.numpy(), f"t0.{name}.loss": loss, f"t0.{name}.logits": logits})
        out.update({f"t0.{name}.gmap.{n}": g_ for n, g_ in grads.items()})


def main():
    clipcap, vct0 = _import_reference()
    out = {}
    for arch in ("gpt2", "opt"):
        causal(clipcap, vct0, arch, out)
    t5(clipcap, vct0, out)
    path = os.path.join(HERE, "incontext.npz")
    np.savez_compressed(path, **out)
    print(f"wrote incontext.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
