"""Generates tests/golden/clip_text.npz: ``text_embeds`` of HF ``CLIPTextModelWithProjection`` (transformers 5.15, CPU, float32, seeded
random weights) on a tiny text tower, for tests/test_clip_text_gpu.py and tests/test_clip_text_ref_cpu.py.  Run where transformers is
installed:

    python tests/golden/make_golden_clip_text.py

Config: vocabulary 256, width 64, one head of 64, 2 layers, MLP 256, projection 64, context 77, QuickGELU, ``eos_token_id = vocab - 1``
(so HF pools at the first EOT, which is also the arg-max of the ids: OpenAI CLIP's rule) and NO ``attention_mask`` (OpenAI applies the
causal mask only).  Rows ``<BOS> tokens <EOT> 0 ...`` with the EOT at index 1 (the empty string), 7, 12, 63, 64 and 76, plus a copy of the
index-12 row whose positions behind the EOT hold random non-zero ids smaller than EOT: under the causal mask it has the same embedding.
The file holds data only: ``cfg``, the weights under ``w.<HF key>``, ``ids`` and ``text_embeds``.
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
VOCAB, WIDTH, HEADS, LAYERS, MLP, PROJ, CTX = 256, 64, 1, 2, 256, 64, 77
EOT_AT = (1, 7, 12, 63, 64, 76)


def main():
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    torch.manual_seed(2021)
    cfg = CLIPTextConfig(vocab_size=VOCAB, hidden_size=WIDTH, intermediate_size=MLP, projection_dim=PROJ, num_hidden_layers=LAYERS,
                         num_attention_heads=HEADS, max_position_embeddings=CTX, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                         bos_token_id=VOCAB - 2, eos_token_id=VOCAB - 1, pad_token_id=0)
    model = CLIPTextModelWithProjection(cfg).eval().float()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():                                   # HF's init leaves biases 0 and LayerNorm 1 / 0: make every term count
        for name, prm in model.named_parameters():
            if name.endswith("bias"):
                prm.copy_(0.05 * torch.randn(prm.shape, generator=g))
            elif "layer_norm" in name:
                prm.copy_(1.0 + 0.1 * torch.randn(prm.shape, generator=g))
            else:
                prm.copy_(prm + 0.05 * torch.randn(prm.shape, generator=g))
    bos, eot = VOCAB - 2, VOCAB - 1
    ids = torch.zeros((len(EOT_AT) + 1, CTX), dtype=torch.int64)
    for r, e in enumerate(EOT_AT):
        ids[r, 0] = bos
        ids[r, 1:e] = torch.randint(1, bos, (e - 1,), generator=g)
        ids[r, e] = eot
    ids[-1] = ids[EOT_AT.index(12)]
    ids[-1, 13:] = torch.randint(1, eot, (CTX - 13,), generator=g)
    with torch.no_grad():
        emb = model(input_ids=ids).text_embeds
    assert torch.equal(ids.argmax(dim=1), torch.tensor(list(EOT_AT) + [12]))
    assert (emb[-1] - emb[EOT_AT.index(12)]).abs().max().item() < 1e-5
    out = {"cfg": np.array([VOCAB, WIDTH, HEADS, LAYERS, MLP, PROJ, CTX], dtype=np.int64), "ids": ids.numpy(),
           "text_embeds": emb.numpy().astype(np.float32)}
    for k, v in model.state_dict().items():
        if v.dtype.is_floating_point:
            out["w." + k] = v.numpy().astype(np.float32)
    np.savez(os.path.join(HERE, "clip_text.npz"), **out)
    print({k: v.shape for k, v in out.items() if not k.startswith("w.")}, os.path.getsize(os.path.join(HERE, "clip_text.npz")))


if __name__ == "__main__":
    main()
