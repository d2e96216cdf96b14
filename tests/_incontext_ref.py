"""Reference for training on interleaved image-text rows: a numpy restatement of the label layout (``ops.build_fewshot_labels``)
and of ``interleave_plan``, the episode inputs the tests share, and the loss / logits / mapper gradients composed from the CPU oracle
(oracle/ref_cpu.py) with autograd:

  causal:  mlp_mapper / mapper_project -> insert_prefix_into_input -> lm_logits -> causal_lm_loss
  T5:      mapper -> insert_prefix_into_input -> t5_encoder(mask) -> t5_decoder(enc_mask) -> t5_lm_logits -> CE

The label layout equals ``insert_prefix_into_input`` applied to the labels as 1-wide "embeddings" with a -100 "prefix"
(:func:`expand_labels_by_oracle`); tests/test_incontext_cpu.py holds the two to each other."""
import numpy as np
import torch

import oracle


def is_sentinel(tokens, n_img, special):
    tokens = np.asarray(tokens)
    return (tokens <= special) & (tokens > special - n_img)


def expand_labels(tokens, labels, L, n_img, special):
    """-> (labels_out int64 [B, T + (L-1)*n_img], scored int32 [B]): the walk of ``fewshot_rows_kernel``.  A row with too few sentinels
    keeps a -100 tail; text behind a surplus sentinel that would leave the row is dropped."""
    tokens, labels = np.asarray(tokens), np.asarray(labels)
    B, T = tokens.shape
    T_out = T + (L - 1) * n_img
    out = np.full((B, T_out), -100, dtype=np.int64)
    scored = np.zeros(B, dtype=np.int32)
    sent = is_sentinel(tokens, n_img, special)
    for b in range(B):
        before = 0
        for t in range(T):
            if sent[b, t]:
                before += 1
                continue
            o = t + before * (L - 1)
            if o < T_out and labels[b, t] != -100:
                out[b, o] = labels[b, t]
                scored[b] += 1
    return out, scored


def expand_labels_by_oracle(tokens, labels, L, n_img, special):
    """The same layout from the oracle's ``insert_prefix_into_input``: labels as 1-wide embeddings, a -100 prefix."""
    tokens, labels = torch.as_tensor(tokens), torch.as_tensor(labels)
    B = tokens.shape[0]
    emb, _ = oracle.insert_prefix_into_input(L, n_img - 1, tokens, labels[..., None].double(), torch.full((B, n_img, L, 1), -100.0, dtype=torch.float64),
                                             torch.ones_like(tokens), special_token_id=special)
    return emb[..., 0].long().numpy()


def expanded_mask(tokens, mask, L, n_img, special):
    """The attention mask of the expanded rows (bool [B, T + (L-1)*n_img]) from the oracle's ``insert_prefix_into_input``."""
    tokens = torch.as_tensor(tokens)
    B, T = tokens.shape
    _, am = oracle.insert_prefix_into_input(L, n_img - 1, tokens, torch.zeros(B, T, 1), torch.zeros(B, n_img, L, 1), torch.as_tensor(mask),
                                            special_token_id=special)
    return am != 0


def plan(tokens, mask, labels, L, n_img, special):
    """-> (lengths [B], label count, T_out) as ``interleave_plan`` returns them for host tensors."""
    tokens = np.asarray(tokens)
    sent = is_sentinel(tokens, n_img, special)
    mask = np.ones_like(tokens) if mask is None else np.asarray(mask)
    lengths = [int(((mask[b] != 0) & ~sent[b]).sum()) + L * n_img for b in range(tokens.shape[0])]
    count = None if labels is None else int(((np.asarray(labels) != -100) & ~sent).sum())
    return lengths, count, tokens.shape[1] + (L - 1) * n_img


def episode(V, special, B=3, n_img=3, seg=4, seed=9):
    """The episode inputs of the fixture tests/golden/incontext.npz (its generator draws them the same way): ``n_img`` images per row,
    sentinel positions that differ between rows, right padding on row 1 -> (tokens, mask, labels_last, labels_all).
    ``labels_last``: the tokens behind the last sentinel; ``labels_all``: the last two tokens of every segment (the "answers")."""
    g = torch.Generator().manual_seed(seed)
    T = n_img * (1 + seg) + 2
    tok = torch.randint(3, special - n_img - 1, (B, T), generator=g)
    sent_pos = [[i * (1 + seg) + (b % 2) for i in range(n_img)] for b in range(B)]
    for b in range(B):
        for i, p in enumerate(sent_pos[b]):
            tok[b, p] = special - i
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, -2:] = 0
    last = torch.full((B, T), -100, dtype=torch.long)
    every = torch.full((B, T), -100, dtype=torch.long)
    for b in range(B):
        p = sent_pos[b]
        last[b, p[-1] + 1:] = tok[b, p[-1] + 1:]
        for i in range(n_img):
            end = p[i + 1] if i + 1 < n_img else T
            every[b, end - 2:end] = tok[b, end - 2:end]
    last[mask == 0] = -100
    every[mask == 0] = -100
    return tok, mask, last, every


def long_episode(V, special, L=3, n_img=3, T=70, attended=(76, 40, 9), seed=21):
    """B = 3 rows of T = 70 tokens, T' = 76 with L = 3: sentinels at the row's start, around the 64-token pass and at its end, right
    padding so that the rows attend ``attended`` expanded positions; labels on the last attended text tokens of every row."""
    g = torch.Generator().manual_seed(seed)
    B = len(attended)
    tok = torch.randint(3, special - n_img - 1, (B, T), generator=g)
    sent_pos = [[0, 63, 64], [1, 20, 30], [0, 1, 2]]
    mask = torch.zeros(B, T, dtype=torch.long)
    labels = torch.full((B, T), -100, dtype=torch.long)
    for b in range(B):
        for i, p in enumerate(sent_pos[b]):
            tok[b, p] = special - i
        n_text = attended[b] - L * n_img                      # attended text tokens; sentinels count as attended columns of the mask too
        seen = 0
        for t in range(T):
            if t in sent_pos[b]:
                mask[b, t] = 1
            elif seen < n_text:
                mask[b, t] = 1
                seen += 1
        assert seen == n_text, (b, seen, n_text)
        text = [t for t in range(T) if mask[b, t] and t not in sent_pos[b]]
        for t in text[-min(4, len(text)):]:
            labels[b, t] = tok[b, t]
    return tok, mask, labels


def _sub(z, prefix):
    return {k[len(prefix):]: torch.from_numpy(np.asarray(v)) for k, v in z.items() if k.startswith(prefix)}


def causal_pieces(z, arch, mapping_type="mlp"):
    """(LM state dict, oracle cfg, mapper state dict, mapper cfg) of a clipcap_*.npz fixture."""
    c = [int(v) for v in z["cfg"]]
    mcfg = dict(prefix_length=c[5], mapping_type=mapping_type)
    if arch == "gpt2":
        mcfg.update(clip_length=c[7], num_layers=c[8])
    return _sub(z, "lm."), dict(arch=arch, n_layer=c[2], n_head=c[3]), _sub(z, "map."), mcfg


def t5_pieces(z):
    """The same of vct0_t0.npz."""
    V, E, DKV, H, F, NL, L, D, gated, tied = [int(v) for v in z["cfg"]]
    return _sub(z, "lm."), dict(n_layer=NL, n_head=H, d_kv=DKV, gated=bool(gated), tied=bool(tied)), _sub(z, "map."), dict(prefix_length=L, mapping_type="mlp")


def fixture_cases(f, family):
    """[(case name, tokens, mask, prefix, labels, special)] of tests/golden/incontext.npz for "gpt2" / "opt" / "t0"."""
    names = ("short", "ragged") if family == "t0" else ("last", "all")
    A = lambda k: torch.from_numpy(np.asarray(f[f"{family}.{k}"]))
    return [(n, A("tokens"), A("mask"), A("prefix"), A(f"{n}.labels"), int(f[f"{family}.special"])) for n in names]


def _leaf(params, dtype):
    return {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}


def _project(prefix, mapper, mcfg, E, n_img):
    B = prefix.shape[0]
    L = mcfg["prefix_length"]
    flat = prefix.reshape(B * n_img, -1).to(next(iter(mapper.values())).dtype)
    pp = oracle.mapper_project(flat, mapper, mcfg.get("mapping_type", "mlp"), L, E, mcfg.get("clip_length"), mcfg.get("num_layers", 8))
    return pp.reshape(B, n_img, L, E)


def causal_oracle(sd, cfg, mapper, mcfg, tokens, prefix, mask, labels, n_img, special, dtype=torch.float64):
    """-> (loss, logits [B, T', V], {mapper parameter: gradient}, expanded labels), computed in ``dtype``: float64 as the reference of the
    GPU tests; float32 against the fixture, whose producer (HF) ran in float32 - only the order of operations differs then."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    mapper = _leaf(mapper, dtype)
    wte = sd["transformer.wte.weight"] if cfg["arch"] == "gpt2" else sd["model.decoder.embed_tokens.weight"]
    L = mcfg["prefix_length"]
    pp = _project(prefix, mapper, mcfg, wte.shape[1], n_img)
    emb, am = oracle.insert_prefix_into_input(L, n_img - 1, tokens, wte[tokens], pp, mask, special_token_id=special)
    logits = oracle.lm_logits(sd, cfg, emb, am.to(dtype))
    full = torch.from_numpy(expand_labels(tokens.numpy(), labels.numpy(), L, n_img, special)[0])
    loss = oracle.causal_lm_loss(logits, full)
    loss.backward()
    return loss.detach(), logits.detach(), {k: v.grad for k, v in mapper.items()}, full


def t5_oracle(sd, cfg, mapper, mcfg, tokens, prefix, mask, labels, n_img, special, dtype=torch.float64):
    """-> (loss, logits [B, Td, V], {mapper parameter: gradient}) in ``dtype`` (see :func:`causal_oracle`): ``labels`` are the decoder targets."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    mapper = _leaf(mapper, dtype)
    shared = sd["shared.weight"]
    L = mcfg["prefix_length"]
    pp = _project(prefix, mapper, mcfg, shared.shape[1], n_img)
    emb, am = oracle.insert_prefix_into_input(L, n_img - 1, tokens, shared[tokens], pp, mask, special_token_id=special)
    enc = oracle.t5_encoder(sd, cfg, emb, am)
    dec_in = shared[oracle.t5_shift_right(labels, cfg.get("decoder_start_token_id", 0), cfg.get("pad_token_id", 0))]
    logits = oracle.t5_lm_logits(sd, cfg, oracle.t5_decoder(sd, cfg, dec_in, enc, am))
    loss = torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1), ignore_index=-100)
    loss.backward()
    return loss.detach(), logits.detach(), {k: v.grad for k, v in mapper.items()}
