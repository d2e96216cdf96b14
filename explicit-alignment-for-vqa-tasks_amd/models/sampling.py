"""The sampling arguments of HF ``generate`` (``do_sample``, ``temperature``, ``top_k``, ``top_p``) plus ``seed``, checked on the host
once for the encoder-decoder (``VCT0Model.generate``) and the causal (``ClipCaptionModel.generate`` / ``generate_fewshot``) path.

The draw itself is ``eavqa_sample_pick`` (one kernel per step).  ``seed`` is an addition: the reference leaves seeding to torch's global
generator, which nothing here uses - the uniforms are Philox4x32-10 of (seed, decoder position, row)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

SAMPLING_KWARGS = ("do_sample", "temperature", "top_k", "top_p", "seed")
MAX_RETURN_SEQUENCES = 8          # the rows-per-item limit of eavqa_t5_decoder_step_beams


@dataclass(frozen=True)
class Sampler:
    """What ``eavqa_sample_pick`` needs besides the logits.  ``top_k`` 0 = off, ``top_p`` 1.0 = off; ``seed`` None = still to be drawn
    (:func:`next_seed`)."""
    temperature: float = 1.0
    top_k: int = 50
    top_p: float = 1.0
    seed: Optional[int] = None
    do_sample: bool = True

    def with_seed(self, seed: int) -> "Sampler":
        return Sampler(self.temperature, self.top_k, self.top_p, int(seed) & (2 ** 64 - 1), True)


def sampling_plan(kw: dict) -> Optional[Sampler]:
    """``kw``: generation arguments by name (missing or None = HF's default).  None when ``do_sample`` is off - then a warper argument is
    an error naming it: HF would ignore it with a warning, but a configuration that meant to sample must not silently run greedy."""
    if not kw.get("do_sample"):
        for name in ("temperature", "top_k", "top_p", "seed"):
            if kw.get(name) is not None:
                raise NotImplementedError(f"{name}={kw[name]!r} without do_sample=True: HF would ignore it with a warning; here a "
                                          f"configuration that meant to sample does not silently run greedy - pass do_sample=True or drop {name}")
        return None
    t = kw.get("temperature")
    t = 1.0 if t is None else float(t)
    if not (t > 0.0 and math.isfinite(t)):
        raise ValueError(f"temperature={t}: a finite value > 0 (HF raises likewise)")
    k = kw["top_k"] if "top_k" in kw else 50              # HF's default; None or 0 = no top-k filter
    k = 0 if k is None else int(k)
    if k < 0:
        raise ValueError(f"top_k={k}: a positive integer, or 0 / None for no top-k filter")
    p = kw.get("top_p")
    p = 1.0 if p is None else float(p)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"top_p={p}: in (0, 1]")
    seed = kw.get("seed")
    return Sampler(t, k, p, None if seed is None else int(seed) & (2 ** 64 - 1))


def resolve(owner, sampler: Optional[Sampler]) -> Optional[Sampler]:
    """The sampler with its seed drawn (:func:`next_seed` on ``owner``) when the call named none."""
    if sampler is None or sampler.seed is not None:
        return sampler
    return sampler.with_seed(next_seed(owner))


def causal_sampler(owner, kw: dict) -> Optional[Sampler]:
    """The sampling arguments of the causal path (``ClipCaptionModel``): the same names, defaults and checks as the encoder-decoder
    path; ``num_return_sequences`` > 1 is not built there (the prompt's K / V cache is per row)."""
    unknown = sorted(set(kw) - set(SAMPLING_KWARGS) - {"num_return_sequences"})
    if unknown:
        raise TypeError(f"unexpected generation arguments: {unknown}")
    if kw.get("num_return_sequences") not in (None, 1):
        raise NotImplementedError("num_return_sequences > 1 on the causal path is not built: the prompt K / V cache is per row there")
    return resolve(owner, sampling_plan(kw))


def check_return_sequences(nrs: int) -> int:
    if nrs < 1:
        raise ValueError(f"num_return_sequences={nrs} has to be >= 1")
    if nrs > MAX_RETURN_SEQUENCES:
        raise NotImplementedError(f"num_return_sequences={nrs}: 1..{MAX_RETURN_SEQUENCES} sampled sequences per item are built")
    return nrs


def next_seed(owner) -> int:
    """A 64-bit seed for a ``generate`` call that named none: ``torch.initial_seed()`` mixed with a per-model call counter, so that
    ``torch.manual_seed(s)`` followed by the same calls on a model gives the same draws.  The counter starts again when the global
    seed changes."""
    base = int(torch.initial_seed())
    seen, calls = getattr(owner, "_sample_seed_state", (None, 0))
    calls = calls + 1 if seen == base else 0
    owner._sample_seed_state = (base, calls)
    return (base * 0x9E3779B97F4A7C15 + calls) & (2 ** 64 - 1)
