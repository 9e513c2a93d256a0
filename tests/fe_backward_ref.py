"""Float64 references and case tables for the input-gradient chain below the encoder (``EmbedderGrad.backward`` from the
positional convolution down to the waveform; tests/test_fe_backward_ref_cpu.py, tests/test_gpu_fe_backward.py).

CPU, float64 and plain torch only: nothing here calls a kernel or a planner.

``dgrad_ref``        the operation ``embedder_grad.plan_conv1d_dgrad`` claims to be: ``F.conv_transpose1d`` on the operands as the
                     kernel reads them (fp16-rounded, or the plane pair ``hi + lo * 2**-11``).
``lower_chain_vjp``  ``hidden_states[0]`` of the oracle and the vector-Jacobian product ``d sum(h * S) / d wave`` by autograd.
``rows``             the row counts of ``HipEmbedder._workspace`` restated: the valid rows ``Ls`` of every feature-encoder level,
                     the padded rows ``P`` (``P[i] = P[i+1] * stride[i+1]``, every ``P[i] >= Ls[i] + 1``), the frames ``T``.
``LENGTHS``          the clip lengths of the suite, each with the claim it is in the table for (asserted, not commented:
                     tests/test_fe_backward_ref_cpu.py::test_length_table_claims).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from oracle import wav2vec2_ref
from oracle.signal_ref import zero_mean_unit_var_norm

WINDOW = 400                 # samples at each end of a clip the GPU suite checks on their own: the receptive field of one frame
# max |dx - ref| / max |ref| the GPU suite allows the chain below the encoder, per precision.  The ceilings are the whole chain's
# tolerances (tests/test_gpu_backward.py); TOL is four times the worst ratio measured over the table, windows included, rounded
# up to one significant digit and never above the ceiling (the measured values: docstring of tests/test_gpu_fe_backward.py).
CEILING = {"f32": 1e-4, "f16": 3e-2}
# f32: worst 2.096e-6 (layer_preln, L = 16000, tail window) -> 8.4e-6 -> 9e-6;  f16: worst 5.153e-3 (layer_preln, L = 645, head
# window) -> 2.06e-2 -> 3e-2, which is the ceiling
TOL = {"f32": 9e-6, "f16": 3e-2}


# ------------------------------------------------------------------------------------------------ operands as stored
def as_f16(x: torch.Tensor) -> torch.Tensor:
    """The fp64 value of ``x`` stored as fp16."""
    return x.to(torch.float16).to(torch.float64)


def split_pair(x: torch.Tensor) -> torch.Tensor:
    """``x`` as the split format stores it (csrc/device_math.h): fp16 ``[2, ...]`` with ``x ~ hi + lo * 2**-11``; ``hi`` is
    flushed to zero below 2**-14."""
    x64 = x.to(torch.float64)
    hi = x64.to(torch.float16)
    hi = torch.where(x64.abs() < 2.0 ** -14, torch.zeros_like(hi), hi)
    lo = ((x64 - hi.to(torch.float64)) * 2048.0).to(torch.float16)
    return torch.stack([hi, lo])


def join_pair(t: torch.Tensor) -> torch.Tensor:
    """The fp64 value of a plane pair ``[2, ...]``."""
    return t[0].to(torch.float64) + t[1].to(torch.float64) * 2.0 ** -11


def as_stored(x: torch.Tensor, split: bool) -> torch.Tensor:
    return join_pair(split_pair(x)) if split else as_f16(x)


# ------------------------------------------------------------------------------------------------ the transposed convolution
def dgrad_ref(dz: torch.Tensor, w: torch.Tensor, s: int, split: bool = False) -> torch.Tensor:
    """Input gradient of the channels-last ``Conv1d(Cin, Cout, k, stride=s)`` (no padding) with weight ``w [Cout, Cin, k]`` at the
    output gradient ``dz [B, L_out, Cout]``: ``[B, s * (L_out - 1) + k, Cin]`` float64, both operands rounded to the format the
    kernel reads (``split``: plane pairs)."""
    x = as_stored(dz, split).transpose(1, 2)                          # [B, Cout, L_out]
    return F.conv_transpose1d(x, as_stored(w, split), stride=s).transpose(1, 2)


# ------------------------------------------------------------------------------------------------ the chain below the encoder
def lower_chain_vjp(cfg, sd: Dict[str, torch.Tensor], waves: torch.Tensor, S: torch.Tensor,
                    dtype: torch.dtype = torch.float64) -> Tuple[torch.Tensor, torch.Tensor]:
    """``h = hidden_states[0]`` of the oracle on the normalised clips ``waves [B, L]`` and ``d sum(h * S) / d waves`` by autograd,
    every tensor in ``dtype``: ``(h [B, T, H], dx [B, L])``."""
    sdd = {k: v.detach().to(dtype) for k, v in sd.items()}
    with torch.enable_grad():
        x = waves.detach().to(dtype).requires_grad_(True)
        h = wav2vec2_ref.hidden_states(zero_mean_unit_var_norm(x), sdd, cfg, upto=0)[0]
        (dx,) = torch.autograd.grad((h * S.to(dtype)).sum(), x)
    return h.detach(), dx.detach()


# ------------------------------------------------------------------------------------------------ row counts
def rows(L: int, cfg) -> SimpleNamespace:
    """``Ls[i]``: valid rows of feature-encoder level ``i`` for a clip of ``L`` samples; ``left[i]``: the input samples / rows
    layer ``i`` leaves over, ``(n - k) % s``; ``P[i]``: padded rows per clip, the smallest with ``P[i] = P[i+1] * stride[i+1]`` and
    ``P[i] >= Ls[i] + 1`` at every level; ``tight``: the levels with exactly one filler row; ``T = Ls[-1]``."""
    ks, ss = cfg.conv_kernel, cfg.conv_stride
    Ls, left, n = [], [], L
    for k, s in zip(ks, ss):
        left.append((n - k) % s)
        n = (n - k) // s + 1
        Ls.append(n)
    nfe = len(Ls)
    down = [1] * nfe                                                  # rows of level i per row of the last level
    for i in range(nfe - 2, -1, -1):
        down[i] = down[i + 1] * ss[i + 1]
    p_last = max(1, max(-(-(Ls[i] + 1) // down[i]) for i in range(nfe)))
    P = [p_last * d for d in down]
    return SimpleNamespace(Ls=Ls, P=P, T=Ls[-1], left=left, tight=[i for i in range(nfe) if P[i] == Ls[i] + 1])


# ------------------------------------------------------------------------------------------------ the clip lengths
# Every entry states, for conv_kernel (10, 3, 3, 3, 3, 2, 2) and conv_stride (5, 2, 2, 2, 2, 2, 2), what rows(L) must give and the
# reason the length is in the table; tests/test_fe_backward_ref_cpu.py asserts every key.  Keys: T, Ls, P, P0 (P[0] alone), tight
# (the levels with exactly one filler row), left (the layers with leftover input, (n - k) % s != 0), fill0 (filler rows at level 0).
ALL_LEVELS = [0, 1, 2, 3, 4, 5, 6]
LENGTHS: Dict[int, dict] = {
    400: dict(why="the shortest clip: one frame, only the last level tight",
              T=1, Ls=[79, 39, 19, 9, 4, 2, 1], P=[128, 64, 32, 16, 8, 4, 2], tight=[6], left=[]),
    401: dict(why="a leftover sample at layer 0", T=1, left=[0], tight=[6]),
    560: dict(why="levels 5 and 6 tight, a leftover row at layer 6", T=1, tight=[5, 6], left=[6]),
    640: dict(why="every level tight at one frame", T=1, tight=ALL_LEVELS, P0=128),
    645: dict(why="no level tight: many filler rows",
              T=1, Ls=[128, 63, 31, 15, 7, 3, 1], P=[192, 96, 48, 24, 12, 6, 3], tight=[], fill0=64),
    719: dict(why="the last length with one frame, leftovers at every layer", T=1, left=ALL_LEVELS, tight=[]),
    720: dict(why="the first length with two frames", T=2, left=[], tight=[6]),
    1039: dict(why="two frames, P[0] = 256, leftovers at every layer", T=2, P0=256, left=ALL_LEVELS, tight=[]),
    4000: dict(why="twelve frames, 33 filler rows at level 0", T=12, P0=832, fill0=33, tight=[6]),
    16079: dict(why="the production frame count with 50 filler rows at level 0", T=49, fill0=50, tight=[], left=ALL_LEVELS),
    16000: dict(why="the class tests/test_gpu_backward.py covers: one filler row at every level",
                T=49, Ls=[3199, 1599, 799, 399, 199, 99, 49], P=[3200, 1600, 800, 400, 200, 100, 50], tight=ALL_LEVELS),
}
SHORTEST = 400               # the receptive field of one frame: a shorter clip has no frame


# ------------------------------------------------------------------------------------------------ the suite's fixed inputs
B_CLIPS, CLIP_SEED, SEED_S = 3, 31, 1
VARIANTS = ("group_postln", "layer_preln")
_cache: dict = {}


def model(variant: str):
    """``(cfg, state dict)`` of a tiny variant: group-norm feature encoder + post-LN encoder, or layer-norm + pre-LN."""
    from addvisor_hip import synthetic as syn
    if ("model", variant) not in _cache:
        cfg = syn.tiny_config(variant == "layer_preln")
        _cache["model", variant] = (cfg, syn.embedder_weights(cfg))
    return _cache["model", variant]


def layer_seed(T: int, H: int, seed: int = SEED_S, B: int = B_CLIPS) -> torch.Tensor:
    """The fixed seed gradient ``S [B, T, H]`` fp32 at ``hidden_states[0]``."""
    return torch.randn(B, T, H, generator=torch.Generator().manual_seed(seed + T))


def reference(variant: str, L: int, clip_seed: int = CLIP_SEED, seed: int = SEED_S, dtype: torch.dtype = torch.float64):
    """``(waves [3, L] fp32, S [3, T, H] fp32, h, dx)`` of one case, computed once per process and never modified."""
    from addvisor_hip import synthetic as syn
    key = (variant, L, clip_seed, seed, dtype)
    if key not in _cache:
        cfg, sd = model(variant)
        waves = syn.make_clips(B_CLIPS, L, seed=clip_seed)
        S = layer_seed(rows(L, cfg).T, cfg.hidden_size, seed)
        _cache[key] = (waves, S) + lower_chain_vjp(cfg, sd, waves, S, dtype)
    return _cache[key]


def window_ratios(got: torch.Tensor, ref: torch.Tensor) -> Dict[str, float]:
    """``max |got - ref| / max |ref|`` over the batch (``all``) and, per clip, over the first and the last ``WINDOW`` samples alone,
    each normalised by that window's own ``max |ref|`` (``head`` / ``tail``: the worst clip)."""
    got, ref = got.to(torch.float64), ref.to(torch.float64)
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    return dict(all=rel(got, ref), head=max(rel(g[:WINDOW], r[:WINDOW]) for g, r in zip(got, ref)),
                tail=max(rel(g[-WINDOW:], r[-WINDOW:]) for g, r in zip(got, ref)))
