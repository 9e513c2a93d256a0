"""Per-clip optimised mask explanations: Fong & Vedaldi's meaningful perturbation (2017) and extremal perturbations (Fong, Patrick
& Vedaldi 2019) over the STFT mask -- the objective the U-Net mask decoder (ADDvisor / L-MAC) amortises, solved for one clip
against the classifier itself.  Restated from the two papers (no Captum class, none in the reference: parity unpinned, like the
rollouts and LRP).  The entry point is ``HipSpectralAttribution.optimize_mask`` (spectral_attribution.py); this module holds its
argument checks (``check_mask_opt_args``, host only), the bindings of csrc/mask_opt.hip and the loop.

Per clip b the parameters ``theta_b [Fc, Tc]`` live on a coarse grid (``cell = (cf, ct)``, ``Fc = ceil(Fm / cf)``,
``Tc = ceil(Tm / ct)``, ``K = Fc * Tc``); ``p = sigmoid(theta)``; ``m = U p`` on ``[Fm, Tm]`` with U the bilinear upsampling of
``F.interpolate(size=(Fm, Tm), mode="bilinear", align_corners=False)`` (``axis_weights``).  With ``z_in = s_b F(m_b)``,
``z_out = s_b F(1 - m_b)`` (F the engine's function in its domain, ``s_b = +-1`` the class explained) and the reward ``phi``
(``"logit"``: z, ``"prob"``: sigmoid(z), ``"log_prob"``: log sigmoid(z), L-MAC's cross-entropy)

    ``J_b = -lam_in phi(z_in) + lam_out phi(z_out) + lam_area A_b + lam_l1 mean(p_b) + lam_tv TV_b``

-- Fong's preservation game, the deletion game (together L-MAC's mask-in / mask-out pair), the 2019 ranked-area constraint
``A_b = (1/K) sum_k (p_k - r[rank_k])^2`` (``rank`` the ascending stable rank of theta, ``r[j] = 1`` for ``j >= K - K1``,
``K1 = floor(area K + 0.5)``; the rank is a constant of the backward) and
``TV_b = (1/K) sum (p[i+1, j] - p[i, j])^2 + (p[i, j+1] - p[i, j])^2``.  Adam (torch.optim.Adam's semantics and defaults) or SGD
with momentum (``v <- mu v + g``, ``theta <- theta - lr v``) minimise it.

Two facts of this model shape the interface:

* Scale invariance.  In the ``linear`` domain ``F(alpha m) = F(m)`` (spectral_attribution.py, "The zero baseline"): the classifier
  does not see the mask's level, so a plain L1 area penalty shrinks the mask uniformly towards the silent clip, where the
  gradient grows as ``1 / alpha`` and the engine raises.  The ranked-area constraint pins a share ``area`` of the cells at 1 and
  has no such degeneracy: ``area`` must lie in (0, 1), and ``area=None`` (the 2017 formulation, ``lam_l1`` / ``lam_tv``) is
  accepted only with ``domain="log1p"``.
* Ties.  The rank breaks ties by index: from a constant start every cell ties and the area term would push the high-index cells
  (high frequency, late frames) to 1.  ``init`` may be a mask (the U-Net's, a normalised attribution), and ``init_noise`` -- the
  sigma of a seeded normal added to theta, drawn once on the host -- defaults to a small non-zero value.

Per step, in order: rank (advh_feature_rank, all clips) and, per chunk of whole clips, rows (advh_mask_opt_rows) -> ISTFT rows ->
forward -> terms (advh_mask_opt_terms: the seeds and the history row) -> backward(seed=) -> ISTFT adjoint -> step
(advh_mask_opt_step).  Nothing is read back inside the loop; one finiteness check at the end."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Optional, Tuple

import torch

from . import _lib, ops
from . import attribution as A

REWARDS = ("logit", "prob", "log_prob")
OPTIMIZERS = ("adam", "sgd")
HISTORY = ("z_in", "z_out", "area", "l1", "tv", "objective")
ADAM = (0.9, 0.999, 1e-8)
NBIN = ops.NBIN
DEFAULT_LAM_AREA = 10.0
DEFAULT_INIT_NOISE = 0.01


class MaskOptDesc(C.Structure):
    """Mirror of ``advh_mask_opt_desc`` (include/addvisor_hip.h)."""
    _fields_ = [("B", C.c_int), ("Fm", C.c_int), ("Tm", C.c_int), ("Fc", C.c_int), ("Tc", C.c_int), ("K1", C.c_int), ("reward", C.c_int),
                ("optimizer", C.c_int), ("lam_in", C.c_float), ("lam_out", C.c_float), ("lam_area", C.c_float), ("lam_l1", C.c_float),
                ("lam_tv", C.c_float), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("momentum", C.c_double)]


def coarse_grid(Fm: int, Tm: int, cell) -> Tuple[int, int]:
    """``(Fc, Tc) = (ceil(Fm / cf), ceil(Tm / ct))``."""
    return -(-Fm // cell[0]), -(-Tm // cell[1])


def ranked_cells(area: Optional[float], K: int) -> int:
    """``K1 = floor(area K + 0.5)``: the cells the ranked-area template sets to 1 (0 without an area)."""
    return 0 if area is None else int(math.floor(area * K + 0.5))


def axis_weights(n: int, N: int):
    """One axis of U: ``(i0, i1, w1)`` for the fine indices ``d = 0 .. N - 1`` over n coarse points (int64, int64, float64):
    ``src = max((d + 0.5) n / N - 0.5, 0)``, ``i0 = min(floor(src), n - 1)``, ``i1 = min(i0 + 1, n - 1)``, ``w1 = src - i0``
    (``w0 = 1 - w1``) -- the rule csrc/mask_opt.hip evaluates in fp32."""
    d = torch.arange(N, dtype=torch.float64)
    src = ((d + 0.5) * n / N - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n - 1)
    return i0, (i0 + 1).clamp(max=n - 1), src - i0.double()


@dataclasses.dataclass
class MaskOptArgs:
    B: int
    Fm: int
    Tm: int
    Fc: int
    Tc: int
    K1: int
    steps: int
    lam: Tuple[float, float, float, float, float]
    reward: int
    optimizer: int
    lr: float
    momentum: float
    sign: Optional[torch.Tensor]           # [B] fp32 +-1 on the host, None: the sign of F(ones)
    theta0: torch.Tensor                   # [B, Fc, Tc] fp32 on the host, the noise included
    clips_per_chunk: int
    trace: Optional[list]

    @property
    def K(self) -> int:
        return self.Fc * self.Tc

    def desc(self) -> MaskOptDesc:
        return MaskOptDesc(self.B, self.Fm, self.Tm, self.Fc, self.Tc, self.K1, self.reward, self.optimizer, *self.lam, self.lr, *ADAM,
                           self.momentum)


@dataclasses.dataclass
class MaskOptResult:
    """``mask [B, Fm, Tm]`` (the rows kernel of ``theta``), ``theta`` / ``coarse`` (= p) ``[B, Fc, Tc]``, ``logit [B]`` the
    unmasked logit ``F(ones)``, ``logits_in`` / ``logits_out [B]`` from one final forward of ``mask`` / ``1 - mask`` (they belong
    to the returned mask, not to the last step's), ``history``: ``[steps, B]`` tensors under the keys ``HISTORY`` (the values the
    update of step k read), ``area_reached [B]``: the share of cells with ``p > 0.5``, ``sign [B]``: the class explained."""
    mask: torch.Tensor
    theta: torch.Tensor
    coarse: torch.Tensor
    logit: torch.Tensor
    logits_in: torch.Tensor
    logits_out: torch.Tensor
    history: dict
    area_reached: torch.Tensor
    sign: torch.Tensor


def _number(v, what, lo=None, lo_open=False, hi=None) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{what} must be a finite number, not {v!r}")
    if lo is not None and (v <= lo if lo_open else v < lo):
        raise ValueError(f"{what} must be {'>' if lo_open else '>='} {lo:g}, not {v!r}")
    if hi is not None and v >= hi:
        raise ValueError(f"{what} must be < {hi:g}, not {v!r}")
    return float(v)


def _pair(v, what) -> Tuple[int, int]:
    if not isinstance(v, (tuple, list)) or len(v) != 2:
        raise ValueError(f"{what} must be a 2-tuple (frequency bins, frames), not {v!r}")
    return A._positive_int(v[0], what), A._positive_int(v[1], what)


def box_average(mask: torch.Tensor, cell) -> torch.Tensor:
    """``[B, Fm, Tm] -> [B, Fc, Tc]``: the mean over each cell's ``cf x ct`` box, the last box of an axis cropped (float64)."""
    return torch.nn.functional.avg_pool2d(mask.double()[:, None], tuple(cell), ceil_mode=True, count_include_pad=False)[:, 0]


def check_mask_opt_args(B: int, T: int, domain: str, area=0.1, steps=100, cell=(16, 4), shape=None, lam_in=1.0, lam_out=1.0,
                        lam_area=None, lam_l1=0.0, lam_tv=0.0, reward="log_prob", target=None, optimizer="adam", lr=0.05, momentum=0.9,
                        init=0.5, init_noise=DEFAULT_INIT_NOISE, seed=None, internal_batch_size=None, trace=None) -> MaskOptArgs:
    """Every argument check of ``optimize_mask`` for an engine of ``B`` clips with ``T`` frames in ``domain``: host only (CPU
    tensors in, nothing launched), ValueError on the first bad argument.  Returns the normalised ``MaskOptArgs``, the start
    ``theta0 = logit(init) + init_noise N(0, 1)`` (one draw from a ``torch.Generator`` seeded with ``seed``) included."""
    if area is None:
        if domain != "log1p":
            raise ValueError("area=None (the 2017 formulation: lam_l1 / lam_tv alone bound the mask) needs domain='log1p': in the "
                             "'linear' domain F(alpha m) = F(m), so an L1 penalty shrinks the mask towards the silent clip, where the "
                             "gradient grows as 1 / alpha and the engine raises; pass an area in (0, 1)")
        if lam_area not in (None, 0, 0.0):
            raise ValueError("lam_area weighs the ranked-area constraint: it needs an area")
        lam_area = 0.0
    else:
        if isinstance(area, bool) or not isinstance(area, (int, float)) or not 0.0 < area < 1.0:
            raise ValueError(f"area must lie in the open interval (0, 1) (the share of cells the ranked-area constraint pins at 1: 0 "
                             f"is the silent clip, 1 the whole clip), not {area!r}")
        lam_area = DEFAULT_LAM_AREA if lam_area is None else lam_area
    steps = A._positive_int(steps, "steps")
    cell = _pair(cell, "cell")
    Fm, Tm = (NBIN, T) if shape is None else _pair(shape, "shape")
    if Fm > NBIN or Tm > T:
        raise ValueError(f"shape must be (Fm <= {NBIN}, Tm <= {T}), not {(Fm, Tm)}")
    if not 1 <= B <= 65535:
        raise ValueError(f"the mask kernels take 1 .. 65535 clips, not {B}")
    Fc, Tc = coarse_grid(Fm, Tm, cell)
    K = Fc * Tc
    lam = tuple(_number(v, n, 0.0) for v, n in ((lam_in, "lam_in"), (lam_out, "lam_out"), (lam_area, "lam_area"), (lam_l1, "lam_l1"),
                                                (lam_tv, "lam_tv")))
    if reward not in REWARDS:
        raise ValueError(f"reward must be one of {REWARDS}, not {reward!r}")
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {OPTIMIZERS}, not {optimizer!r}")
    lr = _number(lr, "lr", 0.0, True)
    momentum = _number(momentum, "momentum", 0.0, False, 1.0)
    sign = None
    if target is not None:
        t = torch.as_tensor(target).detach().cpu()
        if t.dim() != 1 or t.shape[0] != B or t.is_floating_point() or t.is_complex() or not bool(((t == 0) | (t == 1)).all()):
            raise ValueError(f"target must be None (the predicted class) or [{B}] labels in {{0, 1}}")
        sign = (2.0 * t.to(torch.float32) - 1.0).contiguous()
    sigma = _number(init_noise, "init_noise", 0.0)
    if torch.is_tensor(init):
        A._float_tensor(init, "init")
        if init.dim() != 3 or init.shape[0] != B or tuple(init.shape[1:]) not in ((Fc, Tc), (Fm, Tm)):
            raise ValueError(f"init must be a number in (0, 1) or a [{B}, {Fc}, {Tc}] / [{B}, {Fm}, {Tm}] tensor of mask values; got "
                             f"{list(init.shape)}")
        p0 = init.detach().cpu().double()
        if tuple(p0.shape[1:]) != (Fc, Tc):
            p0 = box_average(p0, cell)
    elif isinstance(init, (int, float)) and not isinstance(init, bool):
        p0 = torch.full((B, Fc, Tc), float(init), dtype=torch.float64)
    else:
        raise ValueError(f"init must be a number in (0, 1) or a tensor of mask values, not {init!r}")
    if not bool(((p0 > 0) & (p0 < 1)).all()):                  # NaN fails too
        raise ValueError("init must hold mask values inside the open interval (0, 1): theta = logit(init) is infinite at 0 and 1")
    sd = A._check_seed(seed) if sigma > 0 else 0                # drawn only when used
    if trace is not None and not isinstance(trace, list):
        raise ValueError("trace must be None or a list")
    chunk = A.check_internal_batch(internal_batch_size)
    theta0 = torch.log(p0) - torch.log1p(-p0)
    if sigma > 0:
        gen = torch.Generator().manual_seed(sd % (2 ** 63))
        theta0 = theta0 + sigma * torch.randn((B, Fc, Tc), generator=gen, dtype=torch.float64)
    return MaskOptArgs(B, Fm, Tm, Fc, Tc, ranked_cells(area, K), steps, lam, REWARDS.index(reward), OPTIMIZERS.index(optimizer), lr, momentum,
                       sign, theta0.to(torch.float32).contiguous(), max(1, chunk // 2), trace)


# ---------------------------------------------------------------------------------------------------------------- the three launches
def mask_rows(d: MaskOptDesc, theta: torch.Tensor, b0: int, nb: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rows [2 nb, Fm * Tm]`` of the clips ``b0 .. b0 + nb - 1`` of ``theta [B, Fc, Tc]``: row 2j the mask, 2j + 1 its complement."""
    if out is None:
        out = torch.empty((2 * nb, d.Fm * d.Tm), dtype=torch.float32, device=theta.device)
    A._on_gpu(theta, out)
    _lib.check(_lib.lib().advh_mask_opt_rows(C.byref(d), theta.data_ptr(), b0, nb, out.data_ptr(), A._st()), "advh_mask_opt_rows")
    return out


def mask_terms(d: MaskOptDesc, theta, rank, sign, logits, b0: int, nb: int, p, seeds, hist) -> None:
    """The terms launch: ``logits [2 nb]`` of the chunk's rows -> ``seeds [2 nb]``, ``p [B, K]`` and ``hist [B, 6]`` at the chunk's clips."""
    A._on_gpu(theta, rank, sign, logits, p, seeds, hist)
    _lib.check(_lib.lib().advh_mask_opt_terms(C.byref(d), theta.data_ptr(), rank.data_ptr(), sign.data_ptr(), logits.data_ptr(), b0, nb,
                                              p.data_ptr(), seeds.data_ptr(), hist.data_ptr(), A._st()), "advh_mask_opt_terms")


def bias_corrections(step: int) -> Tuple[float, float]:
    """Adam's ``1 - beta^step`` (``step`` counts from 1), in double."""
    return 1.0 - ADAM[0] ** step, 1.0 - ADAM[1] ** step


def mask_step(d: MaskOptDesc, theta, p, rank, G, b0: int, nb: int, step: int, m1, m2, grad_theta=None) -> None:
    """The step launch (``step`` counts from 1): ``G [2 nb, Fm * Tm]`` -> the update of ``theta``, ``m1``, ``m2`` in place."""
    A._on_gpu(theta, p, rank, G, m1, m2, grad_theta)
    bc1, bc2 = bias_corrections(step)
    _lib.check(_lib.lib().advh_mask_opt_step(C.byref(d), theta.data_ptr(), p.data_ptr(), rank.data_ptr(), G.data_ptr(), b0, nb, bc1, bc2,
                                             m1.data_ptr(), None if m2 is None else m2.data_ptr(),
                                             None if grad_theta is None else grad_theta.data_ptr(), A._st()), "advh_mask_opt_step")


def coarse_of(theta: torch.Tensor) -> torch.Tensor:
    """``p = sigmoid(theta)`` with the kernels' own sigmoid: the rows kernel at the identity geometry, where U is exact."""
    B, Fc, Tc = theta.shape
    d = MaskOptDesc(B, Fc, Tc, Fc, Tc, 0, 0, 0)
    return mask_rows(d, theta, 0, B)[0::2].reshape(B, Fc, Tc)


# --------------------------------------------------------------------------------------------------------------------------- the loop
def optimize(eng, a: MaskOptArgs) -> MaskOptResult:
    """The loop of ``HipSpectralAttribution.optimize_mask`` on the engine ``eng`` with checked arguments."""
    rows_eng = eng._rows
    rows_eng.Fm, rows_eng.Tm = a.Fm, a.Tm
    dev = eng.waves.device
    B, K, n = a.B, a.K, a.Fm * a.Tm
    d = a.desc()
    theta = a.theta0.to(dev).contiguous()
    logit0 = eng.logits(torch.ones((B, a.Fm, a.Tm), dtype=torch.float32, device=dev)).to(torch.float32).contiguous()
    sign = torch.where(logit0 >= 0, 1.0, -1.0).to(torch.float32) if a.sign is None else a.sign.to(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    m1, m2 = torch.zeros((B, K), **f32), (torch.zeros((B, K), **f32) if a.optimizer == 0 else None)
    p, hist = torch.empty((B, K), **f32), torch.zeros((a.steps, B, len(HISTORY)), **f32)
    nbmax = min(B, a.clips_per_chunk)
    rows, seeds = torch.empty((2 * nbmax, n), **f32), torch.empty(2 * B, **f32)
    logits = torch.empty(2 * B, **f32) if a.trace is not None else None
    grad = torch.empty((B, K), **f32) if a.trace is not None else None
    flat = theta.view(B, K)
    cause = (f"the seeds or the gradient chain overflowed at loss_scale={rows_eng.loss_scale:g} (lower lam_in / lam_out, or "
             "HipAttribution.loss_scale by a power of two), or the clips are not finite")
    try:
        for k in range(a.steps):
            rank = A.feature_rank(flat, False)
            theta_k = theta.clone() if a.trace is not None else None
            for b0 in range(0, B, nbmax):
                nb = min(nbmax, B - b0)
                r, sd = rows[:2 * nb], seeds[2 * b0:2 * (b0 + nb)]
                mask_rows(d, theta, b0, nb, r)

                def seeds_of(lg, b0=b0, nb=nb, sd=sd):
                    mask_terms(d, theta, rank, sign, lg, b0, nb, p, sd, hist[k])
                    if logits is not None:
                        logits[2 * b0:2 * (b0 + nb)] = lg
                    return sd

                G = rows_eng._row_gradient_seeded(r, seeds_of, 2 * b0, 1, 2)
                mask_step(d, theta, p, rank, G, b0, nb, k + 1, m1, m2, grad)
            if a.trace is not None:
                a.trace.append((theta_k, grad.view(B, a.Fc, a.Tc).clone(), logits.clone(), seeds.clone()))
        rows_eng._checked(torch.cat([theta.flatten(), hist.flatten()]), "optimised mask", cause)
    except _lib.SplitRangeError as e:                      # the fp32-class planes saturated: the same cause, found by the range flag
        torch.cuda.synchronize(dev)                        # launches still queued raise the sticky flag again: let them finish,
        _lib.lib().advh_split_overflow(1)                  # then clear it, so that the next call starts clean
        raise FloatingPointError(f"non-finite optimised mask: {cause}") from e
    final = mask_rows(d, theta, 0, B)
    mask, mask_out = final[0::2].contiguous().view(B, a.Fm, a.Tm), final[1::2].contiguous().view(B, a.Fm, a.Tm)
    coarse = coarse_of(theta)
    h = {name: hist[:, :, i].clone() for i, name in enumerate(HISTORY)}
    return MaskOptResult(mask, theta, coarse, logit0, eng.logits(mask), eng.logits(mask_out), h,
                         (coarse > 0.5).to(torch.float32).flatten(1).mean(1), sign)
