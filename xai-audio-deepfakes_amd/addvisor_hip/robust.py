"""Adversarial attacks on the waveform -> logit classifier: the semantics of ``captum.robust.FGSM`` and ``captum.robust.PGD``
(restated from Captum 0.7's ``robust/_core/fgsm.py`` and ``pgd.py``: captum is absent) on the HIP gradient chain.

An attack step is one forward + dgrad-only backward of ``EmbedderGrad`` with the unit seed and one launch of
csrc/attribution_robust.hip, which applies the per-clip loss factor ``dL/d logit``, takes the signed step, projects onto PGD's
ball around the clean clip and clamps to the bounds (advh_robust_step).  Nothing inside the loop synchronises with the host; one
finiteness check and one read of the split format's range flag end an attack.  PGD's random start is drawn on the device from
the counter-based generator of the attribution kernels under one seed per call (advh_robust_random_start), so
``torch.manual_seed`` reproduces a result; Captum's own RNG stream is not reproduced.

``fgsm_min_epsilon`` answers "how small a step flips the decision" for a ladder of step sizes with one gradient pass: FGSM's
direction does not depend on epsilon, so the ``B * K`` candidates are built by one kernel, pushed through the plain forward and
folded on the device (advh_robust_first_flip).  It is this build's counterpart of ``captum.robust.MinParamPerturbation`` over
FGSM and claims no Captum signature."""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import attribution as AT

NORMS = {"Linf": 1, "L2": 2}                                            # PGD's norm -> advh_robust_desc.norm (0: no projection)
MAX_P = 64                                                              # ADVH_ROBUST_MAX_P: the rows of one clip in one launch


class RobustDesc(C.Structure):
    """Mirror of ``advh_robust_desc`` (include/addvisor_hip.h)."""
    _fields_ = [("x0", C.c_void_p), ("x", C.c_void_p), ("grad", C.c_void_p), ("seed", C.c_void_p), ("mask", C.c_void_p),
                ("eps", C.c_void_p), ("n", C.c_int64), ("B", C.c_int), ("p", C.c_int), ("x_rows", C.c_int), ("grad_rows", C.c_int),
                ("mask_rows", C.c_int), ("targeted", C.c_int), ("norm", C.c_int), ("radius", C.c_float), ("lo", C.c_float),
                ("hi", C.c_float)]


# ---------------------------------------------------------------------------------------------------- argument checks (no GPU)
def _number(v, what) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what} must be a number, not {v!r}")
    return float(v)


def check_waves(waves) -> Tuple[int, int]:
    """``inputs``: a floating ``[B, L]`` tensor -> ``(B, L)``."""
    if not torch.is_tensor(waves) or waves.dim() != 2 or not waves.is_floating_point() or 0 in waves.shape:
        raise ValueError("inputs must be a non-empty floating-point [B, L] waveform tensor")
    return tuple(waves.shape)


def check_bounds(lower_bound, upper_bound) -> Tuple[float, float]:
    """FGSM / PGD's ``lower_bound <= upper_bound``, numbers, -+inf allowed, NaN rejected."""
    lo, hi = _number(lower_bound, "lower_bound"), _number(upper_bound, "upper_bound")
    if math.isnan(lo) or math.isnan(hi) or lo > hi:
        raise ValueError(f"the bounds must satisfy lower_bound <= upper_bound, not ({lower_bound!r}, {upper_bound!r})")
    return lo, hi


def check_norm(norm) -> int:
    """PGD's ``norm``: "Linf" or "L2" -> advh_robust_desc.norm.  Anything else raises ValueError (Captum asserts)."""
    if not isinstance(norm, str) or norm not in NORMS:
        raise ValueError(f"norm must be 'Linf' or 'L2', not {norm!r}")
    return NORMS[norm]


def check_step_num(step_num) -> int:
    if isinstance(step_num, bool) or not isinstance(step_num, (int, np.integer)) or step_num < 0:
        raise ValueError(f"step_num must be an integer >= 0, not {step_num!r}")
    return int(step_num)


def check_target(target, B: int):
    """The default loss's ``target``: 0 or 1, or a ``[B]`` (``[B, 1]``) tensor of 0s and 1s -> an int or a ``[B]`` fp32 host
    tensor.  A callable loss_func takes any target: this check is not applied to it."""
    if torch.is_tensor(target):
        t = target.detach().reshape(-1).to("cpu", torch.float32)
        if target.dim() > 2 or t.numel() != B or (target.dim() == 2 and target.shape[1] != 1):
            raise ValueError(f"target must be 0, 1 or a [{B}] tensor of 0s and 1s, not a tensor of shape {list(target.shape)}")
        if not bool(((t == 0) | (t == 1)).all()):
            raise ValueError("target must hold only 0s and 1s (the classifier has one logit: binary cross-entropy with logits)")
        return t
    if isinstance(target, bool) or not isinstance(target, (int, np.integer)) or target not in (0, 1):
        raise ValueError(f"target must be 0, 1 or a [{B}] tensor of 0s and 1s, not {target!r}")
    return int(target)


def check_mask(mask, B: int, L: int):
    """``mask``: None, or a ``[1, L]`` / ``[B, L]`` (or ``[L]``) numeric tensor that multiplies the step."""
    if mask is None:
        return None
    if not torch.is_tensor(mask) or mask.dtype == torch.complex64 or mask.dtype == torch.complex128:
        raise ValueError("mask must be a real tensor of shape [1, L] or [B, L]")
    m = mask[None] if mask.dim() == 1 else mask
    if m.dim() != 2 or m.shape[1] != L or m.shape[0] not in (1, B):
        raise ValueError(f"mask must have shape [1, {L}] or [{B}, {L}], not {list(mask.shape)}")
    return m


def check_loss_func(loss_func) -> None:
    if loss_func is not None and not callable(loss_func):
        raise ValueError("loss_func must be None or a callable loss_func(outputs [B, 1], target)")


def check_fgsm_args(waves, epsilon, target, loss_func=None, mask=None, lower_bound=-math.inf, upper_bound=math.inf):
    """Every check of ``fgsm`` -> ``(B, L, eps, target, mask, lo, hi)``.  Raises ValueError before any GPU work."""
    B, L = check_waves(waves)
    eps = AT._finite_scale(epsilon, "epsilon")
    check_loss_func(loss_func)
    tgt = check_target(target, B) if loss_func is None else target
    lo, hi = check_bounds(lower_bound, upper_bound)
    return B, L, eps, tgt, check_mask(mask, B, L), lo, hi


def check_pgd_args(waves, radius, step_size, step_num, target, loss_func=None, norm="Linf", mask=None, lower_bound=-math.inf,
                   upper_bound=math.inf):
    """Every check of ``pgd`` -> ``(B, L, radius, step_size, step_num, target, norm, mask, lo, hi)``.  Raises ValueError before
    any GPU work."""
    B, L = check_waves(waves)
    r, s = AT._finite_scale(radius, "radius"), AT._finite_scale(step_size, "step_size")
    n = check_step_num(step_num)
    nrm = check_norm(norm)
    check_loss_func(loss_func)
    tgt = check_target(target, B) if loss_func is None else target
    lo, hi = check_bounds(lower_bound, upper_bound)
    return B, L, r, s, n, tgt, nrm, check_mask(mask, B, L), lo, hi


def check_epsilons(epsilons) -> list:
    """``fgsm_min_epsilon``'s ladder: a non-empty, strictly increasing sequence of positive finite numbers, at most ``MAX_P``."""
    if torch.is_tensor(epsilons) or isinstance(epsilons, np.ndarray):
        epsilons = epsilons.tolist()
    if not isinstance(epsilons, (list, tuple)) or len(epsilons) == 0:
        raise ValueError("epsilons must be a non-empty sequence of numbers")
    eps = [_number(e, "an epsilon") for e in epsilons]
    if len(eps) > MAX_P:
        raise ValueError(f"at most {MAX_P} epsilons per ladder, not {len(eps)}")
    if not all(math.isfinite(e) and e > 0 for e in eps) or any(b <= a for a, b in zip(eps, eps[1:])):
        raise ValueError("epsilons must be positive, finite and strictly increasing")
    if any(np.float32(b) <= np.float32(a) for a, b in zip(eps, eps[1:])):
        raise ValueError("epsilons must stay strictly increasing in float32")
    return eps


def first_flip(logits, clean_logits, epsilons) -> Tuple[np.ndarray, np.ndarray]:
    """Host model of advh_robust_first_flip: ``logits [B, K]``, ``clean_logits [B]`` -> ``(eps_min [B] float32, first [B]
    int32)``: the first k with ``(logit > 0) != (clean > 0)``; ``inf`` and ``K`` when none."""
    lg = np.asarray(logits, np.float32)
    cl = np.asarray(clean_logits, np.float32).reshape(-1)
    eps = np.asarray(epsilons, np.float32)
    B, K = lg.shape
    out, first = np.full(B, np.inf, np.float32), np.full(B, K, np.int32)
    for b in range(B):
        for k in range(K):
            if (lg[b, k] > 0) != (cl[b] > 0):
                out[b], first[b] = eps[k], k
                break
    return out, first


# ------------------------------------------------------------------------------------------------------------ kernel wrappers
def _ptr(t):
    return None if t is None else t.data_ptr()


def robust_step(x0, x, grad, seed, mask, eps: Sequence[float], targeted: bool, norm: int, radius: float, lo: float, hi: float,
                out: torch.Tensor, row0: int = 0, rows: Optional[int] = None, B: Optional[int] = None) -> torch.Tensor:
    """advh_robust_step: launch rows ``[row0, row0 + rows)`` of the ``B * len(eps)`` rows into ``out [rows, L]`` (which may be the
    same rows of ``x``).  ``x0 [B, L]`` (None when ``norm == 0``), ``x`` / ``grad`` with ``B`` or ``B * len(eps)`` rows,
    ``seed [B]`` or None, ``mask [1 | B, L]`` or None: contiguous fp32 GPU tensors.  ``B`` defaults to the rows of ``x0``, or of
    the shorter of ``x`` and ``grad``."""
    AT._on_gpu(x0, x, grad, seed, mask, out)
    p = len(eps)
    if B is None:
        B = x0.shape[0] if x0 is not None else min(x.shape[0], grad.shape[0])
    arr = (C.c_double * p)(*[float(e) for e in eps])
    d = RobustDesc(_ptr(x0), x.data_ptr(), grad.data_ptr(), _ptr(seed), _ptr(mask), C.addressof(arr), x.shape[1], B, p, x.shape[0],
                   grad.shape[0], 1 if mask is None else mask.shape[0], int(bool(targeted)), norm, radius, lo, hi)
    rows = B * p - row0 if rows is None else rows
    _lib.check(_lib.lib().advh_robust_step(C.byref(d), row0, rows, out.data_ptr(), AT._st()), "advh_robust_step")
    return out


def random_point(x0: torch.Tensor, seed: int, norm: int, radius: float, lo: float, hi: float) -> torch.Tensor:
    """advh_robust_random_start: PGD's bounded random point in the ``norm`` ball of ``radius`` around each row of ``x0 [B, L]``."""
    AT._on_gpu(x0)
    out = torch.empty_like(x0)
    _lib.check(_lib.lib().advh_robust_random_start(x0.data_ptr(), x0.shape[0], x0.shape[1], int(seed), norm, radius, lo, hi,
                                                   out.data_ptr(), AT._st()), "advh_robust_random_start")
    return out


def first_flip_rows(logits: torch.Tensor, clean_logits: torch.Tensor, eps: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """advh_robust_first_flip on ``logits [B * K]``, ``clean_logits [B]``, ``eps [K]`` (fp32, GPU): ``(eps_min [B] fp32, first [B]
    int32)``."""
    AT._on_gpu(logits, clean_logits, eps)
    B, K = clean_logits.numel(), eps.numel()
    out = torch.empty(B, dtype=torch.float32, device=logits.device)
    first = torch.empty(B, dtype=torch.int32, device=logits.device)
    _lib.check(_lib.lib().advh_robust_first_flip(logits.data_ptr(), clean_logits.data_ptr(), eps.data_ptr(), B, K, out.data_ptr(),
                                                 first.data_ptr(), AT._st()), "advh_robust_first_flip")
    return out, first


class HipRobust:
    """FGSM, PGD and the epsilon ladder on the gradient chain of a ``HipAttribution`` (its precision, its ``loss_scale``)."""

    def __init__(self, att: "AT.HipAttribution"):
        self.att, self.eg, self.precision = att, att.eg, att.precision

    # ---------------------------------------------------------------------------------------------------------------- loss
    def loss_seed(self, logit: torch.Tensor, prob: torch.Tensor, target, loss_func: Optional[Callable] = None) -> torch.Tensor:
        """``dL/d logit`` per clip, ``[B]`` fp32 on the device, for the summed loss.

        ``loss_func=None``: binary cross-entropy with logits against ``target`` (0, 1 or a ``[B]`` tensor of them), whose
        derivative is ``prob - target``.  Captum's own default, ``-log(outputs)`` selected by ``target``, presumes that the
        model returns a probability vector; this classifier returns one logit, so the default is the loss that
        ``-log(softmax)`` is for two classes.  A callable ``loss_func(outputs [B, 1], target)`` is differentiated by autograd
        over the ``[B, 1]`` logit leaf alone (``torch.autograd.grad(loss.sum(), logits)``): the model never enters autograd."""
        if loss_func is None:
            t = target.to(prob.device, torch.float32) if torch.is_tensor(target) else float(target)
            return (prob.reshape(-1).to(torch.float32) - t).contiguous()
        with torch.enable_grad():
            leaf = logit.detach().reshape(-1, 1).clone().requires_grad_(True)
            tgt = target.to(leaf.device) if torch.is_tensor(target) else target
            loss = loss_func(leaf, tgt)
            if not torch.is_tensor(loss) or not loss.requires_grad:
                raise ValueError("loss_func must return a tensor that depends on its outputs argument")
            (g,) = torch.autograd.grad(loss.sum(), leaf)
        return g.detach().reshape(-1).to(torch.float32).contiguous()

    def _gradient(self, x, target, loss_func):
        """One forward + unit-seed backward at ``x``: ``(grad [B, L], seed [B], logit [B, 1])``."""
        logit, prob = self.eg.forward(x)
        seed = self.loss_seed(logit, prob, target, loss_func)
        return self.eg.backward(self.att.loss_scale), seed, logit

    def _mask(self, mask, dev):
        return None if mask is None else mask.to(dev, torch.float32).contiguous()

    @staticmethod
    def _target(target, dev):
        """A tensor target goes to the device once, before the loop: no step copies from the host."""
        return target.to(dev) if torch.is_tensor(target) else target

    def _checked(self, out, what):
        return self.att._checked(out, what, "the clips, the loss or the gradient chain are not finite "
                                            f"(loss_scale={self.att.loss_scale:g})")

    # ------------------------------------------------------------------------------------------------------------- attacks
    def fgsm(self, waves, epsilon, target, loss_func=None, targeted=False, mask=None, lower_bound=-math.inf,
             upper_bound=math.inf) -> torch.Tensor:
        """Captum's ``FGSM.perturb``: ``clamp(x + multiplier * epsilon * sign(dL/dx) * mask, lower_bound, upper_bound)`` where
        ``|dL/dx| > 1e-6`` (x elsewhere), multiplier -1 if ``targeted`` (descend towards ``target``) else +1.  ``[B, L]`` fp32."""
        B, L, eps, tgt, m, lo, hi = check_fgsm_args(waves, epsilon, target, loss_func, mask, lower_bound, upper_bound)
        x = self.att._prep(waves)
        g, seed, _ = self._gradient(x, self._target(tgt, x.device), loss_func)
        out = robust_step(None, x, g, seed, self._mask(m, x.device), [eps], targeted, 0, 0.0, lo, hi, torch.empty_like(x))
        return self._checked(out, "FGSM perturbation")

    def pgd(self, waves, radius, step_size, step_num, target, loss_func=None, targeted=False, random_start=False, norm="Linf",
            mask=None, lower_bound=-math.inf, upper_bound=math.inf, seed: Optional[int] = None, trace: Optional[list] = None):
        """Captum's ``PGD.perturb``: an optional bounded random start in the ``norm`` ball, then ``step_num`` times an FGSM step
        of ``step_size``, the projection onto the ball of ``radius`` around the clean clips (``norm="Linf"``: a clamp of the
        difference; ``"L2"``: ``torch.renorm`` of it -- the step itself stays the sign step) and the bounds.  ``seed``: the
        random start's (default: one draw from torch's CPU generator).  ``trace``, a list, receives per step the clones
        ``(x_k, grad_k, seed_k)`` the update read.  ``[B, L]`` fp32."""
        B, L, r, s, n, tgt, nrm, m, lo, hi = check_pgd_args(waves, radius, step_size, step_num, target, loss_func, norm, mask,
                                                            lower_bound, upper_bound)
        sd = AT._check_seed(seed) if random_start else None   # drawn only when used
        if trace is not None and not isinstance(trace, list):
            raise ValueError("trace must be None or a list")
        x0 = self.att._prep(waves)
        m, tgt = self._mask(m, x0.device), self._target(tgt, x0.device)
        x = random_point(x0, sd, nrm, r, lo, hi) if random_start else x0.clone()
        for _ in range(n):
            g, ls, _ = self._gradient(x, tgt, loss_func)
            if trace is not None:
                trace.append((x.clone(), g.clone(), ls.clone()))
            robust_step(x0, x, g, ls, m, [s], targeted, nrm, r, lo, hi, x)      # in place: the backward has read x
        return self._checked(x, "PGD perturbation")

    def fgsm_min_epsilon(self, waves, epsilons, target, loss_func=None, targeted=False, mask=None, lower_bound=-math.inf,
                         upper_bound=math.inf, internal_batch_size: Optional[int] = None, record: Optional[dict] = None):
        """The smallest epsilon of the ladder ``epsilons`` whose FGSM perturbation flips each clip's decision (the sign of the
        logit): ``(eps_min [B] fp32, adversarial [B, L])``; clips that no epsilon flips get ``inf`` and their clean waveform.
        One gradient pass; the ``B * K`` candidates are pushed through the plain forward in chunks of whole clips of at most
        ``internal_batch_size`` rows (default 128, at least one clip).  ``record``, a dict, receives the device's ``logits
        [B, K]``, ``clean_logits [B]``, ``first [B]`` and the ``ladder [B, K, L]``."""
        eps = check_epsilons(epsilons)
        B, L, _, tgt, m, lo, hi = check_fgsm_args(waves, eps[0], target, loss_func, mask, lower_bound, upper_bound)
        K = len(eps)
        clips = max(1, AT.check_internal_batch(internal_batch_size) // K)
        x = self.att._prep(waves)
        m = self._mask(m, x.device)
        g, seed, logit0 = self._gradient(x, self._target(tgt, x.device), loss_func)
        ladder = torch.empty((B * K, L), dtype=torch.float32, device=x.device)
        logits = torch.empty(B * K, dtype=torch.float32, device=x.device)
        for b0 in range(0, B, clips):
            r0, r1 = b0 * K, min(B, b0 + clips) * K
            robust_step(None, x, g, seed, m, eps, targeted, 0, 0.0, lo, hi, ladder[r0:r1], r0, r1 - r0)
            logits[r0:r1] = self.att.logits(ladder[r0:r1])
        clean = logit0.reshape(-1).to(torch.float32).contiguous()
        eps_min, first = first_flip_rows(logits, clean, torch.tensor(eps, dtype=torch.float32, device=x.device))
        flipped = first < K
        pick = ladder.view(B, K, L)[torch.arange(B, device=x.device), first.long().clamp(max=K - 1)]
        adv = torch.where(flipped[:, None], pick, x)
        if record is not None:
            record.update(logits=logits.view(B, K), clean_logits=clean, first=first, ladder=ladder.view(B, K, L))
        self._checked(torch.cat([logits, clean]), "epsilon ladder")
        return eps_min, self._checked(adv, "FGSM perturbation")
