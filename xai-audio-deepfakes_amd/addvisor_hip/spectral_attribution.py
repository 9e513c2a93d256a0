"""Time-frequency attributions: Captum's methods over the STFT mask ``[B, Fm, Tm]`` instead of the waveform ``[B, L]`` -- the
domain ADDvisor itself explains in.  The function attributed is, per clip b with complex spectrogram ``X_b``
(``ops.stft_forward``),

    ``F(m)[b] = logit(embedder(istft(X_b * g(m, |X_b|) / |X_b|)))``

with ``m [Fm, Tm]`` (bins outside the crop count as 0), ``g`` the ``linear`` (loss_function.py:36-45) or
``log1p`` (LMAC_metrics.py:136-153) mask application, mask-in branch only.  The input is usually ``torch.ones(B, Fm, Tm)`` (the
clip itself) or the U-Net's mask.

A mask is the flat row ``[B, Fm * Tm]``, so the points, weights, draws and sums are the waveform engine's own kernels and chunk
loops (attribution.py) with ``n = Fm * Tm``; only the forward / gradient pair differs (``HipAttribution._row_gradient`` /
``_row_logit``): a forward over rows is ``ops.istft_masked_rows`` followed by the embedder, a gradient over rows is
``EmbedderGrad.backward`` followed by ``ops.istft_masked_rows_bwd``.  Both ISTFT launches map row r to its clip by the rows'
layout, so the ``R = B * S`` rows of a path or perturbation batch read B spectrograms, not R copies.  The ISTFT adjoint is fp32
and sits below advh_wave_bwd, which has already divided by ``loss_scale``: the scale is the waveform engine's own.

The zero baseline.  The classifier normalises each clip by its own std + 1e-7, so in the ``linear`` domain
``F(alpha * m) = F(m)`` for every ``alpha > 0``: the logit does not see the mask's overall level.  A straight path through the
zero mask (the silent clip) therefore carries gradients that grow as ``1 / alpha`` and ends at the point that
``HipAttribution.integrated_gradients`` documents as raising FloatingPointError (a constant clip).  ``baselines=None`` and 0 are
accepted for Captum compatibility, but a mask baseline is the meaningful choice: a random mask, the complement of the U-Net's
mask, or -- GradientShap -- a ``[N_b, Fm, Tm]`` distribution.  The same invariance gives Euler's identity
``sum_j m_j dF/dm_j = 0`` in the ``linear`` domain, a check on any gradient this engine returns.

``perturbation_curve`` / ``curve_summary`` score a mask-domain attribution (the U-Net's mask included) by its deletion / insertion
curves over the features of ``tf_feature_mask`` (attribution.py; csrc/attribution_curve.hip).  There too a mask baseline, such as
a constant 0.5, is the meaningful choice: the zero mask resynthesises silence.

``optimize_mask`` solves for a mask instead of attributing one: the per-clip optimised mask of Fong & Vedaldi (2017, 2019), the
objective the U-Net mask decoder amortises (mask_opt.py; csrc/mask_opt.hip).

Not in this engine: KernelShap, Lime, FeaturePermutation, NoiseTunnel, the metrics and the attacks over masks
(NotImplementedError)."""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional, Tuple

import torch

from . import _lib, ops
from . import attribution as A
from . import mask_opt as MO
from .attribution import HipAttribution

DOMAINS = ("linear", "log1p")
NBIN = ops.NBIN


def occlusion2d_windows(Fm: int, Tm: int, window, stride) -> Tuple[int, int]:
    """``(Kf, Kt)``: Captum's shift counts per axis, ``ceil((n - w) / s) + 1``; window ``k = kf * Kt + kt`` (first dimension
    slowest, as Captum's ``_occlusion_mask`` enumerates) covers ``[kf * sf, min(kf * sf + wf, Fm)) x [kt * st, min(kt * st + wt,
    Tm))``."""
    return A.occlusion_windows(Fm, window[0], stride[0]), A.occlusion_windows(Tm, window[1], stride[1])


def _two_dims(v, what) -> Tuple[int, int]:
    if not isinstance(v, (tuple, list)) or len(v) != 2:
        raise ValueError(f"{what} must be a 2-tuple (frequency bins, frames) for a [B, Fm, Tm] input, not {v!r}")
    return A._positive_int(v[0], what), A._positive_int(v[1], what)


def check_occlusion2d_args(Fm: int, Tm: int, window, stride=None):
    """Occlusion's 2-tuples -> ``((wf, wt), (sf, st), (Kf, Kt))`` (``stride=None`` is ``(1, 1)``).  Raises ValueError before any
    GPU work on Captum's assertions, per axis: ``w <= n``, and ``s <= w`` unless ``w == n``."""
    w = _two_dims(window, "sliding_window_shapes")
    s = (1, 1) if stride is None else _two_dims(stride, "strides")
    for n, wi, si, name in ((Fm, w[0], s[0], "frequency"), (Tm, w[1], s[1], "time")):
        if wi > n:
            raise ValueError(f"the {name} occlusion window ({wi}) is longer than the input ({n})")
        if si > wi and wi != n:
            raise ValueError(f"the {name} stride ({si}) exceeds the window ({wi}): bins between windows would be skipped")
    return w, s, occlusion2d_windows(Fm, Tm, w, s)


def check_mask_inputs(inputs, target=None, T: Optional[int] = None) -> Tuple[int, int, int]:
    """``inputs``: a floating ``[B, Fm <= 513, Tm (<= T)]`` mask; ``target`` None (one output).  -> ``(B, Fm, Tm)``."""
    if target is not None:
        raise ValueError("the classifier has a single output; target must be None")
    if not torch.is_tensor(inputs) or inputs.dim() != 3 or not inputs.is_floating_point():
        raise ValueError("inputs must be a floating [B, Fm, Tm] mask over the STFT bins")
    B, Fm, Tm = inputs.shape
    if B < 1 or not 1 <= Fm <= NBIN or Tm < 1 or (T is not None and Tm > T):
        raise ValueError(f"inputs must be [B, Fm <= {NBIN}, Tm{'' if T is None else f' <= {T}'}]; got {list(inputs.shape)}")
    return B, Fm, Tm


def check_mask_baselines(baselines, B: int, Fm: int, Tm: int):
    """None (zero), a number, ``[1, Fm, Tm]`` or ``[B, Fm, Tm]`` -> the flat ``[1 | B, Fm * Tm]`` tensor of
    ``check_ig_baselines``."""
    if torch.is_tensor(baselines):
        b = A._float_tensor(baselines, "baselines")
        if b.dim() != 3 or tuple(b.shape[1:]) != (Fm, Tm) or b.shape[0] not in (1, B):
            raise ValueError(f"baselines must be a number, [1, {Fm}, {Tm}] or [{B}, {Fm}, {Tm}]; got {list(b.shape)}")
        baselines = b.reshape(b.shape[0], Fm * Tm)
    return A.check_ig_baselines(baselines, B, Fm * Tm)


def check_mask_distribution(baselines, B: int, Fm: int, Tm: int, n_samples, stdevs):
    """GradientShap's ``[N_b, Fm, Tm]`` baseline distribution -> flat ``[N_b, Fm * Tm]`` (``check_shap_args``)."""
    b = A._float_tensor(baselines, "baselines")
    if b.dim() != 3 or tuple(b.shape[1:]) != (Fm, Tm) or b.shape[0] < 1:
        raise ValueError(f"baselines must be [N_b, {Fm}, {Tm}]; got {list(b.shape)}")
    return A.check_shap_args(b.reshape(b.shape[0], Fm * Tm), B, Fm * Tm, n_samples, stdevs)


def flat_feature_mask(feature_mask, B: int, Fm: int, Tm: int):
    """None or an integer ``[1, Fm, Tm]`` / ``[B, Fm, Tm]`` tensor of feature ids -> the ``[1 | B, Fm * Tm]`` form."""
    if feature_mask is None:
        return None
    if not torch.is_tensor(feature_mask):
        raise ValueError("feature_mask must be a tensor")
    if feature_mask.dim() != 3 or tuple(feature_mask.shape[1:]) != (Fm, Tm) or feature_mask.shape[0] not in (1, B):
        raise ValueError(f"feature_mask must be [1, {Fm}, {Tm}] or [{B}, {Fm}, {Tm}]; got {list(feature_mask.shape)}")
    return feature_mask.reshape(feature_mask.shape[0], Fm * Tm)


def tf_feature_mask(Fm: int, Tm: int, band_bins: int = 64, seg_frames: Optional[int] = None) -> torch.Tensor:
    """Feature ids ``[1, Fm, Tm]`` (int64), one per band of ``band_bins`` bins (64 bins = 1 kHz on ``linspace(0, 8000, 513)``:
    the band-swap generator's bands; bin 512 = 8 kHz is a band of its own) and, with ``seg_frames``, per segment of that many
    frames: ``id = band * n_seg + segment``."""
    Fm, Tm, bw = A._positive_int(Fm, "Fm"), A._positive_int(Tm, "Tm"), A._positive_int(band_bins, "band_bins")
    sw = Tm if seg_frames is None else A._positive_int(seg_frames, "seg_frames")
    ns = -(-Tm // sw)
    return ((torch.arange(Fm) // bw)[:, None] * ns + (torch.arange(Tm) // sw)[None, :])[None]


class Occlusion2dDesc(C.Structure):
    """Mirror of ``advh_occlusion2d_desc`` (include/addvisor_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("base", C.c_void_p), ("B", C.c_int), ("base_rows", C.c_int), ("Fm", C.c_int), ("Tm", C.c_int),
                ("wf", C.c_int), ("wt", C.c_int), ("sf", C.c_int), ("st", C.c_int), ("Kf", C.c_int), ("Kt", C.c_int)]


def occlusion2d_desc(x, base, Fm, Tm, window, stride, K) -> Occlusion2dDesc:
    d = Occlusion2dDesc(x.data_ptr(), base.data_ptr(), x.shape[0], base.shape[0], Fm, Tm, window[0], window[1], stride[0], stride[1],
                        K[0], K[1])
    d.tensors = (x, base)                                                 # kept alive as long as the desc
    return d


def occlusion2d_points(d: Occlusion2dDesc, row0: int, rows: int, out: torch.Tensor) -> None:
    """Occluded rows ``[row0, row0 + rows)`` (window-major ``k * B + b``, rows past ``K * B`` copy x) into ``out [rows, n]``."""
    A._on_gpu(*d.tensors, out)
    _lib.check(_lib.lib().advh_occlusion2d_points(C.byref(d), row0, rows, out.data_ptr(), A._st()), "advh_occlusion2d_points")


def occlusion2d_accumulate(d: Occlusion2dDesc, f0: torch.Tensor, fk: torch.Tensor, attr: torch.Tensor) -> None:
    """``attr [B, Fm * Tm]`` from ``f0 = F(x) [B]`` and ``fk = F(occluded) [Kf * Kt * B]``."""
    A._on_gpu(*d.tensors, f0, fk, attr)
    _lib.check(_lib.lib().advh_occlusion2d_accumulate(C.byref(d), f0.data_ptr(), fk.data_ptr(), attr.data_ptr(), A._st()),
               "advh_occlusion2d_accumulate")


def tf_pool(attr: torch.Tensor, band_bins: int = 64, seg_frames: Optional[int] = None) -> torch.Tensor:
    """``attr [B, Fm, Tm]`` -> ``[B, ceil(Fm / band_bins), ceil(Tm / seg_frames)]``: the sums over boxes of ``band_bins`` bins x
    ``seg_frames`` frames (None: all frames), the last box of an axis cropped -- the per-band, per-segment relevance
    (advh_tf_pool: one fixed-shape tree per box, no atomics)."""
    if not torch.is_tensor(attr) or attr.dim() != 3:
        raise ValueError("attr must be a [B, Fm, Tm] tensor")
    A._on_gpu(attr)
    B, Fm, Tm = attr.shape
    bw = A._positive_int(band_bins, "band_bins")
    sw = Tm if seg_frames is None else A._positive_int(seg_frames, "seg_frames")
    a = attr.to(torch.float32).contiguous()
    out = torch.empty((B, -(-Fm // bw), -(-Tm // sw)), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().advh_tf_pool(a.data_ptr(), B, Fm, Tm, bw, sw, out.data_ptr(), A._st()), "advh_tf_pool")
    return out


class _MaskRows(HipAttribution):
    """The waveform engine with its forward / gradient pair replaced: a row is a flat mask, resynthesised from its clip's
    spectrogram before the embedder and chained through the ISTFT adjoint after the backward.  Shares the embedder, the gradient
    chain and the loss scale of the ``HipAttribution`` it is made from."""

    def __init__(self, att: HipAttribution, owner: "HipSpectralAttribution"):
        self.emb, self.eg, self.loss_scale = att.emb, att.eg, att.loss_scale
        self.neuron_loss_scale, self.precision = att.neuron_loss_scale, att.precision
        self.owner, self.Fm, self.Tm = owner, 0, 0

    def _prep(self, masks: torch.Tensor) -> torch.Tensor:
        return masks.reshape(masks.shape[0], -1).to(self.emb.dev, torch.float32).contiguous()

    def _waves(self, pts, row0, clip_major, S):
        o = self.owner
        m = pts.view(pts.shape[0], self.Fm, self.Tm)
        return m, ops.istft_masked_rows(o.spec, m, o.L, o.domain, row0, clip_major, S, o.hop, o.win)

    def _row_gradient(self, pts, row0=0, clip_major=0, S=1):
        o = self.owner
        m, waves = self._waves(pts, row0, clip_major, S)
        self.eg.forward(waves)
        g = self.eg.backward(self.loss_scale)
        return ops.istft_masked_rows_bwd(g, o.spec, m, o.domain, row0, clip_major, S, o.hop, o.win).view(pts.shape)

    def _row_gradient_seeded(self, pts, seeds_of, row0=0, clip_major=0, S=1):
        """``_row_gradient`` under per-row seeds: ``seeds_of(logits [R]) -> seed [R]`` (device tensors; ``dJ / d logit`` of each
        row) runs between the forward and the backward, and the result is the vector-Jacobian product ``[R, n]`` of the rows."""
        o = self.owner
        m, waves = self._waves(pts, row0, clip_major, S)
        logit = self.eg.forward(waves)[0].view(-1).to(torch.float32)
        g = self.eg.backward(self.loss_scale, seed=seeds_of(logit))
        return ops.istft_masked_rows_bwd(g, o.spec, m, o.domain, row0, clip_major, S, o.hop, o.win).view(pts.shape)

    def _row_logit(self, pts, row0=0, clip_major=0, S=1):
        return self.eg.emb.forward(self._waves(pts, row0, clip_major, S)[1], want_hidden=False)[1].view(-1)


class HipSpectralAttribution:
    """``HipSpectralAttribution(att, waves, domain="linear", hop=322, win=644)``: the mask-domain engine over the clips
    ``waves [B, L]`` (their spectrograms are computed once, here) on the gradient chain of ``att``.  Every method takes a mask
    ``[B, Fm <= 513, Tm <= T]`` and returns an attribution of its shape; see the module docstring for the function attributed
    and for the zero baseline."""

    def __init__(self, att: HipAttribution, waves, domain: str = "linear", hop: int = 322, win: int = 644):
        if domain not in DOMAINS:
            raise ValueError(f"domain must be one of {DOMAINS}, not {domain!r}")
        A._dims(waves)
        self.att, self.domain, self.hop, self.win = att, domain, int(hop), int(win)
        self.waves = att._prep(waves)
        self.B, self.L = self.waves.shape
        self.spec = ops.stft_forward(self.waves, self.L, self.hop, self.win, want_mag=False, want_phase=False)[0]
        self.T = self.spec.shape[2]
        self._rows = _MaskRows(att, self)

    def _enter(self, masks) -> Tuple[int, int, int]:
        B, Fm, Tm = check_mask_inputs(masks, None, self.T)
        if B != self.B:
            raise ValueError(f"the engine holds {self.B} clips; the mask has {B} rows")
        self._rows.Fm, self._rows.Tm = Fm, Tm
        return B, Fm, Tm

    def _full_base(self, baselines, B, Fm, Tm) -> torch.Tensor:
        # F(baseline) depends on the clip: always one baseline row per clip, so that row B + b of cat([x, base]) is clip b's
        base = check_mask_baselines(baselines, B, Fm, Tm)
        return base.to(self.waves.device, torch.float32).expand(B, Fm * Tm).contiguous()

    def logits(self, masks) -> torch.Tensor:
        """``F(m) [B]`` fp32."""
        self._enter(masks)
        return self._rows.logits(self._rows._prep(masks))

    def input_gradient(self, masks) -> torch.Tensor:
        """``dF/dm [B, Fm, Tm]`` fp32."""
        self._enter(masks)
        return self._rows._checked(self._rows.input_gradient(self._rows._prep(masks))).view(masks.shape)

    def saliency(self, masks) -> torch.Tensor:
        self._enter(masks)
        return self._rows.saliency(self._rows._prep(masks)).view(masks.shape)

    def input_x_gradient(self, masks) -> torch.Tensor:
        self._enter(masks)
        return self._rows.input_x_gradient(self._rows._prep(masks)).view(masks.shape)

    def integrated_gradients(self, masks, n_steps: int = 50, internal_batch_size: Optional[int] = None, baselines=None,
                             method: str = "gausslegendre", multiply_by_inputs: bool = True, return_convergence_delta: bool = False):
        """Captum's IntegratedGradients along the straight path of masks from ``baselines`` (None = 0, a number, ``[1, Fm, Tm]``
        or ``[B, Fm, Tm]``) to ``masks``; every rule of ``attribution.METHODS``; ``return_convergence_delta`` adds ``delta [B]``
        with ``F(baseline)`` evaluated on each clip's own spectrogram.  Prefer a mask baseline to the zero mask (module
        docstring): a path point at the zero mask raises FloatingPointError."""
        B, Fm, Tm = self._enter(masks)
        base = self._full_base(baselines, B, Fm, Tm)
        out = self._rows.integrated_gradients(self._rows._prep(masks), n_steps=n_steps, internal_batch_size=internal_batch_size, baselines=base,
                                              method=method, multiply_by_inputs=multiply_by_inputs,
                                              return_convergence_delta=return_convergence_delta)
        if return_convergence_delta:
            return out[0].view(masks.shape), out[1]
        return out.view(masks.shape)

    def gradient_shap(self, masks, baselines, n_samples: int = 5, stdevs: float = 0.0, multiply_by_inputs: bool = True,
                      return_convergence_delta: bool = False, seed: Optional[int] = None, internal_batch_size: Optional[int] = None):
        """Captum's GradientShap with a ``[N_b, Fm, Tm]`` distribution of baseline masks (draws as
        ``HipAttribution.gradient_shap``).  The convergence delta is not computed here."""
        B, Fm, Tm = self._enter(masks)
        if callable(baselines) and not torch.is_tensor(baselines):
            raise NotImplementedError("HipSpectralAttribution.gradient_shap takes a [N_b, Fm, Tm] tensor of baseline masks, not a callable")
        base = check_mask_distribution(baselines, B, Fm, Tm, n_samples, stdevs)
        if return_convergence_delta:
            raise NotImplementedError("HipSpectralAttribution.gradient_shap does not compute the convergence delta")
        return self._rows.gradient_shap(self._rows._prep(masks), base, n_samples=n_samples, stdevs=stdevs, multiply_by_inputs=multiply_by_inputs,
                                        seed=seed, internal_batch_size=internal_batch_size).view(masks.shape)

    def occlusion(self, masks, window, stride=None, baselines=None, internal_batch_size: Optional[int] = None):
        """Captum's Occlusion for the ``(Fm, Tm)`` input: windows ``window = (wf, wt)`` every ``stride = (sf, st)`` (None:
        ``(1, 1)``), cropped at the edges, are replaced by ``baselines``; window ``k = kf * Kt + kt`` is row ``k * B + b``, and
        ``attr[b, f, t]`` is the sum of ``F(m)[b] - F(occluded_k)[b]`` over the windows covering the bin, in increasing k,
        divided by their count -- bit for bit Captum's ``total_attrib / weights`` given the same logits."""
        B, Fm, Tm = self._enter(masks)
        w, s, K = check_occlusion2d_args(Fm, Tm, window, stride)
        base = check_mask_baselines(baselines, B, Fm, Tm)
        chunk = A.check_internal_batch(internal_batch_size)
        x = self._rows._prep(masks)
        d = occlusion2d_desc(x, A._device_base(base, x), Fm, Tm, w, s, K)
        return self._rows._ablate(x, K[0] * K[1] * B, chunk, functools.partial(occlusion2d_points, d),
                                  functools.partial(occlusion2d_accumulate, d), "occlusion",
                                  "a logit of the masks or of their occlusions is not finite (check the inputs and baselines)"
                                  ).view(masks.shape)

    def feature_ablation(self, masks, baselines=None, feature_mask=None, internal_batch_size: Optional[int] = None):
        """Captum's FeatureAblation; ``feature_mask``: None or integer ids ``[1, Fm, Tm]`` / ``[B, Fm, Tm]`` (``tf_feature_mask``)."""
        B, Fm, Tm = self._enter(masks)
        base = check_mask_baselines(baselines, B, Fm, Tm)
        fm = flat_feature_mask(feature_mask, B, Fm, Tm)
        return self._rows.feature_ablation(self._rows._prep(masks), baselines=base, feature_mask=fm,
                                           internal_batch_size=internal_batch_size).view(masks.shape)

    def shapley_value_sampling(self, masks, baselines=None, feature_mask=None, n_samples: int = 25, seed: Optional[int] = None,
                               internal_batch_size: Optional[int] = None):
        """Captum's ShapleyValueSampling over the features of ``feature_mask`` (ids >= 0; draws as the waveform engine's)."""
        B, Fm, Tm = self._enter(masks)
        base = check_mask_baselines(baselines, B, Fm, Tm)
        fm = flat_feature_mask(feature_mask, B, Fm, Tm)
        return self._rows.shapley_value_sampling(self._rows._prep(masks), baselines=base, feature_mask=fm, n_samples=n_samples, seed=seed,
                                                 internal_batch_size=internal_batch_size).view(masks.shape)

    def _curve_args(self, masks, attributions, feature_mask, baselines):
        B, Fm, Tm = self._enter(masks)
        if not torch.is_tensor(attributions) or tuple(attributions.shape) != (B, Fm, Tm):
            raise ValueError(f"attributions must be a [{B}, {Fm}, {Tm}] tensor like the masks")
        base = check_mask_baselines(baselines, B, Fm, Tm)
        # flat views only: the rows engine checks the remaining arguments before it moves anything to the device
        return masks.reshape(B, Fm * Tm), attributions.reshape(B, Fm * Tm), base, flat_feature_mask(feature_mask, B, Fm, Tm)

    def perturbation_curve(self, masks, attributions, mode: str = "deletion", order: str = "morf", feature_mask=None, steps=None,
                           baselines=None, output: str = "prob", use_abs: bool = False, pool: str = "sum", seed: Optional[int] = None,
                           internal_batch_size: Optional[int] = None):
        """``HipAttribution.perturbation_curve`` over the STFT bins: ``attributions [B, Fm, Tm]`` ranks the features of
        ``feature_mask`` (None: every bin; ``tf_feature_mask`` is the natural grouping), and each step's masks are resynthesised
        on their clip's spectrogram.  The zero-mask baseline (``baselines=None``) resynthesises silence, the point the module
        docstring warns about (see "The zero baseline" there): prefer a mask baseline, e.g. a constant 0.5 mask."""
        x, attr, base, fm = self._curve_args(masks, attributions, feature_mask, baselines)
        return self._rows.perturbation_curve(x, attr, mode=mode, order=order, feature_mask=fm, steps=steps, baselines=base, output=output,
                                             use_abs=use_abs, pool=pool, seed=seed, internal_batch_size=internal_batch_size)

    def curve_summary(self, masks, attributions, feature_mask=None, steps=None, baselines=None, use_abs: bool = False, pool: str = "sum",
                      internal_batch_size: Optional[int] = None) -> dict:
        """``HipAttribution.curve_summary`` over the STFT bins; baselines as ``perturbation_curve`` (prefer a mask baseline to the
        zero mask: module docstring)."""
        x, attr, base, fm = self._curve_args(masks, attributions, feature_mask, baselines)
        return self._rows.curve_summary(x, attr, feature_mask=fm, steps=steps, baselines=base, use_abs=use_abs, pool=pool,
                                        internal_batch_size=internal_batch_size)

    def optimize_mask(self, area=0.1, steps: int = 100, cell=(16, 4), shape=None, lam_in: float = 1.0, lam_out: float = 1.0,
                      lam_area: Optional[float] = None, lam_l1: float = 0.0, lam_tv: float = 0.0, reward: str = "log_prob", target=None,
                      optimizer: str = "adam", lr: float = 0.05, momentum: float = 0.9, init=0.5,
                      init_noise: float = MO.DEFAULT_INIT_NOISE, seed: Optional[int] = None, internal_batch_size: Optional[int] = None,
                      trace: Optional[list] = None) -> "MO.MaskOptResult":
        """The per-clip optimised mask (Fong & Vedaldi 2017; Fong, Patrick & Vedaldi 2019; mask_opt.py states the objective):
        "the smallest ``area`` * 100 % of the spectrogram that keeps the decision", solved for each clip of the engine against the
        classifier itself, ``steps`` updates of ``optimizer`` (``"adam"``: torch.optim.Adam's defaults at ``lr``; ``"sgd"``:
        ``momentum``) on a coarse grid of ``cell = (bins, frames)`` cells under the mask ``shape = (Fm, Tm)`` (None: the full
        ``(513, T)``).  ``reward``: ``"logit"``, ``"prob"`` or ``"log_prob"``; ``target``: None (each clip's predicted class, the
        sign of ``F(ones)``) or ``[B]`` labels in {0, 1}; ``lam_area`` defaults to 10 with an area and to 0 without one.

        Scale invariance: in the ``linear`` domain ``F(alpha m) = F(m)``, so a plain L1 penalty shrinks the mask towards the
        silent clip, where the gradient grows as ``1 / alpha`` and the engine raises; the ranked-area constraint pins a share
        ``area`` in (0, 1) of the cells at 1 instead.  ``area=None`` (the 2017 formulation with ``lam_l1`` / ``lam_tv``) is
        accepted only with ``domain="log1p"``; otherwise ValueError, before any device work.

        Ties: the rank breaks ties by index, so from a constant start the area term would push the high-index cells (high
        frequency, late frames) to 1.  ``init`` is a number in (0, 1) or a ``[B, Fc, Tc]`` / ``[B, Fm, Tm]`` tensor of mask values
        (a fine-grid one is box-averaged to the grid: the U-Net's mask, a normalised attribution); ``init_noise`` is the sigma of
        a normal added to theta, drawn once on the host from a ``torch.Generator`` seeded with ``seed``, and defaults to a small
        non-zero value.

        Chunks hold whole clips (at most ``internal_batch_size`` rows, default 128, two rows per clip, at least one clip); the
        clips are independent, so the result does not depend on the chunking.  ``trace``, a list, receives per step the clones
        ``(theta_k, grad_theta_k, logits_k [2B], seeds_k [2B])`` the update read.  One finiteness check at the end:
        FloatingPointError naming ``loss_scale`` instead of a poisoned mask.  Returns a ``MaskOptResult``."""
        return MO.optimize(self, MO.check_mask_opt_args(self.B, self.T, self.domain, area, steps, cell, shape, lam_in, lam_out, lam_area,
                                                        lam_l1, lam_tv, reward, target, optimizer, lr, momentum, init, init_noise, seed,
                                                        internal_batch_size, trace))

    def pool(self, attr, band_bins: int = 64, seg_frames: Optional[int] = None) -> torch.Tensor:
        """``tf_pool``: the per-band (x per-segment) relevance of an attribution map."""
        return tf_pool(attr, band_bins, seg_frames)


def _not_here(name):
    def method(self, *args, **kwargs):
        raise NotImplementedError(f"HipSpectralAttribution does not implement {name} over STFT masks; it offers logits, saliency, "
                                  "input_x_gradient, integrated_gradients, gradient_shap, occlusion, feature_ablation, "
                                  "shapley_value_sampling, optimize_mask and pool")
    method.__name__ = name
    return method


for _name in ("kernel_shap", "lime", "feature_permutation", "shapley_values", "noise_tunnel", "infidelity", "sensitivity_max"):
    setattr(HipSpectralAttribution, _name, _not_here(_name))
