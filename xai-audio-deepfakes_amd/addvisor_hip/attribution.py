"""Gradient attributions of the waveform -> logit classifier on the HIP backward path: the semantics of
``captum.attr.Saliency / InputXGradient / IntegratedGradients / GradientShap`` as the reference calls them
(captum_saliency.py:3, 116-118, 131-143; Captum defaults: ``abs=True``; IG ``n_steps=50``,
``method="gausslegendre"``, zero baseline, ``multiply_by_inputs=True``, scaled inputs concatenated step-major;
GradientShap ``n_samples=5``, ``stdevs=0.0``, expanded inputs clip-major).

IntegratedGradients is path-batched: the ``n_steps * B`` interpolation points are pushed through one
forward + dgrad-only backward in chunks of ``internal_batch_size`` rows (whole steps per chunk).  The path points and the
weighted, baseline-aware sums of every baseline, rule and option (the default zero baseline included) run on
csrc/attribution_paths.hip, in one loop that the layer and neuron path methods share (``_integrate_path``); so does
GradientShap, whose Gaussian input noise comes from the same counter-based generator (``philox_normal``) on the device.

The perturbation attributions ``captum.attr.Occlusion / FeatureAblation`` need no gradient: the ablated batch is built on the
device (csrc/attribution_ablation.hip), pushed through the classifier forward in chunks, and the logit differences are
accumulated in Captum's order by one launch.  The Shapley attributions ``captum.attr.ShapleyValueSampling / ShapleyValues /
KernelShap`` build coalition rows the same way (csrc/attribution_shapley.hip): marginal contributions along permutations are
accumulated on the device in Captum's order; KernelShap's per-clip weighted regression is a host float64 solve whose
coefficients a kernel scatters back to the samples.  ``captum.attr.Lime`` reuses KernelShap's coalition rows with Bernoulli(0.5)
draws; the similarity weight of every row is reduced on the device from the chunk the forward reads, and each clip's
interpretable model (a weighted Lasso by default, addvisor_hip.linear_model) is fitted on the host.  ``captum.attr.FeaturePermutation``
builds FeatureAblation's rows with each feature taken from another clip of the batch (csrc/attribution_lime.hip).

``captum.attr.NoiseTunnel`` wraps any of them (``noise_tunnel``): the noisy rows of each partition of samples come from the same
counter-based generator through the path-point kernel, the wrapped method attributes them, and the first and second moments are
folded in fp64 on the device (csrc/attribution_paths.hip).

The layer methods (``captum.attr.Layer*``, ``InternalInfluence``) attribute to ``hidden_states[l]`` on the chain started and
stopped at a layer (csrc/attribution_layer.hip); the neuron methods (``captum.attr.Neuron*``) attribute one unit, or one band of
units, of ``hidden_states[l]`` to the waveform on the forward stopped at the layer and the backward started there from a seed
(csrc/attribution_neuron.hip), reusing the path, draw and ablation helpers above.

``captum.metrics.infidelity`` / ``sensitivity_max`` score any of them (``infidelity``, ``sensitivity_max``): the perturbed rows
of each chunk of samples come from the same counter-based generator (or a Python perturb_func), and the per-row dot products,
norms and per-clip folds run on csrc/attribution_metrics.hip.

``perturbation_curve`` / ``curve_summary`` rank any of them on the scale the attribution literature uses: the deletion /
insertion curves of Petsiuk et al. (2018) and the AOPC of Samek et al. (2017) in MoRF / LeRF / random order (restated from the
papers; there is no Captum class).  Per-clip feature scores, a stable rank, the curve rows and the curve fold run on
csrc/attribution_curve.hip; the rows go through the same forward seam as the perturbation attributions.
"""
from __future__ import annotations

import ctypes as C
import functools
import inspect
import itertools
import math
import warnings
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .embedder import HipEmbedder
from .embedder_grad import EmbedderGrad, LrpRules, check_layer  # noqa: F401  (check_layer(layer, nl): the Layer* methods' layer check)


def _st():
    return torch.cuda.current_stream().cuda_stream


def gauss_legendre(n_steps: int) -> Tuple[np.ndarray, np.ndarray]:
    """Captum's ``gausslegendre`` rule: alphas = (1 + x) / 2, step sizes = w / 2."""
    x, w = np.polynomial.legendre.leggauss(n_steps)
    return 0.5 * (1.0 + x), 0.5 * w


METHODS = ("gausslegendre", "riemann_left", "riemann_right", "riemann_middle", "riemann_trapezoid")


def approximation(method: str, n_steps: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(alphas, step_sizes)`` of Captum's ``approximation_methods`` (restated: captum is absent).  Riemann rules need
    ``n_steps > 1``: step sizes ``1/n`` each (the first and last halved for the trapezoid), alphas ``linspace(0, 1, n)``
    (trapezoid), ``linspace(0, 1 - 1/n, n)`` (left), ``linspace(1/(2n), 1 - 1/(2n), n)`` (middle), ``linspace(1/n, 1, n)``
    (right)."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    if method == "gausslegendre":
        return gauss_legendre(n_steps)
    n = int(n_steps)
    if n <= 1:
        raise ValueError("Riemann rules need n_steps > 1")
    steps = np.full(n, 1.0 / n)
    if method == "riemann_trapezoid":
        steps[0] /= 2
        steps[-1] /= 2
        return np.linspace(0.0, 1.0, n), steps
    lo, hi = {"riemann_left": (0.0, 1.0 - 1.0 / n), "riemann_middle": (1.0 / (2 * n), 1.0 - 1.0 / (2 * n)),
              "riemann_right": (1.0 / n, 1.0)}[method]
    return np.linspace(lo, hi, n), steps


def shap_draws(seed: int, B: int, S: int, n_base: int) -> Tuple[np.ndarray, np.ndarray]:
    """GradientShap's host-side draws for ``B`` clips x ``S`` samples, clip-major (expanded row ``b * S + s``):
    baseline indices ``[B*S]`` int32 uniform in ``[0, n_base)``, then path coefficients ``[B*S]`` float32 uniform in
    ``[0, 1)``, both from ``numpy.random.Generator(PCG64(seed))``.  Captum draws from its own RNG stream, which is not
    reproduced (captum is absent); the distributions are the same."""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    idx = rng.integers(0, n_base, size=B * S, dtype=np.int32)
    alpha = rng.random(B * S, dtype=np.float32)
    return idx, alpha


def draw_seed() -> int:
    """One 63-bit seed from torch's default CPU generator: ``torch.manual_seed`` reproduces a GradientShap run."""
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())


HEAD_FUSIONS = {None: 0, "mean": 1, "max": 2, "min": 3}    # advh_attention_maps' fuse codes


def check_head_fusion(head_fusion, allow_none: bool = True) -> int:
    """``head_fusion`` of the attention methods as advh_attention_maps' ``fuse`` code.  Raises ValueError."""
    ok = (None, "mean", "max", "min") if allow_none else ("mean", "max", "min")
    if not (head_fusion is None or isinstance(head_fusion, str)) or head_fusion not in ok:
        raise ValueError(f"head_fusion must be one of {ok}, not {head_fusion!r}")
    return HEAD_FUSIONS[head_fusion]


def check_attention_target(target, B: int):
    """``target`` of the gradient-weighted attention methods: None or 1 explains ``+F``, 0 explains ``-F``, ``"predicted"``
    explains ``sign(F(x_b)) F`` per clip, a ``[B]`` tensor of 0 / 1 picks per clip.  Returns None (``+F``), ``"predicted"`` or
    the per-clip signs ``[B]`` (fp32, on the CPU).  Raises ValueError."""
    if target is None:
        return None
    if isinstance(target, str):
        if target != "predicted":
            raise ValueError(f"target must be None, 0, 1, 'predicted' or a [B] tensor of 0 / 1, not {target!r}")
        return target
    if torch.is_tensor(target):
        t = target.detach().cpu()
        if t.dtype == torch.bool or t.dim() != 1 or t.shape[0] != B or not bool(((t == 0) | (t == 1)).all()):
            raise ValueError(f"a target tensor must be [{B}] with values 0 / 1")
        return t.to(torch.float32) * 2.0 - 1.0
    if isinstance(target, bool) or not isinstance(target, (int, np.integer)) or target not in (0, 1):
        raise ValueError(f"target must be None, 0, 1, 'predicted' or a [B] tensor of 0 / 1, not {target!r}")
    return None if target == 1 else torch.full((B,), -1.0)


def _dims(waves) -> Tuple[int, int]:
    if not torch.is_tensor(waves) or waves.dim() not in (1, 2):
        raise ValueError("waves must be a [B, L] (or [L]) tensor")
    return (1, waves.shape[0]) if waves.dim() == 1 else tuple(waves.shape)


def _float_tensor(t, what):
    if not torch.is_tensor(t):
        raise ValueError(f"{what} must be a tensor")
    if not t.is_floating_point():
        raise ValueError(f"{what} must be a floating-point tensor, not {t.dtype}")
    return t


def check_ig_baselines(baselines, B: int, L: int):
    """IntegratedGradients baselines: None (zero), a number, a ``[1, L]`` or a ``[B, L]`` floating tensor.  Returns a
    ``[1, L]`` / ``[B, L]`` tensor (on the host for a number).  Raises ValueError before any GPU work."""
    if baselines is None:
        baselines = 0.0
    if isinstance(baselines, (int, float)) and not isinstance(baselines, bool):
        return torch.full((1, L), float(baselines))
    b = _float_tensor(baselines, "baselines")
    if b.dim() != 2 or b.shape[1] != L or b.shape[0] not in (1, B):
        raise ValueError(f"baselines must be a number, [1, {L}] or [{B}, {L}]; got {list(b.shape)}")
    return b


def check_shap_args(baselines, B: int, L: int, n_samples: int, stdevs: float):
    """GradientShap arguments: a ``[N_b, L]`` floating baseline distribution (N_b >= 1), ``n_samples >= 1``,
    ``stdevs >= 0``.  Raises ValueError before any GPU work."""
    b = _float_tensor(baselines, "baselines")
    if b.dim() != 2 or b.shape[1] != L or b.shape[0] < 1:
        raise ValueError(f"baselines must be [N_b, {L}]; got {list(b.shape)}")
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or n_samples < 1:
        raise ValueError("n_samples must be an integer >= 1")
    if not isinstance(stdevs, (int, float)) or not np.isfinite(stdevs) or stdevs < 0:
        raise ValueError("stdevs must be a finite number >= 0")
    return b


def occlusion_windows(L: int, win: int, stride: int) -> int:
    """Captum's Occlusion shift count: ``K = ceil((L - win) / stride) + 1`` windows; window k covers
    ``[k * stride, min(k * stride + win, L))``."""
    return -(-(L - win) // stride) + 1


def _positive_int(v, what) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{what} must be an integer >= 1, not {v!r}")
    return int(v)


def _one_dim(v, what) -> int:
    """An int or a 1-tuple of ints (Captum passes one shape per input dimension; the input here is ``[B, L]``)."""
    if isinstance(v, (tuple, list)):
        if len(v) != 1:
            raise ValueError(f"{what} must have one entry (the time dimension), not {len(v)}")
        v = v[0]
    return _positive_int(v, what)


def check_occlusion_args(L: int, window, stride=None) -> Tuple[int, int, int]:
    """Occlusion's window and stride (an int or a 1-tuple; ``stride=None`` is 1) -> ``(win, stride, K)``.  Raises ValueError
    before any GPU work on Captum's assertions: ``win <= L``, and ``stride <= win`` unless ``win == L``."""
    win = _one_dim(window, "sliding_window_shapes")
    stride = 1 if stride is None else _one_dim(stride, "strides")
    if win > L:
        raise ValueError(f"the occlusion window ({win}) is longer than the input ({L})")
    if stride > win and win != L:
        raise ValueError(f"the stride ({stride}) exceeds the window ({win}): samples between windows would be skipped")
    return win, stride, occlusion_windows(L, win, stride)


def check_internal_batch(internal_batch_size) -> int:
    """Rows per forward of the perturbation attributions (default 128)."""
    return 128 if internal_batch_size is None else _positive_int(internal_batch_size, "internal_batch_size")


def feature_indices(feature_mask, B: int, L: int) -> Tuple[torch.Tensor, int]:
    """FeatureAblation's ``feature_mask``: None (every sample its own feature) or an integer ``[1, L]`` / ``[B, L]`` tensor of
    feature ids.  Returns ``(index, K)``: ``index`` int32 on the host, same shape, the rank of each sample's id among the ids
    present (increasing id order, so ``id - id_min`` for contiguous ids), and K the number of ids present.  Captum up to 0.7
    also ablates the absent ids of ``[min, max]``; no sample takes their attribution, so skipping them changes nothing.  Raises
    ValueError before any GPU work on a non-integer mask, a wrong shape or an id range wider than int32."""
    if feature_mask is None:
        return torch.arange(L, dtype=torch.int32)[None], L
    if not torch.is_tensor(feature_mask):
        raise ValueError("feature_mask must be a tensor")
    if feature_mask.is_floating_point() or feature_mask.is_complex() or feature_mask.dtype == torch.bool:
        raise ValueError(f"feature_mask must be an integer tensor, not {feature_mask.dtype}")
    if feature_mask.dim() != 2 or feature_mask.shape[1] != L or feature_mask.shape[0] not in (1, B):
        raise ValueError(f"feature_mask must be [1, {L}] or [{B}, {L}]; got {list(feature_mask.shape)}")
    m = feature_mask.detach().to("cpu", torch.int64)
    if int(m.max()) - int(m.min()) > 2 ** 31 - 1:
        raise ValueError("the feature ids of feature_mask span more than the int32 range")
    ids, index = torch.unique(m, sorted=True, return_inverse=True)
    return index.to(torch.int32).reshape(m.shape), ids.numel()


def _nonnegative_ids(feature_mask):
    if torch.is_tensor(feature_mask) and feature_mask.numel() and not (feature_mask.is_floating_point() or feature_mask.is_complex()
                                                                       or feature_mask.dtype == torch.bool):
        if int(feature_mask.min()) < 0:
            raise ValueError("the Shapley attributions take feature ids >= 0 (Captum would leave a negative id at the baseline)")


def shapley_feature_indices(feature_mask, B: int, L: int) -> Tuple[torch.Tensor, int]:
    """``feature_indices`` for ShapleyValueSampling / ShapleyValues: the K ids present in the whole mask are the features;
    negative ids raise ValueError (Captum's Shapley methods take ids in ``[0, max]``)."""
    _nonnegative_ids(feature_mask)
    return feature_indices(feature_mask, B, L)


def per_clip_feature_indices(feature_mask, B: int, L: int) -> Tuple[torch.Tensor, list]:
    """The features of each clip on its own: returns ``(index, Ks)``, ``index`` int32 ``[1, L]`` (a None or ``[1, L]`` mask: the
    same features in every clip) or ``[B, L]``, the rank of each sample's id among the ids present in its clip, and ``Ks`` the
    number of those ids per clip.  Any integer id is a feature (``feature_indices`` checks the mask)."""
    index, K = feature_indices(feature_mask, B, L)
    if index.shape[0] == 1:
        return index, [K] * B
    rows = [torch.unique(m, sorted=True, return_inverse=True) for m in index]
    return torch.stack([inv.to(torch.int32) for _, inv in rows]), [ids.numel() for ids, _ in rows]


def kernel_shap_feature_indices(feature_mask, B: int, L: int) -> Tuple[torch.Tensor, list]:
    """KernelShap's features, per clip (each clip is fitted on its own): ``per_clip_feature_indices``.  Raises ValueError on
    negative ids or a clip with fewer than two features (the regression needs two)."""
    _nonnegative_ids(feature_mask)
    index, Ks = per_clip_feature_indices(feature_mask, B, L)
    if min(Ks) < 2:
        raise ValueError(f"KernelShap needs at least two features per clip; feature_mask gives {min(Ks)}")
    return index, Ks


def check_n_samples(n_samples, least: int = 1) -> int:
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or n_samples < least:
        raise ValueError(f"n_samples must be an integer >= {least}, not {n_samples!r}")
    return int(n_samples)


def _check_seed(seed) -> int:
    seed = draw_seed() if seed is None else int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2**64)")
    return seed


def _check_delta(return_convergence_delta, multiply_by_inputs) -> None:
    if return_convergence_delta and not multiply_by_inputs:
        raise NotImplementedError("the convergence delta needs multiply_by_inputs=True")


def _device_base(base: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """A checked baseline (or baseline distribution) as contiguous fp32 rows on the device of ``x``."""
    return base.to(x.device, torch.float32).contiguous()


def _permutation_stream(seed: int):
    """``rng.random((P, K))`` rows ranked, group by group: ``next_ranks(P, K)`` continues the stream, so drawing P permutations
    at once or in groups gives the same ones."""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    return lambda P, K: np.argsort(np.argsort(rng.random((P, K)), axis=1, kind="stable"), axis=1, kind="stable").astype(np.int32)


def shapley_permutations(seed: int, P: int, K: int) -> np.ndarray:
    """ShapleyValueSampling's host draws: ``P`` uniform permutations of the K features from
    ``numpy.random.Generator(PCG64(seed))``, as an int32 rank table ``[P, K]`` (``rank[p][k]``: the step at which permutation p
    switches feature k; the permutation itself is ``argsort(rank[p])``).  Captum draws ``torch.randperm`` from its own
    stream, which is not reproduced; the distribution is the same."""
    return _permutation_stream(seed)(P, K)


def exact_permutation_stream(K: int):
    """ShapleyValues' permutations: ``next_ranks(G)`` is the int32 rank table ``[G, K]`` of the next G of
    ``itertools.permutations(range(K))`` (``rank[p][perm[p][j]] = j``), so the K! permutations are never held at once."""
    perms = itertools.permutations(range(K))

    def next_ranks(G):
        p = np.array(list(itertools.islice(perms, G)), dtype=np.int32).reshape(-1, K)
        rank = np.empty_like(p)
        np.put_along_axis(rank, p, np.arange(K, dtype=np.int32)[None], axis=1)
        return rank
    return next_ranks


def kernel_shap_probs(K: int) -> np.ndarray:
    """The coalition size law of Captum's ``kernel_shap_perturb_generator``: ``p(k) = (K - 1) / (k (K - k))``, k = 1 .. K - 1,
    normalised."""
    k = np.arange(1, K, dtype=np.float64)
    w = (K - 1) / (k * (K - k))
    return w / w.sum()


def kernel_shap_draws(seed: int, Ks, S: int) -> list:
    """KernelShap's host draws: per clip (in order, one ``numpy.random.Generator(PCG64(seed))``) ``S`` binary coalitions
    ``uint8 [S, K_b]``: all ones, all zeros, then for each further row a size k in ``[1, K_b - 1]`` drawn with
    ``kernel_shap_probs`` and a uniform k-subset (the k smallest of K_b uniform draws).  Captum's stream is not reproduced."""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    out = []
    for K in Ks:
        z = np.zeros((S, K), np.uint8)
        z[0] = 1
        if S > 2:
            k = rng.choice(np.arange(1, K), size=S - 2, p=kernel_shap_probs(K))
            order = np.argsort(np.argsort(rng.random((S - 2, K)), axis=1, kind="stable"), axis=1, kind="stable")
            z[2:] = order < k[:, None]
        out.append(z)
    return out


def kernel_shap_weights(z: np.ndarray) -> np.ndarray:
    """Captum's ``kernel_shap_similarity_kernel`` on drawn coalitions: 1e6 for the all-zero and all-one rows, 1 otherwise (the
    size law already carries the Shapley kernel)."""
    n = z.sum(1)
    return np.where((n == 0) | (n == z.shape[1]), 1e6, 1.0)


def kernel_shap_fit(z: np.ndarray, y: np.ndarray) -> Tuple[np.ndarray, float]:
    """One clip's KernelShap regression: ``weighted_linear_fit`` with the weights of ``kernel_shap_weights``."""
    return weighted_linear_fit(z, y, kernel_shap_weights(z))


def weighted_linear_fit(z: np.ndarray, y: np.ndarray, w: np.ndarray) -> Tuple[np.ndarray, float]:
    """A weighted linear regression with intercept, as sklearn's ``LinearRegression().fit(z, y, sample_weight=w)`` (Captum's
    ``SkLearnLinearRegression``): centre z and y by their weighted means, scale the rows by sqrt(w), min-norm ``lstsq`` in
    float64, intercept = mean(y) - mean(z) . coef.  Returns ``(coef [K] float64, intercept)``."""
    X = np.asarray(z).astype(np.float64)
    y = np.asarray(y, np.float64)
    w = np.asarray(w, np.float64)
    xm = np.average(X, axis=0, weights=w)
    ym = np.average(y, weights=w)
    sw = np.sqrt(w)
    coef = np.linalg.lstsq((X - xm) * sw[:, None], (y - ym) * sw, rcond=None)[0]
    return coef, float(ym - xm @ coef)


def lime_draws(seed: int, Ks, S: int) -> list:
    """Lime's default draws (Captum's ``default_perturb_func``, Bernoulli(0.5) per feature): per clip (in order, one
    ``numpy.random.Generator(PCG64(seed))``) ``uint8 [S, K_b]`` = ``rng.random((S, K_b)) < 0.5``; no forced all-on or all-off
    rows.  Captum's stream is not reproduced."""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    return [(rng.random((S, K)) < 0.5).astype(np.uint8) for K in Ks]


def feature_permutation_draws(seed: int, K: int, B: int) -> np.ndarray:
    """FeaturePermutation's draws: ``int32 [K, B]``, row k a uniform permutation of the B clips that is not the identity
    (Captum's rejection loop in ``_permute_feature``), from ``numpy.random.Generator(PCG64(seed))``: all K drawn as
    ``argsort(rng.random((K, B)))``, then the identity rows drawn again, in feature order, until none is left.  Captum's stream
    is not reproduced."""
    if B < 2:
        raise ValueError("FeaturePermutation permutes the clips of the batch: it needs at least two")
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    ident = np.arange(B)
    perm = np.argsort(rng.random((K, B)), axis=1, kind="stable")
    same = (perm == ident).all(1)
    while same.any():
        perm[same] = np.argsort(rng.random((int(same.sum()), B)), axis=1, kind="stable")
        same = (perm == ident).all(1)
    return perm.astype(np.int32)


def check_permutation_args(feature_mask, B: int, L: int) -> Tuple[torch.Tensor, int]:
    """FeaturePermutation's input rules, Captum's asserts raised as ValueError before any GPU work: ``B >= 2``; ``feature_mask``
    None or one ``[1, L]`` integer mask for every clip.  Returns ``feature_indices``' ``(index [1, L], K)``."""
    if B < 2:
        raise ValueError("FeaturePermutation permutes the clips of the batch: it needs at least two")
    if torch.is_tensor(feature_mask) and feature_mask.dim() == 2 and feature_mask.shape[0] != 1:
        raise ValueError("FeaturePermutation takes one [1, L] feature_mask (the same features permuted in every clip), "
                         f"not {list(feature_mask.shape)}")
    return feature_indices(feature_mask, B, L)


def check_steps(n_steps, method: str, least: int = 1) -> int:
    """``n_steps`` and ``method`` of the path methods: an integer >= ``least`` and one of ``METHODS`` (ValueError)."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < least:
        raise ValueError(f"n_steps must be an integer >= {least}, not {n_steps!r}")
    return int(n_steps)


def check_layer_path_args(layer, nl: int, baselines, B: int, L: int, n_steps, method: str, internal_batch_size=None,
                          extra_point: bool = False):
    """The arguments of LayerIntegratedGradients / LayerConductance / InternalInfluence, before any GPU work (ValueError):
    ``check_layer``; waveform-space ``baselines`` as ``check_ig_baselines``; ``n_steps`` and ``method`` as ``check_steps`` --
    the rule is evaluated at ``n_steps`` points, ``n_steps + 1`` with ``extra_point`` (LayerConductance), and a Riemann rule
    needs more than one; ``internal_batch_size`` None or an integer >= 1.  Returns ``(layer, baselines [1|B, L], alphas,
    step_sizes)``."""
    l = check_layer(layer, nl)
    base = check_ig_baselines(baselines, B, L)
    n = check_steps(n_steps, method) + int(extra_point)
    alphas, steps = approximation(method, n)
    if internal_batch_size is not None:
        _positive_int(internal_batch_size, "internal_batch_size")
    return l, base, alphas, steps


def _selector_axis(sel, dim: int, what: str) -> Tuple[int, int, int]:
    if isinstance(sel, slice):
        for v in (sel.start, sel.stop, sel.step):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
                raise ValueError(f"neuron_selector: the {what} slice must have integer bounds and step, not {sel!r}")
        step = 1 if sel.step is None else int(sel.step)
        if step <= 0:
            raise ValueError(f"neuron_selector: the {what} slice needs a step >= 1, not {sel!r}")
        lo, hi, _ = slice(sel.start, sel.stop, step).indices(dim)          # negative and open bounds as in Python
        if lo >= hi:
            raise ValueError(f"neuron_selector: the {what} slice {sel!r} selects nothing of {dim}")
        return lo, hi, step
    if isinstance(sel, bool) or not isinstance(sel, (int, np.integer)):
        raise ValueError(f"neuron_selector: the {what} entry must be an int or a slice, not {sel!r}")
    i = int(sel) + (dim if sel < 0 else 0)
    if not 0 <= i < dim:
        raise ValueError(f"neuron_selector: {what} index {int(sel)} is out of range for {dim}")
    return i, i + 1, 1


def check_neuron_selector(selector, T: int, H: int) -> Tuple[int, int, int, int, int, int]:
    """``neuron_selector`` of the ``captum.attr.Neuron*`` methods over the ``[T, H]`` frame of ``hidden_states[l]``: a ``(t, h)``
    tuple of ints or slices.  Negative indices and open or negative slice bounds behave as in Python; a slice is half-open with
    a step >= 1, and several selected units are aggregated by sum, as Captum does.  Returns the selection box
    ``(t0, t1, tstep, h0, h1, hstep)`` of advh_layer_seed / advh_neuron_values (an int ``i`` is ``(i, i + 1, 1)``).  A bare int, a
    wrong arity, a step <= 0, an empty slice and an index out of range raise ValueError; a callable selector raises
    NotImplementedError."""
    if callable(selector):
        raise NotImplementedError("a callable neuron_selector is not supported (HIP build): pass a (t, h) tuple of ints or slices")
    if not isinstance(selector, (tuple, list)) or len(selector) != 2:
        raise ValueError(f"neuron_selector must be a (t, h) tuple of ints or slices into the [{T}, {H}] frame, not {selector!r}")
    return _selector_axis(selector[0], T, "frame") + _selector_axis(selector[1], H, "channel")


def frame_index(L: int, T: int, hop: int = 320) -> np.ndarray:
    """The encoder frame of each waveform sample: sample j belongs to frame ``min(j // hop, T - 1)`` (``hop``: the product of
    the feature encoder's strides, 320 for wav2vec2; the samples behind the last whole hop go to the last frame).  int64 ``[L]``."""
    if L < 1 or T < 1 or hop < 1:
        raise ValueError("frame_index needs L, T and hop >= 1")
    return np.minimum(np.arange(L, dtype=np.int64) // hop, T - 1)


SIM_MODES = ("cosine", "euclidean")                                    # advh_row_similarity's mode = the index


def check_kernel(distance_mode, kernel_width) -> Tuple[int, float]:
    """Captum's ``get_exp_kernel_similarity_function`` arguments -> ``(mode, width)``: ``distance_mode`` "cosine" or
    "euclidean", ``kernel_width`` a finite number > 0.  Raises ValueError."""
    if distance_mode not in SIM_MODES:
        raise ValueError(f"distance_mode must be 'cosine' or 'euclidean', not {distance_mode!r}")
    if isinstance(kernel_width, bool) or not isinstance(kernel_width, (int, float, np.integer, np.floating)) \
            or not np.isfinite(kernel_width) or not 0 < kernel_width <= float(np.finfo(np.float32).max):
        raise ValueError(f"kernel_width must be a finite number > 0, not {kernel_width!r}")
    return SIM_MODES.index(distance_mode), float(kernel_width)


class ExpKernelSimilarity:
    """Captum's ``get_exp_kernel_similarity_function(distance_mode, kernel_width)``: ``exp(-d^2 / (2 w^2))`` between the clip
    and a perturbed row, ``d = 1 - cos`` (``torch.nn.CosineSimilarity(dim=0)``: each norm clamped at 1e-8) or ``||x - v||_2``.
    ``lime`` recognises it and computes the weights on the device (advh_row_similarity, fp64 sums); called directly it is
    Captum's function, in torch on the inputs' device."""

    def __init__(self, distance_mode: str = "cosine", kernel_width: float = 1.0):
        check_kernel(distance_mode, kernel_width)
        self.distance_mode, self.kernel_width = distance_mode, kernel_width

    def __call__(self, original_inp, perturbed_inp, interpretable_sample=None, **kwargs) -> float:
        a = original_inp.reshape(-1).float()
        v = perturbed_inp.reshape(-1).float()
        if self.distance_mode == "cosine":
            d = 1 - torch.nn.CosineSimilarity(dim=0)(a, v)
        else:
            d = torch.norm(a - v)
        return math.exp(-1 * float(d) ** 2 / (2 * self.kernel_width ** 2))

    def __repr__(self):
        return f"ExpKernelSimilarity(distance_mode={self.distance_mode!r}, kernel_width={self.kernel_width!r})"


def check_lime_callables(similarity_func, perturb_func, interpretable_model):
    """Lime's pluggable parts, checked before any GPU work (ValueError): a callable ``similarity_func`` (an
    ``ExpKernelSimilarity`` with a valid mode and width), a plain callable ``perturb_func`` -- a generator function is refused --
    and an ``interpretable_model`` with ``fit`` and ``representation``.  None stands for the default of each."""
    if similarity_func is not None:
        if not callable(similarity_func):
            raise ValueError("similarity_func must be callable")
        if isinstance(similarity_func, ExpKernelSimilarity):
            check_kernel(similarity_func.distance_mode, similarity_func.kernel_width)
    if perturb_func is not None:
        if not callable(perturb_func):
            raise ValueError("perturb_func must be callable")
        if inspect.isgeneratorfunction(perturb_func) or inspect.isgeneratorfunction(getattr(perturb_func, "__call__", None)):
            raise ValueError("perturb_func must return one interpretable sample per call, not be a generator function")
    if interpretable_model is not None and not (callable(getattr(interpretable_model, "fit", None))
                                                and callable(getattr(interpretable_model, "representation", None))):
        raise ValueError("interpretable_model must have fit(DataLoader) and representation()")


NT_TYPES = ("smoothgrad", "smoothgrad_sq", "vargrad")                 # advh_nt_finalize's nt_type = the index


def check_noise_tunnel_args(nt_type, nt_samples, nt_samples_batch_size=None, stdevs=1.0, target=None) -> Tuple[int, int, float]:
    """NoiseTunnel's own arguments -> ``(S, p, stdevs)``: ``S = nt_samples >= 1``, partitions of ``p = min(S,
    nt_samples_batch_size or S)`` samples, ``stdevs`` a finite number >= 0 (or a 1-tuple of one: the input is a single
    tensor).  ``target`` must be None (one output).  Raises ValueError before any GPU work."""
    if nt_type not in NT_TYPES:
        raise ValueError(f"nt_type must be one of {NT_TYPES}, not {nt_type!r}")
    S = _positive_int(nt_samples, "nt_samples")
    p = S if nt_samples_batch_size is None else min(S, _positive_int(nt_samples_batch_size, "nt_samples_batch_size"))
    if isinstance(stdevs, (tuple, list)):
        if len(stdevs) != 1:
            raise ValueError(f"stdevs must be a number or a 1-tuple (one input tensor), not {len(stdevs)} entries")
        stdevs = stdevs[0]
    if isinstance(stdevs, bool) or not isinstance(stdevs, (int, float, np.integer, np.floating)) or not np.isfinite(stdevs) \
            or stdevs < 0:
        raise ValueError(f"stdevs must be a finite number >= 0, not {stdevs!r}")
    if target is not None:
        raise ValueError("the classifier has a single output; target must be None")
    return S, p, float(stdevs)


def noise_tunnel_partitions(S: int, p: int) -> list:
    """Captum's partition loop: ``S // p`` partitions of p samples, then one of ``S % p`` if non-zero, as ``[(s0, p'), ...]``."""
    return [(s0, min(p, S - s0)) for s0 in range(0, S, p)]


def noise_tunnel_rows(B: int, S: int, s0: int, pp: int) -> np.ndarray:
    """The global (clip, sample) index ``g = b * S + s0 + s'`` of each row ``b * pp + s'`` of the partition ``[s0, s0 + pp)``:
    the noise counter of the row, and its entry in ``noise_tunnel_baseline_draws``."""
    return (np.arange(B)[:, None] * S + s0 + np.arange(pp)[None]).reshape(-1)


def noise_tunnel_baseline_draws(seed: int, B: int, S: int, n_base: int) -> np.ndarray:
    """``draw_baseline_from_distrib=True``: the baseline row of each (clip, sample) ``b * S + s``, drawn up front as
    ``numpy.random.Generator(PCG64(seed)).integers(0, n_base, B * S)``.  Captum's stream is not reproduced."""
    return np.random.Generator(np.random.PCG64(int(seed))).integers(0, n_base, B * S)


def check_baseline_distribution(baselines, L: int):
    """``draw_baseline_from_distrib=True`` needs ``baselines``, a floating ``[N_b, L]`` tensor (N_b >= 1)."""
    b = _float_tensor(baselines, "baselines (draw_baseline_from_distrib=True)")
    if b.dim() != 2 or b.shape[1] != L or b.shape[0] < 1:
        raise ValueError(f"draw_baseline_from_distrib=True takes baselines [N_b, {L}]; got {list(b.shape)}")
    return b


def noise_tunnel_kwargs(kwargs: dict, B: int, pp: int, drawn_rows=None) -> dict:
    """The wrapped method's arguments for a partition of ``pp`` samples, Captum's expansion: ``baselines`` ->
    ``baselines[drawn_rows]`` when drawn from the distribution (``drawn_rows``: the partition's indices), else a tensor with
    first dimension ``B > 1`` is ``repeat_interleave``d by pp; ``feature_mask`` with first dimension > 1 is
    ``repeat_interleave``d; everything else passes unchanged."""
    kw = dict(kwargs)
    base = kw.get("baselines")
    if drawn_rows is not None:
        kw["baselines"] = base[torch.as_tensor(drawn_rows, dtype=torch.long, device=base.device)]
    elif torch.is_tensor(base) and base.dim() >= 1 and base.shape[0] == B and B > 1:
        kw["baselines"] = base.repeat_interleave(pp, 0)
    mask = kw.get("feature_mask")
    if torch.is_tensor(mask) and mask.dim() >= 1 and mask.shape[0] > 1:
        kw["feature_mask"] = mask.repeat_interleave(pp, 0)
    return kw


def nt_noisy_rows(x: torch.Tensor, seed: int, S: int, s0: int, pp: int, stdevs: float, out: Optional[torch.Tensor] = None):
    """The partition's ``[B * pp, L]`` rows ``x[b] + stdevs * N(seed, b * S + s0 + s', :)`` (row ``b * pp + s'``):
    advh_attr_path_points with base 0 and alpha 1 (``0 + 1 * x~ = x~`` exactly), one launch per clip unless the partition
    holds every sample (then the rows are one contiguous run)."""
    B, L = x.shape
    if out is None:
        out = torch.empty((B * pp, L), dtype=torch.float32, device=x.device)
    zero = torch.zeros((1, L), dtype=torch.float32, device=x.device)
    ones = torch.ones(B * S, dtype=torch.float32, device=x.device)
    d = _desc(x, zero, None, S, 1, float(stdevs), seed)
    if pp == S:
        _points(d, ones, 0, B * S, out)
    else:
        for b in range(B):
            _points(d, ones, b * S + s0, pp, out[b * pp:(b + 1) * pp])
    return out


def nt_fold(attr: torch.Tensor, B: int, pp: int, total: torch.Tensor, total_sq: torch.Tensor) -> None:
    """``total += a``, ``total_sq += a * a`` (fp64 ``[B, L]``) over the partition's attributions ``attr [B * pp, L]``."""
    _lib.check(_lib.lib().advh_nt_fold(attr.data_ptr(), B, pp, attr.shape[1], total.data_ptr(), total_sq.data_ptr(), _st()),
               "advh_nt_fold")


def nt_finalize(total: torch.Tensor, total_sq: torch.Tensor, S: int, nt_type: str) -> torch.Tensor:
    """The fp32 ``[B, L]`` NoiseTunnel attribution from the fp64 sums over S samples."""
    out = torch.empty(total.shape, dtype=torch.float32, device=total.device)
    _lib.check(_lib.lib().advh_nt_finalize(total.data_ptr(), total_sq.data_ptr(), total.shape[0], total.shape[1], S,
                                           NT_TYPES.index(nt_type), out.data_ptr(), _st()), "advh_nt_finalize")
    return out


NORM_ORDS = {"fro": 0, 2: 0, 1: 1, math.inf: 2}                       # norm_ord -> advh_row_norm's ord


def metric_partitions(B: int, S: int, max_examples_per_batch=None) -> list:
    """Captum's ``_divide_and_aggregate_metrics`` plan as ``[(s0, p'), ...]``: with ``m = max_examples_per_batch // B < S``,
    ``S // m`` chunks of m samples, then one of ``S % m`` if non-zero; otherwise one chunk of S.  ``m == 0`` raises ValueError
    (Captum asserts).  The plan of NoiseTunnel's partitions (``noise_tunnel_partitions``) with p = m."""
    if max_examples_per_batch is None or max_examples_per_batch // B >= S:
        return noise_tunnel_partitions(S, S)
    m = max_examples_per_batch // B
    if m == 0:
        raise ValueError(f"max_examples_per_batch ({max_examples_per_batch}) must be at least the batch size ({B})")
    return noise_tunnel_partitions(S, m)


_NO_ATTR = object()


def check_metric_args(inputs, n_perturb_samples, max_examples_per_batch=None, target=None, additional_forward_args=None,
                      attributions=_NO_ATTR) -> Tuple[int, int, int, list]:
    """The checks common to infidelity and sensitivity_max -> ``(B, L, S, plan)``: ``inputs`` a ``[B, L]`` tensor, the
    attributions (infidelity) a tensor of its shape, ``n_perturb_samples >= 1``, ``max_examples_per_batch`` None or an integer
    >= B, ``target`` and ``additional_forward_args`` None (one input, one output).  Raises ValueError before any GPU work."""
    if target is not None:
        raise ValueError("the classifier has a single output; target must be None")
    if additional_forward_args is not None:
        raise ValueError("the classifier takes no additional forward arguments; additional_forward_args must be None")
    if not torch.is_tensor(inputs) or inputs.dim() != 2:
        raise ValueError("inputs must be a [B, L] waveform tensor")
    B, L = inputs.shape
    if attributions is not _NO_ATTR and (not torch.is_tensor(attributions) or tuple(attributions.shape) != (B, L)):
        raise ValueError(f"attributions must be a tensor of the inputs' shape [{B}, {L}], not "
                         f"{list(attributions.shape) if torch.is_tensor(attributions) else type(attributions).__name__}")
    S = _positive_int(n_perturb_samples, "n_perturb_samples")
    if max_examples_per_batch is not None:
        _positive_int(max_examples_per_batch, "max_examples_per_batch")
    return B, L, S, metric_partitions(B, S, max_examples_per_batch)


def check_norm_ord(norm_ord) -> int:
    """sensitivity_max's ``norm_ord``: "fro" or 2, 1, inf -> advh_row_norm's ord; anything else raises ValueError."""
    if isinstance(norm_ord, bool) or not isinstance(norm_ord, (str, int, float, np.integer, np.floating)):
        raise ValueError(f"norm_ord must be 'fro', 2, 1 or inf, not {norm_ord!r}")
    key = norm_ord if isinstance(norm_ord, str) else float(norm_ord)
    if key not in NORM_ORDS:
        raise ValueError(f"norm_ord must be 'fro', 2, 1 or inf, not {norm_ord!r}")
    return NORM_ORDS[key]


def _finite_scale(v, what) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
        raise ValueError(f"{what} must be a finite number >= 0, not {v!r}")
    return float(v)


def expand_metric_baselines(baselines, B: int, L: int, pp: int):
    """Captum's expansion of ``baselines`` for a chunk of pp samples (infidelity's ``_generate_perturbations``,
    ``_expand_and_update_baselines``): a ``[B, L]`` tensor with B > 1 is ``repeat_interleave``d; ``[1, L]`` tensors, numbers
    and None pass unchanged."""
    if torch.is_tensor(baselines) and tuple(baselines.shape) == (B, L) and B > 1:
        return baselines.repeat_interleave(pp, 0)
    return baselines


def sensitivity_kwargs(kwargs: dict, B: int, L: int, pp: int) -> dict:
    """The explanation function's keyword arguments for a chunk of pp samples: ``baselines`` expanded as
    ``expand_metric_baselines``, everything else -- ``feature_mask`` included, unlike ``noise_tunnel_kwargs`` -- unchanged."""
    kw = dict(kwargs)
    if "baselines" in kw:
        kw["baselines"] = expand_metric_baselines(kw["baselines"], B, L, pp)
    return kw


def _perturb_params(fn) -> int:
    try:
        return len(inspect.signature(fn).parameters)
    except (TypeError, ValueError):
        return 1


class MetricDesc(C.Structure):
    """Mirror of ``advh_metric_desc`` (include/addvisor_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("attr", C.c_void_p), ("base", C.c_void_p), ("n", C.c_int64), ("seed", C.c_uint64),
                ("B", C.c_int), ("S", C.c_int), ("s0", C.c_int), ("p", C.c_int), ("base_rows", C.c_int), ("mode", C.c_int),
                ("mul", C.c_int), ("scale", C.c_float)]


MR_UNIFORM, MR_GAUSS = 0, 1                                            # advh_metric_desc.mode


def metric_device(t: torch.Tensor) -> torch.device:
    """The GPU the metric kernels run on for ``t``: its own device when it is on a GPU, else the current one."""
    return t.device if t.is_cuda else torch.device("cuda")


def _on_gpu(*tensors) -> None:
    """Every tensor whose pointer goes to a kernel must be GPU memory: a host pointer would reach the device.  Raises ValueError
    before any launch."""
    for t in tensors:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise ValueError("the metric kernels take GPU tensors; got " + (f"a tensor on {t.device}" if torch.is_tensor(t)
                                                                             else type(t).__name__))


def metric_desc(x, seed, S, s0, pp, mode, scale, attr=None, base=None, mul=False) -> MetricDesc:
    B, L = x.shape
    d = MetricDesc(x.data_ptr(), None if attr is None else attr.data_ptr(), None if base is None else base.data_ptr(), L, seed,
                   B, S, s0, pp, 1 if base is None else base.shape[0], mode, int(mul), scale)
    d.tensors = (x, attr, base)                             # checked by metric_rows, and kept alive as long as the desc
    return d


def metric_rows(d: MetricDesc, row0: int, rows: int, out: torch.Tensor, dot: Optional[torch.Tensor] = None) -> None:
    """Chunk rows ``[row0, row0 + rows)`` into ``out [rows, L]``; Gaussian mode also writes ``dot[row0:row0 + rows]``."""
    _on_gpu(*d.tensors, out, dot)
    _lib.check(_lib.lib().advh_metric_rows(C.byref(d), row0, rows, out.data_ptr(), None if dot is None else dot.data_ptr(), _st()),
               "advh_metric_rows")


def uniform_rows(x: torch.Tensor, seed: int, S: int, s0: int, pp: int, radius: float) -> torch.Tensor:
    """sensitivity_max's default perturbation of the chunk ``[s0, s0 + pp)``: row ``b * pp + s'`` =
    ``x_b + radius * (2u - 1)``, u the uniform of the Philox words of row ``b * S + s0 + s'``."""
    B, L = x.shape
    out = torch.empty((B * pp, L), dtype=torch.float32, device=x.device)
    metric_rows(metric_desc(x, seed, S, s0, pp, MR_UNIFORM, radius), 0, B * pp, out)
    return out


def metric_row_dot(pert: torch.Tensor, attr: torch.Tensor, pp: int) -> torch.Tensor:
    """``dot[r] = sum_j pert[r, j] * attr[r // pp, j]`` (``[B * pp]`` fp32)."""
    _on_gpu(pert, attr)
    dot = torch.empty(pert.shape[0], dtype=torch.float32, device=pert.device)
    _lib.check(_lib.lib().advh_metric_row_dot(pert.data_ptr(), attr.data_ptr(), attr.shape[0], pp, attr.shape[1], dot.data_ptr(),
                                              _st()), "advh_metric_row_dot")
    return dot


def infidelity_fold(dot, f0, fk, B: int, pp: int, normalize: bool, acc) -> None:
    _on_gpu(dot, f0, fk, acc)
    _lib.check(_lib.lib().advh_infidelity_fold(dot.data_ptr(), f0.data_ptr(), fk.data_ptr(), B, pp, int(normalize), acc.data_ptr(),
                                               _st()), "advh_infidelity_fold")


def infidelity_finalize(acc, B: int, S: int, normalize: bool) -> torch.Tensor:
    _on_gpu(acc)
    out = torch.empty(B, dtype=torch.float32, device=acc.device)
    _lib.check(_lib.lib().advh_infidelity_finalize(acc.data_ptr(), B, S, int(normalize), out.data_ptr(), _st()),
               "advh_infidelity_finalize")
    return out


def row_norm(v: torch.Tensor, ord_: int) -> torch.Tensor:
    _on_gpu(v)
    out = torch.empty(v.shape[0], dtype=torch.float32, device=v.device)
    _lib.check(_lib.lib().advh_row_norm(v.data_ptr(), v.shape[0], v.shape[1], ord_, out.data_ptr(), _st()), "advh_row_norm")
    return out


def sensitivity_fold(e, et, enorm, pp: int, ord_: int, smax) -> None:
    _on_gpu(e, et, enorm, smax)
    ratio = torch.empty(et.shape[0], dtype=torch.float32, device=et.device)
    _lib.check(_lib.lib().advh_sensitivity_fold(e.data_ptr(), et.data_ptr(), enorm.data_ptr(), e.shape[0], pp, e.shape[1], ord_,
                                                ratio.data_ptr(), smax.data_ptr(), _st()), "advh_sensitivity_fold")


class NoisyPerturbation:
    """Infidelity's noisy perturbation (an extension of this build, not a Captum name): ``noise = stdevs * N(0, 1)``, returning
    ``(noise, inputs - noise)`` as in Captum's tutorial and Yeh et al., or -- ``multiply_by_inputs=True`` -- the perturbation of
    ``infidelity_perturb_func_decorator(True)`` around it, ``safe_div(x - x~, x - baselines)`` (denominator 1 where zero).
    ``infidelity`` recognises it and runs fused: the rows ``x_b - stdevs * N(seed, b * S + s, :)`` go straight into the forward's
    workspace and the dot product with the attribution is formed in the same pass (advh_metric_rows).  Called directly it is an
    ordinary perturb_func: one seed from torch's default CPU generator, ``N(seed, r, :)`` for row r of ``inputs [R, L]``, drawn
    on ``metric_device(inputs)`` (a host tensor's noise is drawn on the current GPU); both results come back on the inputs'
    device."""

    def __init__(self, stdevs: float = 0.01, multiply_by_inputs: bool = False):
        self.stdevs = _finite_scale(stdevs, "stdevs")
        self.multiply_by_inputs = bool(multiply_by_inputs)

    def __call__(self, inputs, baselines=None):
        if not torch.is_tensor(inputs) or inputs.dim() != 2:
            raise ValueError("inputs must be a [R, L] waveform tensor")
        dev = metric_device(inputs)
        noise = self.stdevs * philox_normal(draw_seed(), 0, inputs.shape[0], inputs.shape[1], dev)
        x = inputs.to(dev, torch.float32)
        xt = x - noise
        if self.multiply_by_inputs:
            den = x if baselines is None else x - (baselines.to(dev, torch.float32) if torch.is_tensor(baselines) else baselines)
            noise = (x - xt) / torch.where(den != 0, den, torch.ones_like(den))
        return noise.to(inputs.device), xt.to(inputs.device)


def _checked_metric(out: torch.Tensor, what: str, cause: str) -> torch.Tensor:
    """The engine's ``_checked`` for a metric: one synchronisation, the split-format range flag, then finiteness."""
    finite = bool(torch.isfinite(out).all())
    _lib.check_overflow(what)
    if not finite:
        raise FloatingPointError(f"non-finite {what}: {cause}")
    return out


def sensitivity_max(explain, waves, device, perturb_func=None, perturb_radius: float = 0.02, n_perturb_samples: int = 10,
                    norm_ord="fro", max_examples_per_batch=None, seed: Optional[int] = None, **kwargs) -> torch.Tensor:
    """Captum's sensitivity_max (restated from Captum 0.7's ``metrics/_core/sensitivity.py``: captum is absent) on ``device``;
    ``HipAttribution.sensitivity_max`` documents it.  The metric needs no model: ``explain`` brings its own.  ``device`` must
    be a GPU: the kernel wrappers reject host tensors with ValueError before any launch."""
    B, L, S, plan = check_metric_args(waves, n_perturb_samples, max_examples_per_batch, kwargs.pop("target", None),
                                      kwargs.pop("additional_forward_args", None))     # None once checked: not passed on
    ord_ = check_norm_ord(norm_ord)
    radius = _finite_scale(perturb_radius, "perturb_radius")
    if perturb_func is not None and not callable(perturb_func):
        raise ValueError("perturb_func must be callable")
    seed = _check_seed(seed)                                 # drawn before explain draws its own
    x = waves.to(device, torch.float32).contiguous()

    def explained(rows, kw, R):
        res = explain(rows, **kw)
        if not torch.is_tensor(res) or tuple(res.shape) != (R, L):
            raise ValueError(f"explanation_func must return a [{R}, {L}] attribution, "
                             f"not {tuple(res.shape) if torch.is_tensor(res) else type(res).__name__}")
        return res.to(device, torch.float32).contiguous()

    def perturbed(s0, pp):
        R = B * pp
        if perturb_func is None:
            return uniform_rows(x, seed, S, s0, pp, radius)
        xe = x.repeat_interleave(pp, 0)
        xt = perturb_func(xe, perturb_radius) if _perturb_params(perturb_func) > 1 else perturb_func(xe)
        if isinstance(xt, (tuple, list)) and len(xt) == 1:
            xt = xt[0]
        if not torch.is_tensor(xt) or tuple(xt.shape) != (R, L):
            raise ValueError(f"perturb_func must return the [{R}, {L}] perturbed inputs, "
                             f"not {tuple(xt.shape) if torch.is_tensor(xt) else type(xt).__name__}")
        return xt.to(device, torch.float32).contiguous()

    xt = perturbed(*plan[0])                                 # a perturb_func of the wrong shape raises before any explanation
    e = explained(x, kwargs, B)
    enorm = row_norm(e, ord_)
    smax = torch.zeros(B, dtype=torch.float32, device=device)
    for k, (s0, pp) in enumerate(plan):
        xt = xt if k == 0 else perturbed(s0, pp)
        sensitivity_fold(e, explained(xt, sensitivity_kwargs(kwargs, B, L, pp), B * pp), enorm, pp, ord_, smax)
    return _checked_metric(smax, "sensitivity_max", "an explanation of the clips or of their perturbations is not finite")


class CoalitionDesc(C.Structure):
    """Mirror of ``advh_coalition_desc`` (include/addvisor_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("base", C.c_void_p), ("index", C.c_void_p), ("rank", C.c_void_p), ("present", C.c_void_p),
                ("n", C.c_int64), ("p0", C.c_int64), ("rows", C.c_int64), ("B", C.c_int), ("base_rows", C.c_int),
                ("index_rows", C.c_int), ("mode", C.c_int), ("K", C.c_int), ("P", C.c_int)]


COAL_RANK, COAL_PRESENCE = 0, 1                                        # advh_coalition_desc.mode


def coalition_desc(x, base, index, K, rank=None, p0=0, present=None) -> CoalitionDesc:
    """Rank mode with ``rank [P, K]`` int32 (the table of permutations ``p0 .. p0 + P - 1``), presence mode with
    ``present [rows, K]`` uint8."""
    B, L = x.shape
    mode = COAL_RANK if present is None else COAL_PRESENCE
    return CoalitionDesc(x.data_ptr(), base.data_ptr(), index.data_ptr(), None if rank is None else rank.data_ptr(),
                         None if present is None else present.data_ptr(), L, p0, 0 if present is None else present.shape[0], B,
                         base.shape[0], index.shape[0], mode, K, 0 if rank is None else rank.shape[0])


def coalition_points(d: CoalitionDesc, row0: int, rows: int, out: torch.Tensor) -> None:
    """Coalition rows ``[row0, row0 + rows)`` (rows past the table copy x) into ``out [rows, L]``."""
    _lib.check(_lib.lib().advh_coalition_points(C.byref(d), row0, rows, out.data_ptr(), _st()), "advh_coalition_points")


def shapley_accumulate(d: CoalitionDesc, fbase: torch.Tensor, fk: torch.Tensor, p0: int, np_: int, total: torch.Tensor,
                       finalize_div: float = 0.0) -> None:
    """``total [B, L] +=`` the marginal contributions of permutations ``[p0, p0 + np_)``; ``finalize_div > 0`` divides once."""
    _lib.check(_lib.lib().advh_shapley_accumulate(C.byref(d), fbase.data_ptr(), fk.data_ptr(), p0, np_, total.data_ptr(),
                                                  finalize_div, _st()), "advh_shapley_accumulate")


def coalition_scatter(d: CoalitionDesc, coef: torch.Tensor, attr: torch.Tensor) -> None:
    """``attr[b, t] = coef[b, index[b, t]]`` (``coef [B, K]`` fp32)."""
    _lib.check(_lib.lib().advh_coalition_scatter(C.byref(d), coef.data_ptr(), attr.data_ptr(), _st()), "advh_coalition_scatter")


GROUP_ROWS = 1 << 16                                                   # coalition rows per permutation group (fk, rank table)


class AblationDesc(C.Structure):
    """Mirror of ``advh_ablation_desc`` (include/addvisor_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("base", C.c_void_p), ("mask", C.c_void_p), ("n", C.c_int64), ("B", C.c_int),
                ("base_rows", C.c_int), ("mask_rows", C.c_int), ("mode", C.c_int), ("win", C.c_int), ("stride", C.c_int),
                ("K", C.c_int)]


ABL_OCCLUSION, ABL_FEATURE = 0, 1                                      # advh_ablation_desc.mode
_ABLATION_CAUSE = "a logit of the clips or of their ablations is not finite (check the inputs and baselines)"


def ablation_desc(x, base, mode, K, win=0, stride=0, mask=None) -> AblationDesc:
    B, L = x.shape
    return AblationDesc(x.data_ptr(), base.data_ptr(), None if mask is None else mask.data_ptr(), L, B, base.shape[0],
                        0 if mask is None else mask.shape[0], mode, win, stride, K)


def ablation_points(d: AblationDesc, row0: int, rows: int, out: torch.Tensor) -> None:
    """Ablated rows ``[row0, row0 + rows)`` (perturbation-major, rows past ``K * B`` copy x) into ``out [rows, L]``."""
    _lib.check(_lib.lib().advh_ablation_points(C.byref(d), row0, rows, out.data_ptr(), _st()), "advh_ablation_points")


def ablation_accumulate(d: AblationDesc, f0: torch.Tensor, fk: torch.Tensor, attr: torch.Tensor) -> None:
    """The attribution ``attr [B, L]`` from ``f0 = F(x) [B]`` and ``fk = F(ablated) [K * B]``."""
    _lib.check(_lib.lib().advh_ablation_accumulate(C.byref(d), f0.data_ptr(), fk.data_ptr(), attr.data_ptr(), _st()),
               "advh_ablation_accumulate")


class CurveDesc(C.Structure):
    """Mirror of ``advh_curve_desc`` (include/addvisor_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("base", C.c_void_p), ("index", C.c_void_p), ("rank", C.c_void_p), ("counts", C.c_void_p),
                ("n", C.c_int64), ("B", C.c_int), ("base_rows", C.c_int), ("index_rows", C.c_int), ("K", C.c_int), ("S1", C.c_int),
                ("mode", C.c_int)]


CURVE_MODES = ("deletion", "insertion")                                # advh_curve_desc.mode: 0, 1
CURVE_ORDERS = ("morf", "lerf", "random")
CURVE_OUTPUTS = ("prob", "logit")
CURVE_POOLS = ("sum", "mean")


def curve_counts(steps, K: int) -> np.ndarray:
    """The schedule of a perturbation curve: int32 ``[S + 1]`` counts of switched features, strictly increasing from 0 to K.
    ``steps``: None (``S = min(K, 20)``), an int ``S`` in ``[1, K]`` (``c_j = (j * K + S // 2) // S``) or a strictly increasing
    sequence of fractions from 0.0 to 1.0 (``c = floor(f * K + 0.5)``).  Raises ValueError on anything else and on counts that
    collide after rounding."""
    if steps is None:
        steps = min(K, 20)
    if isinstance(steps, (int, np.integer)) and not isinstance(steps, bool):
        S = int(steps)
        if not 1 <= S <= K:
            raise ValueError(f"steps must be in [1, {K}] (the number of features), not {S}")
        return np.array([(j * K + S // 2) // S for j in range(S + 1)], dtype=np.int32)
    if isinstance(steps, (bool, str)) or not isinstance(steps, (list, tuple, np.ndarray, torch.Tensor)):
        raise ValueError(f"steps must be None, an integer or a sequence of fractions, not {steps!r}")
    f = np.asarray(steps.detach().cpu() if torch.is_tensor(steps) else steps, dtype=np.float64)
    if f.ndim != 1 or f.size < 2 or not np.isfinite(f).all() or f[0] != 0.0 or f[-1] != 1.0 or not (np.diff(f) > 0).all():
        raise ValueError("the fractions of steps must be strictly increasing, start at 0.0 and end at 1.0")
    counts = np.floor(f * K + 0.5).astype(np.int64)
    if not (np.diff(counts) > 0).all():
        raise ValueError(f"the fractions of steps collide after rounding to counts of {K} features: {counts.tolist()}")
    return counts.astype(np.int32)


def _one_of(v, choices, what) -> int:
    if v not in choices:
        raise ValueError(f"{what} must be one of {choices}, not {v!r}")
    return choices.index(v)


def check_curve_features(index: torch.Tensor, K: int) -> None:
    """Every clip must hold at least one sample of each of the K features (a ``[1, L]`` index does by construction): a feature
    without samples has no score (advh_feature_scores gives it -inf)."""
    if index.shape[0] > 1:
        for b, row in enumerate(index):
            if int(torch.unique(row).numel()) != K:
                raise ValueError(f"clip {b} holds no sample of some of the {K} features of feature_mask; a perturbation curve "
                                 "needs every feature in every clip")


def feature_scores(attr: torch.Tensor, index: Optional[torch.Tensor], K: int, use_abs: bool = False, mean: bool = False) -> torch.Tensor:
    """``score [B, K]``: the per-clip fp32 sum (``mean``: average) of ``attr [B, n]`` (``use_abs``: its magnitude) over the samples
    of each feature of ``index [1 | B, n]`` (None: the identity, ``K == n``), in increasing sample order."""
    B, n = attr.shape
    _on_gpu(attr, *(() if index is None else (index,)))
    score = torch.empty((B, K), dtype=torch.float32, device=attr.device)
    _lib.check(_lib.lib().advh_feature_scores(attr.data_ptr(), None if index is None else index.data_ptr(),
                                              0 if index is None else index.shape[0], B, n, K, int(use_abs), int(mean), score.data_ptr(),
                                              _st()), "advh_feature_scores")
    return score


def feature_rank(score: torch.Tensor, descending: bool) -> torch.Tensor:
    """``rank [B, K]`` int32: the position of each feature in its clip's order (``descending``: highest score first); ties go to
    the lower feature number."""
    B, K = score.shape
    _on_gpu(score)
    rank = torch.empty((B, K), dtype=torch.int32, device=score.device)
    _lib.check(_lib.lib().advh_feature_rank(score.data_ptr(), B, K, int(descending), rank.data_ptr(), _st()), "advh_feature_rank")
    return rank


def curve_desc(x, base, index, rank, counts, mode: int) -> CurveDesc:
    B, L = x.shape
    d = CurveDesc(x.data_ptr(), base.data_ptr(), None if index is None else index.data_ptr(), rank.data_ptr(), counts.data_ptr(), L, B,
                  base.shape[0], 0 if index is None else index.shape[0], rank.shape[1], counts.numel(), mode)
    d.tensors = tuple(t for t in (x, base, index, rank, counts) if t is not None)     # kept alive as long as the desc
    return d


def curve_points(d: CurveDesc, row0: int, rows: int, out: torch.Tensor) -> None:
    """Curve rows ``[row0, row0 + rows)`` (step-major ``j * B + b``, rows past ``S1 * B`` copy x) into ``out [rows, n]``."""
    _on_gpu(*d.tensors, out)
    _lib.check(_lib.lib().advh_curve_points(C.byref(d), row0, rows, out.data_ptr(), _st()), "advh_curve_points")


def curve_fold(fk: torch.Tensor, counts: torch.Tensor, B: int, K: int, prob: bool, ref_last: bool):
    """``(curve [B, S1], auc [B], aopc [B])`` from the rows' logits ``fk [S1 * B]`` and the device counts ``[S1]``."""
    S1 = counts.numel()
    _on_gpu(fk, counts)
    curve = torch.empty((B, S1), dtype=torch.float32, device=fk.device)
    auc, aopc = torch.empty(B, dtype=torch.float32, device=fk.device), torch.empty(B, dtype=torch.float32, device=fk.device)
    _lib.check(_lib.lib().advh_curve_fold(fk.data_ptr(), counts.data_ptr(), B, S1, K, int(prob), int(ref_last), curve.data_ptr(),
                                          auc.data_ptr(), aopc.data_ptr(), _st()), "advh_curve_fold")
    return curve, auc, aopc


class PerturbationCurve(NamedTuple):
    """The result of ``HipAttribution.perturbation_curve``: ``curve [B, S + 1]`` (the output at each step), ``fractions [S + 1]``
    (float64: the share of features switched), ``auc [B]``, ``aopc [B]`` and ``rank [B, K]`` (int32: the step order of each
    clip's features)."""
    curve: torch.Tensor
    fractions: torch.Tensor
    auc: torch.Tensor
    aopc: torch.Tensor
    rank: torch.Tensor


class PermutationDesc(C.Structure):
    """Mirror of ``advh_permutation_desc`` (include/addvisor_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("index", C.c_void_p), ("perm", C.c_void_p), ("n", C.c_int64), ("B", C.c_int), ("K", C.c_int)]


def permutation_desc(x, index, perm) -> PermutationDesc:
    """``index [1, L]`` int32 feature ranks, ``perm [K, B]`` int32 (``feature_permutation_draws``)."""
    B, L = x.shape
    d = PermutationDesc(x.data_ptr(), index.data_ptr(), perm.data_ptr(), L, B, perm.shape[0])
    d.tensors = (x, index, perm)                                          # kept alive as long as the desc
    return d


def permutation_points(d: PermutationDesc, row0: int, rows: int, out: torch.Tensor) -> None:
    """Permuted rows ``[row0, row0 + rows)`` (perturbation-major, rows past ``K * B`` copy x) into ``out [rows, L]``."""
    _on_gpu(*d.tensors, out)
    _lib.check(_lib.lib().advh_permutation_points(C.byref(d), row0, rows, out.data_ptr(), _st()), "advh_permutation_points")


def row_similarity(rows: torch.Tensor, x: torch.Tensor, row0: int, n_rows: int, mode: int, kernel_width: float,
                   sim: torch.Tensor) -> None:
    """``sim[row0 + r]`` = the exp-kernel weight of ``rows[r]`` against its clip ``x[(row0 + r) % B]``, ``r < n_rows``."""
    _on_gpu(rows, x, sim)
    _lib.check(_lib.lib().advh_row_similarity(rows.data_ptr(), x.data_ptr(), row0, n_rows, x.shape[0], x.shape[1], mode,
                                              kernel_width, sim.data_ptr(), _st()), "advh_row_similarity")


class PathDesc(C.Structure):
    """Mirror of ``advh_path_desc`` (include/addvisor_hip.h)."""
    _fields_ = [("x", C.c_void_p), ("base", C.c_void_p), ("bidx", C.c_void_p), ("n", C.c_int64), ("seed", C.c_uint64),
                ("B", C.c_int), ("S", C.c_int), ("base_rows", C.c_int), ("clip_major", C.c_int), ("sigma", C.c_float)]


ACC_IG, ACC_SHAP, ACC_SHAP_GRAD, FIN_IG, FIN_MEAN = range(5)          # advh_attr_path_accumulate modes


def _desc(x, base, bidx, S, clip_major, sigma=0.0, seed=0) -> PathDesc:
    B, L = x.shape
    return PathDesc(x.data_ptr(), base.data_ptr(), None if bidx is None else bidx.data_ptr(), L, seed, B, S, base.shape[0],
                    clip_major, sigma)


def _points(d, alpha, row0, rows, out):
    _lib.check(_lib.lib().advh_attr_path_points(C.byref(d), alpha.data_ptr(), row0, rows, out.data_ptr(), _st()),
               "advh_attr_path_points")


def _accumulate(d, grad, w, mode, row0, rows, total, row_sum=None):
    _lib.check(_lib.lib().advh_attr_path_accumulate(C.byref(d), grad.data_ptr(), None if w is None else w.data_ptr(), mode, row0,
                                                    rows, total.data_ptr(), None if row_sum is None else row_sum.data_ptr(), _st()),
               "advh_attr_path_accumulate")


def _steps_per_chunk(B: int, n_points: int, internal_batch_size: Optional[int]) -> int:
    """Whole path steps (B rows each) per chunk of ``internal_batch_size`` (default 128) rows: at least one, at most all."""
    return min(max(1, (internal_batch_size or 128) // B), n_points)


def _step_major(alphas: np.ndarray, B: int, device) -> torch.Tensor:
    """One value per step (the alphas, or the step sizes) as the fp32 device vector of the step-major rows ``s * B + b``."""
    return torch.tensor(np.repeat(alphas, B), dtype=torch.float32, device=device)


def philox_normal(seed: int, row0: int, rows: int, n: int, device, raw: bool = False) -> torch.Tensor:
    """``[rows, n]`` fp32 standard normals N(seed, row0 + r, j): exactly the noise GradientShap adds to expanded row g
    (``stdevs * N(seed, g, :)``).  ``raw=True``: the Philox words instead, ``[rows, n]`` int32 (bit patterns).
    advh_philox_normal.  ``device`` must be a GPU (ValueError before any launch: a host buffer would reach the kernel)."""
    if torch.device(device).type != "cuda":
        raise ValueError(f"philox_normal draws on a GPU, not on {device}")
    out = torch.empty((rows, n), dtype=torch.float32, device=device)
    _lib.check(_lib.lib().advh_philox_normal(int(seed), row0, rows, n, int(raw), out.data_ptr(), _st()), "advh_philox_normal")
    return out.view(torch.int32) if raw else out


# The seed of the neuron methods at hidden_states[l]: the largest power of two for which the largest gradient-plane magnitude
# measured over the cases of tests/test_gpu_neuron_attr.py stays at or under 65 504 / 16 (DESIGN, "Neuron attributions").
NEURON_LOSS_SCALE = 128.0


class HipAttribution:
    _lens = None          # the per-clip lengths of the ragged call in flight (``lengths=``), None outside one

    def __init__(self, emb: HipEmbedder, loss_scale: float = 4096.0, precision: Optional[str] = None,
                 neuron_loss_scale: float = NEURON_LOSS_SCALE, long_clips: bool = False, long_maps: bool = False):
        """``precision``: None = the embedder's (an fp32-class embedder gives the fp32-class gradient chain, the reference's
        fp32 autograd class); "f16" = the fp16-operand chain.  ``neuron_loss_scale``: the power of two the neuron methods seed
        ``hidden_states[l]`` with (a unit seed there is far larger than the logit's ``coef / T``; DESIGN).  ``long_clips``: passed
        to the ``EmbedderGrad`` -- True lets every method built on the gradient chain take clips above 256 frames, except
        ``attention_maps``, ``attention_rollout``, ``attention_grad_rollout`` and ``transformer_lrp``, which ``long_maps=True``
        (it needs ``long_clips=True``) lifts as well and gives their ``lengths=`` argument."""
        v = neuron_loss_scale
        if not (isinstance(v, (int, float)) and not isinstance(v, bool) and v > 0 and math.isfinite(v) and math.frexp(v)[0] == 0.5):
            raise ValueError(f"neuron_loss_scale must be a positive power of two, not {v!r}")
        kw = {} if long_maps is False else dict(long_maps=long_maps)       # the keyword only when asked for (as the runtime does)
        self.emb, self.eg, self.loss_scale = emb, EmbedderGrad(emb, precision, long_clips=long_clips, **kw), loss_scale
        self.neuron_loss_scale = float(neuron_loss_scale)
        self.precision = self.eg.precision

    def _prep(self, waves: torch.Tensor) -> torch.Tensor:
        if waves.dim() == 1:
            waves = waves[None]
        return waves.to(self.emb.dev, torch.float32).contiguous()

    # The seam of the chunk loops below: every batch of rows they build goes through this forward / gradient pair, which is told
    # the rows' layout -- row r of ``pts`` is global row ``row0 + r``, of clip ``(row0 + r) % B`` (``clip_major=0``: rows
    # ``s * B + b``, ``k * B + b``, ``(p * K + j) * B + b``) or ``(row0 + r) // S`` (``clip_major=1``: rows ``b * S + s``).  A
    # waveform row is the classifier's input itself, so the layout is not used here; the mask-domain engine
    # (spectral_attribution.py) overrides the pair and resynthesises each row from its clip's spectrogram first.
    # A ragged call (``lengths=``, ``_ragged``): row ``row0 + r`` carries the length of its clip ``(row0 + r) % B`` -- the methods
    # that take lengths build clip-minor rows only -- so a path point of clip b has ``lengths[b]`` samples whatever the chunking.
    def _row_gradient(self, pts: torch.Tensor, row0: int = 0, clip_major: int = 0, S: int = 1) -> torch.Tensor:
        """d logit / d row over ``pts [R, n]``, ``[R, n]`` fp32."""
        self.eg.forward(pts, lengths=self._row_lengths(pts.shape[0], row0))
        return self.eg.backward(self.loss_scale)

    def _row_logit(self, pts: torch.Tensor, row0: int = 0, clip_major: int = 0, S: int = 1) -> torch.Tensor:
        """``[R]`` fp32 logits of the rows ``pts [R, n]``."""
        return self.eg.emb.forward(pts, want_hidden=False, lengths=self._row_lengths(pts.shape[0], row0))[1].view(-1)

    def _row_lengths(self, R: int, row0: int):
        lens = self._lens
        return None if lens is None else [lens[(row0 + r) % len(lens)] for r in range(R)]

    def _ragged(self, waves, lengths):
        """The clips of a ragged call, ``(x [B, L] on the device, lens)``: ``lengths`` checked on the host before anything is
        allocated (``HipEmbedder._check_lengths``), and the samples past each length replaced by zeros, so that ``x * g`` and
        ``x - baseline`` are exactly 0 there whatever the padding holds (the chain itself never reads it)."""
        B, L = _dims(waves)
        lens = self.emb._check_lengths(lengths, B, L)
        return self._mask_tail(self._prep(waves), lens), lens

    @staticmethod
    def _mask_tail(x: torch.Tensor, lens) -> torch.Tensor:
        keep = torch.arange(x.shape[1], device=x.device)[None] < torch.tensor(lens, device=x.device)[:, None]
        return torch.where(keep, x, torch.zeros((), dtype=x.dtype, device=x.device))

    def input_gradient(self, waves: torch.Tensor, lengths=None) -> torch.Tensor:
        """d logit / d wave, ``[B, L]`` fp32.  ``lengths`` (one sample count per clip, ``EmbedderGrad.forward``): clip b is
        ``waves[b, :lengths[b]]`` and its gradient the one of that clip run alone, exactly 0 past its length."""
        if lengths is None:
            return self._row_gradient(self._prep(waves))
        return self._ragged_rows(self._row_gradient, *self._ragged(waves, lengths))

    def _ragged_rows(self, fn, x, lens):
        """``fn(x)`` (``_row_gradient`` / ``_row_logit``) with the rows of ``x`` carrying ``lens``."""
        self._lens = lens
        try:
            return fn(x)
        finally:
            self._lens = None

    def _finalize(self, g, x, mode):
        out = torch.empty_like(g)
        _lib.check(_lib.lib().advh_attr_finalize(g.data_ptr(), x.data_ptr(), out.data_ptr(), mode, g.numel(), _st()), "advh_attr_finalize")
        return self._checked(out)

    def _checked(self, out, what: str = "attribution", cause: Optional[str] = None):
        # the planes between the dgrad GEMMs have fp16's exponent range: an overflow (|scaled gradient| > 65504 somewhere in the
        # chain) surfaces as inf / NaN in the input gradient and in every sum over path points.  One flag read per attribution:
        # raise instead of handing back a poisoned attribution map.
        finite = bool(torch.isfinite(out).all())             # synchronises: every kernel of the chain has run
        _lib.check_overflow(what)                            # fp32-class chain: saturated planes raise SplitRangeError (a FloatingPointError)
        if not finite:
            raise FloatingPointError(f"non-finite {what}: " + (cause or f"the gradient chain overflowed at loss_scale={self.loss_scale:g} "
                                                                      "(lower HipAttribution.loss_scale by a power of two)"))
        return out

    def saliency(self, waves, lengths=None):
        """``|d logit / d wave|``.  ``lengths``: as ``input_gradient``; values past a length are exactly 0."""
        if lengths is None:
            x = self._prep(waves)
            return self._finalize(self.input_gradient(x), x, 0)
        x, lens = self._ragged(waves, lengths)
        return self._finalize(self._ragged_rows(self._row_gradient, x, lens), x, 0)

    def input_x_gradient(self, waves, lengths=None):
        """``wave * d logit / d wave``.  ``lengths``: as ``input_gradient``; values past a length are exactly 0."""
        if lengths is None:
            x = self._prep(waves)
            return self._finalize(self.input_gradient(x), x, 1)
        x, lens = self._ragged(waves, lengths)
        return self._finalize(self._ragged_rows(self._row_gradient, x, lens), x, 1)

    def logits(self, waves, lengths=None) -> torch.Tensor:
        """``[B]`` fp32 logits of the gradient chain's own forward (the F of the convergence deltas).  ``lengths``: the ragged
        forward, clip b pooled over its own frames."""
        if lengths is None:
            return self._row_logit(self._prep(waves))
        return self._ragged_rows(self._row_logit, *self._ragged(waves, lengths))

    def integrated_gradients(self, waves, n_steps: int = 50, internal_batch_size: Optional[int] = None, baselines=None,
                             method: str = "gausslegendre", multiply_by_inputs: bool = True, return_convergence_delta: bool = False,
                             lengths=None):
        """Captum's IntegratedGradients.  ``baselines``: None (zero), a number, ``[1, L]`` or ``[B, L]``; ``method``: one of
        ``METHODS``.  With ``return_convergence_delta`` returns ``(attr, delta)``, ``delta[b] = sum_j attr[b, j] -
        (F(x_b) - F(base_b))`` ``[B]`` (F from one extra forward over x and the baselines).  A constant clip (the alpha = 0
        point of a number baseline under ``riemann_left`` / ``riemann_trapezoid``) is where the classifier's per-clip
        normalisation has no scale: its gradient can leave the chain's range, and the call then raises FloatingPointError.
        ``lengths`` (one sample count per clip): a ragged batch.  Every path point of clip b carries ``lengths[b]`` whatever the
        chunking, the input and the baseline count as zero past it, so the attribution is exactly 0 there, and the delta's F is
        the ragged forward (a shared ``[1, L]`` baseline is scored once per clip, under that clip's length)."""
        B, L = _dims(waves)
        lens = None if lengths is None else self.emb._check_lengths(lengths, B, L)
        base = check_ig_baselines(baselines, B, L)
        alphas, steps = approximation(method, n_steps)
        _check_delta(return_convergence_delta, multiply_by_inputs)
        x = self._prep(waves)
        base = _device_base(base, x)
        if lens is not None:
            x, base = self._mask_tail(x, lens), self._mask_tail(base.expand(B, L), lens)
        self._lens = lens
        try:
            out, sums = self._integrate_path(x, base, alphas, steps, internal_batch_size, self._row_gradient,
                                             FIN_IG if multiply_by_inputs else FIN_MEAN, return_convergence_delta)
            out = self._checked(out)
            if not return_convergence_delta:
                return out
            f = self._row_logit(torch.cat([x, base])).double()
        finally:
            self._lens = None
        fb = f[B:].expand(B) if base.shape[0] == 1 else f[B:]
        return out, (sums.double() - (f[:B] - fb)).float()

    def _integrate_path(self, x, base, alphas, steps, internal_batch_size, point_gradient, finalize=None, want_sums: bool = False):
        """The one straight-path loop: ``sum_k steps[k] * point_gradient(base + alphas[k] (x - base))`` over ``x [B, ...]`` and
        ``base [1 | B, ...]`` (flattened to rows), then the optional finalize -- ``FIN_IG``: times ``x - base``, with the per-clip
        sums of the result when ``want_sums`` (the convergence deltas); ``FIN_MEAN``: the sum itself through the kernel; None:
        the sum as accumulated.  Returns ``(out, sums)``, unchecked.

        ``point_gradient(pts, row0) -> [rows, ...]`` is the gradient at the step-major rows ``pts`` (row ``row0 + r`` is step
        ``(row0 + r) // B`` of clip ``(row0 + r) % B``).  Whole steps per chunk (``_steps_per_chunk``); the schedule is padded
        with zero-weight copies of the last step to whole chunks, so every chunk has the same shape: one ``pts`` workspace that
        every chunk fills completely (hence ``torch.empty``), and one accumulate launch per chunk.  The gradient's rows need not
        have the points' shape (InternalInfluence: waveform points, layer gradients): the sum takes the gradient's."""
        B, n_steps = x.shape[0], len(alphas)
        per = _steps_per_chunk(B, n_steps, internal_batch_size)
        npad = -(-n_steps // per) * per
        alphas = np.concatenate([alphas, np.full(npad - n_steps, alphas[-1])])
        steps = np.concatenate([steps, np.zeros(npad - n_steps)])               # padding steps carry zero weight
        a_all, w_all = _step_major(alphas, B, x.device), _step_major(steps, B, x.device)
        d = _desc(x.view(B, -1), base.view(base.shape[0], -1), None, npad, 0)
        pts = torch.empty((per * B,) + x.shape[1:], dtype=torch.float32, device=x.device)
        total = dt = None
        for s0 in range(0, npad, per):
            _points(d, a_all, s0 * B, per * B, pts)
            g = point_gradient(pts, s0 * B)                                     # [per*B, ...], step-major
            if total is None:
                total = torch.zeros_like(g[:B])
                flat = total.view(B, -1)
                dt = d if flat.shape[1] == d.n else _desc(flat, flat, None, npad, 0)   # ACC_IG reads neither x nor the baseline
            _accumulate(dt, g, w_all, ACC_IG, s0 * B, per * B, total)
        if finalize is None:
            return total, None
        out = torch.empty_like(total)
        sums = torch.empty(B, dtype=torch.float32, device=x.device) if want_sums else None
        if finalize == FIN_MEAN:
            d.S = 1                                                             # FIN_MEAN with S = 1: the sum itself
        _accumulate(d, total, None, finalize, 0, B, out, sums)
        return out, sums

    def gradient_shap(self, waves, baselines, n_samples: int = 5, stdevs: float = 0.0, multiply_by_inputs: bool = True,
                      return_convergence_delta: bool = False, seed: Optional[int] = None, internal_batch_size: Optional[int] = None):
        """Captum's GradientShap (NoiseTunnel "smoothgrad" over InputBaselineXGradient): each clip is expanded to
        ``n_samples`` rows (clip-major, row ``b * S + s``); row g draws a baseline ``base[idx[g]]`` uniformly from
        ``baselines [N_b, L]`` (or a callable returning it, called with ``waves`` if it takes an argument), a coefficient
        ``alpha[g] ~ U[0, 1)`` and the noisy input ``x~ = x_b + stdevs * N(seed, g, :)``; the attribution is the mean over
        samples of ``(x~ - b) * dF/dx(b + alpha (x~ - b))`` (the gradient alone with ``multiply_by_inputs=False``).
        ``delta`` ``[B*S]`` (clip-major): ``sum_j (x~ - b)_j dF_j - (F(x~) - F(b))`` per expanded row.

        ``seed=None`` draws one from torch's default CPU generator (``draw_seed``); the host draws are ``shap_draws(seed, ...)``
        and the noise ``philox_normal(seed, ...)``, so a seed fixes the result bit for bit.  Captum's RNG stream is not
        reproduced (captum is absent)."""
        B, L = _dims(waves)
        base, S, seed, draws = self._shap_args(waves, baselines, B, L, n_samples, stdevs, seed, return_convergence_delta,
                                               multiply_by_inputs)
        x = self._prep(waves)
        dev = x.device
        base = _device_base(base, x)
        R = B * S
        row_sum = torch.empty(R, dtype=torch.float32, device=dev) if return_convergence_delta else None
        out, bidx, pts = self._expanded_samples(x, base, draws, S, stdevs, seed, multiply_by_inputs, internal_batch_size,
                                                self._row_gradient, row_sum)
        out = self._checked(out)
        chunk = pts.shape[0]
        if not return_convergence_delta:
            return out
        fb = self.logits(base).double()[bidx.long()]
        if stdevs == 0:
            fx = self.logits(x).double().repeat_interleave(S)
        else:                                  # F(x~): x~ = 0 + 1 * (x~ - 0) exactly, through the path-point kernel
            zero = torch.zeros((1, L), dtype=torch.float32, device=dev)
            dn = _desc(x, zero, None, S, 1, float(stdevs), seed)
            ones = torch.ones(R, dtype=torch.float32, device=dev)
            fx = torch.empty(R, dtype=torch.float64, device=dev)
            for row0 in range(0, R, chunk):
                rows = min(chunk, R - row0)
                _points(dn, ones, row0, rows, pts)
                fx[row0:row0 + rows] = self.logits(pts)[:rows].double()
        return out, (row_sum.double() - (fx - fb)).float()

    @staticmethod
    def _shap_args(waves, baselines, B: int, L: int, n_samples, stdevs, seed, return_convergence_delta: bool = False,
                   multiply_by_inputs: bool = True, internal_batch_size: Optional[int] = None):
        """The arguments of the expanded-sample methods after their own first checks, in the order the errors are promised:
        a callable ``baselines`` unwrapped, ``check_shap_args``, the delta and ``internal_batch_size`` checks of the method that
        passes them, the seed, then the host draws.  Returns ``(baselines [N_b, L], S, seed, shap_draws(...))``."""
        if callable(baselines) and not torch.is_tensor(baselines):
            baselines = baselines(waves) if inspect.signature(baselines).parameters else baselines()
        base = check_shap_args(baselines, B, L, n_samples, stdevs)
        _check_delta(return_convergence_delta, multiply_by_inputs)
        if internal_batch_size is not None:
            _positive_int(internal_batch_size, "internal_batch_size")
        seed, S = _check_seed(seed), int(n_samples)
        return base, S, seed, shap_draws(seed, B, S, base.shape[0])

    def _expanded_samples(self, x, base, draws, S: int, stdevs, seed: int, multiply_by_inputs: bool, internal_batch_size, row_gradient,
                          row_sum=None):
        """The one expanded-sample (GradientShap) loop over the clip-major rows ``b * S + s``: the mean over a clip's samples of
        ``(x~ - b) * row_gradient(b + alpha (x~ - b))`` (the gradient alone without ``multiply_by_inputs``), ``draws = (idx,
        alpha)`` from ``shap_draws``; ``row_sum [B * S]`` takes the per-row sums for the convergence delta.
        ``row_gradient(pts, row0, 1, S)`` as ``_row_gradient``.  Returns ``(out, bidx, pts)``, unchecked: the device copy of
        ``idx`` and the ``[chunk, L]`` workspace, which the delta reuses."""
        B, L = x.shape
        bidx, a_all = (torch.from_numpy(v).to(x.device) for v in draws)
        R = B * S
        chunk = min(internal_batch_size or 128, R)
        d = _desc(x, base, bidx, S, 1, float(stdevs), seed)
        total = torch.zeros_like(x)
        # one workspace shape: a short last chunk leaves the previous chunk's (finite) points in the rows it does not use
        # (unlike the path integrator, whose padded schedule fills every chunk whole)
        pts = torch.zeros((chunk, L), dtype=torch.float32, device=x.device)
        for row0 in range(0, R, chunk):
            rows = min(chunk, R - row0)
            _points(d, a_all, row0, rows, pts)
            g = row_gradient(pts, row0, 1, S)                                   # [chunk, L], clip-major
            _accumulate(d, g, None, ACC_SHAP if multiply_by_inputs else ACC_SHAP_GRAD, row0, rows, total, row_sum)
        out = torch.empty_like(x)
        _accumulate(d, total, None, FIN_MEAN, 0, B, out)
        return out, bidx, pts

    def occlusion(self, waves, window, stride=1, baselines=None, internal_batch_size: Optional[int] = None):
        """Captum's Occlusion (restated: captum is absent).  ``window``, ``stride``: ints (or 1-tuples); ``baselines``: None
        (zero), a number, ``[1, L]`` or ``[B, L]``.  ``K = occlusion_windows(L, window, stride)`` ablated rows per clip, row
        ``k * B + b`` holding the baseline in ``[k * stride, min(k * stride + window, L))`` and x elsewhere;
        ``diff[k, b] = F(x)[b] - F(ablated)[k, b]`` (fp32 logits) and ``attr[b, t]`` = the sum of ``diff[k, b]`` over the
        windows k covering t, in increasing k, divided by their count -- Captum's ``total_attrib / weights``, bit for bit
        given the same logits.  The ablated rows run through the forward ``internal_batch_size`` (default 128) at a time."""
        B, L = _dims(waves)
        win, stride, K = check_occlusion_args(L, window, stride)
        base = check_ig_baselines(baselines, B, L)
        chunk = check_internal_batch(internal_batch_size)
        x = self._prep(waves)
        base = _device_base(base, x)                          # a local: the descriptor holds the pointer only
        d = ablation_desc(x, base, ABL_OCCLUSION, K, win, stride)
        return self._ablate(x, K * B, chunk, functools.partial(ablation_points, d), functools.partial(ablation_accumulate, d),
                            "occlusion")

    def feature_ablation(self, waves, baselines=None, feature_mask=None, internal_batch_size: Optional[int] = None):
        """Captum's FeatureAblation (restated: captum is absent).  ``feature_mask``: None (each sample its own feature: L
        ablations) or an integer ``[1, L]`` / ``[B, L]`` tensor of feature ids; ``baselines`` as ``occlusion``.  Ablation k
        replaces the samples of the k-th id present (increasing id order) by the baseline in every clip at once, and
        ``attr[b, t] = F(x)[b] - F(ablated)[k(b, t), b]``."""
        B, L = _dims(waves)
        base = check_ig_baselines(baselines, B, L)
        index, K = feature_indices(feature_mask, B, L)
        chunk = check_internal_batch(internal_batch_size)
        x = self._prep(waves)
        base, index = _device_base(base, x), index.to(x.device).contiguous()   # locals: the descriptor holds the pointers only
        d = ablation_desc(x, base, ABL_FEATURE, K, mask=index)
        return self._ablate(x, K * B, chunk, functools.partial(ablation_points, d), functools.partial(ablation_accumulate, d),
                            "feature ablation")

    def _ablate(self, x, R: int, chunk: int, points, accumulate, what: str, cause: str = _ABLATION_CAUSE, value=None):
        """The one "perturbed rows -> values -> one accumulate launch" loop: ``points(row0, rows, out)`` builds the rows
        ``[row0, row0 + rows)`` of the ``R``, ``value(rows, row0) -> [rows]`` scores them (None: ``_row_logit``) and
        ``accumulate(f0, fk, attr)`` turns ``f0 = value(x) [B]`` and ``fk [R]`` into the attribution.  Every chunk has
        ``min(chunk, R)`` rows (the last one padded by ``points`` with copies of x), so one forward workspace serves them all.
        The tensors a descriptor behind ``points`` / ``accumulate`` points into are the caller's to keep alive."""
        chunk = min(chunk, R)
        pts = torch.empty((chunk, x.shape[1]), dtype=torch.float32, device=x.device)
        fk = self._row_logits(lambda row0, out: points(row0, chunk, out), 0, R, pts, value)
        f0 = (value or self._row_logit)(x)
        attr = torch.empty_like(x)
        accumulate(f0, fk, attr)
        return self._checked(attr, what, cause)

    def _row_logits(self, points, row0: int, R: int, pts: torch.Tensor, value=None) -> torch.Tensor:
        """Values of the perturbed rows ``[row0, row0 + R)``: ``points(first_row, pts)`` fills the ``[chunk, L]`` workspace,
        ``value(pts, first_row)`` (None: the classifier forward, ``_row_logit``) runs on it, and the values land in ``fk[:R]``
        (``fk`` has whole chunks: the rows past ``R`` of the last chunk are the kernels' padding, copies of x)."""
        value = value or self._row_logit
        chunk = pts.shape[0]
        nchunk = -(-R // chunk)
        fk = torch.empty(nchunk * chunk, dtype=torch.float32, device=pts.device)
        for c in range(nchunk):
            points(row0 + c * chunk, pts)
            fk[c * chunk:(c + 1) * chunk] = value(pts, row0 + c * chunk)
        return fk

    def perturbation_curve(self, waves, attributions, mode: str = "deletion", order: str = "morf", feature_mask=None, steps=None,
                           baselines=None, output: str = "prob", use_abs: bool = False, pool: str = "sum", seed: Optional[int] = None,
                           internal_batch_size: Optional[int] = None) -> PerturbationCurve:
        """The perturbation curve of an attribution map: features are removed (``mode="deletion"``: replaced by ``baselines``)
        or restored (``"insertion"``: starting from the baseline) in the order of their relevance, and the classifier's output
        is recorded along the way -- the deletion / insertion curves of Petsiuk et al. (RISE, 2018) and, through ``aopc``, the
        AOPC of Samek et al. (2017), i.e. DeYoung et al.'s (2020) comprehensiveness (deletion) and sufficiency (insertion).
        Restated from the papers: no Captum class exists, so parity is not pinned to one.

        ``attributions``: a floating ``[B, L]`` map of any method.  ``feature_mask`` / ``baselines`` / ``internal_batch_size`` as
        ``shapley_value_sampling`` (ids >= 0; every clip must hold every feature).  A feature's score is the sum (``pool="mean"``:
        the average) of its samples' attributions (``use_abs``: magnitudes), in fp32 in increasing sample order.  ``order``:
        ``"morf"`` most relevant first, ``"lerf"`` least relevant first -- equal scores go lower feature number first in both --
        or ``"random"``: one uniform permutation per clip drawn on the host from ``seed`` (``shapley_permutations``' stream), the
        chance-level curve the other two are read against.  ``steps``: see ``curve_counts``; step j switches the ``c_j`` first
        features of each clip's own order, so row ``j * B + b`` is clip b with those features at the baseline (deletion) or only
        those features present (insertion).  ``output``: ``"prob"`` (the sigmoid of the logit) or ``"logit"``.

        Returns a ``PerturbationCurve``: ``curve [B, S + 1]``, ``fractions = c / K``, ``auc`` (trapezoid over the fractions,
        divided by their span) and ``aopc = mean_j (y_ref - y_j)`` over the S steps other than the reference step, the one that
        equals the clip itself (step 0 of a deletion, step S of an insertion) -- no separate ``F(x)`` forward is run.  The
        ``(S + 1) * B`` rows go through the forward ``internal_batch_size`` (default 128) at a time."""
        plan = self._curve_plan(waves, attributions, feature_mask, steps, baselines, use_abs, pool, internal_batch_size)
        m, o, p = _one_of(mode, CURVE_MODES, "mode"), _one_of(order, CURVE_ORDERS, "order"), _one_of(output, CURVE_OUTPUTS, "output")
        rank = None
        if order == "random":
            rank = torch.from_numpy(_permutation_stream(_check_seed(seed))(plan["B"], plan["K"]))
        self._curve_upload(plan, waves, attributions)
        if rank is None:
            rank = self._curve_rank(plan, descending=o == 0)
        return self._curve(plan, rank.to(plan["x"].device), m, p == 0)

    def curve_summary(self, waves, attributions, feature_mask=None, steps=None, baselines=None, use_abs: bool = False, pool: str = "sum",
                      internal_batch_size: Optional[int] = None) -> dict:
        """Deletion and insertion curves in MoRF order on the probability, from one shared rank: ``{"deletion_auc",
        "insertion_auc", "comprehensiveness", "sufficiency"}``, each ``[B]`` -- comprehensiveness is the deletion AOPC (how far
        removing the most relevant features drops the output: higher is better), sufficiency the insertion AOPC (how far the
        most relevant features alone fall short of it: lower is better).  Arguments as ``perturbation_curve``."""
        plan = self._curve_plan(waves, attributions, feature_mask, steps, baselines, use_abs, pool, internal_batch_size)
        self._curve_upload(plan, waves, attributions)
        rank = self._curve_rank(plan, descending=True)
        dele, ins = self._curve(plan, rank, 0, True), self._curve(plan, rank, 1, True)
        return {"deletion_auc": dele.auc, "insertion_auc": ins.auc, "comprehensiveness": dele.aopc, "sufficiency": ins.aopc}

    def _curve_plan(self, waves, attributions, feature_mask, steps, baselines, use_abs, pool, internal_batch_size) -> dict:
        """Every argument check of the perturbation curve, on the host, before any GPU work."""
        B, L = _dims(waves)
        if _dims(_float_tensor(attributions, "attributions")) != (B, L):
            raise ValueError(f"attributions must be [{B}, {L}] like the inputs; got {list(attributions.shape)}")
        base = check_ig_baselines(baselines, B, L)
        index, K = shapley_feature_indices(feature_mask, B, L)
        check_curve_features(index, K)
        chunk = check_internal_batch(internal_batch_size)
        if not isinstance(use_abs, (bool, np.bool_)):
            raise ValueError(f"use_abs must be a bool, not {use_abs!r}")
        return {"B": B, "L": L, "K": K, "base": base, "index": None if feature_mask is None else index, "chunk": chunk,
                "counts": curve_counts(steps, K), "use_abs": bool(use_abs), "mean": _one_of(pool, CURVE_POOLS, "pool") == 1}

    def _curve_upload(self, plan: dict, waves, attributions) -> None:
        x = self._prep(waves)
        plan["x"], plan["attr"] = x, self._prep(attributions)
        plan["base"] = _device_base(plan["base"], x)
        if plan["index"] is not None:
            plan["index"] = plan["index"].to(x.device).contiguous()
        plan["counts_dev"] = torch.from_numpy(plan["counts"]).to(x.device)

    def _curve_rank(self, plan: dict, descending: bool) -> torch.Tensor:
        score = feature_scores(plan["attr"], plan["index"], plan["K"], plan["use_abs"], plan["mean"])
        if not bool(torch.isfinite(score).all()):
            raise ValueError("attributions must be finite: a feature's score is inf or NaN")
        return feature_rank(score, descending)

    def _curve(self, plan: dict, rank: torch.Tensor, mode: int, prob: bool) -> PerturbationCurve:
        """The chunk loop of one curve: rows -> forward logits -> one fold launch."""
        x, B, K, counts = plan["x"], plan["B"], plan["K"], plan["counts_dev"]
        R = counts.numel() * B
        chunk = min(plan["chunk"], R)
        d = curve_desc(x, plan["base"], plan["index"], rank, counts, mode)
        pts = torch.empty((chunk, x.shape[1]), dtype=torch.float32, device=x.device)
        fk = self._row_logits(lambda row0, out: curve_points(d, row0, chunk, out), 0, R, pts)
        curve, auc, aopc = curve_fold(fk, counts, B, K, prob, ref_last=mode == 1)
        self._checked(curve, "perturbation curve", "a logit of the clips or of their perturbed rows is not finite (check the "
                                                   "inputs and baselines)")
        fractions = torch.from_numpy(plan["counts"].astype(np.float64) / K).to(x.device)
        return PerturbationCurve(curve, fractions, auc, aopc, rank)

    def _shapley_args(self, waves, baselines, feature_mask, internal_batch_size):
        B, L = _dims(waves)
        base = check_ig_baselines(baselines, B, L)
        index, K = shapley_feature_indices(feature_mask, B, L)
        chunk = check_internal_batch(internal_batch_size)
        return base, index, K, chunk

    def shapley_value_sampling(self, waves, baselines=None, feature_mask=None, n_samples: int = 25, seed: Optional[int] = None,
                               internal_batch_size: Optional[int] = None):
        """Captum's ShapleyValueSampling (restated: captum is absent).  ``feature_mask``: None (each sample its own feature) or
        an integer ``[1, L]`` / ``[B, L]`` tensor of ids >= 0; the K ids present are the features (ranked as
        ``feature_indices`` ranks them).  ``baselines`` as ``occlusion``.  ``n_samples`` permutations are drawn on the host
        (``shapley_permutations(seed, ...)``; ``seed=None`` draws one from torch's default CPU generator, so ``torch.manual_seed``
        reproduces a run).  Along permutation p, step j switches feature ``perm_p[j]`` from the baseline to x in every clip at
        once: row ``(p * K + j) * B + b``; ``diff[p][j][b] = F(row p, j) - F(row p, j - 1)`` with ``F(row p, -1) = F(base)``
        (one forward over B rows), and ``attr[b, t] = (sum_p diff[p][rank_p(id(b, t))][b]) / n_samples``, summed in
        increasing p from 0 in fp32 and divided once -- Captum's ``total_attrib += eval_diff * mask; total_attrib /
        iter_count``, bit for bit given the same logits.  The rows run through the forward ``internal_batch_size`` (default 128)
        at a time, in groups of whole permutations (``GROUP_ROWS``)."""
        base, index, K, chunk = self._shapley_args(waves, baselines, feature_mask, internal_batch_size)
        P = check_n_samples(n_samples)
        draw = _permutation_stream(_check_seed(seed))
        return self._shapley(waves, base, index, K, P, lambda G: draw(G, K), chunk)

    def shapley_values(self, waves, baselines=None, feature_mask=None, internal_batch_size: Optional[int] = None):
        """Captum's ShapleyValues: ``shapley_value_sampling`` over all K! permutations in ``itertools.permutations`` order,
        divided by K!.  The permutations are streamed in groups; more than 10 features warn (UserWarning), as Captum does."""
        base, index, K, chunk = self._shapley_args(waves, baselines, feature_mask, internal_batch_size)
        if K > 10:
            warnings.warn(f"ShapleyValues with {K} features evaluates {K}! permutations; consider ShapleyValueSampling", UserWarning)
        return self._shapley(waves, base, index, K, math.factorial(K), exact_permutation_stream(K), chunk)

    def _shapley(self, waves, base, index, K: int, P: int, draw, chunk: int):
        """The permutation loop: groups of G whole permutations (G * K * B <= max(GROUP_ROWS, chunk) rows, at least one), each
        ``draw(G) -> rank [G, K]``, its rows through ``_row_logits`` and one accumulate launch; the last one divides by P."""
        x = self._prep(waves)
        B, L = x.shape
        dev = x.device
        base = _device_base(base, x)
        index = index.to(dev).contiguous()
        kb = K * B
        G = max(1, min(P, max(GROUP_ROWS, chunk) // kb))
        pts = torch.empty((min(chunk, G * kb), L), dtype=torch.float32, device=dev)
        fbase = self._row_logit(base.expand(B, L).contiguous())
        total = torch.zeros_like(x)
        for p0 in range(0, P, G):
            g = min(G, P - p0)
            rank = torch.from_numpy(draw(g)).to(dev)
            d = coalition_desc(x, base, index, K, rank=rank, p0=p0)
            fk = self._row_logits(lambda row0, out: coalition_points(d, row0, out.shape[0], out), p0 * kb, g * kb, pts)
            shapley_accumulate(d, fbase, fk, p0, g, total, float(np.float32(P)) if p0 + g == P else 0.0)
        return self._checked(total, "Shapley attribution", "a logit of the clips, the baselines or a coalition is not finite "
                                                           "(check the inputs and baselines)")

    def kernel_shap(self, waves, baselines=None, feature_mask=None, n_samples: int = 25, seed: Optional[int] = None,
                    internal_batch_size: Optional[int] = None, return_input_shape: bool = True):
        """Captum's KernelShap (restated: captum is absent).  Each clip is fitted on its own, over the ids >= 0 present in it
        (``kernel_shap_feature_indices``; K_b >= 2): ``n_samples`` (>= 2) coalitions ``z`` are drawn on the host
        (``kernel_shap_draws(seed, ...)``: all ones, all zeros, then sizes with the Shapley kernel's law and uniform subsets),
        row ``s * B + b`` keeps x on the features of ``z_b[s]`` and the baseline elsewhere, and the logits are fitted by
        ``kernel_shap_fit`` (weights 1e6 on the two end coalitions, 1 elsewhere; float64 on the host).  ``attr[b, t] =
        coef_b[id(b, t)]`` in fp32; ``return_input_shape=False`` returns the ``[K]`` coefficients of a single clip."""
        fit = self._kernel_shap_fit(waves, baselines, feature_mask, n_samples, seed, internal_batch_size, return_input_shape)
        x, d, coefs = fit["x"], fit["desc"], fit["coef"]
        B = x.shape[0]
        if not return_input_shape:
            return torch.from_numpy(coefs[0].astype(np.float32)).to(x.device)
        coef = np.zeros((B, d.K), np.float32)
        for b, c in enumerate(coefs):
            coef[b, :c.shape[0]] = c
        coef = torch.from_numpy(coef).to(x.device)
        attr = torch.empty_like(x)
        coalition_scatter(d, coef, attr)
        return self._checked(attr, "KernelShap attribution", "a logit of the clips or of a coalition is not finite "
                                                             "(check the inputs and baselines)")

    def _kernel_shap_fit(self, waves, baselines, feature_mask, n_samples, seed, internal_batch_size, return_input_shape=True):
        """KernelShap up to the per-clip fits: a dict with the draws ``z`` (per clip ``[S, K_b]``), the logits ``y`` ``[S, B]``
        float64, ``coef`` (per clip ``[K_b]`` float64), ``intercept`` ``[B]``, the seed, and the device state (``x``, ``desc`` and
        the tensors it points into)."""
        B, L = _dims(waves)
        base = check_ig_baselines(baselines, B, L)
        index, Ks = kernel_shap_feature_indices(feature_mask, B, L)
        S = check_n_samples(n_samples, 2)
        chunk = check_internal_batch(internal_batch_size)
        if not return_input_shape and B > 1:
            raise ValueError("return_input_shape=False returns one clip's coefficients: pass a single clip")
        seed = _check_seed(seed)
        z = kernel_shap_draws(seed, Ks, S)
        Kmax = max(Ks)
        table = np.zeros((S * B, Kmax), np.uint8)
        for b, zb in enumerate(z):
            table[b::B, :Ks[b]] = zb                                                        # row s * B + b
        x = self._prep(waves)
        dev = x.device
        base = _device_base(base, x)
        present = torch.from_numpy(table).to(dev)
        index = index.to(dev).contiguous()
        d = coalition_desc(x, base, index, Kmax, present=present)
        pts = torch.empty((min(chunk, S * B), L), dtype=torch.float32, device=dev)
        fk = self._row_logits(lambda row0, out: coalition_points(d, row0, out.shape[0], out), 0, S * B, pts)
        y = fk[:S * B].view(S, B).double().cpu().numpy()
        fits = [kernel_shap_fit(z[b], y[:, b]) for b in range(B)]
        return {"x": x, "desc": d, "z": z, "y": y, "seed": seed, "coef": [c for c, _ in fits],
                "intercept": np.array([i for _, i in fits]), "tensors": (base, present, index)}   # the desc points into them

    def lime(self, waves, baselines=None, feature_mask=None, n_samples: int = 50, seed: Optional[int] = None,
             internal_batch_size: Optional[int] = None, return_input_shape: bool = True, interpretable_model=None,
             similarity_func=None, perturb_func=None):
        """Captum's Lime (restated from Captum 0.7's ``attr/_core/lime.py``: captum is absent).  Each clip is fitted on its own
        over the integer ids present in it, negative ids included (``per_clip_feature_indices``; Captum also fits columns for the
        ids of ``[min, max]`` absent from a clip, which touch no sample: they are left out).  ``n_samples`` interpretable samples
        ``z [S, K_b]`` per clip: ``perturb_func=None`` draws Captum's Bernoulli(0.5) on the host (``lime_draws(seed, ...)``;
        ``seed=None`` draws one from torch's default CPU generator); a callable is called once per sample, clip by clip, as
        ``perturb_func(x_b [1, L], num_interp_features=K_b, baselines=base_b, feature_mask=index_b [1, L])`` and returns a
        ``[1, K_b]`` 0/1 tensor.  Row ``s * B + b`` keeps x on the features that are on and the baseline elsewhere (KernelShap's
        presence rows, advh_coalition_points); ``baselines`` as ``occlusion``.

        The weight of a row is ``similarity_func(x_b, row, z)``: None is ``ExpKernelSimilarity("cosine", 1.0)``, and an
        ``ExpKernelSimilarity`` runs on the device over the chunk the forward reads (advh_row_similarity, the raw waveform row
        before the classifier's own normalisation, as Captum passes it); any other callable is called once per row, in row order,
        on device slices ``(x_b [1, L], row [1, L], z [1, K_b], num_interp_features=, baselines=, feature_mask=)``.  The logits
        y and the weights w are fitted clip by clip as Captum does: ``interpretable_model.fit(DataLoader(TensorDataset(z, y, w),
        batch_size=S))`` (float32 tensors), then ``representation()`` ``[1, K_b]``; None is ``SkLearnLasso(alpha=0.01)``
        (addvisor_hip.linear_model, whose three models get the same arrays through ``fit_arrays``, without the DataLoader's
        per-sample collation).  ``attr[b, t] = coef_b[id(b, t)]`` in fp32 (advh_coalition_scatter);
        ``return_input_shape=False`` returns the ``[1, K]`` coefficients of a single clip.  The rows run through the forward
        ``internal_batch_size`` (default 128) at a time.  Raises FloatingPointError when a logit is not finite or a clip's weights
        sum to zero (an underflowing kernel), ValueError on bad arguments before any GPU work."""
        fit = self._lime_fit(waves, baselines, feature_mask, n_samples, seed, internal_batch_size, return_input_shape,
                             interpretable_model, similarity_func, perturb_func)
        x, d, coefs = fit["x"], fit["desc"], fit["coef"]
        B = x.shape[0]
        if not return_input_shape:
            return torch.from_numpy(coefs[0]).view(1, -1).to(x.device)
        coef = np.zeros((B, d.K), np.float32)
        for b, c in enumerate(coefs):
            coef[b, :c.shape[0]] = c
        attr = torch.empty_like(x)
        coalition_scatter(d, torch.from_numpy(coef).to(x.device), attr)
        return self._checked(attr, "Lime attribution", "an interpretable model's coefficient is not finite")

    def _lime_fit(self, waves, baselines=None, feature_mask=None, n_samples=50, seed=None, internal_batch_size=None,
                  return_input_shape=True, interpretable_model=None, similarity_func=None, perturb_func=None):
        """Lime up to the per-clip fits: a dict with the draws ``z`` (per clip ``[S, K_b]`` uint8), the logits ``y`` and the
        weights ``w`` (``[S, B]`` float32, row ``s * B + b``), ``coef`` (per clip ``[K_b]`` float32, the representation), the
        seed, and the device state (``x``, ``desc`` and the tensors it points into)."""
        B, L = _dims(waves)
        base = check_ig_baselines(baselines, B, L)
        index, Ks = per_clip_feature_indices(feature_mask, B, L)
        S = check_n_samples(n_samples)
        chunk = check_internal_batch(internal_batch_size)
        if not return_input_shape and B > 1:
            raise ValueError("return_input_shape=False returns one clip's coefficients: pass a single clip")
        check_lime_callables(similarity_func, perturb_func, interpretable_model)
        sim_fn = ExpKernelSimilarity() if similarity_func is None else similarity_func
        on_device = isinstance(sim_fn, ExpKernelSimilarity)
        if interpretable_model is None:
            from .linear_model import SkLearnLasso
            interpretable_model = SkLearnLasso(alpha=0.01)
        seed = _check_seed(seed)
        x = self._prep(waves)
        dev = x.device
        base = _device_base(base, x)
        index = index.to(dev).contiguous()
        base_of = lambda b: base[0 if base.shape[0] == 1 else b][None]
        index_of = lambda b: index[0 if index.shape[0] == 1 else b][None].long()
        kw_of = lambda b: {"num_interp_features": Ks[b], "baselines": base_of(b), "feature_mask": index_of(b)}
        z = lime_draws(seed, Ks, S) if perturb_func is None else self._lime_user_draws(perturb_func, x, Ks, S, kw_of)
        Kmax = max(Ks)
        table = np.zeros((S * B, Kmax), np.uint8)
        for b, zb in enumerate(z):
            table[b::B, :Ks[b]] = zb                                                        # row s * B + b
        present = torch.from_numpy(table).to(dev)
        d = coalition_desc(x, base, index, Kmax, present=present)
        R = S * B
        pts = torch.empty((min(chunk, R), L), dtype=torch.float32, device=dev)
        if on_device:
            mode, width = check_kernel(sim_fn.distance_mode, sim_fn.kernel_width)
            sim = torch.empty(R, dtype=torch.float32, device=dev)
        else:
            zt = [torch.from_numpy(zb).to(dev, torch.long) for zb in z]
            sim = np.empty(R, np.float32)

        def points(row0, out):
            coalition_points(d, row0, out.shape[0], out)
            n = min(out.shape[0], R - row0)
            if on_device:                                   # the chunk the forward reads next, on the same stream
                row_similarity(out, x, row0, n, mode, width, sim)
                return
            for r in range(n):
                g = row0 + r
                b, s = g % B, g // B
                v = sim_fn(x[b][None], out[r][None], zt[b][s][None], **kw_of(b))
                v = torch.as_tensor(v).reshape(-1)
                if v.numel() != 1:
                    raise ValueError(f"similarity_func must return one number per row, not {v.numel()}")
                sim[g] = float(v[0])

        fk = self._row_logits(points, 0, R, pts)
        self._checked(fk[:R], "Lime logits", "a logit of the clips or of a perturbed row is not finite (check the inputs and "
                                             "baselines)")
        y = fk[:R].view(S, B).cpu().numpy()
        w = (sim.cpu().numpy() if on_device else sim).reshape(S, B)
        what = f"kernel_width={sim_fn.kernel_width}" if on_device else f"similarity_func={sim_fn!r}"
        for b in range(B):
            wb = w[:, b].astype(np.float64)
            if not np.isfinite(wb).all():
                raise FloatingPointError(f"non-finite Lime similarity weight in clip {b} ({what})")
            if wb.sum() == 0:
                raise FloatingPointError(f"the Lime similarity weights of clip {b} sum to zero ({what}): the kernel underflows "
                                         "for every perturbed row; widen it")
        from torch.utils.data import DataLoader, TensorDataset
        from .linear_model import _SkLearnModel
        coefs = []
        for b in range(B):
            zb, yb, wb = z[b].astype(np.float32), y[:, b].copy(), w[:, b].copy()
            if isinstance(interpretable_model, _SkLearnModel):     # the arrays the DataLoader would hand it, without the collation
                interpretable_model.fit_arrays(zb, yb, wb)
            else:
                interpretable_model.fit(DataLoader(TensorDataset(torch.from_numpy(zb), torch.from_numpy(yb), torch.from_numpy(wb)),
                                                   batch_size=S))
            c = torch.as_tensor(interpretable_model.representation()).detach().to("cpu", torch.float32).reshape(-1)
            if c.numel() != Ks[b]:
                raise ValueError(f"interpretable_model.representation() must hold {Ks[b]} coefficients, not {c.numel()}")
            coefs.append(c.numpy())
        return {"x": x, "desc": d, "z": z, "y": y, "w": w, "seed": seed, "coef": coefs, "tensors": (base, present, index)}

    @staticmethod
    def _lime_user_draws(perturb_func, x, Ks, S, kw_of) -> list:
        """A user perturb_func's samples, ``S`` calls per clip in clip order, each a ``[1, K_b]`` 0/1 tensor (ValueError
        otherwise)."""
        out = []
        for b, K in enumerate(Ks):
            zb = np.empty((S, K), np.uint8)
            for s in range(S):
                v = perturb_func(x[b][None], **kw_of(b))
                v = torch.as_tensor(v).detach().cpu().reshape(-1)
                if v.numel() != K or not bool(((v == 0) | (v == 1)).all()):
                    raise ValueError(f"perturb_func must return a [1, {K}] tensor of zeros and ones")
                zb[s] = v.numpy()
            out.append(zb)
        return out

    def feature_permutation(self, waves, feature_mask=None, seed: Optional[int] = None, internal_batch_size: Optional[int] = None):
        """Captum's FeaturePermutation (restated from Captum 0.7's ``attr/_core/feature_permutation.py``: captum is absent):
        FeatureAblation with the baseline of each feature taken from another clip of the batch.  ``feature_mask``: None (each
        sample its own feature) or one integer ``[1, L]`` mask; ``B >= 2`` (Captum's asserts, ValueError).  For feature k a
        uniform permutation ``perm_k`` of the clips that is not the identity is drawn on the host
        (``feature_permutation_draws(seed, ...)``; ``seed=None`` draws one from torch's default CPU generator); row ``k * B + b``
        is ``x[b]`` with the samples of feature k taken from ``x[perm_k[b]]`` (advh_permutation_points, FeatureAblation's
        perturbation-major order), and ``attr[b, t] = F(x)[b] - F(row k(t), b)`` -- advh_ablation_accumulate in FeatureAblation
        mode, its arithmetic bit for bit.  The rows run through the forward ``internal_batch_size`` (default 128) at a time."""
        B, L = _dims(waves)
        index, K = check_permutation_args(feature_mask, B, L)
        chunk = check_internal_batch(internal_batch_size)
        perm = feature_permutation_draws(_check_seed(seed), K, B)
        x = self._prep(waves)
        index = index.to(x.device).contiguous()
        pd = permutation_desc(x, index, torch.from_numpy(perm).to(x.device))
        ad = ablation_desc(x, x, ABL_FEATURE, K, mask=index)                  # the accumulate reads the mask only
        return self._ablate(x, K * B, chunk, functools.partial(permutation_points, pd), functools.partial(ablation_accumulate, ad),
                            "feature permutation")

    def noise_tunnel(self, waves, attribute, nt_type: str = "smoothgrad", nt_samples: int = 5,
                     nt_samples_batch_size: Optional[int] = None, stdevs: float = 1.0, draw_baseline_from_distrib: bool = False,
                     seed: Optional[int] = None, return_convergence_delta: bool = False, **kwargs):
        """Captum's NoiseTunnel (restated from Captum 0.7's ``noise_tunnel.py``: captum is absent) around ``attribute``, the
        callable that attributes a ``[rows, L]`` batch (an engine method, or a ``captum.attr`` shim object's ``attribute``).
        The S = ``nt_samples`` samples of each clip run in partitions of ``p = min(S, nt_samples_batch_size or S)`` (the last
        one holds ``S mod p``); partition ``[s0, s0 + p')`` attributes ``B * p'`` rows, row ``b * p' + s'`` =
        ``x_b + stdevs * N(seed, b * S + s0 + s', :)`` (``nt_noisy_rows``), with ``kwargs`` expanded by
        ``noise_tunnel_kwargs``; with ``draw_baseline_from_distrib`` row (b, s) takes ``baselines[idx[b * S + s]]``
        (``noise_tunnel_baseline_draws``).  The attributions a are folded into fp64 sums on the device (advh_nt_fold) and
        finalized (advh_nt_finalize): ``smoothgrad`` E[a], ``smoothgrad_sq`` E[a^2], ``vargrad`` E[a^2] - E[a]^2.

        ``seed=None`` draws one from torch's default CPU generator before any wrapped call, so a wrapped method that draws its
        own seed draws it afterwards, once per partition, and ``torch.manual_seed`` reproduces the whole call.
        ``return_convergence_delta`` needs an ``attribute`` that takes it (IntegratedGradients, GradientShap, or a callable
        with ``**kwargs`` that passes it on) and returns
        ``(attr, delta)``, delta = the wrapped deltas concatenated in partition order."""
        B, L = _dims(waves)
        S, p, sigma = check_noise_tunnel_args(nt_type, nt_samples, nt_samples_batch_size, stdevs)
        if return_convergence_delta:
            params = inspect.signature(attribute).parameters
            if "return_convergence_delta" not in params and not any(v.kind is v.VAR_KEYWORD for v in params.values()):
                raise ValueError("return_convergence_delta=True needs a wrapped method with a convergence delta "
                                 "(IntegratedGradients, GradientShap)")
            kwargs["return_convergence_delta"] = True
        dist = check_baseline_distribution(kwargs.get("baselines"), L) if draw_baseline_from_distrib else None
        seed = _check_seed(seed)
        idx = noise_tunnel_baseline_draws(seed, B, S, dist.shape[0]) if dist is not None else None
        x = self._prep(waves)
        total = torch.zeros((B, L), dtype=torch.float64, device=x.device)
        total_sq = torch.zeros_like(total)
        rows = torch.empty((B * p, L), dtype=torch.float32, device=x.device)
        deltas = []
        for s0, pp in noise_tunnel_partitions(S, p):
            noisy = nt_noisy_rows(x, seed, S, s0, pp, sigma, rows[:B * pp])
            drawn = idx[noise_tunnel_rows(B, S, s0, pp)] if idx is not None else None
            res = attribute(noisy, **noise_tunnel_kwargs(kwargs, B, pp, drawn))
            if return_convergence_delta:
                res, delta = res
                deltas.append(delta)
            if not torch.is_tensor(res) or tuple(res.shape) != (B * pp, L):
                raise ValueError(f"the wrapped method must return a [{B * pp}, {L}] attribution of the noisy rows, "
                                 f"not {tuple(res.shape) if torch.is_tensor(res) else type(res).__name__}")
            nt_fold(res.to(x.device, torch.float32).contiguous(), B, pp, total, total_sq)
        out = self._checked(nt_finalize(total, total_sq, S, nt_type), "NoiseTunnel attribution")
        return (out, torch.cat(deltas)) if return_convergence_delta else out

    def infidelity(self, waves, perturb_func, attributions, baselines=None, n_perturb_samples: int = 10,
                   max_examples_per_batch: Optional[int] = None, normalize: bool = False, seed: Optional[int] = None,
                   internal_batch_size: Optional[int] = None, target=None, additional_forward_args=None) -> torch.Tensor:
        """Captum's infidelity (Yeh et al., NeurIPS 2019; restated from Captum 0.7's ``metrics/_core/infidelity.py``: captum is
        absent) of ``attributions [B, L]`` of the classifier logit F, ``[B]`` fp32.  The S = ``n_perturb_samples`` samples of
        each clip run in Captum's chunks (``metric_partitions`` of ``max_examples_per_batch``); chunk ``[s0, s0 + p')`` has
        ``B * p'`` rows, row ``b * p' + s'`` (``repeat_interleave``).  ``perturb_func(inputs_expanded[, baselines_expanded])``
        returns ``(perturbation, perturbed_inputs)``, ``[B * p', L]`` each (``baselines`` expanded by
        ``expand_metric_baselines``); per row ``a = sum_j perturbation_j * attr_b,j`` and ``d = F(x_b) - F(x~)`` (fp32).  The
        result is ``sum_s (a - d)^2 / S``, or with ``normalize`` ``(beta^2 sum a^2 - 2 beta sum a d + sum d^2) / S`` with
        ``beta = safe_div(sum a d, sum a^2, 1)``: the sums are fp64 on the device in sample order (advh_infidelity_fold), so
        they do not depend on the chunking; only the forward's logits can.  The perturbed rows go through the forward
        ``internal_batch_size`` (default 128) at a time.

        A ``NoisyPerturbation`` runs fused: row (b, s) = ``x_b - stdevs * N(seed, b * S + s, :)`` written into the forward's
        workspace with its dot product (advh_metric_rows); any other callable is called once per chunk (the generic path).
        ``seed=None`` draws one from torch's default CPU generator first, so ``torch.manual_seed`` reproduces a call; Captum's
        own RNG stream is not reproduced.  The perturbed rows share one forward workspace of
        ``min(internal_batch_size, B * p_0)`` rows (p_0: the first chunk's samples); a chunk with fewer rows forwards only its
        own, and the last forward batch inside a chunk is padded to the workspace with the previous batch's rows, as
        ``_row_logits`` pads.  A Python perturb_func is called for the first chunk before the forward of the clips, so that a
        result of the wrong shape raises ValueError before any GPU work.  Raises ValueError on bad arguments before any GPU
        work, FloatingPointError (or SplitRangeError) when a logit or the attribution is not finite."""
        B, L, S, plan = check_metric_args(waves, n_perturb_samples, max_examples_per_batch, target, additional_forward_args,
                                          attributions)
        if not callable(perturb_func):
            raise ValueError("perturb_func must be callable")
        if baselines is not None:
            check_ig_baselines(baselines, B, L)
        chunk = check_internal_batch(internal_batch_size)
        fused = isinstance(perturb_func, NoisyPerturbation)
        seed = _check_seed(seed)
        x = self._prep(waves)
        dev = x.device
        attr = attributions.to(dev, torch.float32).contiguous()
        base = baselines.to(dev, torch.float32) if torch.is_tensor(baselines) else baselines
        if fused and perturb_func.multiply_by_inputs and base is not None:
            base = _device_base(check_ig_baselines(baselines, B, L), x)                         # a number -> [1, L]

        def generic(pp):
            """The chunk's ``(perturbation, perturbed rows)`` from the Python perturb_func, shapes checked."""
            R = B * pp
            be = expand_metric_baselines(base, B, L, pp)
            xe = x.repeat_interleave(pp, 0)
            res = perturb_func(xe, be) if be is not None else perturb_func(xe)
            if not isinstance(res, (tuple, list)) or len(res) != 2:
                raise ValueError("perturb_func must return (perturbations, perturbed_inputs)")
            pert, xt = (t[0] if isinstance(t, (tuple, list)) and len(t) == 1 else t for t in res)
            for t, what in ((pert, "perturbations"), (xt, "perturbed inputs")):
                if not torch.is_tensor(t) or tuple(t.shape) != (R, L):
                    raise ValueError(f"perturb_func must return [{R}, {L}] {what}, "
                                     f"not {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
            return pert.to(dev, torch.float32).contiguous(), xt.to(dev, torch.float32).contiguous()

        first = None if fused else generic(plan[0][1])      # a perturb_func of the wrong shape raises before the forward
        acc = torch.zeros(3 * B if normalize else B, dtype=torch.float64, device=dev)
        f0 = self.eg.emb.forward(x, want_hidden=False)[1].view(-1)
        # one workspace for every chunk: the first chunk fills it whole, a shorter chunk leaves the previous (finite) rows behind
        pts = torch.empty((min(chunk, B * plan[0][1]), L), dtype=torch.float32, device=dev)
        for k, (s0, pp) in enumerate(plan):
            R = B * pp
            if fused:
                d = metric_desc(x, seed, S, s0, pp, MR_GAUSS, perturb_func.stdevs, attr,
                                base if perturb_func.multiply_by_inputs else None, perturb_func.multiply_by_inputs)
                dot = torch.empty(R, dtype=torch.float32, device=dev)
                fill = lambda row0, out, d=d, dot=dot, R=R: metric_rows(d, row0, min(out.shape[0], R - row0), out, dot)
            else:
                pert, xt = first if k == 0 else generic(pp)
                dot = metric_row_dot(pert, attr, pp)
                fill = lambda row0, out, xt=xt, R=R: out[:min(out.shape[0], R - row0)].copy_(xt[row0:row0 + out.shape[0]])
            fk = self._row_logits(fill, 0, R, pts if R >= pts.shape[0] else pts[:R])
            infidelity_fold(dot, f0, fk, B, pp, normalize, acc)
        return self._checked(infidelity_finalize(acc, B, S, normalize), "infidelity",
                             "a logit of the clips or of their perturbations, or the attribution, is not finite")

    def sensitivity_max(self, explain, waves, perturb_func=None, perturb_radius: float = 0.02, n_perturb_samples: int = 10,
                        norm_ord="fro", max_examples_per_batch: Optional[int] = None, seed: Optional[int] = None, **kwargs):
        """Captum's sensitivity_max (restated from Captum 0.7's ``metrics/_core/sensitivity.py``: captum is absent), ``[B]``
        fp32: ``e = explain(x, **kwargs)``; the S = ``n_perturb_samples`` samples of each clip run in Captum's chunks
        (``metric_partitions``), chunk ``[s0, s0 + p')`` explains its ``B * p'`` perturbed rows (row ``b * p' + s'``) with
        ``explain(x~, **kwargs_expanded)`` (``sensitivity_kwargs``: a ``[B, L]`` baseline is ``repeat_interleave``d, every other
        argument passes unchanged), and the result is ``max_s ||e_b - e~||_ord / ||e_b||_ord`` (a zero norm counts as 1) over a
        fixed tree on the device (advh_sensitivity_fold).  ``norm_ord``: "fro" / 2, 1 or inf.  ``explain`` is any callable
        attributing a ``[R, L]`` tensor (an engine method, a ``captum.attr`` object's ``attribute``, ``NoiseTunnel.attribute``).

        ``perturb_func=None`` (Captum's ``default_perturb_func``, ``x + U(-r, r)``) runs on the device: row (b, s) =
        ``x_b + r * (2u - 1)``, u from the Philox words of row ``b * S + s`` (advh_metric_rows), so the rows do not depend on the
        chunking.  A callable gets the expanded inputs (and ``perturb_radius`` if it takes two parameters) and returns the
        perturbed inputs.  Unlike Captum, which explains the clips first, the first chunk's perturbation is made before the
        explanation of the clips, so that a perturb_func result of the wrong shape raises ValueError before any explanation
        runs.  ``target`` and ``additional_forward_args`` must be None and are not passed on to ``explain``.  ``seed=None``
        draws one from torch's default CPU generator before ``explain`` runs, so a method that draws its own seed draws it
        afterwards and ``torch.manual_seed`` reproduces the call; Captum's RNG stream is not reproduced."""
        return sensitivity_max(explain, waves, self.emb.dev, perturb_func, perturb_radius, n_perturb_samples, norm_ord,
                               max_examples_per_batch, seed, **kwargs)

    # ------------------------------------------------------------------ layer attributions (captum.attr.Layer*, InternalInfluence)
    def _expand_base(self, base, x):
        return base.to(x.device, torch.float32).expand(x.shape[0], -1).contiguous()

    def layer_activation(self, waves, layer: int):
        """Captum's LayerActivation: ``hidden_states[layer](x)``, ``[B, T, H]`` fp32."""
        l = check_layer(layer, self.eg.emb.nl)
        x = self._prep(waves)
        self.eg.forward(x)
        return self._checked(self.eg.hidden(l), "layer activation", "the forward pass produced a non-finite activation")

    def layer_gradient_x_activation(self, waves, layer: int, multiply_by_inputs: bool = True):
        """Captum's LayerGradientXActivation: ``dF/dh_l`` times ``h_l = hidden_states[layer](x)`` (the gradient alone with
        ``multiply_by_inputs=False``), ``[B, T, H]`` fp32: one forward, one backward stopped at the layer."""
        l = check_layer(layer, self.eg.emb.nl)
        x = self._prep(waves)
        self.eg.forward(x)
        g = self.eg.backward(self.loss_scale, to_layer=l)
        if multiply_by_inputs:
            g = self.eg.layer_tap(g, 1.0, self.eg.hidden(l))
        return self._checked(g)

    def layer_integrated_gradients(self, waves, layer: int, baselines=None, n_steps: int = 50, method: str = "gausslegendre",
                                   internal_batch_size: Optional[int] = None, multiply_by_inputs: bool = True,
                                   return_convergence_delta: bool = False):
        """Captum's LayerIntegratedGradients: the path runs in the layer's activation space, from ``hb = h_l(b)`` to
        ``hx = h_l(x)`` (one full forward each; ``b`` a waveform-space baseline as for ``integrated_gradients``), through
        ``forward_from(l, .)`` and ``backward(to_layer=l)`` -- nothing below the layer runs per path point.
        ``attr = (sum_k w_k g_k) * (hx - hb)`` ``[B, T, H]`` (the sum alone with ``multiply_by_inputs=False``);
        ``delta[b] = sum attr[b] - (F(x_b) - F(b_b))`` with F from the two full forwards."""
        B, L = _dims(waves)
        l, base, alphas, steps = check_layer_path_args(layer, self.eg.emb.nl, baselines, B, L, n_steps, method, internal_batch_size)
        _check_delta(return_convergence_delta, multiply_by_inputs)
        x = self._prep(waves)
        eg = self.eg
        fx = eg.forward(x)[0].view(-1)
        hx = eg.hidden(l)
        fb = eg.forward(self._expand_base(base, x))[0].view(-1)
        hb = eg.hidden(l)

        def point_gradient(pts, row0):                                          # pts [rows, T, H]: nothing below the layer runs
            eg.forward_from(l, pts)
            return eg.backward(self.loss_scale, to_layer=l)
        out, sums = self._integrate_path(hx, hb, alphas, steps, internal_batch_size, point_gradient,
                                         FIN_IG if multiply_by_inputs else None, return_convergence_delta)
        out = self._checked(out)
        if not return_convergence_delta:
            return out
        return out, (sums.double() - (fx.double() - fb.double())).float()

    def _wave_path(self, waves, layer, baselines, n_steps, method, internal_batch_size, extra_point):
        B, L = _dims(waves)
        l, base, alphas, steps = check_layer_path_args(layer, self.eg.emb.nl, baselines, B, L, n_steps, method, internal_batch_size,
                                                       extra_point)
        x = self._prep(waves)
        return x, _device_base(base, x), l, alphas, steps

    def layer_conductance(self, waves, layer: int, baselines=None, n_steps: int = 50, method: str = "gausslegendre",
                          internal_batch_size: Optional[int] = None):
        """Captum's LayerConductance: the ``n_steps + 1`` points ``b + alpha_k (x - b)`` of ``approximation(method, n_steps + 1)``
        in waveform space, each through a full forward and a backward stopped at the layer;
        ``attr = sum_{k < n_steps} g_k * (h_{k+1} - h_k)`` ``[B, T, H]`` (the last point needs no backward), summed in step order
        by advh_layer_conductance_accumulate: the result does not depend on ``internal_batch_size``."""
        x, base, l, alphas, _ = self._wave_path(waves, layer, baselines, n_steps, method, internal_batch_size, True)
        B, L = x.shape
        eg, lib = self.eg, _lib.lib()
        npts = n_steps + 1
        per = _steps_per_chunk(B, npts, internal_batch_size)
        a_all = _step_major(alphas, B, x.device)
        d = _desc(x, base, None, npts, 0)
        # one workspace shape: a short last chunk leaves the previous chunk's (finite) points in the rows it does not use
        pts = torch.zeros((per * B, L), dtype=torch.float32, device=x.device)
        total = prev_g = prev_a = None
        for s0 in range(0, npts, per):
            ns = min(per, npts - s0)
            ngrad = min(ns, n_steps - s0)                                       # the path's last point needs no gradient
            _points(d, a_all, s0 * B, ns * B, pts)
            eg.forward(pts)
            act = eg.hidden(l)                                                  # [per*B, T, H], step-major
            g = eg.backward(self.loss_scale, to_layer=l) if ngrad > 0 else None
            if total is None:
                total, prev_g, prev_a = (torch.zeros_like(act[:B]) for _ in range(3))
            _lib.check(lib.advh_layer_conductance_accumulate(None if g is None else g.data_ptr(), act.data_ptr(), B, act[0].numel(), ns,
                                                             ngrad, int(s0 == 0), prev_g.data_ptr(), prev_a.data_ptr(), total.data_ptr(),
                                                             _st()), "advh_layer_conductance_accumulate")
        return self._checked(total)

    def internal_influence(self, waves, layer: int, baselines=None, n_steps: int = 50, method: str = "gausslegendre",
                           internal_batch_size: Optional[int] = None):
        """Captum's InternalInfluence: ``attr = sum_k w_k g_k`` ``[B, T, H]``, ``g_k = dF/dh_l`` at the ``n_steps`` waveform-space
        points ``b + alpha_k (x - b)`` (a full forward and a backward stopped at the layer each)."""
        x, base, l, alphas, steps = self._wave_path(waves, layer, baselines, n_steps, method, internal_batch_size, False)
        eg = self.eg

        def point_gradient(pts, row0):                                          # [rows, L] -> [rows, T, H]
            eg.forward(pts)
            return eg.backward(self.loss_scale, to_layer=l)
        return self._checked(self._integrate_path(x, base, alphas, steps, internal_batch_size, point_gradient)[0])

    def frames_to_wave(self, rel: torch.Tensor, L: int) -> torch.Tensor:
        """Per-frame relevance ``[B, T]`` spread to the ``L`` samples of each clip (``frame_index``): ``[B, L]`` fp32."""
        T = rel.shape[1]
        hop = int(np.prod(self.emb.cfg.conv_stride))
        idx = torch.from_numpy(frame_index(L, T, hop)).to(rel.device)
        return rel.float().index_select(1, idx).contiguous()

    def layer_relevance(self, attr: torch.Tensor, L: int) -> torch.Tensor:
        """A layer attribution ``[B, T, H]`` as waveform relevance ``[B, L]``: summed over the channels of each frame
        (advh_layer_tap's row sums), then ``frames_to_wave``."""
        attr = attr.contiguous()
        B, T, H = attr.shape
        rel = torch.empty(B * T, dtype=torch.float32, device=attr.device)
        self.eg.layer_tap(attr.view(B * T, H), 1.0, want_out=False, row_sum=rel)
        return self.frames_to_wave(rel.view(B, T), L)

    # ------------------------------------------------------------------ attention maps and rollout
    # Abnar & Zuidema 2020 (rollout) and the self-attention rule of Chefer et al. 2021 (gradient rollout), restated from the
    # publications: Captum has no class for them.  csrc/attention_maps.hip recomputes the T x T maps the attention kernels never write.
    def check_attention_layer(self, layer, what: str = "layer") -> int:
        """An encoder layer with an attention block: ``check_layer`` and ``layer < nl``.  Raises ValueError."""
        nl = self.eg.emb.nl
        l = check_layer(layer, nl)
        if l >= nl:
            raise ValueError(f"{what} must name an encoder layer with an attention block, 0 <= layer < {nl}; got {layer!r}")
        return l

    def _attention_args(self, waves, lengths=None) -> Tuple[int, int, int]:
        """``(B, L, T)`` before any GPU work; the whole-clip maps kernel takes ``T <= 256`` frames -- a ``long_maps`` engine any
        number, and ``lengths`` -- and head dims ``8, 16, .. 128``."""
        B, L = _dims(waves)
        cfg = self.eg.emb.cfg
        T, dm = self.eg.emb._lengths(L)[-1], cfg.hidden_size // cfg.num_attention_heads
        long_maps = getattr(self.eg, "long_maps", False)
        if lengths is not None and not long_maps:
            raise ValueError("lengths= on the attention maps, rollout and LRP needs an engine built with long_maps=True "
                             "(HipAttribution(long_clips=True, long_maps=True); ADDVISOR_LONG_MAPS=1 for the runtime singleton)")
        if (T > 256 and not long_maps) or dm % 8 or dm > 128:
            raise ValueError(f"attention maps need T <= 256 frames and a head dim that is a multiple of 8 up to 128; got T = {T}, head dim {dm}"
                             " (long_maps=True lifts the frame limit)")
        return B, L, T

    def _attention_input(self, waves, lengths):
        """``(x, lens, frames)``: the clips on the device -- of a ragged call with the samples past each length zeroed
        (``_ragged``) -- their checked lengths or None, and the frame counts as int32 ``[B]`` on the device or None."""
        if lengths is None:
            return self._prep(waves), None, None
        x, lens = self._ragged(waves, lengths)
        return x, lens, torch.tensor(self.emb.frame_lengths(lens), dtype=torch.int32).to(x.device)

    def _target_seed(self, spec, logits: torch.Tensor) -> Optional[torch.Tensor]:
        if spec is None:
            return None
        if isinstance(spec, str):                              # "predicted": the sign of the forward's logit, on the device
            return torch.sign(logits.view(-1))
        return spec.to(self.emb.dev)

    def _rollout_step(self, M, X, Y, alpha, beta, gamma, normalize, frames=None):
        B, T = X.shape[0], X.shape[1]
        if frames is not None or T > 256:                      # long_maps (_attention_args): any T, every bound of clip b at frames[b]
            _lib.check(_lib.lib().advh_rollout_step_long(M.data_ptr(), X.data_ptr(), Y.data_ptr(), alpha, beta, gamma, int(normalize),
                                                         None if frames is None else frames.data_ptr(), B, T, _st()),
                       "advh_rollout_step_long")
            return
        _lib.check(_lib.lib().advh_rollout_step(M.data_ptr(), X.data_ptr(), Y.data_ptr(), alpha, beta, gamma, int(normalize), B, T, _st()),
                   "advh_rollout_step")

    def _rollout_relevance(self, X: torch.Tensor, frames=None) -> torch.Tensor:
        B, T = X.shape[0], X.shape[1]
        rel = torch.empty((B, T), dtype=torch.float32, device=X.device)
        if frames is not None or T > 256:
            _lib.check(_lib.lib().advh_rollout_relevance_long(X.data_ptr(), rel.data_ptr(), None if frames is None else frames.data_ptr(),
                                                              B, T, _st()), "advh_rollout_relevance_long")
            return rel
        _lib.check(_lib.lib().advh_rollout_relevance(X.data_ptr(), rel.data_ptr(), B, T, _st()), "advh_rollout_relevance")
        return rel

    def attention_maps(self, waves, layer: int, head_fusion: Optional[str] = None, grad: bool = False, target=None, lengths=None):
        """The attention maps of encoder layer ``layer`` (``0 <= layer < nl``), fp32, rows = queries: the probabilities
        ``A = softmax(Q K^T / sqrt(d))``, or with ``grad=True`` the gradient-weighted maps ``(dF/dA * A)^+`` of Chefer et al. 2021
        (``target``: None / 1 explains ``+F``, 0 ``-F``, ``"predicted"`` ``sign(F(x_b)) F``, or a ``[B]`` tensor of 0 / 1).
        ``head_fusion=None``: ``[B, heads, T, T]``; ``"mean"`` / ``"max"`` / ``"min"`` reduce over heads: ``[B, T, T]``.
        ``lengths`` (a ``long_maps`` engine; one sample count per clip, ``EmbedderGrad.forward``): clip b is ``waves[b, :lengths[b]]``
        and its map the one of that clip run alone, in the top-left ``T_b x T_b`` block, exactly 0 elsewhere."""
        l = self.check_attention_layer(layer)
        fuse = check_head_fusion(head_fusion)
        B, _, T = self._attention_args(waves, lengths)
        if not isinstance(grad, bool):
            raise ValueError(f"grad must be a bool, not {grad!r}")
        if target is not None and not grad:
            raise ValueError("target picks the explained output of the gradient-weighted maps: pass grad=True")
        spec = check_attention_target(target, B)
        x, lens, _ = self._attention_input(waves, lengths)
        if not grad:
            self.eg.forward(x, to_layer=l + 1, lengths=lens)
            return self._checked(self.eg.attention_probs(l, fuse), "attention map", "the forward pass produced a non-finite activation")
        logits, _ = self.eg.forward(x, lengths=lens)
        heads = self.eg.cfg.num_attention_heads
        out = torch.empty((1, B, T, T) if fuse else (1, B, heads, T, T), dtype=torch.float32, device=x.device)
        self.eg.backward(self.loss_scale, seed=self._target_seed(spec, logits), to_layer=l, attention_maps=(out, fuse))
        return self._checked(out[0], "attention map")

    def attention_rollout(self, waves, head_fusion: str = "mean", start_layer: int = 0, return_joint: bool = False, lengths=None):
        """Attention rollout (Abnar & Zuidema 2020): ``R = I``; for ``l = start_layer .. nl-1`` with ``M`` the head-fused
        probabilities of layer ``l``, ``R <- rownorm(R + M R)`` (row ``i`` divided by ``1 + sum_k M[i,k]``; ``"mean"``: ``0.5 A +
        0.5 I``).  The classifier mean-pools over time: the per-frame relevance is ``rel[b, j] = (1/T) sum_i R[b, i, j]``,
        ``[B, T]`` fp32, rows summing to 1 (``frames_to_wave`` spreads it to the samples).  ``return_joint``: ``(rel, R [B, T, T])``.
        ``lengths`` (a ``long_maps`` engine): clip b is ``waves[b, :lengths[b]]``; ``R[b]`` is the cropped clip's in the top-left
        ``T_b x T_b`` block and 0 elsewhere, ``rel[b, j]`` divides by ``T_b`` and is exactly 0 for ``j >= T_b``."""
        fuse = check_head_fusion(head_fusion, allow_none=False)
        s0 = self.check_attention_layer(start_layer, "start_layer")
        B, _, T = self._attention_args(waves, lengths)
        x, lens, frames = self._attention_input(waves, lengths)
        self.eg.forward(x, lengths=lens)
        R = torch.eye(T, dtype=torch.float32, device=x.device).expand(B, T, T).contiguous()
        Y = torch.empty_like(R)
        for l in range(s0, self.eg.emb.nl):
            self._rollout_step(self.eg.attention_probs(l, fuse), R, Y, 1.0, 1.0, 0.0, True, frames)
            R, Y = Y, R
        rel = self._checked(self._rollout_relevance(R, frames), "attention rollout", "the forward pass produced a non-finite activation")
        return (rel, R) if return_joint else rel

    def attention_grad_rollout(self, waves, target=None, start_layer: int = 0, return_joint: bool = False, lengths=None):
        """Gradient-weighted attention rollout (the self-attention rule of Chefer et al. 2021): ``Abar_l = mean_h (dF/dA_l^h *
        A_l^h)^+`` and ``R <- R + Abar_l R`` from ``R = I``, carried as ``D = R - I`` (``D <- D + Abar_l + Abar_l D`` from 0: the
        identity is never added and subtracted again).  One forward, one backward stopped at ``start_layer`` that writes every
        layer's map on its way.  ``rel[b, j] = (1/T) sum_i D[b, i, j]``, ``[B, T]`` fp32 -- without the identity, which would add a
        constant ``1/T`` that dwarfs the relevance.  ``target`` as ``attention_maps``; ``return_joint``: ``(rel, D [B, T, T])``.
        ``lengths``: as ``attention_rollout`` (``"predicted"`` takes the ragged forward's logit)."""
        s0 = self.check_attention_layer(start_layer, "start_layer")
        B, _, T = self._attention_args(waves, lengths)
        spec = check_attention_target(target, B)
        x, lens, frames = self._attention_input(waves, lengths)
        logits, _ = self.eg.forward(x, lengths=lens)
        nl = self.eg.emb.nl
        maps = torch.empty((nl - s0, B, T, T), dtype=torch.float32, device=x.device)
        self.eg.backward(self.loss_scale, seed=self._target_seed(spec, logits), to_layer=s0, attention_maps=(maps, 1))
        D = torch.zeros((B, T, T), dtype=torch.float32, device=x.device)
        Y = torch.empty_like(D)
        for l in range(s0, nl):
            self._rollout_step(maps[l - s0], D, Y, 1.0, 1.0, 1.0, False, frames)
            D, Y = Y, D
        rel = self._checked(self._rollout_relevance(D, frames), "attention gradient rollout")
        return (rel, D) if return_joint else rel

    # ------------------------------------------------------------------ conservative LRP for the transformer encoder
    # Ali et al., ICML 2022 (LN-rule, AH-rule) and the GELU identity rule of AttnLRP (Achtibat et al. 2024), restated from the
    # publications: Captum's LRP has no rule for LayerNorm, softmax attention or GELU, and the reference has no such method.
    def transformer_lrp(self, waves, target=None, start_layer: int = 0, ln_rule: bool = True, attention_rule: bool = True,
                        gelu_rule: str = "gradient", return_hidden: bool = False, lengths=None):
        """Conservative propagation through the encoder: gradient x input at ``x = hidden_states[start_layer]`` of ``F~``, the
        logit with -- in the layers ``>= start_layer`` and the final LayerNorm of a full-depth pre-LN model -- ``ln_rule``: every
        LayerNorm's ``1/sigma`` held constant (``LN(x) = gamma (x - mean(x)) / sg(sigma) + beta``); ``attention_rule``: the
        attention probabilities held constant (``ctx = sg(P) V``); ``gelu_rule="identity"``: the FFN's ``GELU(x) = x sg(Phi(x))``
        (``"gradient"``, the default of Ali et al., leaves GELU's backward alone).  ``R[b, t, h] = x[b, t, h] * d(+-F~)/dx[b, t, h]``
        and ``rel[b, t] = sum_h R[b, t, h]``, ``[B, T]`` fp32 (``frames_to_wave`` spreads it to the samples); ``return_hidden``:
        ``(rel, R [B, T, H])``.  With all three rules on ``x -> F~`` is affine: on a model without biases ``sum_t rel[b] = +-F(x_b)``.
        With all rules off it is ``layer_gradient_x_activation(waves, start_layer)`` summed over the channels.  ``target`` as
        ``attention_maps``.  One forward, one backward stopped at ``start_layer`` (``EmbedderGrad.backward(rules=...)``).
        ``lengths`` (a ``long_maps`` engine): clip b is ``waves[b, :lengths[b]]``, its relevance that of the clip run alone and
        exactly 0 on the frames ``t >= T_b``."""
        s0 = self.check_attention_layer(start_layer, "start_layer")
        rules = LrpRules(ln_rule, attention_rule, gelu_rule)
        if not isinstance(return_hidden, bool):
            raise ValueError(f"return_hidden must be a bool, not {return_hidden!r}")
        B, _, T = self._attention_args(waves, lengths)
        spec = check_attention_target(target, B)
        x, lens, _ = self._attention_input(waves, lengths)
        logits, _ = self.eg.forward(x, lengths=lens)
        g = self.eg.backward(self.loss_scale, seed=self._target_seed(spec, logits), to_layer=s0, rules=rules)
        H = g.shape[2]
        rel = torch.empty(B * T, dtype=torch.float32, device=x.device)
        R = self.eg.layer_tap(g.view(B * T, H), 1.0, act=self.eg.hidden(s0).view(B * T, H), want_out=return_hidden, row_sum=rel)
        rel = self._checked(rel.view(B, T), "transformer LRP")
        return (rel, R.view(B, T, H)) if return_hidden else rel

    # ------------------------------------------------------------------ neuron attributions (captum.attr.Neuron*)
    def _neuron_args(self, waves, layer, neuron):
        """``(B, L, layer, box)`` before any GPU work: ``check_layer`` and ``check_neuron_selector`` against the frame count of
        an ``L``-sample clip."""
        B, L = _dims(waves)
        emb = self.eg.emb
        l = check_layer(layer, emb.nl)
        return B, L, l, check_neuron_selector(neuron, emb._lengths(L)[-1], emb.cfg.hidden_size)

    def _checked_neuron(self, out, what: str = "neuron attribution"):
        return self._checked(out, what, f"the gradient chain overflowed at neuron_loss_scale={self.neuron_loss_scale:g} (lower "
                             "HipAttribution.neuron_loss_scale by a power of two), or a path point has no scale (a constant clip)")

    def neuron_gradient(self, waves, layer: int, neuron):
        """Captum's NeuronGradient: ``d s_n / d x`` ``[B, L]`` fp32, ``s_n(x)`` the sum over the selection ``neuron`` (a
        ``(t, h)`` tuple of ints or slices, ``check_neuron_selector``) of ``hidden_states[layer](x)``: one forward stopped at
        the layer, one backward started there from the selection's indicator."""
        _, _, l, box = self._neuron_args(waves, layer, neuron)
        x = self._prep(waves)
        self.eg.forward(x, to_layer=l)
        return self._checked_neuron(self.eg.backward(self.neuron_loss_scale, from_layer=l, neuron=box))

    def _neuron_path_args(self, waves, layer, neuron, baselines, n_steps, method, internal_batch_size):
        B, L, l, box = self._neuron_args(waves, layer, neuron)
        base = check_ig_baselines(baselines, B, L)
        alphas, steps = approximation(method, check_steps(n_steps, method))
        if internal_batch_size is not None:
            _positive_int(internal_batch_size, "internal_batch_size")
        return l, box, base, alphas, steps

    def neuron_integrated_gradients(self, waves, layer: int, neuron, baselines=None, n_steps: int = 50, method: str = "gausslegendre",
                                    internal_batch_size: Optional[int] = None, multiply_by_inputs: bool = True):
        """Captum's NeuronIntegratedGradients: ``integrated_gradients`` with ``s_n`` (``neuron_gradient``) in the place of the
        logit -- every path point runs the chain below the layer only, forward and backward.  ``[B, L]``; no convergence delta
        (Captum's class has none)."""
        l, box, base, alphas, steps = self._neuron_path_args(waves, layer, neuron, baselines, n_steps, method, internal_batch_size)
        x = self._prep(waves)
        eg, scale = self.eg, self.neuron_loss_scale

        def point_gradient(pts, row0):
            eg.forward(pts, to_layer=l)
            return eg.backward(scale, from_layer=l, neuron=box)
        return self._checked_neuron(self._integrate_path(x, _device_base(base, x), alphas, steps, internal_batch_size, point_gradient,
                                                         FIN_IG if multiply_by_inputs else FIN_MEAN)[0])

    def neuron_conductance(self, waves, layer: int, neuron, baselines=None, n_steps: int = 50, method: str = "gausslegendre",
                           internal_batch_size: Optional[int] = None, multiply_by_inputs: bool = True):
        """Captum's NeuronConductance of a single neuron ``h_n`` (``neuron``: two ints; a slice raises ValueError -- Captum's
        aggregate multiplies a summed layer gradient into a summed neuron gradient, which is not restated): over the ``n_steps``
        waveform-space points ``x_k`` of the rule, ``attr = (x - b) * sum_k w_k m_k (d h_n / d x)(x_k)`` with
        ``m_k = dF/dh_n(x_k)`` (the sum alone with ``multiply_by_inputs=False``).  Per chunk: a full forward, the backward
        stopped at the layer, advh_neuron_values on that gradient, then the backward from the layer seeded with ``m``."""
        l, box, base, alphas, steps = self._neuron_path_args(waves, layer, neuron, baselines, n_steps, method, internal_batch_size)
        if any(isinstance(s, slice) for s in neuron):
            raise ValueError("neuron_conductance takes a single neuron (two ints): Captum's aggregate over a slice is ambiguous")
        x = self._prep(waves)
        eg = self.eg

        def point_gradient(pts, row0):
            eg.forward(pts)
            m = eg.neuron_values(eg.backward(self.loss_scale, to_layer=l), box)        # dF/dh_n of every row
            return eg.backward(self.neuron_loss_scale, from_layer=l, neuron=box, row_scale=m)
        return self._checked_neuron(self._integrate_path(x, _device_base(base, x), alphas, steps, internal_batch_size, point_gradient,
                                                         FIN_IG if multiply_by_inputs else FIN_MEAN)[0])

    def neuron_gradient_shap(self, waves, layer: int, neuron, baselines, n_samples: int = 5, stdevs: float = 0.0,
                             multiply_by_inputs: bool = True, seed: Optional[int] = None, internal_batch_size: Optional[int] = None):
        """Captum's NeuronGradientShap: ``gradient_shap`` with ``s_n`` in the place of the logit, on the same draws
        (``shap_draws(seed, ...)``, ``philox_normal(seed, ...)``).  ``[B, L]``."""
        B, L, l, box = self._neuron_args(waves, layer, neuron)
        base, S, seed, draws = self._shap_args(waves, baselines, B, L, n_samples, stdevs, seed, internal_batch_size=internal_batch_size)
        x = self._prep(waves)
        eg = self.eg

        def row_gradient(pts, row0, clip_major, S):
            eg.forward(pts, to_layer=l)
            return eg.backward(self.neuron_loss_scale, from_layer=l, neuron=box)
        return self._checked_neuron(self._expanded_samples(x, _device_base(base, x), draws, S, stdevs, seed, multiply_by_inputs,
                                                           internal_batch_size, row_gradient)[0])

    def neuron_feature_ablation(self, waves, layer: int, neuron, baselines=None, feature_mask=None,
                                internal_batch_size: Optional[int] = None):
        """Captum's NeuronFeatureAblation: ``feature_ablation`` with ``s_n`` in the place of the logit --
        ``attr[b, t] = s_n(x)[b] - s_n(ablated)[k(b, t), b]``; the ablated rows run through the forward stopped at the layer and
        advh_neuron_values."""
        B, L, l, box = self._neuron_args(waves, layer, neuron)
        base = check_ig_baselines(baselines, B, L)
        index, K = feature_indices(feature_mask, B, L)
        chunk = check_internal_batch(internal_batch_size)
        x = self._prep(waves)
        eg = self.eg
        base, index = _device_base(base, x), index.to(x.device).contiguous()   # locals: the descriptor holds the pointers only
        d = ablation_desc(x, base, ABL_FEATURE, K, mask=index)
        return self._ablate(x, K * B, chunk, functools.partial(ablation_points, d), functools.partial(ablation_accumulate, d),
                            "neuron feature ablation",
                            "the neuron's activation of the clips or of their ablations is not finite (check the inputs and baselines)",
                            value=lambda rows, row0=0: eg.neuron_values(eg.forward(rows, to_layer=l), box))

    def time_mask(self, attr: torch.Tensor, waves: Optional[torch.Tensor] = None):
        """``|attr| / (max|attr| + 1e-8)`` per clip and, with ``waves``, the relevant / irrelevant waveforms
        (captum_saliency.py:136-143)."""
        attr = attr.contiguous()
        B, L = attr.shape
        mask = torch.empty_like(attr)
        if waves is None:
            _lib.check(_lib.lib().advh_time_mask(attr.data_ptr(), mask.data_ptr(), None, None, None, B, L, _st()), "advh_time_mask")
            return mask
        x = self._prep(waves)
        win, wout = torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.lib().advh_time_mask(attr.data_ptr(), mask.data_ptr(), win.data_ptr(), wout.data_ptr(), x.data_ptr(), B, L, _st()),
                   "advh_time_mask")
        return mask, win, wout
