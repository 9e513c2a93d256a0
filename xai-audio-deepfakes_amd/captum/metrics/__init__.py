"""``captum.metrics``-compatible front ends over the HIP kernels: ``infidelity`` (Yeh et al., NeurIPS 2019), ``sensitivity_max``
and ``infidelity_perturb_func_decorator``, restated from Captum 0.7's ``metrics/_core/infidelity.py``,
``metrics/_core/sensitivity.py`` and the helpers they use (``_divide_and_aggregate_metrics``, ``safe_div``,
``_expand_and_update_baselines``) -- captum is absent.

Both metrics run the perturbed samples of each clip in Captum's chunks of ``max_examples_per_batch // B`` samples (``S // m``
chunks of m, then one of ``S % m``), rows clip-major (``repeat_interleave``).  ``infidelity`` pushes the perturbed rows through
the HIP forward and folds ``(a, d)`` into fp64 per-clip sums on the device; ``sensitivity_max`` re-runs the explanation on them
and folds the relative norm of the change into a per-clip maximum on the device.  Two perturbations run fused on the device:
``sensitivity_max``'s default ``x + U(-r, r)`` and ``NoisyPerturbation`` (an extension of this build, not a Captum name:
``noise = stdevs * N(0, 1)``, ``(noise, x - noise)``, Captum's tutorial perturbation for infidelity).  Any other Python
``perturb_func`` goes through the generic path, called once per chunk as Captum calls it.

Randomness follows ``torch``'s default CPU generator through one seed per call, drawn before the explanation function draws its
own (``torch.manual_seed`` reproduces a result); Captum's own RNG stream is not reproduced.  Out of scope: multi-input tuples,
``target`` / ``additional_forward_args`` other than None (ValueError)."""
import torch

from addvisor_hip import attribution as _A
from addvisor_hip.attribution import NoisyPerturbation  # noqa: F401  (exported)

__all__ = ["infidelity", "infidelity_perturb_func_decorator", "sensitivity_max", "default_perturb_func", "NoisyPerturbation"]


def safe_div(numerator, denom, default_denom=1.0):
    """Captum's ``safe_div``: ``numerator / denom``, dividing by ``default_denom`` where ``denom`` is zero."""
    if isinstance(denom, (int, float)):
        return numerator / (denom if denom != 0 else default_denom)
    if not torch.is_tensor(default_denom):
        default_denom = torch.tensor(default_denom, dtype=denom.dtype, device=denom.device)
    return numerator / torch.where(denom != 0, denom, default_denom)


def infidelity_perturb_func_decorator(multiply_by_inputs=True):
    """Captum's decorator: turns ``perturb_func(inputs[, baselines]) -> perturbed inputs`` into the infidelity perturb_func
    ``(perturbations, perturbed_inputs)``, the perturbation being ``safe_div(x - x~, x - baselines)`` (``safe_div(x - x~, x)``
    without baselines; denominator 1 where zero), or ``x - x~`` when ``multiply_by_inputs`` is False.  Plain torch on the tensors
    the metric hands it (the chunk's expanded inputs and baselines, on the device)."""
    def decorator(pertub_func):
        def default_perturb_func(inputs, baselines=None):
            perturbed = pertub_func(inputs, baselines) if baselines is not None else pertub_func(inputs)
            if isinstance(perturbed, (tuple, list)) and len(perturbed) == 1:
                perturbed = perturbed[0]
            if not multiply_by_inputs:
                return inputs - perturbed, perturbed
            denom = inputs if baselines is None else inputs - baselines
            return safe_div(inputs - perturbed, denom, default_denom=1.0), perturbed
        return default_perturb_func
    return decorator


def default_perturb_func(inputs, perturb_radius=0.02):
    """Captum's ``default_perturb_func``: ``inputs + U(-perturb_radius, perturb_radius)``.  ``sensitivity_max`` recognises it and
    draws the rows on the device with the global (clip, sample) counter; called directly, row r is ``x_r + r (2u - 1)`` with u
    from the Philox words of counter r under one seed drawn from torch's default CPU generator, drawn on the GPU (a host
    tensor's rows on the current one) and returned on the inputs' device, as Captum returns them."""
    if not torch.is_tensor(inputs) or inputs.dim() != 2:
        raise ValueError("inputs must be a [R, L] waveform tensor")
    radius = _A._finite_scale(perturb_radius, "perturb_radius")
    x = inputs.to(_A.metric_device(inputs), torch.float32).contiguous()
    return _A.uniform_rows(x, _A.draw_seed(), 1, 0, 1, radius).to(inputs.device)


def _device(inputs):
    return _A.metric_device(inputs) if torch.is_tensor(inputs) else torch.device("cuda")


def infidelity(forward_func, perturb_func, inputs, attributions, baselines=None, additional_forward_args=None, target=None,
               n_perturb_samples=10, max_examples_per_batch=None, normalize=False):
    """Captum's infidelity of ``attributions [B, L]`` for ``forward_func``, a ``captum_saliency.Wav2vec2LogReg`` (or anything
    exposing ``.hip_attribution()``; anything else raises TypeError): ``[B]`` fp32,
    ``E_s[(sum_j I_j attr_j - (F(x) - F(x - I)))^2]``, normalised by the best scale beta of the attributions when
    ``normalize``.  ``perturb_func(inputs[, baselines]) -> (perturbations, perturbed_inputs)``; a ``NoisyPerturbation`` runs
    fused on the device.  ``HipAttribution.infidelity`` states the arithmetic.  Bad arguments raise ValueError before any GPU
    work."""
    if hasattr(forward_func, "hip_mask_attribution"):
        raise NotImplementedError("infidelity over STFT masks is not implemented (HipSpectralAttribution)")
    if not hasattr(forward_func, "hip_attribution"):
        raise TypeError("captum.metrics (HIP build) only scores captum_saliency.Wav2vec2LogReg models")
    B, L, _, _ = _A.check_metric_args(inputs, n_perturb_samples, max_examples_per_batch, target, additional_forward_args,
                                      attributions)
    if not callable(perturb_func):
        raise ValueError("perturb_func must be callable")
    if baselines is not None:
        _A.check_ig_baselines(baselines, B, L)
    return forward_func.hip_attribution().infidelity(inputs, perturb_func, attributions, baselines=baselines,
                                                     n_perturb_samples=n_perturb_samples,
                                                     max_examples_per_batch=max_examples_per_batch, normalize=bool(normalize))


def sensitivity_max(explanation_func, inputs, perturb_func=default_perturb_func, perturb_radius=0.02, n_perturb_samples=10,
                    norm_ord="fro", max_examples_per_batch=None, **kwargs):
    """Captum's sensitivity_max: ``[B]`` fp32, ``max_s ||e(x) - e(x~_s)|| / ||e(x)||`` over ``n_perturb_samples`` perturbations
    of each clip (a zero norm counts as 1).  ``explanation_func`` is any callable attributing a ``[R, L]`` tensor -- an engine
    method, a ``captum.attr`` object's ``attribute`` or ``NoiseTunnel(...).attribute`` -- and receives the tensor (not Captum's
    1-tuple) with ``**kwargs``; a ``[B, L]`` ``baselines`` is ``repeat_interleave``d per chunk, every other keyword passes
    unchanged; ``target`` and ``additional_forward_args`` must be None and are not passed on.  ``norm_ord``: "fro" / 2, 1 or
    inf.  ``perturb_func`` left at ``default_perturb_func`` runs on the device; a callable with more than one parameter also
    gets ``perturb_radius``.  Unlike Captum, which explains the clips first, the first chunk's perturbation is made before the
    explanation of the clips (a perturbation of the wrong shape raises before any explanation runs).  Bad arguments raise
    ValueError before any GPU work."""
    if not callable(explanation_func):
        raise ValueError("explanation_func must be callable")
    _A.check_metric_args(inputs, n_perturb_samples, max_examples_per_batch, kwargs.get("target"),
                         kwargs.get("additional_forward_args"))
    _A.check_norm_ord(norm_ord)
    _A._finite_scale(perturb_radius, "perturb_radius")
    return _A.sensitivity_max(explanation_func, inputs, _device(inputs), None if perturb_func is default_perturb_func else perturb_func,
                              perturb_radius, n_perturb_samples, norm_ord, max_examples_per_batch, **kwargs)
