"""``captum.attr``-compatible front ends (captum_saliency.py:3, 116-118, 131-135) over the HIP kernels: the gradient methods
(Saliency, InputXGradient, IntegratedGradients, GradientShap) on the HIP backward path, the perturbation methods (Occlusion,
FeatureAblation, FeaturePermutation), the Shapley methods (ShapleyValueSampling, ShapleyValues, KernelShap) and Lime on the HIP
forward with the ablated, permuted or coalition batches built on the device; NoiseTunnel (SmoothGrad, SmoothGrad-squared,
VarGrad) around any of those eleven, with the noisy rows and the moments on the device; and the layer methods (LayerActivation,
LayerGradientXActivation, LayerIntegratedGradients, LayerConductance, InternalInfluence) at ``hidden_states[layer]`` of the
encoder, on the HIP chain started and stopped at that layer (csrc/attribution_layer.hip).  They return ``[B, T, H]`` maps;
NoiseTunnel does not wrap them.  The neuron methods (NeuronGradient, NeuronIntegratedGradients, NeuronGradientShap,
NeuronConductance, NeuronFeatureAblation) attribute one unit, or one band of units, of ``hidden_states[layer]`` to the waveform
(``[B, L]``), on the forward stopped at the layer and the backward started there (csrc/attribution_neuron.hip); NoiseTunnel
does not wrap them either.

``Method(model).attribute(inputs, target=None, ...)`` expects ``model`` to be a
``captum_saliency.Wav2vec2LogReg`` (or anything exposing ``.hip_attribution()``): the waveform -> logit
classifier whose frozen embedder runs on the GPU kernels.  Arbitrary ``nn.Module``s are not supported --
there is no autograd fallback.

A model exposing ``.hip_mask_attribution()`` (``captum_saliency.MaskedSpectrogramLogReg``) is attributed over the STFT mask
instead: Saliency, InputXGradient, IntegratedGradients, GradientShap, Occlusion, FeatureAblation and ShapleyValueSampling then
take ``[B, Fm, Tm]`` inputs, baselines and feature masks (Occlusion: 2-tuples) and run on
``addvisor_hip.spectral_attribution.HipSpectralAttribution``; every other method raises NotImplementedError for such a model."""
import torch

from addvisor_hip import attribution as _A
from addvisor_hip import spectral_attribution as _S
from addvisor_hip.linear_model import SkLearnLasso
from ._core.feature_permutation import _permute_feature
from ._core.lime import default_perturb_func, get_exp_kernel_similarity_function


def _masked(model) -> bool:
    """The model is attributed over the STFT mask (``[B, Fm, Tm]`` inputs) on ``HipSpectralAttribution``."""
    return hasattr(model, "hip_mask_attribution")


def _mask_checks(model, inputs, target):
    """``[B, Fm, Tm]`` mask inputs of a mask-domain model, before its engine exists (ValueError) -> ``(B, Fm, Tm)``."""
    B, Fm, Tm = _S.check_mask_inputs(inputs, target, model.mask_frames() if hasattr(model, "mask_frames") else None)
    if hasattr(model, "num_clips") and B != model.num_clips():
        raise ValueError(f"the model holds {model.num_clips()} clips; inputs has {B} masks")
    return B, Fm, Tm


def _mask_batch(model, inputs, target, perturbations_per_eval):
    B, Fm, Tm = _mask_checks(model, inputs, target)
    ppe = _A._positive_int(perturbations_per_eval, "perturbations_per_eval")
    return B, Fm, Tm, (None if ppe == 1 else ppe * B)


def _no_masks(model, what):
    if _masked(model):
        raise NotImplementedError(f"{what} over STFT masks is not implemented: HipSpectralAttribution offers Saliency, "
                                  "InputXGradient, IntegratedGradients, GradientShap, Occlusion, FeatureAblation and "
                                  "ShapleyValueSampling")


def _engine(model):
    _no_masks(model, "this method")
    if not hasattr(model, "hip_attribution"):
        raise TypeError("captum.attr (HIP build) only attributes captum_saliency.Wav2vec2LogReg models")
    return model.hip_attribution()


class _Method:
    def __init__(self, forward_func):
        self.model = forward_func

    @staticmethod
    def _check(inputs, target):
        if target is not None:
            raise NotImplementedError("the classifier has a single output; target must be None")
        if not torch.is_tensor(inputs) or inputs.dim() != 2:
            raise ValueError("inputs must be a [B, L] waveform tensor")


class Saliency(_Method):
    def attribute(self, inputs, target=None, abs=True, additional_forward_args=None):
        if _masked(self.model):
            _mask_checks(self.model, inputs, target)
            eng = self.model.hip_mask_attribution()
            return eng.saliency(inputs) if abs else eng.input_gradient(inputs)
        self._check(inputs, target)
        eng = _engine(self.model)
        return eng.saliency(inputs) if abs else eng.input_gradient(inputs)


class InputXGradient(_Method):
    def attribute(self, inputs, target=None, additional_forward_args=None):
        if _masked(self.model):
            _mask_checks(self.model, inputs, target)
            return self.model.hip_mask_attribution().input_x_gradient(inputs)
        self._check(inputs, target)
        return _engine(self.model).input_x_gradient(inputs)


class IntegratedGradients(_Method):
    def __init__(self, forward_func, multiply_by_inputs=True):
        super().__init__(forward_func)
        self.multiply_by_inputs = multiply_by_inputs

    def attribute(self, inputs, baselines=None, target=None, additional_forward_args=None, n_steps=50,
                  method="gausslegendre", internal_batch_size=None, return_convergence_delta=False):
        """Baselines: None (zero), a number, ``[1, L]`` or ``[B, L]``; methods: ``gausslegendre`` and the four Riemann
        rules.  ``return_convergence_delta=True`` returns ``(attributions, delta [B])``."""
        if _masked(self.model):
            B, Fm, Tm = _mask_checks(self.model, inputs, target)
            _S.check_mask_baselines(baselines, B, Fm, Tm)
            _A.approximation(method, _A.check_steps(n_steps, method))
            if internal_batch_size is not None:
                _A._positive_int(internal_batch_size, "internal_batch_size")
            return self.model.hip_mask_attribution().integrated_gradients(
                inputs, n_steps=n_steps, internal_batch_size=internal_batch_size, baselines=baselines, method=method,
                multiply_by_inputs=self.multiply_by_inputs, return_convergence_delta=return_convergence_delta)
        self._check(inputs, target)
        return _engine(self.model).integrated_gradients(inputs, n_steps=n_steps, internal_batch_size=internal_batch_size,
                                                        baselines=baselines, method=method,
                                                        multiply_by_inputs=self.multiply_by_inputs,
                                                        return_convergence_delta=return_convergence_delta)


class GradientShap(_Method):
    """Captum's GradientShap: the expected gradients of ``n_samples`` random points between a noisy input and a baseline
    drawn from ``baselines [N_b, L]`` (or a callable returning it).  The random draws follow ``torch``'s default CPU
    generator through one seed per call (``torch.manual_seed`` reproduces a result); Captum's own RNG stream is not
    reproduced.  ``return_convergence_delta=True`` returns ``(attributions, delta [B * n_samples])``."""

    def __init__(self, forward_func, multiply_by_inputs=True):
        super().__init__(forward_func)
        self.multiply_by_inputs = multiply_by_inputs

    def attribute(self, inputs, baselines, n_samples=5, stdevs=0.0, target=None, additional_forward_args=None,
                  return_convergence_delta=False):
        if _masked(self.model):
            B, Fm, Tm = _mask_checks(self.model, inputs, target)
            if callable(baselines) and not torch.is_tensor(baselines):
                raise NotImplementedError("GradientShap over STFT masks takes a [N_b, Fm, Tm] tensor of baseline masks, not a callable")
            _S.check_mask_distribution(baselines, B, Fm, Tm, n_samples, stdevs)
            if return_convergence_delta:
                raise NotImplementedError("GradientShap over STFT masks (HipSpectralAttribution) does not compute the convergence delta")
            return self.model.hip_mask_attribution().gradient_shap(inputs, baselines, n_samples=n_samples, stdevs=stdevs,
                                                                   multiply_by_inputs=self.multiply_by_inputs)
        self._check(inputs, target)
        return _engine(self.model).gradient_shap(inputs, baselines, n_samples=n_samples, stdevs=stdevs,
                                                 multiply_by_inputs=self.multiply_by_inputs,
                                                 return_convergence_delta=return_convergence_delta)


def _perturbation_batch(inputs, target, perturbations_per_eval):
    """Checks shared by the perturbation methods, before any GPU work (ValueError).  Returns the engine's rows per forward:
    None (its default) for Captum's default of 1 -- the attribution does not depend on the chunking -- else
    ``perturbations_per_eval * B``."""
    if target is not None:
        raise ValueError("the classifier has a single output; target must be None")
    if not torch.is_tensor(inputs) or inputs.dim() != 2:
        raise ValueError("inputs must be a [B, L] waveform tensor")
    ppe = _A._positive_int(perturbations_per_eval, "perturbations_per_eval")
    return None if ppe == 1 else ppe * inputs.shape[0]


class Occlusion(_Method):
    """Captum's Occlusion: windows of ``sliding_window_shapes = (win,)`` samples every ``strides`` samples (default 1) are
    replaced by ``baselines`` (None = 0, a number, ``[1, L]`` or ``[B, L]``); ``K = ceil((L - win) / strides) + 1`` windows,
    the last one cropped at L.  ``attr[b, t]`` is the mean over the windows covering t of ``F(x)[b] - F(occluded)[b]``,
    summed in window order as Captum does.  Captum's assertions (``win <= L``; ``strides <= win`` unless ``win == L``) raise
    ValueError."""

    def attribute(self, inputs, sliding_window_shapes, strides=None, baselines=None, target=None, additional_forward_args=None,
                  perturbations_per_eval=1, show_progress=False):
        if _masked(self.model):                               # a (Fm, Tm) input: 2-tuples, windows cropped at the edges
            B, Fm, Tm, ibs = _mask_batch(self.model, inputs, target, perturbations_per_eval)
            w, s, _ = _S.check_occlusion2d_args(Fm, Tm, sliding_window_shapes, strides)
            _S.check_mask_baselines(baselines, B, Fm, Tm)
            return self.model.hip_mask_attribution().occlusion(inputs, w, s, baselines=baselines, internal_batch_size=ibs)
        ibs = _perturbation_batch(inputs, target, perturbations_per_eval)
        B, L = inputs.shape
        win, stride, _ = _A.check_occlusion_args(L, sliding_window_shapes, strides)
        _A.check_ig_baselines(baselines, B, L)
        return _engine(self.model).occlusion(inputs, win, stride, baselines=baselines, internal_batch_size=ibs)


class FeatureAblation(_Method):
    """Captum's FeatureAblation: each feature id of ``feature_mask`` (None = every sample its own feature, else an integer
    ``[1, L]`` or ``[B, L]`` tensor) is replaced by ``baselines`` in every clip at once, and every sample of the feature gets
    ``F(x)[b] - F(ablated)[b]``."""

    def attribute(self, inputs, baselines=None, target=None, additional_forward_args=None, feature_mask=None,
                  perturbations_per_eval=1, show_progress=False):
        if _masked(self.model):
            B, Fm, Tm, ibs = _mask_batch(self.model, inputs, target, perturbations_per_eval)
            _S.check_mask_baselines(baselines, B, Fm, Tm)
            _A.feature_indices(_S.flat_feature_mask(feature_mask, B, Fm, Tm), B, Fm * Tm)
            return self.model.hip_mask_attribution().feature_ablation(inputs, baselines=baselines, feature_mask=feature_mask,
                                                                      internal_batch_size=ibs)
        ibs = _perturbation_batch(inputs, target, perturbations_per_eval)
        B, L = inputs.shape
        _A.check_ig_baselines(baselines, B, L)
        _A.feature_indices(feature_mask, B, L)
        return _engine(self.model).feature_ablation(inputs, baselines=baselines, feature_mask=feature_mask,
                                                    internal_batch_size=ibs)


def _shapley_checks(inputs, target, perturbations_per_eval, baselines, feature_mask):
    ibs = _perturbation_batch(inputs, target, perturbations_per_eval)
    B, L = inputs.shape
    _A.check_ig_baselines(baselines, B, L)
    _A.shapley_feature_indices(feature_mask, B, L)
    return ibs


class ShapleyValueSampling(_Method):
    """Captum's ShapleyValueSampling: ``n_samples`` random permutations of the features of ``feature_mask`` (None = every
    sample its own feature, else an integer ``[1, L]`` or ``[B, L]`` tensor of ids >= 0); along each, the features are switched
    from ``baselines`` (None = 0, a number, ``[1, L]`` or ``[B, L]``) to the input one at a time, and every sample gets the mean
    over permutations of the logit change its feature caused.  The permutations follow ``torch``'s default CPU generator
    through one seed per call (``torch.manual_seed`` reproduces a result); Captum's own RNG stream is not reproduced."""

    def attribute(self, inputs, baselines=None, target=None, additional_forward_args=None, feature_mask=None, n_samples=25,
                  perturbations_per_eval=1, show_progress=False):
        if _masked(self.model):
            B, Fm, Tm, ibs = _mask_batch(self.model, inputs, target, perturbations_per_eval)
            _S.check_mask_baselines(baselines, B, Fm, Tm)
            _A.shapley_feature_indices(_S.flat_feature_mask(feature_mask, B, Fm, Tm), B, Fm * Tm)
            _A.check_n_samples(n_samples)
            return self.model.hip_mask_attribution().shapley_value_sampling(inputs, baselines=baselines, feature_mask=feature_mask,
                                                                            n_samples=n_samples, internal_batch_size=ibs)
        ibs = _shapley_checks(inputs, target, perturbations_per_eval, baselines, feature_mask)
        _A.check_n_samples(n_samples)
        return _engine(self.model).shapley_value_sampling(inputs, baselines=baselines, feature_mask=feature_mask,
                                                          n_samples=n_samples, internal_batch_size=ibs)


class ShapleyValues(_Method):
    """Captum's ShapleyValues: ShapleyValueSampling over all K! permutations of the K features (a UserWarning above 10)."""

    def attribute(self, inputs, baselines=None, target=None, additional_forward_args=None, feature_mask=None,
                  perturbations_per_eval=1, show_progress=False):
        _no_masks(self.model, "ShapleyValues")
        ibs = _shapley_checks(inputs, target, perturbations_per_eval, baselines, feature_mask)
        return _engine(self.model).shapley_values(inputs, baselines=baselines, feature_mask=feature_mask, internal_batch_size=ibs)


class KernelShap(_Method):
    """Captum's KernelShap: per clip, ``n_samples`` (>= 2) coalitions of the features present in the clip (all, none, then
    sizes drawn with the Shapley kernel's law) and a weighted linear regression of the logits on them; every sample gets its
    feature's coefficient (``return_input_shape=False``: the ``[K]`` coefficients of a single clip).  Draws as
    ShapleyValueSampling; the regression is solved in float64 on the host."""

    def attribute(self, inputs, baselines=None, target=None, additional_forward_args=None, feature_mask=None, n_samples=25,
                  perturbations_per_eval=1, return_input_shape=True, show_progress=False):
        _no_masks(self.model, "KernelShap")
        ibs = _perturbation_batch(inputs, target, perturbations_per_eval)
        B, L = inputs.shape
        _A.check_ig_baselines(baselines, B, L)
        _A.kernel_shap_feature_indices(feature_mask, B, L)
        _A.check_n_samples(n_samples, 2)
        if not return_input_shape and B > 1:
            raise ValueError("return_input_shape=False returns one clip's coefficients: pass a single clip")
        return _engine(self.model).kernel_shap(inputs, baselines=baselines, feature_mask=feature_mask, n_samples=n_samples,
                                               internal_batch_size=ibs, return_input_shape=return_input_shape)


class Lime(_Method):
    """Captum's Lime: per clip, ``n_samples`` interpretable samples over the features present in the clip (``feature_mask``:
    None = every sample its own feature, else an integer ``[1, L]`` or ``[B, L]`` tensor; any id, negative included), drawn by
    ``perturb_func`` (default Bernoulli(0.5), drawn on the host from one seed per call of torch's default CPU generator, so
    ``torch.manual_seed`` reproduces a result); each sample keeps the clip on the features that are on and ``baselines``
    (None = 0, a number, ``[1, L]`` or ``[B, L]``) elsewhere, and is weighted by ``similarity_func`` against the clip (default
    ``get_exp_kernel_similarity_function("cosine", 1.0)``, computed on the device).  ``interpretable_model`` (default
    ``SkLearnLasso(alpha=0.01)``) is fitted on (samples, logits, weights); every sample of the clip gets its feature's
    coefficient (``return_input_shape=False``: the ``[1, K]`` coefficients of a single clip)."""

    def __init__(self, forward_func, interpretable_model=None, similarity_func=None, perturb_func=None):
        super().__init__(forward_func)
        self.interpretable_model = SkLearnLasso(alpha=0.01) if interpretable_model is None else interpretable_model
        self.similarity_func = get_exp_kernel_similarity_function() if similarity_func is None else similarity_func
        self.perturb_func = default_perturb_func if perturb_func is None else perturb_func

    def attribute(self, inputs, baselines=None, target=None, additional_forward_args=None, feature_mask=None, n_samples=50,
                  perturbations_per_eval=1, return_input_shape=True, show_progress=False):
        _no_masks(self.model, "Lime")
        ibs = _perturbation_batch(inputs, target, perturbations_per_eval)
        B, L = inputs.shape
        _A.check_ig_baselines(baselines, B, L)
        _A.per_clip_feature_indices(feature_mask, B, L)
        _A.check_n_samples(n_samples)
        if not return_input_shape and B > 1:
            raise ValueError("return_input_shape=False returns one clip's coefficients: pass a single clip")
        perturb = None if self.perturb_func is default_perturb_func else self.perturb_func
        _A.check_lime_callables(self.similarity_func, perturb, self.interpretable_model)
        return _engine(self.model).lime(inputs, baselines=baselines, feature_mask=feature_mask, n_samples=n_samples,
                                        internal_batch_size=ibs, return_input_shape=return_input_shape,
                                        interpretable_model=self.interpretable_model, similarity_func=self.similarity_func,
                                        perturb_func=perturb)


class FeaturePermutation(_Method):
    """Captum's FeaturePermutation: each feature of ``feature_mask`` (None = every sample its own feature, else one integer
    ``[1, L]`` mask) is replaced in every clip by the same samples of another clip of the batch (a permutation of the clips
    that is not the identity, one per feature), and every sample of the feature gets ``F(x)[b] - F(permuted)[b]``.  Needs at
    least two clips.  The permutations follow ``torch``'s default CPU generator through one seed per call (``torch.manual_seed``
    reproduces a result); Captum's own RNG stream is not reproduced.  Only the default ``perm_func`` is supported."""

    def __init__(self, forward_func, perm_func=_permute_feature):
        super().__init__(forward_func)
        if perm_func is not _permute_feature:
            raise ValueError("FeaturePermutation (HIP build) permutes on the device: only the default perm_func is supported")
        self.perm_func = perm_func

    def attribute(self, inputs, target=None, additional_forward_args=None, feature_mask=None, perturbations_per_eval=1,
                  show_progress=False):
        _no_masks(self.model, "FeaturePermutation")
        ibs = _perturbation_batch(inputs, target, perturbations_per_eval)
        B, L = inputs.shape
        _A.check_permutation_args(feature_mask, B, L)
        return _engine(self.model).feature_permutation(inputs, feature_mask=feature_mask, internal_batch_size=ibs)


def _layer_checks(model, inputs, target, layer, attribute_to_layer_input):
    """The checks every layer method shares, before the engine is touched: one output (``target`` None), a ``[B, L]`` input, the
    layer's output only (``attribute_to_layer_input=True`` raises NotImplementedError) and ``check_layer`` against the model's
    ``layer_index`` (ValueError)."""
    _no_masks(model, "a layer or neuron method")
    _Method._check(inputs, target)
    if attribute_to_layer_input:
        raise NotImplementedError("the layer methods (HIP build) attribute to a layer's output, hidden_states[layer]; "
                                  "attribute_to_layer_input=True is not supported")
    if not hasattr(model, "hip_attribution"):
        raise TypeError("captum.attr (HIP build) only attributes captum_saliency.Wav2vec2LogReg models")
    nl = model.num_layers() if hasattr(model, "num_layers") else None
    if nl is not None:
        _A.check_layer(layer, nl)
    elif isinstance(layer, bool) or not isinstance(layer, int) or layer < 0:
        raise ValueError(f"layer must be an integer index into hidden_states, not {layer!r}")


class _LayerMethod(_Method):
    """``Method(forward_func, layer)``: ``layer`` is an integer index ``l`` into the encoder's ``hidden_states``,
    ``0 <= l <= layer_index`` -- not an ``nn.Module`` (the frozen embedder has none to hook).  Attributions are ``[B, T, H]``."""

    def __init__(self, forward_func, layer, device_ids=None):
        super().__init__(forward_func)
        self.layer = layer


class LayerActivation(_LayerMethod):
    """Captum's LayerActivation: ``hidden_states[layer](inputs)``."""

    def attribute(self, inputs, additional_forward_args=None, attribute_to_layer_input=False):
        _layer_checks(self.model, inputs, None, self.layer, attribute_to_layer_input)
        return _engine(self.model).layer_activation(inputs, self.layer)


class LayerGradientXActivation(_LayerMethod):
    """Captum's LayerGradientXActivation: ``dF/dh_l * h_l`` (the gradient alone with ``multiply_by_inputs=False``)."""

    def __init__(self, forward_func, layer, device_ids=None, multiply_by_inputs=True):
        super().__init__(forward_func, layer)
        self.multiply_by_inputs = multiply_by_inputs

    def attribute(self, inputs, target=None, additional_forward_args=None, attribute_to_layer_input=False):
        _layer_checks(self.model, inputs, target, self.layer, attribute_to_layer_input)
        return _engine(self.model).layer_gradient_x_activation(inputs, self.layer, multiply_by_inputs=self.multiply_by_inputs)


def _layer_path_checks(method_obj, inputs, target, attribute_to_layer_input, baselines, n_steps, method, internal_batch_size,
                       extra_point=False):
    _layer_checks(method_obj.model, inputs, target, method_obj.layer, attribute_to_layer_input)
    B, L = inputs.shape
    _A.check_ig_baselines(baselines, B, L)
    _A.approximation(method, _A.check_steps(n_steps, method) + int(extra_point))
    if internal_batch_size is not None:
        _A._positive_int(internal_batch_size, "internal_batch_size")


class LayerIntegratedGradients(_LayerMethod):
    """Captum's LayerIntegratedGradients: integrated gradients along the straight path between the layer's activations of the
    baseline and of the input (``baselines`` live in waveform space: None, a number, ``[1, L]`` or ``[B, L]``).
    ``return_convergence_delta=True`` returns ``(attributions, delta [B])``."""

    def __init__(self, forward_func, layer, device_ids=None, multiply_by_inputs=True):
        super().__init__(forward_func, layer)
        self.multiply_by_inputs = multiply_by_inputs

    def attribute(self, inputs, baselines=None, target=None, additional_forward_args=None, n_steps=50, method="gausslegendre",
                  internal_batch_size=None, return_convergence_delta=False, attribute_to_layer_input=False):
        _layer_path_checks(self, inputs, target, attribute_to_layer_input, baselines, n_steps, method, internal_batch_size)
        return _engine(self.model).layer_integrated_gradients(
            inputs, self.layer, baselines=baselines, n_steps=n_steps, method=method, internal_batch_size=internal_batch_size,
            multiply_by_inputs=self.multiply_by_inputs, return_convergence_delta=return_convergence_delta)


class LayerConductance(_LayerMethod):
    """Captum's LayerConductance: ``sum_k dF/dh_l(x_k) * (h_l(x_{k+1}) - h_l(x_k))`` over ``n_steps + 1`` points of the
    waveform-space path from the baseline to the input.  The convergence delta is not computed."""

    def attribute(self, inputs, baselines=None, target=None, additional_forward_args=None, n_steps=50, method="gausslegendre",
                  internal_batch_size=None, return_convergence_delta=False, attribute_to_layer_input=False):
        _layer_path_checks(self, inputs, target, attribute_to_layer_input, baselines, n_steps, method, internal_batch_size, True)
        if return_convergence_delta:
            raise NotImplementedError("LayerConductance (HIP build) does not compute the convergence delta")
        return _engine(self.model).layer_conductance(inputs, self.layer, baselines=baselines, n_steps=n_steps, method=method,
                                                     internal_batch_size=internal_batch_size)


class InternalInfluence(_LayerMethod):
    """Captum's InternalInfluence: the layer gradient integrated along the waveform-space path from the baseline to the input."""

    def attribute(self, inputs, baselines=None, target=None, additional_forward_args=None, n_steps=50, method="gausslegendre",
                  internal_batch_size=None, attribute_to_layer_input=False):
        _layer_path_checks(self, inputs, target, attribute_to_layer_input, baselines, n_steps, method, internal_batch_size)
        return _engine(self.model).internal_influence(inputs, self.layer, baselines=baselines, n_steps=n_steps, method=method,
                                                      internal_batch_size=internal_batch_size)


def _neuron_checks(method_obj, inputs, target, neuron_selector, attribute_to_neuron_input):
    """The checks every neuron method shares, before the engine is touched: those of ``_layer_checks``; the neuron's output only
    (``attribute_to_neuron_input=True`` raises NotImplementedError); ``check_neuron_selector`` against the model's frame shape
    (ValueError; NotImplementedError for a callable)."""
    model = method_obj.model
    _layer_checks(model, inputs, target, method_obj.layer, False)
    if attribute_to_neuron_input:
        raise NotImplementedError("the neuron methods (HIP build) attribute a neuron's output, an entry of hidden_states[layer]; "
                                  "attribute_to_neuron_input=True is not supported")
    if hasattr(model, "frame_shape"):
        _A.check_neuron_selector(neuron_selector, *model.frame_shape(inputs.shape[1]))
    elif callable(neuron_selector):
        raise NotImplementedError("a callable neuron_selector is not supported (HIP build)")
    elif not isinstance(neuron_selector, (tuple, list)) or len(neuron_selector) != 2:
        raise ValueError(f"neuron_selector must be a (t, h) tuple of ints or slices, not {neuron_selector!r}")


class _NeuronMethod(_LayerMethod):
    """``Method(forward_func, layer)`` with ``attribute(inputs, neuron_selector, ...)``: ``layer`` as for the layer methods,
    ``neuron_selector`` a ``(t, h)`` tuple of ints or slices into the ``[T, H]`` frame of ``hidden_states[layer]`` (several
    units are summed, as Captum does; a callable raises NotImplementedError).  Attributions are ``[B, L]``."""

    def __init__(self, forward_func, layer, device_ids=None, multiply_by_inputs=True):
        super().__init__(forward_func, layer)
        self.multiply_by_inputs = multiply_by_inputs

    def _path_checks(self, inputs, target, neuron_selector, attribute_to_neuron_input, baselines, n_steps, method, internal_batch_size):
        _neuron_checks(self, inputs, target, neuron_selector, attribute_to_neuron_input)
        B, L = inputs.shape
        _A.check_ig_baselines(baselines, B, L)
        _A.approximation(method, _A.check_steps(n_steps, method))
        if internal_batch_size is not None:
            _A._positive_int(internal_batch_size, "internal_batch_size")


class NeuronGradient(_NeuronMethod):
    """Captum's NeuronGradient: the gradient of the selected neuron with respect to the waveform."""

    def __init__(self, forward_func, layer, device_ids=None):
        super().__init__(forward_func, layer)

    def attribute(self, inputs, neuron_selector, additional_forward_args=None, attribute_to_neuron_input=False):
        _neuron_checks(self, inputs, None, neuron_selector, attribute_to_neuron_input)
        return _engine(self.model).neuron_gradient(inputs, self.layer, neuron_selector)


class NeuronIntegratedGradients(_NeuronMethod):
    """Captum's NeuronIntegratedGradients: integrated gradients of the selected neuron along the waveform-space path from
    ``baselines`` (None, a number, ``[1, L]`` or ``[B, L]``) to the input.  It has no convergence delta."""

    def attribute(self, inputs, neuron_selector, baselines=None, target=None, additional_forward_args=None, n_steps=50,
                  method="gausslegendre", internal_batch_size=None, attribute_to_neuron_input=False):
        self._path_checks(inputs, target, neuron_selector, attribute_to_neuron_input, baselines, n_steps, method, internal_batch_size)
        return _engine(self.model).neuron_integrated_gradients(
            inputs, self.layer, neuron_selector, baselines=baselines, n_steps=n_steps, method=method,
            internal_batch_size=internal_batch_size, multiply_by_inputs=self.multiply_by_inputs)


class NeuronGradientShap(_NeuronMethod):
    """Captum's NeuronGradientShap: GradientShap of the selected neuron (``baselines [N_b, L]`` or a callable returning it;
    draws as GradientShap)."""

    def attribute(self, inputs, neuron_selector, baselines, n_samples=5, stdevs=0.0, additional_forward_args=None,
                  attribute_to_neuron_input=False):
        _neuron_checks(self, inputs, None, neuron_selector, attribute_to_neuron_input)
        return _engine(self.model).neuron_gradient_shap(inputs, self.layer, neuron_selector, baselines, n_samples=n_samples,
                                                        stdevs=stdevs, multiply_by_inputs=self.multiply_by_inputs)


class NeuronConductance(_NeuronMethod):
    """Captum's NeuronConductance: the conductance of a single neuron (``neuron_selector``: two ints; a slice raises ValueError)
    along the waveform-space path, ``(x - b) * sum_k w_k dF/dh_n(x_k) dh_n/dx(x_k)``.  ``method`` defaults to Captum's
    ``riemann_trapezoid`` here."""

    def attribute(self, inputs, neuron_selector, baselines=None, target=None, additional_forward_args=None, n_steps=50,
                  method="riemann_trapezoid", internal_batch_size=None, attribute_to_neuron_input=False):
        self._path_checks(inputs, target, neuron_selector, attribute_to_neuron_input, baselines, n_steps, method, internal_batch_size)
        if any(isinstance(s, slice) for s in neuron_selector):
            raise ValueError("NeuronConductance (HIP build) takes a single neuron: two ints, not slices")
        return _engine(self.model).neuron_conductance(
            inputs, self.layer, neuron_selector, baselines=baselines, n_steps=n_steps, method=method,
            internal_batch_size=internal_batch_size, multiply_by_inputs=self.multiply_by_inputs)


class NeuronFeatureAblation(_NeuronMethod):
    """Captum's NeuronFeatureAblation: FeatureAblation with the selected neuron's activation in the place of the logit."""

    def __init__(self, forward_func, layer, device_ids=None):
        super().__init__(forward_func, layer)

    def attribute(self, inputs, neuron_selector, baselines=None, additional_forward_args=None, feature_mask=None,
                  attribute_to_neuron_input=False, perturbations_per_eval=1):
        ibs = _perturbation_batch(inputs, None, perturbations_per_eval)
        _neuron_checks(self, inputs, None, neuron_selector, attribute_to_neuron_input)
        B, L = inputs.shape
        _A.check_ig_baselines(baselines, B, L)
        _A.feature_indices(feature_mask, B, L)
        return _engine(self.model).neuron_feature_ablation(inputs, self.layer, neuron_selector, baselines=baselines,
                                                           feature_mask=feature_mask, internal_batch_size=ibs)


_WRAPPABLE = (Saliency, InputXGradient, IntegratedGradients, GradientShap, Occlusion, FeatureAblation, FeaturePermutation,
              ShapleyValueSampling, ShapleyValues, KernelShap, Lime)


class NoiseTunnel:
    """Captum's NoiseTunnel, restated from Captum 0.7's ``noise_tunnel.py`` (captum is absent): the wrapped method attributes
    ``nt_samples`` noisy copies ``x + stdevs * N(0, 1)`` of each clip, ``nt_samples_batch_size`` samples per call (Captum's
    partitions, rows ``repeat_interleave``d), and the attributions a are reduced per element to ``smoothgrad`` E[a],
    ``smoothgrad_sq`` E[a^2] or ``vargrad`` E[a^2] - E[a]^2.  ``baselines`` / ``feature_mask`` and the other keyword arguments
    go to the wrapped method's ``attribute``, expanded per partition as Captum does; ``draw_baseline_from_distrib=True`` draws
    each noisy row's baseline from ``baselines [N_b, L]``.  ``return_convergence_delta=True`` (IntegratedGradients and
    GradientShap only) returns ``(attributions, delta)``, the wrapped deltas concatenated over partitions.  The noise and the
    draws follow ``torch``'s default CPU generator through one seed per call, drawn before the wrapped method draws its own
    (``torch.manual_seed`` reproduces a result); Captum's own RNG stream is not reproduced."""

    def __init__(self, attribution_method):
        if not isinstance(attribution_method, _WRAPPABLE):
            raise TypeError("NoiseTunnel (HIP build) wraps Saliency, InputXGradient, IntegratedGradients, GradientShap, Occlusion, "
                            "FeatureAblation, FeaturePermutation, ShapleyValueSampling, ShapleyValues, KernelShap or Lime, not "
                            f"{type(attribution_method).__name__}")
        self.attribution_method = attribution_method
        self.is_delta_supported = isinstance(attribution_method, (IntegratedGradients, GradientShap))

    def has_convergence_delta(self):
        return self.is_delta_supported

    def attribute(self, inputs, nt_type="smoothgrad", nt_samples=5, nt_samples_batch_size=None, stdevs=1.0,
                  draw_baseline_from_distrib=False, **kwargs):
        _no_masks(self.attribution_method.model, "NoiseTunnel")
        return_convergence_delta = kwargs.pop("return_convergence_delta", False)
        _A.check_noise_tunnel_args(nt_type, nt_samples, nt_samples_batch_size, stdevs, kwargs.pop("target", None))
        if not torch.is_tensor(inputs) or inputs.dim() != 2:
            raise ValueError("inputs must be a [B, L] waveform tensor")
        if return_convergence_delta and not self.is_delta_supported:
            raise ValueError(f"{type(self.attribution_method).__name__} has no convergence delta")
        if draw_baseline_from_distrib:
            _A.check_baseline_distribution(kwargs.get("baselines"), inputs.shape[1])
        return _engine(self.attribution_method.model).noise_tunnel(
            inputs, self.attribution_method.attribute, nt_type=nt_type, nt_samples=nt_samples,
            nt_samples_batch_size=nt_samples_batch_size, stdevs=stdevs, draw_baseline_from_distrib=draw_baseline_from_distrib,
            return_convergence_delta=return_convergence_delta, **kwargs)
