"""Drop-in for the reference's ``captum_saliency`` module (captum_saliency.py:1-219): ``Wav2vec2LogReg``,
the metric helpers and ``compute_camptum_saliency_metrics``, on the HIP forward + dgrad-only backward.
Nothing runs at import (the reference executes the whole evaluation at import, captum_saliency.py:215-219)."""
import os

import torch
import torch.nn as nn

from addvisor_hip import pipeline as _P, runtime as _rt
from audioprocessor import AudioProcessor
from captum.attr import Saliency, InputXGradient, IntegratedGradients, GradientShap, NoiseTunnel  # noqa: F401
from captum.attr import Occlusion, FeatureAblation  # noqa: F401
from captum.attr import ShapleyValueSampling, ShapleyValues, KernelShap  # noqa: F401
from captum.attr import Lime, FeaturePermutation  # noqa: F401
from captum.attr import LayerActivation, LayerGradientXActivation, LayerIntegratedGradients, LayerConductance  # noqa: F401
from captum.attr import InternalInfluence  # noqa: F401
from captum.attr import NeuronGradient, NeuronIntegratedGradients, NeuronGradientShap, NeuronConductance  # noqa: F401
from captum.attr import NeuronFeatureAblation  # noqa: F401
from captum.attr._core.lime import get_exp_kernel_similarity_function  # noqa: F401
from captum._utils.models.linear_model import SkLearnLasso, SkLearnRidge, SkLearnLinearRegression  # noqa: F401
from captum.metrics import infidelity, sensitivity_max, NoisyPerturbation  # noqa: F401
from captum.robust import FGSM, PGD  # noqa: F401
from classifier_embedder import TorchLogReg  # noqa: F401  (name kept for callers of the reference module)

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
audioprocessor = AudioProcessor()


@torch.no_grad()
def compute_fidelity(theta_out, predictions, threshold=0.5):
    """captum_saliency.py:68-75."""
    return ((predictions > threshold).long() == (theta_out > threshold).long()).float()


def compute_faithfulness(predictions, predictions_masked):
    """captum_saliency.py:78-81."""
    return ((predictions - predictions_masked) * torch.sign(predictions - 0.5)).squeeze(dim=1)


class Wav2vec2LogReg(nn.Module):
    """captum_saliency.py:84-100: waveform -> logit, pooled over time per example."""

    def __init__(self, audioprocessor, logReg):
        super().__init__()
        self.ap = audioprocessor
        self.logReg = logReg
        self._att = None
        self._rob = None

    def forward(self, waveform, lengths=None):
        """``lengths``: per-clip sample counts of a ragged batch (forward only: the attribution methods take none)."""
        logits, _ = self.ap.classify(waveform) if lengths is None else self.ap.classify(waveform, lengths=lengths)
        return logits

    def num_layers(self):
        """``nl``: the last index into ``hidden_states`` that reaches the logit (``HipEmbedder.nl``), from the configuration
        alone -- the layer methods check their ``layer`` against it before any GPU work."""
        cfg, _ = _rt.embedder_config_and_weights()
        return min(cfg.layer_index, cfg.num_hidden_layers)

    def frame_shape(self, n_samples):
        """``(T, H)`` of ``hidden_states[l]`` for clips of ``n_samples`` samples, from the configuration alone -- the neuron
        methods check their ``neuron_selector`` against it before any GPU work."""
        cfg, _ = _rt.embedder_config_and_weights()
        n = int(n_samples)
        for k, s in zip(cfg.conv_kernel, cfg.conv_stride):
            n = (n - k) // s + 1
        return n, cfg.hidden_size

    def hip_attribution(self):
        if self._att is None:
            from addvisor_hip.attribution import HipAttribution
            kw = {}                                            # ADDVISOR_LONG_CLIPS / ADDVISOR_LONG_MAPS, as the runtime's singleton reads them
            if _rt.long_clips():
                kw["long_clips"] = True
            if _rt.long_maps():
                kw["long_maps"] = True
            self._att = HipAttribution(_rt.hip_embedder(), **kw)
        return self._att

    def hip_robust(self):
        if self._rob is None:
            from addvisor_hip.robust import HipRobust
            self._rob = HipRobust(self.hip_attribution())
        return self._rob


class MaskedSpectrogramLogReg(nn.Module):
    """STFT mask -> logit: ``F(m)[b] = logit(embedder(istft(X_b * g(m, |X_b|) / |X_b|)))`` over the clips ``waves [B, L]``
    (``domain``: ``"linear"`` loss_function.py:36-45, or ``"log1p"`` LMAC_metrics.py:136-153; mask-in branch, bins outside the
    mask's crop count as 0).  ``model`` is the ``Wav2vec2LogReg`` whose classifier is attributed.  The ``captum.attr`` methods
    given this model attribute ``[B, Fm, Tm]`` masks (usually ``torch.ones(B, Fm, Tm)``, the clip itself, or the U-Net's mask)
    on ``addvisor_hip.spectral_attribution.HipSpectralAttribution``."""

    def __init__(self, model, waves, domain="linear"):
        super().__init__()
        from addvisor_hip import spectral_attribution as _S
        if not hasattr(model, "hip_attribution"):
            raise TypeError("MaskedSpectrogramLogReg wraps a captum_saliency.Wav2vec2LogReg")
        if domain not in _S.DOMAINS:
            raise ValueError(f"domain must be one of {_S.DOMAINS}, not {domain!r}")
        if not torch.is_tensor(waves) or waves.dim() not in (1, 2):
            raise ValueError("waves must be a [B, L] (or [L]) tensor")
        self.model, self.domain = model, domain
        self.waves = waves[None] if waves.dim() == 1 else waves
        self.hop, self.win = 322, 644
        self._eng = None

    def num_clips(self):
        return self.waves.shape[0]

    def mask_frames(self):
        """``T``: the frames of the clips' spectrograms, the largest ``Tm`` a mask may have."""
        return 1 + self.waves.shape[1] // self.hop

    def forward(self, mask):
        return self.hip_mask_attribution().logits(mask).view(-1, 1)

    def hip_mask_attribution(self):
        if self._eng is None:
            from addvisor_hip.spectral_attribution import HipSpectralAttribution
            self._eng = HipSpectralAttribution(self.model.hip_attribution(), self.waves, self.domain, self.hop, self.win)
        return self._eng


def tf_feature_mask(Fm, Tm, band_bins=64, seg_frames=None):
    """Feature ids ``[1, Fm, Tm]`` for FeatureAblation / ShapleyValueSampling over STFT masks: one per 1 kHz band
    (``band_bins = 64`` of the 513 bins) and, with ``seg_frames``, per time segment (``id = band * n_seg + segment``)."""
    from addvisor_hip.spectral_attribution import tf_feature_mask as _tf
    return _tf(Fm, Tm, band_bins, seg_frames)


SPECTRAL_METHODS = ("saliency", "input_x_gradient", "integrated_gradients", "occlusion", "feature_ablation",
                    "shapley_value_sampling", "optimized_mask")


def explain_spectrogram(model, waves, method="input_x_gradient", mask=None, baselines=None, n_steps=50, window=(64, 8),
                        stride=(64, 4), band_bins=64, seg_frames=16, n_samples=25, domain="linear", mask_opt=None):
    """``explain_waves`` in the time-frequency domain for a batch ``[B, L]``: ``method`` (one of ``SPECTRAL_METHODS``) attributes
    the classifier to the STFT mask ``mask`` (default ``ones(B, 513, T)``: the clip itself) through ``F`` of
    ``MaskedSpectrogramLogReg(model, waves, domain)``; the explanation mask is ``|attr| / (max|attr| + 1e-8)`` per clip, and the
    mask-in / mask-out signals are resynthesised from it in the ``log1p`` domain (``ops.istft_masked_c64``, LMAC_metrics.py:136-153).
    ``"occlusion"`` uses ``window`` / ``stride`` (bins, frames); ``"feature_ablation"`` and ``"shapley_value_sampling"`` the
    features of ``tf_feature_mask(Fm, Tm, band_bins, seg_frames)``; ``baselines`` as the engine's methods take them (for
    ``"integrated_gradients"`` pass a mask baseline, not the zero mask: HipSpectralAttribution).  Three classifier passes in one
    forward; returns ``(predictions, theta_out, masked_predictions)``, each ``[B, 1]``, ready for ``compute_faithfulness``,
    ``compute_fidelity`` and ``lmac_metrics``.
    ``"optimized_mask"`` attributes nothing: the explanation mask is the per-clip optimised mask itself
    (``HipSpectralAttribution.optimize_mask(shape=(Fm, Tm), **mask_opt)``, ``mask_opt`` a dict of its keywords or None), not
    ``|attr| / max``; the three outputs come out as for every other method."""
    if method not in SPECTRAL_METHODS:
        raise ValueError(f"method must be one of {SPECTRAL_METHODS}, not {method!r}")
    if not torch.is_tensor(waves) or waves.dim() != 2:
        raise ValueError("waves must be a [B, L] tensor")
    if mask_opt is not None and (method != "optimized_mask" or not isinstance(mask_opt, dict) or "shape" in mask_opt):
        raise ValueError("mask_opt is the dict of optimize_mask's keywords for method='optimized_mask' (the shape is the mask's)")
    eng = MaskedSpectrogramLogReg(model, waves, domain).hip_mask_attribution()
    B, T = eng.B, eng.T
    m = torch.ones((B, 513, T), dtype=torch.float32, device=eng.waves.device) if mask is None else mask.to(eng.waves.device, torch.float32)
    Fm, Tm = m.shape[1], m.shape[2]
    if method == "optimized_mask":
        rel = eng.optimize_mask(shape=(Fm, Tm), **(mask_opt or {})).mask
        return _mask_outputs(model, eng, rel)
    if method == "saliency":
        attr = eng.saliency(m)
    elif method == "input_x_gradient":
        attr = eng.input_x_gradient(m)
    elif method == "integrated_gradients":
        attr = eng.integrated_gradients(m, n_steps=n_steps, baselines=baselines)
    elif method == "occlusion":
        attr = eng.occlusion(m, window, stride, baselines=baselines)
    else:
        ids = tf_feature_mask(Fm, Tm, band_bins, seg_frames)
        attr = (eng.feature_ablation(m, baselines=baselines, feature_mask=ids) if method == "feature_ablation" else
                eng.shapley_value_sampling(m, baselines=baselines, feature_mask=ids, n_samples=n_samples))
    return _mask_outputs(model, eng, model.hip_attribution().time_mask(attr.reshape(B, Fm * Tm)).view(B, Fm, Tm))


def _mask_outputs(model, eng, rel):
    """The three ``[B, 1]`` outputs of an explanation mask ``rel [B, Fm, Tm]``: the clip, its mask-in and its mask-out ``log1p``
    resynthesis in one forward."""
    from addvisor_hip import ops as _ops
    B = eng.B
    w_rel, w_irr = _ops.istft_masked_c64(eng.spec, rel, eng.L, "log1p", hop=eng.hop, win=eng.win)
    _, _, p = model.hip_attribution().emb.forward(torch.cat([eng.waves, w_rel, w_irr], 0), want_hidden=False)
    return p[:B], p[B:2 * B], p[2 * B:]


def extract_wavs(metadata):
    """captum_saliency.py:103-109."""
    audio_files = []
    with open(metadata, "r") as f:
        for line in f:
            audio_files.append(line.strip().split(",")[0])
    return audio_files


def _segments(waves, window):
    """Feature ids of consecutive ``window``-sample segments, ``[1, L]``."""
    return (torch.arange(waves.shape[-1], device=waves.device) // window)[None]


def _check_batch(method, waves):
    """``"feature_permutation"`` permutes segments across the clips of the batch: a single clip raises ValueError before any GPU
    work."""
    if method == "feature_permutation" and (waves.dim() < 2 or waves.shape[0] < 2):
        raise ValueError("method='feature_permutation' takes each segment from another clip of the batch: pass two clips or more")


def _explainer(att, method, n_steps=50, window=1600, stride=800, nt_type=None, nt_samples=5, stdevs=0.01, layer=None, neuron=None):
    """The attribution of ``explain_waves``'s ``method`` (wrapped in NoiseTunnel when ``nt_type`` is set) as a callable
    ``[R, L] -> [R, L]`` on the engine ``att``.  The layer methods attribute ``hidden_states[layer]`` (default: the layer the
    classifier reads); their ``[R, T, H]`` map is summed over the channels and each frame's relevance spread to its samples
    (``HipAttribution.layer_relevance``).  The neuron methods attribute the unit(s) ``neuron`` (a ``(t, h)`` tuple of ints or
    slices) of that layer to the waveform directly.  ``"attention_rollout"`` / ``"attention_grad_rollout"`` roll the encoder's
    attention maps out from ``layer`` (the ``start_layer``, default 0; checked here, before any GPU work) and spread the
    per-frame relevance to the samples (``HipAttribution.frames_to_wave``); NoiseTunnel may wrap them.  ``"transformer_lrp"``
    (conservative propagation, Ali et al. 2022: ``HipAttribution.transformer_lrp`` with its default rules) takes ``layer`` as its
    ``start_layer`` the same way; it stands for no Captum class."""
    if method in ("neuron_gradient", "neuron_integrated_gradients"):
        if nt_type is not None:
            raise ValueError("NoiseTunnel does not wrap the neuron methods")
        if neuron is None:
            raise ValueError(f"method={method!r} needs neuron=(t, h)")
        l = att.eg.emb.nl if layer is None else layer
        if method == "neuron_integrated_gradients":
            return lambda w: att.neuron_integrated_gradients(w, l, neuron, n_steps=n_steps)
        return lambda w: att.neuron_gradient(w, l, neuron)
    if method in ("layer_integrated_gradients", "layer_gradient_x_activation"):
        if nt_type is not None:
            raise ValueError("NoiseTunnel does not wrap the layer methods")
        l = att.eg.emb.nl if layer is None else layer
        if method == "layer_integrated_gradients":
            return lambda w: att.layer_relevance(att.layer_integrated_gradients(w, l, n_steps=n_steps), w.shape[-1])
        return lambda w: att.layer_relevance(att.layer_gradient_x_activation(w, l), w.shape[-1])
    s0 = 0
    if method in ("attention_rollout", "attention_grad_rollout", "transformer_lrp"):
        s0 = att.check_attention_layer(0 if layer is None else layer, "layer (the method's start_layer)")
    fn = {"saliency": att.saliency, "input_x_gradient": att.input_x_gradient,
          "attention_rollout": lambda w: att.frames_to_wave(att.attention_rollout(w, start_layer=s0), w.shape[-1]),
          "attention_grad_rollout": lambda w: att.frames_to_wave(att.attention_grad_rollout(w, start_layer=s0), w.shape[-1]),
          "transformer_lrp": lambda w: att.frames_to_wave(att.transformer_lrp(w, start_layer=s0), w.shape[-1]),
          "integrated_gradients": lambda w: att.integrated_gradients(w, n_steps=n_steps),
          "occlusion": lambda w: att.occlusion(w, window, stride),
          "shapley_value_sampling": lambda w: att.shapley_value_sampling(w, feature_mask=_segments(w, window)),
          "kernel_shap": lambda w: att.kernel_shap(w, feature_mask=_segments(w, window)),
          "lime": lambda w: att.lime(w, feature_mask=_segments(w, window)),
          "feature_permutation": lambda w: att.feature_permutation(w, feature_mask=_segments(w, window))}[method]
    if nt_type is None:
        return fn
    return lambda w: att.noise_tunnel(w, fn, nt_type=nt_type, nt_samples=nt_samples, stdevs=stdevs)


def explain_waves(model, waves, method="input_x_gradient", n_steps=50, window=1600, stride=800, nt_type=None, nt_samples=5,
                  stdevs=0.01, layer=None, neuron=None):
    """Loop body of compute_camptum_saliency_metrics (captum_saliency.py:125-192) for a batch ``[B, L]``:
    attribution -> |attr|/max time mask -> wave*mask, wave*(1-mask) -> three classifier passes.
    ``method="occlusion"`` occludes ``window``-sample windows every ``stride`` samples (default 100 ms / 50 ms at 16 kHz);
    ``method="shapley_value_sampling"`` / ``"kernel_shap"`` attribute ``window``-sample segments (default n_samples = 25), as do
    ``"lime"`` (n_samples = 50, the cosine kernel, a Lasso with alpha = 0.01) and ``"feature_permutation"`` (each segment taken
    from another clip of the batch: it needs two clips or more, ValueError before any GPU work otherwise).
    ``method="layer_integrated_gradients"`` / ``"layer_gradient_x_activation"`` attribute ``hidden_states[layer]`` (``layer=None``:
    the layer the classifier reads) and mask the waveform with each frame's relevance summed over the channels;
    ``method="neuron_gradient"`` / ``"neuron_integrated_gradients"`` attribute the unit(s) ``neuron`` (a ``(t, h)`` tuple of ints
    or slices) of ``hidden_states[layer]`` to the waveform.
    ``method="attention_rollout"`` (Abnar & Zuidema 2020) / ``"attention_grad_rollout"`` (the self-attention rule of Chefer et al.
    2021) roll the encoder's head-fused attention maps out from ``layer`` (default 0) and mask the waveform with each frame's
    relevance (``HipAttribution.attention_rollout`` / ``attention_grad_rollout``).
    ``method="transformer_lrp"`` (conservative propagation, Ali et al. 2022) masks it with gradient x input of the locally
    linearised encoder at ``hidden_states[layer]`` (default 0), summed over the channels (``HipAttribution.transformer_lrp``).
    ``nt_type`` ("smoothgrad", "smoothgrad_sq", "vargrad") wraps the method in NoiseTunnel over ``nt_samples`` noisy copies
    of each clip; ``stdevs`` is the noise's standard deviation in waveform units (Captum's default of 1.0 would drown a
    waveform in [-1, 1]).  Returns ``(predictions, theta_out, masked_predictions)``, each ``[B,1]``."""
    _check_batch(method, waves)
    att = model.hip_attribution()
    x = waves.to(device, torch.float32)
    attr = _explainer(att, method, n_steps, window, stride, nt_type, nt_samples, stdevs, layer, neuron)(x)
    _, w_rel, w_irr = att.time_mask(attr, x)
    emb = _rt.hip_embedder()
    B = x.shape[0]
    _, _, p = emb.forward(torch.cat([x, w_rel, w_irr], 0), want_hidden=False)
    return p[:B], p[B:2 * B], p[2 * B:]


def score_explanations(model, waves, method="input_x_gradient", n_steps=50, window=1600, stride=800, nt_type=None, nt_samples=5,
                       stdevs=0.01, n_perturb_samples=10, perturb_radius=0.02, norm_ord="fro", multiply_by_inputs=False, layer=None, neuron=None):
    """Captum's two explanation metrics of ``explain_waves``'s attribution (``method``, optionally in NoiseTunnel) for a batch
    ``[B, L]``: ``{"infidelity": [B], "sensitivity_max": [B]}`` fp32.  Infidelity perturbs each clip ``n_perturb_samples``
    times with ``NoisyPerturbation(stdevs, multiply_by_inputs)`` (``x - stdevs * N(0, 1)``; ``stdevs`` in waveform units, as in
    ``explain_waves``); sensitivity_max re-runs the attribution on ``n_perturb_samples`` copies ``x + U(-perturb_radius,
    perturb_radius)`` and takes the largest relative change in ``norm_ord``."""
    _check_batch(method, waves)
    att = model.hip_attribution()
    x = waves.to(device, torch.float32)
    explain = _explainer(att, method, n_steps, window, stride, nt_type, nt_samples, stdevs, layer, neuron)
    attr = explain(x)
    return {"infidelity": infidelity(model, NoisyPerturbation(stdevs, multiply_by_inputs), x, attr,
                                     n_perturb_samples=n_perturb_samples),
            "sensitivity_max": sensitivity_max(explain, x, perturb_radius=perturb_radius, n_perturb_samples=n_perturb_samples,
                                               norm_ord=norm_ord)}


def evaluate_explanation(model, waves, attributions, domain="wave", mask=None, segment=1600, **kw):
    """Deletion / insertion curves of an attribution map for a batch ``[B, L]`` (Petsiuk et al. 2018; Samek et al. 2017; DeYoung
    et al. 2020): ``{"deletion_auc", "insertion_auc", "comprehensiveness", "sufficiency"}``, each ``[B]``
    (``HipAttribution.curve_summary``).  ``domain="wave"``: ``attributions [B, L]`` of any waveform method, features =
    ``segment``-sample segments (``arange(L) // segment``, default 100 ms).  ``domain="spectrogram"``: ``attributions
    [B, Fm, Tm]`` over the STFT mask ``mask`` (default ``ones(B, Fm, Tm)``), features = ``tf_feature_mask(Fm, Tm, band_bins,
    seg_frames)`` (keywords ``band_bins=64``, ``seg_frames=16``, ``mask_domain="linear"``); pass a mask baseline
    (``baselines=0.5``), not the zero mask.  The other keywords (``steps``, ``baselines``, ``use_abs``, ``pool``,
    ``internal_batch_size``) go to ``curve_summary``."""
    if domain not in ("wave", "spectrogram"):
        raise ValueError(f"domain must be 'wave' or 'spectrogram', not {domain!r}")
    if not torch.is_tensor(waves) or waves.dim() != 2:
        raise ValueError("waves must be a [B, L] tensor")
    if not torch.is_tensor(attributions):
        raise ValueError("attributions must be a tensor")
    if domain == "wave":
        if mask is not None:
            raise ValueError("mask belongs to domain='spectrogram'")
        if isinstance(segment, bool) or not isinstance(segment, int) or segment < 1:
            raise ValueError(f"segment must be an integer >= 1, not {segment!r}")
        return model.hip_attribution().curve_summary(waves, attributions, feature_mask=_segments(waves, segment).cpu(), **kw)
    band_bins, seg_frames, mask_domain = kw.pop("band_bins", 64), kw.pop("seg_frames", 16), kw.pop("mask_domain", "linear")
    if attributions.dim() != 3:
        raise ValueError("attributions must be [B, Fm, Tm] for domain='spectrogram'")
    Fm, Tm = attributions.shape[1], attributions.shape[2]
    ids = tf_feature_mask(Fm, Tm, band_bins, seg_frames)
    eng = MaskedSpectrogramLogReg(model, waves, mask_domain).hip_mask_attribution()
    m = torch.ones((eng.B, Fm, Tm), dtype=torch.float32, device=eng.waves.device) if mask is None else mask.to(eng.waves.device, torch.float32)
    return eng.curve_summary(m, attributions, feature_mask=ids, **kw)


ATTACKS = ("fgsm", "pgd")
PGD_DEFAULTS = dict(radius=2e-3, step_size=5e-4, step_num=5)            # waveform units: a clip lives in [-1, 1]


def attack_waves(model, waves, labels, attack="pgd", explain=None, **attack_kwargs):
    """Attack a batch ``[B, L]`` against its ``labels`` (0 / 1, an int or ``[B]``: the default loss's target) with
    ``captum.robust.FGSM`` (``attack="fgsm"``; ``epsilon``, default 1e-3) or ``PGD`` (``"pgd"``; ``radius``, ``step_size``,
    ``step_num``, default 2e-3 / 5e-4 / 5), passing ``attack_kwargs`` (``loss_func``, ``lower_bound``, ``upper_bound`` go to the
    constructor, the rest to ``perturb``).  Returns ``{"adversarial": [B, L], "predictions": [B, 1], "adversarial_predictions":
    [B, 1]}`` (both from one forward over ``cat([x, x_adv])``) and, when ``explain`` names an ``explain_waves`` method (its
    defaults, the attention rollouts and ``"transformer_lrp"`` included), ``"explanation_shift" [B]``: ``||a(x_adv) - a(x)||_2 / ||a(x)||_2`` (a zero norm counts as 1), reduced on the
    device by sensitivity_max's row-norm kernels."""
    if attack not in ATTACKS:
        raise ValueError(f"attack must be one of {ATTACKS}, not {attack!r}")
    if explain is not None:
        _check_batch(explain, waves)
    kw = dict(attack_kwargs)
    ctor = {k: kw.pop(k) for k in ("loss_func", "lower_bound", "upper_bound") if k in kw}
    x = waves.to(device, torch.float32) if torch.is_tensor(waves) else waves
    if attack == "fgsm":
        x_adv = FGSM(model, **ctor).perturb(x, kw.pop("epsilon", 1e-3), labels, **kw)
    else:
        args = [kw.pop(k, v) for k, v in PGD_DEFAULTS.items()]
        x_adv = PGD(model, **ctor).perturb(x, *args, labels, **kw)
    B = x.shape[0]
    _, _, p = _rt.hip_embedder().forward(torch.cat([x, x_adv], 0), want_hidden=False)
    out = {"predictions": p[:B], "adversarial_predictions": p[B:], "adversarial": x_adv}
    if explain is not None:
        from addvisor_hip import attribution as _A
        fn = _explainer(model.hip_attribution(), explain)
        e, et = fn(x).contiguous(), fn(x_adv).contiguous()
        shift = torch.zeros(B, dtype=torch.float32, device=e.device)
        _A.sensitivity_fold(e, et, _A.row_norm(e, 0), 1, 0, shift)          # max(0, ratio) = ratio
        out["explanation_shift"] = shift
    return out


def compute_camptum_saliency_metrics(model, metadata_path, target_class=None, root="LJSpeech_vocoded",
                                     method="input_x_gradient", batch_size=8, nt_type=None, nt_samples=5, stdevs=0.01,
                                     explanation_metrics=False):
    """captum_saliency.py:112-212 (name kept as in the reference); prints faithfulness and fidelity.  ``nt_type`` runs the
    masks of NoiseTunnel over ``method`` (``explain_waves``: any of its waveform methods, ``"attention_rollout"``,
    ``"attention_grad_rollout"`` and ``"transformer_lrp"`` included).  ``explanation_metrics=True`` also prints the means of
    Captum's infidelity and sensitivity_max of the attributions (``score_explanations``)."""
    model.eval()
    wav_paths = extract_wavs(metadata_path)
    print(f"computing saliency for {len(wav_paths)} files")
    preds, thetas, masked, infid, sens = [], [], [], [], []
    for i in range(0, len(wav_paths), batch_size):
        waves = torch.stack([audioprocessor.load_audio(os.path.join(root, p))[0] for p in wav_paths[i:i + batch_size]])
        p, t, o = explain_waves(model, waves, method, nt_type=nt_type, nt_samples=nt_samples, stdevs=stdevs)
        preds.append(p), thetas.append(t), masked.append(o)
        if explanation_metrics:
            sc = score_explanations(model, waves, method, nt_type=nt_type, nt_samples=nt_samples, stdevs=stdevs)
            infid.append(sc["infidelity"]), sens.append(sc["sensitivity_max"])
    predictions, theta_out, masked_predictions = torch.cat(preds), torch.cat(thetas), torch.cat(masked)
    m = _P.lmac_metrics(predictions, theta_out, masked_predictions)
    print(f"faithfulness : {m['faithfulness']:.2f}")
    print(f"fidelity: {m['fidelity']:.2f}")
    if explanation_metrics:
        print(f"infidelity: {torch.cat(infid).mean().item():.4g}")
        print(f"sensitivity_max: {torch.cat(sens).mean().item():.4g}")
    counter = int((theta_out[-batch_size:] >= 0.5).sum().item())
    print(f"number of relevant masks classified as manipulated: {counter} out of {min(batch_size, len(wav_paths))}")
    return None
