"""``captum.attr._core.lime``'s helpers, restated from Captum 0.7 (captum is absent): the default similarity kernel and the
default interpretable sampler of ``captum.attr.Lime``."""
import torch

from addvisor_hip.attribution import ExpKernelSimilarity


def get_exp_kernel_similarity_function(distance_mode="cosine", kernel_width=1.0):
    """Captum's exponential kernel ``exp(-d^2 / (2 kernel_width^2))`` between the original and the perturbed input, ``d = 1 -
    cos`` (``distance_mode="cosine"``) or the Euclidean distance (``"euclidean"``).  Returns an ``ExpKernelSimilarity``, which
    Lime evaluates on the device; called directly it computes Captum's formula in torch.  A mode other than the two, or a
    kernel_width that is not a finite number > 0, raises ValueError here (Captum raises on the mode at the first call)."""
    return ExpKernelSimilarity(distance_mode, kernel_width)


def default_perturb_func(original_inp, **kwargs):
    """Captum's default sampler: a ``[1, num_interp_features]`` long tensor of Bernoulli(0.5) draws from torch's generator.  Lime
    recognises it and draws the same law on the host instead (``addvisor_hip.attribution.lime_draws``, one seed per call)."""
    assert "num_interp_features" in kwargs, "Must provide num_interp_features to use default interpretable sampling function"
    device = original_inp.device if torch.is_tensor(original_inp) else original_inp[0].device
    probs = torch.ones(1, kwargs["num_interp_features"]) * 0.5
    return torch.bernoulli(probs).to(device=device).long()
