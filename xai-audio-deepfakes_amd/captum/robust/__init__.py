"""``captum.robust``-compatible front ends over the HIP gradient chain: ``FGSM`` (Goodfellow et al., ICLR 2015) and ``PGD``
(Madry et al., ICLR 2018), restated from Captum 0.7's ``robust/_core/fgsm.py`` and ``robust/_core/pgd.py`` -- captum is absent,
so the classes are unpinned, like the attribution front ends: signatures, defaults and the arithmetic of ``_perturb``, ``_clip``,
``_random_point`` and ``bound`` follow the published source, and tests/robust_ref.py restates them in torch.

``forward_func`` must be a ``captum_saliency.Wav2vec2LogReg`` (or anything exposing ``.hip_robust()``); anything else raises
TypeError -- there is no autograd fallback.  The classifier returns one logit, so the default loss (``loss_func=None``) is binary
cross-entropy with logits against ``target`` (0, 1 or a ``[B]`` tensor of them) in place of Captum's ``-log(outputs)[target]``,
which presumes a probability vector (``HipRobust.loss_seed``); a callable ``loss_func(outputs [B, 1], target)`` is differentiated
over the logit alone.  ``additional_forward_args`` other than None raises NotImplementedError.  PGD's random start follows
``torch``'s default CPU generator through one seed per call (``torch.manual_seed`` reproduces a result); Captum's own RNG stream
is not reproduced.  ``MinParamPerturbation`` and ``AttackComparator`` are out of scope; ``HipRobust.fgsm_min_epsilon`` answers
the minimal-perturbation question at the engine level."""
from addvisor_hip import robust as _R

__all__ = ["FGSM", "PGD"]


def _check_model(forward_func, additional_forward_args):
    if hasattr(forward_func, "hip_mask_attribution"):
        raise NotImplementedError("attacks over STFT masks are not implemented (HipSpectralAttribution)")
    if not hasattr(forward_func, "hip_robust"):
        raise TypeError("captum.robust (HIP build) only attacks captum_saliency.Wav2vec2LogReg models")
    if additional_forward_args is not None:
        raise NotImplementedError("the classifier takes no additional forward arguments; additional_forward_args must be None")


class FGSM:
    """Captum's Fast Gradient Sign Method: ``x' = clamp(x + epsilon * sign(dL/dx) * mask, lower_bound, upper_bound)`` where
    ``|dL/dx| > zero_thresh`` (untargeted: ascend the loss of ``target``; ``targeted=True``: descend it)."""

    def __init__(self, forward_func, loss_func=None, lower_bound=float("-inf"), upper_bound=float("inf")):
        self.forward_func = forward_func
        self.loss_func = loss_func
        self.lower_bound, self.upper_bound = lower_bound, upper_bound
        self.bound = lambda x: x.clamp(min=lower_bound, max=upper_bound)
        self.zero_thresh = 10 ** -6                       # a constant of advh_robust_step: changing it here changes nothing

    def perturb(self, inputs, epsilon, target, additional_forward_args=None, targeted=False, mask=None):
        _check_model(self.forward_func, additional_forward_args)
        _R.check_fgsm_args(inputs, epsilon, target, self.loss_func, mask, self.lower_bound, self.upper_bound)   # before the engine
        eng = self.forward_func.hip_robust()
        return eng.fgsm(inputs, epsilon, target, loss_func=self.loss_func, targeted=targeted, mask=mask,
                        lower_bound=self.lower_bound, upper_bound=self.upper_bound)


class PGD:
    """Captum's Projected Gradient Descent: ``step_num`` FGSM steps of ``step_size``, each projected onto the ``norm`` ball
    ("Linf" or "L2") of ``radius`` around ``inputs`` and clamped to the bounds, from ``inputs`` or (``random_start``) a random
    point of the ball."""

    def __init__(self, forward_func, loss_func=None, lower_bound=float("-inf"), upper_bound=float("inf")):
        self.forward_func = forward_func
        self.fgsm = FGSM(forward_func, loss_func)
        self.loss_func = loss_func
        self.lower_bound, self.upper_bound = lower_bound, upper_bound
        self.bound = lambda x: x.clamp(min=lower_bound, max=upper_bound)

    def perturb(self, inputs, radius, step_size, step_num, target, additional_forward_args=None, targeted=False,
                random_start=False, norm="Linf", mask=None):
        _check_model(self.forward_func, additional_forward_args)
        _R.check_pgd_args(inputs, radius, step_size, step_num, target, self.loss_func, norm, mask, self.lower_bound,
                          self.upper_bound)                                                                      # before the engine
        eng = self.forward_func.hip_robust()
        return eng.pgd(inputs, radius, step_size, step_num, target, loss_func=self.loss_func, targeted=targeted,
                       random_start=random_start, norm=norm, mask=mask, lower_bound=self.lower_bound,
                       upper_bound=self.upper_bound)
