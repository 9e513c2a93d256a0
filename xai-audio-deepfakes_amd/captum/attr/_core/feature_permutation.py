"""``captum.attr._core.feature_permutation``'s default ``perm_func``, restated from Captum 0.7 (captum is absent)."""
import torch


def _permute_feature(x, feature_mask):
    """Captum's default ``perm_func``: the rows of ``x`` permuted by a uniform permutation that is not the identity, on the
    samples where ``feature_mask`` is set.  ``FeaturePermutation`` recognises it and builds its rows on the device instead
    (``advh_permutation_points``, permutations drawn by ``addvisor_hip.attribution.feature_permutation_draws``)."""
    n = x.size(0)
    assert n > 1, "cannot permute features with batch_size = 1"
    perm = torch.randperm(n)
    while (perm == torch.arange(n)).all():
        perm = torch.randperm(n)
    return x[perm] * feature_mask.to(dtype=x.dtype) + x * feature_mask.bitwise_not().to(dtype=x.dtype)
