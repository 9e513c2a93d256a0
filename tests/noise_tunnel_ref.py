"""CPU restatement of Captum's NoiseTunnel for tests/test_noise_tunnel_cpu.py and tests/test_gpu_noise_tunnel.py, written the way
Captum 0.7's ``noise_tunnel.py`` loops (captum is absent): ``nt_samples // nt_samples_batch_size`` partitions of the batch size,
then one of the remainder; per partition the inputs ``repeat_interleave``d and noised, the keyword arguments expanded
(``baselines`` of the batch's first dimension > 1 ``repeat_interleave``d, or drawn per noisy row from the distribution;
``feature_mask`` with first dimension > 1 ``repeat_interleave``d), the wrapped method called, and the attributions summed per
sample -- here in float64, in sample order -- into the first and second moments; ``smoothgrad`` E[a], ``smoothgrad_sq`` E[a^2],
``vargrad`` E[a^2] - E[a]^2.

The noise is the engine's: row (b, s) is ``x_b + stdevs * N(seed, b * S + s, :)``, ``N`` from ``R.philox_normal`` (numpy
Philox4x32-10 / Box-Muller), and drawn baselines take ``integers(0, N_b, B * S)`` of ``numpy.random.Generator(PCG64(seed))``.
The wrapped methods are callables ``rows [R, L] -> attr [R, L]`` (or ``(attr, delta)``), built below on the existing
restatements: ``oracle.attribution_ref.input_gradient`` (Saliency, InputXGradient), ``attribution_baselines_ref``
(IntegratedGradients, GradientShap), ``ablation_ref`` (Occlusion, FeatureAblation) and ``shapley_ref`` (ShapleyValues)."""
import numpy as np
import torch

import ablation_ref
import attribution_baselines_ref as R
import shapley_ref
from oracle import attribution_ref as A


def partitions(nt_samples, nt_samples_batch_size=None):
    """Captum's loop, literally: the sizes of the partitions, in order."""
    batch = nt_samples if nt_samples_batch_size is None else min(nt_samples, nt_samples_batch_size)
    sizes = [batch] * (nt_samples // batch)
    if nt_samples % batch > 0:
        sizes.append(nt_samples % batch)
    return sizes


def noise(seed, B, S, L):
    """``[B, S, L]`` float32: the clip-b block is ``R.philox_normal(seed, b * S, S, L)``."""
    return torch.from_numpy(np.stack([R.philox_normal(seed, b * S, S, L) for b in range(B)]).astype(np.float32))


def baseline_draws(seed, B, S, n_base):
    return np.random.Generator(np.random.PCG64(int(seed))).integers(0, n_base, B * S)


def expand_kwargs(kwargs, B, n, drawn=None):
    """Captum's ``expand_partial`` for one partition of n samples (``drawn``: the partition's baseline rows of the distribution)."""
    kw = dict(kwargs)
    if "baselines" in kw:
        b = kw["baselines"]
        if drawn is not None:
            kw["baselines"] = b[torch.as_tensor(drawn, dtype=torch.long)]
        elif isinstance(b, torch.Tensor) and b.shape[0] == B and b.shape[0] > 1:
            kw["baselines"] = b.repeat_interleave(n, dim=0)
    if kw.get("feature_mask") is not None and kw["feature_mask"].shape[0] > 1:
        kw["feature_mask"] = kw["feature_mask"].repeat_interleave(n, dim=0)
    return kw


def noise_tunnel(x, attribute, nt_type="smoothgrad", nt_samples=5, nt_samples_batch_size=None, stdevs=1.0, seed=0,
                 draw_baseline_from_distrib=False, return_convergence_delta=False, z=None, **kwargs):
    """NoiseTunnel of ``x [B, L]`` (fp32, CPU) around ``attribute``.  Returns ``attr [B, L]`` fp32 (``nt_type="all"``: the
    three modes ``(smoothgrad, smoothgrad_sq, vargrad)`` of one loop) and, with ``return_convergence_delta``, the wrapped
    deltas concatenated over partitions.  ``z``: the ``[B, S, L]`` noise, if not ``noise(seed, ...)``."""
    B, L = x.shape
    S = nt_samples
    z = noise(seed, B, S, L) if z is None else z
    idx = baseline_draws(seed, B, S, kwargs["baselines"].shape[0]) if draw_baseline_from_distrib else None
    s1 = torch.zeros(B, L, dtype=torch.float64)
    s2 = torch.zeros(B, L, dtype=torch.float64)
    deltas = []
    s0 = 0
    for n in partitions(S, nt_samples_batch_size):
        rows = (x[:, None] + stdevs * z[:, s0:s0 + n]).reshape(B * n, L)
        drawn = None if idx is None else idx.reshape(B, S)[:, s0:s0 + n].reshape(-1)
        kw = expand_kwargs(kwargs, B, n, drawn)
        res = attribute(rows, **kw, return_convergence_delta=True) if return_convergence_delta else attribute(rows, **kw)
        if return_convergence_delta:
            res, d = res
            deltas.append(torch.as_tensor(d))
        a = res.double().view(B, n, L)
        for s in range(n):
            s1 += a[:, s]
            s2 += a[:, s] * a[:, s]
        s0 += n
    m, m2 = s1 / S, s2 / S
    outs = {"smoothgrad": m, "smoothgrad_sq": m2, "vargrad": m2 - m * m}
    out = tuple(outs[k].float() for k in ("smoothgrad", "smoothgrad_sq", "vargrad")) if nt_type == "all" else outs[nt_type].float()
    return (out, torch.cat(deltas)) if return_convergence_delta else out


# ---- the wrapped methods as ``rows -> attr`` callables of the CPU restatements (model = (emb_sd, cfg, coef, icpt))

def saliency(model, rows_per_call=8):
    return lambda w: torch.cat([A.input_gradient(w[i:i + rows_per_call], *model) for i in range(0, w.shape[0], rows_per_call)]).abs()


def input_x_gradient(model, rows_per_call=8):
    return lambda w: w * torch.cat([A.input_gradient(w[i:i + rows_per_call], *model) for i in range(0, w.shape[0], rows_per_call)])


def integrated_gradients(model, n_steps, method="gausslegendre", internal_batch=8):
    """``(rows, baselines, return_convergence_delta=False)``; a number baseline is a ``[1, L]`` constant."""
    def ig(w, baselines=None, return_convergence_delta=False, **_):
        b = torch.full((1, w.shape[1]), float(baselines or 0.0)) if not torch.is_tensor(baselines) else baselines.cpu()
        attr, delta = R.integrated_gradients(w, b, model, n_steps, method, internal_batch=internal_batch)
        return (attr, delta) if return_convergence_delta else attr
    return ig


def gradient_shap(model, n_samples, stdevs, seed):
    """GradientShap with the engine's draws of ``seed`` (``shap_draws``, Philox noise) for each call's rows."""
    from addvisor_hip.attribution import shap_draws

    def gs(w, baselines, **_):
        Bn, L = w.shape
        idx, alpha = shap_draws(seed, Bn, n_samples, baselines.shape[0])
        z = torch.from_numpy(R.philox_normal(seed, 0, Bn * n_samples, L).astype(np.float32))
        return R.gradient_shap(w, baselines.cpu(), idx, alpha, z, stdevs, n_samples, model)[0]
    return gs


def occlusion(model, win, stride):
    fwd = ablation_ref.model_forward(model)
    return lambda w, baselines=None, **_: ablation_ref.occlusion(w, 0.0 if baselines is None else baselines.cpu(), win, stride,
                                                                 forward=fwd)[0]


def feature_ablation(model):
    fwd = ablation_ref.model_forward(model)
    return lambda w, baselines=None, feature_mask=None, **_: ablation_ref.feature_ablation(
        w, 0.0 if baselines is None else baselines.cpu(), None if feature_mask is None else feature_mask.cpu(), forward=fwd)[0]


def shapley_values(model):
    """ShapleyValues over a feature mask of contiguous ids ``0 .. K-1`` (the engine's ranks are then the ids)."""
    fwd = ablation_ref.model_forward(model)

    def sv(w, baselines=None, feature_mask=None, **_):
        index = feature_mask.cpu()
        K = int(index.max()) + 1
        return shapley_ref.shapley(w, 0.0 if baselines is None else baselines.cpu(), index, shapley_ref.all_permutations(K),
                                   forward=fwd)
    return sv
