"""CPU restatement of Captum's infidelity and sensitivity_max for tests/test_metrics_cpu.py and tests/test_gpu_metrics.py, written
the way Captum 0.7's ``metrics/_core/infidelity.py`` and ``metrics/_core/sensitivity.py`` loop (captum is absent):
``_divide_and_aggregate_metrics`` splits the S samples into chunks of ``max_examples_per_batch // B`` (then the remainder), each
chunk ``repeat_interleave``s the inputs (and a ``[B, L]`` baseline), calls the perturbation, and returns the chunk's aggregates
-- infidelity: the sums of ``(a - d)^2`` or of ``(a^2, a d, d^2)``, here in float64; sensitivity: the per-clip maximum of
``||e - e~|| / ||e||`` -- which ``agg_func`` (sum, max) folds across chunks; infidelity then normalises with
``beta = safe_div(sum a d, sum a^2)`` and divides by S.

The noise is the engine's: infidelity's noisy rows ``x_b - stdevs * N(seed, b * S + s, :)`` (``R.philox_normal``) and
sensitivity's default rows ``x_b + r * (2u - 1)`` from the same Philox words (``uniform`` below, float32 arithmetic).  The model
is ``oracle.attribution_ref.model_logit``; the explanations are the ``noise_tunnel_ref`` callables."""
import numpy as np
import torch

import attribution_baselines_ref as R
from oracle import attribution_ref as A


def divide_and_aggregate(bsz, n_perturb_samples, metric_func, agg_func, max_examples_per_batch=None):
    """Captum's ``_divide_and_aggregate_metrics``: ``metric_func(n)`` per chunk of n samples, folded by ``agg_func``."""
    if max_examples_per_batch is not None and max_examples_per_batch // bsz < n_perturb_samples:
        current_n_steps = max_examples_per_batch // bsz
        assert current_n_steps > 0, "`max_examples_per_batch` must be at least equal to the input batch size or greater."
        metrics_sum = metric_func(current_n_steps)
        for done in range(current_n_steps, n_perturb_samples, current_n_steps):
            metrics_sum = agg_func(metrics_sum, metric_func(min(current_n_steps, n_perturb_samples - done)))
        return metrics_sum
    return metric_func(n_perturb_samples)


def chunk_sizes(B, S, max_examples_per_batch=None):
    sizes = []
    divide_and_aggregate(B, S, lambda n: sizes.append(n) or 0, lambda a, b: 0, max_examples_per_batch)
    return sizes


def safe_div(numerator, denom, default_denom=1.0):
    if isinstance(denom, (int, float)):
        return numerator / (denom if denom != 0 else default_denom)
    return numerator / torch.where(denom != 0, denom, torch.tensor(default_denom, dtype=denom.dtype))


def uniform(seed, row0, rows, n):
    """``[rows, n]`` float32 ``2u - 1`` of the Philox words, u = (2 (w >> 9) + 1) 2^-24 (both steps exact in float32)."""
    w = R.philox_words(seed, row0, rows, n).reshape(rows, -1)[:, :n]
    u = ((w >> np.uint32(9)).astype(np.float32) * np.float32(2) + np.float32(1)) * np.float32(2.0 ** -24)
    return np.float32(2) * u - np.float32(1)


def global_rows(B, S, s0, n, fn):
    """``fn(row0, rows)`` stacked for the chunk's rows ``b * n + s'`` (global row ``b * S + s0 + s'``)."""
    return np.concatenate([fn(b * S + s0, n) for b in range(B)])


def uniform_rows(x, seed, S, s0, n, radius):
    """sensitivity_max's default rows of the chunk ``[s0, s0 + n)``: ``x_b + r * (2u - 1)`` in float32 (two roundings)."""
    B, L = x.shape
    t = global_rows(B, S, s0, n, lambda g, k: uniform(seed, g, k, L))
    xe = np.repeat(np.asarray(x, np.float32), n, 0)
    return xe + np.float32(radius) * t


def noise_rows(seed, B, S, s0, n, L, stdevs):
    """infidelity's noise ``stdevs * N(seed, b * S + s0 + s', :)`` of the chunk, float32 (the product rounded once)."""
    z = global_rows(B, S, s0, n, lambda g, k: R.philox_normal(seed, g, k, L)).astype(np.float32)
    return np.float32(stdevs) * z


class NoisyChunks:
    """A perturb_func restating NoisyPerturbation's fused rows: call k gets chunk k of ``plan`` and returns
    ``(perturbation, x - noise)``, the perturbation ``noise`` or the decorator's ``safe_div(x - x~, x - baselines)``."""

    def __init__(self, seed, B, S, stdevs, multiply_by_inputs=False, max_examples_per_batch=None):
        self.seed, self.B, self.S, self.stdevs, self.mul = seed, B, S, stdevs, multiply_by_inputs
        self.plan = chunk_sizes(B, S, max_examples_per_batch)
        self.s0 = 0

    def __call__(self, inputs, baselines=None):
        n = inputs.shape[0] // self.B
        noise = torch.from_numpy(noise_rows(self.seed, self.B, self.S, self.s0, n, inputs.shape[1], self.stdevs)).to(inputs.device)
        self.s0 += n
        xt = inputs - noise
        if not self.mul:
            return noise, xt
        den = inputs if baselines is None else inputs - baselines
        return safe_div(inputs - xt, den), xt


def fold_model(a, d, plan, normalize):
    """advh_infidelity_fold / advh_infidelity_finalize restated in numpy on
    rows ``(a, d)`` ``[B, S]`` float64 (d already the fp32 difference of the logits): fp64 sums per clip in sample order, then the finalize's expression."""
    B, S = a.shape
    acc = np.zeros((B, 3))
    for s0, pp in plan:
        for b in range(B):
            for s in range(s0, s0 + pp):
                if normalize:
                    acc[b] += (a[b, s] * a[b, s], a[b, s] * d[b, s], d[b, s] * d[b, s])
                else:
                    acc[b, 0] += (a[b, s] - d[b, s]) * (a[b, s] - d[b, s])
    if not normalize:
        return (acc[:, 0] / S).astype(np.float32)
    A, AD, D = acc.T
    beta = AD / np.where(A != 0, A, 1.0)
    return ((((beta * beta) * A - (2 * beta) * AD) + D) / S).astype(np.float32)


def model_forward(model, rows_per_call=8):
    return lambda w: torch.cat([A.model_logit(w[i:i + rows_per_call], *model).view(-1) for i in range(0, w.shape[0], rows_per_call)])


def infidelity(forward, perturb_func, inputs, attributions, baselines=None, n_perturb_samples=10, max_examples_per_batch=None,
               normalize=False, record=None):
    """Captum's infidelity loop on the CPU (one input tensor, no target); sums in float64.  Returns ``[B]`` float64; ``record``
    (a dict) receives the per-row ``a`` and ``d`` (``[B, S]`` float64) and the chunk's ``|perturbation| . |attr|`` sums."""
    bsz = inputs.shape[0]
    with torch.no_grad():
        f_inputs = forward(inputs).double()

    def next_infidelity_tensors(n):
        inputs_expanded = inputs.repeat_interleave(n, 0)
        baselines_expanded = baselines
        if torch.is_tensor(baselines) and baselines.shape[0] == inputs.shape[0] and baselines.shape[0] > 1:
            baselines_expanded = baselines.repeat_interleave(n, 0)
        pert, inputs_perturbed = (perturb_func(inputs_expanded, baselines_expanded) if baselines_expanded is not None
                                  else perturb_func(inputs_expanded))
        with torch.no_grad():
            d = (f_inputs.repeat_interleave(n, 0) - forward(inputs_perturbed).double()).view(bsz, -1)
        prod = attributions.double().repeat_interleave(n, 0) * pert.double()
        a = prod.sum(1).view(bsz, -1)
        if record is not None:
            for k, v in (("a", a), ("d", d), ("abs", prod.abs().sum(1).view(bsz, -1))):
                record[k] = torch.cat([record[k], v], 1) if k in record else v
        if normalize:
            return (a.pow(2).sum(-1), (a * d).sum(-1), d.pow(2).sum(-1))
        return ((a - d).pow(2).sum(-1),)

    agg = divide_and_aggregate(bsz, n_perturb_samples, next_infidelity_tensors, lambda x, y: tuple(p + q for p, q in zip(x, y)),
                               max_examples_per_batch)
    if normalize:
        beta = safe_div(agg[1], agg[0])
        values = beta ** 2 * agg[0] - 2 * beta * agg[1] + agg[2]
    else:
        values = agg[0]
    return values / n_perturb_samples


def _norm(v, norm_ord):
    """Row norms ``[R]``; a tuple of orders gives ``[len, R]``."""
    if isinstance(norm_ord, tuple):
        return torch.stack([_norm(v, o) for o in norm_ord])
    return torch.linalg.vector_norm(v, ord=2 if norm_ord == "fro" else norm_ord, dim=1)


def sensitivity_max(explanation_func, inputs, perturb_func, n_perturb_samples=10, norm_ord="fro", max_examples_per_batch=None,
                    **kwargs):
    """Captum's sensitivity_max loop on the CPU: ``perturb_func(inputs_expanded, s0)`` returns the chunk's perturbed rows (the
    restatement passes the chunk's first sample so that the rows can follow the engine's counters).  Norms in float64; a tuple
    ``norm_ord`` returns ``[len, B]``, one row per order, from the same explanations."""
    bsz = inputs.shape[0]
    with torch.no_grad():
        expl = explanation_func(inputs, **kwargs).double()
    enorm = _norm(expl, norm_ord)
    enorm = torch.where(enorm == 0.0, torch.ones_like(enorm), enorm)
    s0 = [0]

    def next_sensitivity_max(n):
        kw = dict(kwargs)
        b = kw.get("baselines")
        if torch.is_tensor(b) and b.shape == inputs.shape and b.shape[0] > 1:
            kw["baselines"] = b.repeat_interleave(n, 0)
        rows = perturb_func(inputs.repeat_interleave(n, 0), s0[0])
        s0[0] += n
        with torch.no_grad():
            et = explanation_func(rows, **kw).double()
        sens = _norm(expl.repeat_interleave(n, 0) - et, norm_ord) / enorm.repeat_interleave(n, -1)
        return sens.view(*sens.shape[:-1], bsz, -1).max(-1).values

    return divide_and_aggregate(bsz, n_perturb_samples, next_sensitivity_max, torch.max, max_examples_per_batch)


def default_rows(seed, B, S, radius):
    """``perturb_func(inputs_expanded, s0)`` of ``sensitivity_max`` above: the engine's default rows."""
    return lambda xe, s0: torch.from_numpy(uniform_rows(xe[::xe.shape[0] // B].numpy(), seed, S, s0, xe.shape[0] // B, radius))
