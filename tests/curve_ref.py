"""CPU restatement of the perturbation curves (deletion / insertion AUC of Petsiuk et al., RISE, BMVC 2018, sec. 4.1; AOPC in
MoRF / LeRF order of Samek et al. 2017; the comprehensiveness / sufficiency of DeYoung et al. 2020) for tests/test_curve_cpu.py
and tests/test_gpu_curve.py, in plain numpy / float64.  Written from the papers' definitions: there is no Captum class and no
counterpart in the reference project, so these functions ARE the definition the kernels are held to.

Notation: ``attr [B, n]``; ``index [1 | B, n]`` in ``[0, K)`` the feature of each sample (None: the identity); ``rank [B, K]`` the
position of each feature in its clip's order; ``counts [S + 1]`` the features switched at each step; rows are step-major,
``g = j * B + b``."""
import numpy as np


def _index(index, B, n):
    if index is None:
        return np.broadcast_to(np.arange(n), (B, n))
    return np.broadcast_to(np.asarray(index), (B, n))


def scores64(attr, index, K, use_abs=False, mean=False):
    """``[B, K]`` float64 sums (means) of the attributions (their magnitudes) over each feature's samples; a feature without
    samples scores -inf."""
    a = np.asarray(attr, np.float64)
    a = np.abs(a) if use_abs else a
    B, n = a.shape
    idx = _index(index, B, n)
    out = np.full((B, K), -np.inf)
    for b in range(B):
        for k in range(K):
            sel = idx[b] == k
            if sel.any():
                out[b, k] = a[b, sel].mean() if mean else a[b, sel].sum()
    return out


def scores32_replay(attr, index, K, use_abs=False, mean=False):
    """The kernel's order in float32: from 0.f, add the feature's samples one by one in increasing t; ``mean`` divides once by the
    count.  ``[B, K]`` float32, bit for bit what advh_feature_scores writes."""
    a = np.asarray(attr, np.float32)
    a = np.abs(a) if use_abs else a
    B, n = a.shape
    idx = _index(index, B, n)
    out = np.full((B, K), -np.inf, np.float32)
    for b in range(B):
        order = np.argsort(idx[b], kind="stable")                       # samples grouped by feature, increasing t inside a group
        feats = idx[b][order]
        vals = a[b][order]
        starts = np.searchsorted(feats, np.arange(K), side="left")
        ends = np.searchsorted(feats, np.arange(K), side="right")
        for k in range(K):
            if ends[k] > starts[k]:
                acc = np.float32(0.0)
                for v in vals[starts[k]:ends[k]]:
                    acc = np.float32(acc + v)
                out[b, k] = np.float32(acc / np.float32(ends[k] - starts[k])) if mean else acc
    return out


def rank_pairwise(score, descending):
    """The definition: ``rank[b, k]`` = the number of features j that come before k -- ``s_j > s_k`` (``descending``; else
    ``s_j < s_k``), or ``s_j == s_k and j < k``.  O(K^2): for small K."""
    s = np.asarray(score, np.float64)
    B, K = s.shape
    j = np.arange(K)
    out = np.empty((B, K), np.int32)
    for b in range(B):
        sj, sk = s[b][:, None], s[b][None, :]
        first = (sj > sk) if descending else (sj < sk)
        out[b] = (first | ((sj == sk) & (j[:, None] < j[None, :]))).sum(0)
    return out


def rank_argsort(score, descending):
    """The same ranks from a stable sort: ``argsort(argsort(-s or s, stable), stable)`` (``-0 == +0`` and ``+-inf`` order as
    numbers under numpy's comparison, as in the definition)."""
    s = np.asarray(score, np.float64)
    key = -s if descending else s
    return np.argsort(np.argsort(key, axis=1, kind="stable"), axis=1, kind="stable").astype(np.int32)


def counts_from_steps(steps, K):
    """The schedule: None -> ``S = min(K, 20)``; an int S in ``[1, K]`` -> ``c_j = (j K + S // 2) // S``; fractions (strictly
    increasing, 0.0 .. 1.0) -> ``floor(f K + 0.5)``.  ValueError on anything else and on colliding counts."""
    if steps is None:
        steps = min(K, 20)
    if isinstance(steps, (int, np.integer)) and not isinstance(steps, bool):
        S = int(steps)
        if not 1 <= S <= K:
            raise ValueError("steps outside [1, K]")
        return np.array([(j * K + S // 2) // S for j in range(S + 1)], np.int32)
    f = np.asarray(steps, np.float64)
    if f.ndim != 1 or f.size < 2 or f[0] != 0.0 or f[-1] != 1.0 or not (np.diff(f) > 0).all():
        raise ValueError("fractions must increase strictly from 0.0 to 1.0")
    c = np.floor(f * K + 0.5).astype(np.int64)
    if not (np.diff(c) > 0).all():
        raise ValueError("counts collide")
    return c.astype(np.int32)


def rows(x, base, index, rank, counts, mode, n_rows=None, row0=0):
    """Curve rows ``[row0, row0 + n_rows)`` (default: all ``S1 * B``), float32: sample t of row ``(j, b)`` is switched when
    ``rank[b, index[t]] < counts[j]``; deletion (``mode=0``) puts the baseline on the switched samples, insertion (``mode=1``) x.
    Rows past ``S1 * B`` copy ``x[g % B]``; a feature index outside ``[0, K)`` gives NaN."""
    x = np.asarray(x, np.float32)
    B, n = x.shape
    base = np.broadcast_to(np.asarray(base, np.float32), (B, n))
    idx = _index(index, B, n)
    rank = np.asarray(rank)
    K = rank.shape[1]
    S1 = len(counts)
    n_rows = S1 * B - row0 if n_rows is None else n_rows
    out = np.empty((n_rows, n), np.float32)
    for r in range(n_rows):
        g = row0 + r
        b = g % B
        if g >= S1 * B:
            out[r] = x[b]
            continue
        ok = (idx[b] >= 0) & (idx[b] < K)
        switched = rank[b][np.where(ok, idx[b], 0)] < counts[g // B]
        take_base = switched if mode == 0 else ~switched
        out[r] = np.where(ok, np.where(take_base, base[b], x[b]), np.float32(np.nan))
    return out


def fold(fk, counts, B, K, prob, ref_last):
    """``(curve [B, S1], auc [B], aopc [B])`` in float64 from the rows' logits ``fk [S1 * B]``: ``y = fk`` or its sigmoid,
    ``auc = sum (f_{j+1} - f_j)(y_j + y_{j+1}) / 2 / (f_last - f_0)`` with ``f = counts / K``,
    ``aopc = sum_{j != ref} (y_ref - y_j) / (S1 - 1)``."""
    S1 = len(counts)
    z = np.asarray(fk, np.float64)[:S1 * B].reshape(S1, B).T
    y = 1.0 / (1.0 + np.exp(-z)) if prob else z
    f = np.asarray(counts, np.float64) / K
    auc = ((f[1:] - f[:-1])[None] * (y[:, 1:] + y[:, :-1]) / 2).sum(1) / (f[-1] - f[0])
    ref = S1 - 1 if ref_last else 0
    aopc = (y[:, [ref]] - np.delete(y, ref, axis=1)).sum(1) / (S1 - 1)
    return y, auc, aopc


def perturbation_curve(forward, x, attr, mode="deletion", order="morf", index=None, K=None, steps=None, base=0.0, prob=True,
                       use_abs=False, mean=False, rank=None):
    """The whole metric on the host.  ``forward``: ``[rows, n] float32 -> [rows]`` logits.  The ranks come from the float32
    replay of the scores (the order the device sums in), so that ties and near-ties fall the same way; ``rank`` given
    (``order="random"``): used as is.  Returns ``(curve, fractions, auc, aopc, rank)``."""
    x = np.asarray(x, np.float32)
    B, n = x.shape
    K = n if K is None else K
    if rank is None:
        rank = rank_argsort(scores32_replay(attr, index, K, use_abs, mean), descending=order == "morf")
    counts = counts_from_steps(steps, K)
    m = 0 if mode == "deletion" else 1
    b = np.full((1, n), base, np.float32) if np.isscalar(base) else np.asarray(base, np.float32)
    fk = np.asarray(forward(rows(x, b, index, rank, counts, m)), np.float64)
    curve, auc, aopc = fold(fk, counts, B, K, prob, ref_last=m == 1)
    return curve, counts / K, auc, aopc, rank
