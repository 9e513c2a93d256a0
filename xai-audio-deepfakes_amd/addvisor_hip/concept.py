"""Concept attributions (TCAV, Kim et al. 2018; Captum 0.7's ``captum.concept``, restated: captum is absent) on the HIP chain.

A concept is a set of clips; a concept activation vector (CAV) is the normal of a linear classifier that separates the
activations ``hidden_states[l]`` of one concept's clips from another's; the TCAV score of an input is the directional derivative
``<dF/dh_l, w>`` of the logit along it.  A concept example is a flattened ``[T * H]`` activation (152 832 floats at wav2vec2-base,
4 s) and there are ``N << F`` of them, so the fit runs in the dual: only the ``N x N`` Gram matrix (``advh_concept_gram``, fp64
out) crosses to the host, the solve is float64 numpy on it, and the CAV ``w = X^T a`` is built on the device
(``advh_concept_combine``).  The scores of every experimental set are one more ``advh_concept_gram`` launch, gradients against
CAVs.  Activations never leave the device (except for a user-supplied classifier, the slow path).

What is Captum's and what is not:

- ``compute_cavs`` / ``interpret`` follow ``captum.concept.TCAV``: the key of an experimental set is ``concepts_to_str``
  (``"0-1"``), two concepts give the weight rows ``[-w, w]`` of ``DefaultClassifier``, ``sign_count = mean_b(score > 0)``, and
  ``magnitude="mean"`` is Captum 0.7's ``mean_b(score)``; ``magnitude="normalized"`` is the earlier Captum form
  ``sum|s * [s > 0]| / sum|s|``.  Parity with Captum is unpinned: the formulas are restated from its source.
- The default classifier is NOT Captum's: see ``LogisticCAV``.
- The train / test split is a seeded numpy permutation, not ``torch.randperm``.
"""
from __future__ import annotations

import math
import os
import warnings
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .attribution import HipAttribution, _positive_int
from .embedder_grad import check_layer


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- the three kernels
def _rows(t: torch.Tensor, what: str) -> Tuple[int, int, int]:
    """``(rows, F, row stride)`` of a CUDA fp32 matrix whose rows are contiguous."""
    if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f"{what} must be a CUDA fp32 matrix [rows, F]")
    if t.shape[0] < 1 or t.shape[1] < 1 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{what} must have contiguous rows and a row stride >= F (shape {list(t.shape)}, strides {list(t.stride())})")
    return t.shape[0], t.shape[1], (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def gram_workspace(M: int, N: int, F: int) -> int:
    """Bytes of the partial buffer of ``gram`` (``advh_concept_gram_workspace``)."""
    n = _lib.lib().advh_concept_gram_workspace(M, N, F)
    if n < 0:
        raise _lib.AdvhError(f"advh_concept_gram_workspace({M}, {N}, {F}): {_lib.ERRORS.get(n, n)}")
    return n


def gram(X: torch.Tensor, Y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``G[i][j] = sum_f X[i, f] * Y[j, f]`` as a float64 ``[M, N]`` device tensor; ``Y=None``: the symmetric ``X X^T``."""
    M, F, ldx = _rows(X, "X")
    sym = Y is None
    N, Fy, ldy = (M, F, ldx) if sym else _rows(Y, "Y")
    if Fy != F:
        raise ValueError(f"X has {F} features, Y has {Fy}")
    ws = torch.empty(gram_workspace(M, N, F) // 4, dtype=torch.float32, device=X.device)
    G = torch.empty((M, N), dtype=torch.float64, device=X.device)
    _lib.check(_lib.lib().advh_concept_gram(X.data_ptr(), ldx, (X if sym else Y).data_ptr(), ldy, M, N, F, int(sym), ws.data_ptr(),
                                            G.data_ptr(), _st()), "advh_concept_gram")
    return G


def combine(A: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """``W[c, f] = sum_i A[c, i] * X[i, f]``, ``[C, F]`` fp32: one fmaf chain per output, ``i`` ascending."""
    N, F, ldx = _rows(X, "X")
    if not torch.is_tensor(A) or A.dim() != 2 or A.dtype != torch.float32 or not A.is_cuda or A.shape[1] != N or A.shape[0] < 1:
        raise ValueError(f"A must be a CUDA fp32 matrix [C, {N}]")
    A = A.contiguous()
    W = torch.empty((A.shape[0], F), dtype=torch.float32, device=X.device)
    _lib.check(_lib.lib().advh_concept_combine(A.data_ptr(), X.data_ptr(), ldx, A.shape[0], N, F, W.data_ptr(), F, _st()),
               "advh_concept_combine")
    return W


def time_pool(X: torch.Tensor, mean: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``[R, T, H] -> [R, H]``: the sum over ``t`` (ascending, fp32), times ``float(1 / T)`` with ``mean=True``."""
    if not torch.is_tensor(X) or X.dim() != 3 or X.dtype != torch.float32 or not X.is_cuda or X.numel() == 0:
        raise ValueError("X must be a non-empty CUDA fp32 tensor [R, T, H]")
    X = X.contiguous()
    R, T, H = X.shape
    if out is None:
        out = torch.empty((R, H), dtype=torch.float32, device=X.device)
    elif tuple(out.shape) != (R, H) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous fp32 [{R}, {H}] tensor")
    _lib.check(_lib.lib().advh_concept_time_pool(X.data_ptr(), R, T, H, int(bool(mean)), out.data_ptr(), _st()), "advh_concept_time_pool")
    return out


# ---------------------------------------------------------------------------------------------- host solves on the Gram matrix
def _sig_neg(z: np.ndarray) -> np.ndarray:
    """``sigma(-z) = 1 / (1 + e^z)`` without overflow."""
    return np.exp(-np.logaddexp(0.0, z))


def logistic_dual(K, y, alpha: float, tol: float = 1e-12, max_iter: int = 100) -> Tuple[np.ndarray, float, int]:
    """The minimiser of ``(1/n) sum_i log(1 + exp(-y_i (w . x_i + b))) + (alpha / 2) ||w||^2`` (``b`` free) from the Gram matrix
    ``K = X X^T`` alone: ``w = X^T a``.  Returns ``(a [n], b, iterations)``.

    With ``m = K a + b`` and ``s_i = sigma(-y_i m_i)`` the minimiser satisfies ``alpha a = y * s / n`` and ``sum_i y_i s_i = 0``
    (multiply the first by ``X^T``: the primal gradient).  Newton on that system of ``n + 1`` equations is Newton on the primal
    objective restricted to the span of the rows, so its step is a descent direction of the (strictly convex in ``w``) objective
    and is damped by backtracking on it.  Stops when the largest update of ``(a, b)`` is ``<= tol``; warns at ``max_iter``."""
    K = np.asarray(K, np.float64)
    y = np.asarray(y, np.float64).reshape(-1)
    n = y.shape[0]
    if K.shape != (n, n) or n < 2:
        raise ValueError(f"K must be [n, n] with n = len(y) >= 2; got {K.shape} and {n}")
    if not (np.abs(y) == 1).all() or (y == 1).all() or (y == -1).all():
        raise ValueError("the labels must be +-1 with both classes present")
    if not (isinstance(alpha, (int, float)) and not isinstance(alpha, bool) and math.isfinite(alpha) and alpha > 0):
        raise ValueError(f"alpha must be a finite number > 0, not {alpha!r}")
    if not np.isfinite(K).all():
        raise FloatingPointError("the Gram matrix is not finite")

    def objective(a, b):
        m = K @ a + b
        return np.logaddexp(0.0, -y * m).mean() + 0.5 * alpha * float(a @ (K @ a)), m

    a, b = np.zeros(n), 0.0
    J, m = objective(a, b)
    for it in range(1, max_iter + 1):
        s = _sig_neg(y * m)
        D = s * (1.0 - s)
        Fa = alpha * a - y * s / n
        Fb = float(y @ s)
        Jm = np.empty((n + 1, n + 1))
        Jm[:n, :n] = (D[:, None] * K) / n
        Jm[:n, :n][np.diag_indices(n)] += alpha
        Jm[:n, n] = D / n
        Jm[n, :n] = -(D @ K)
        Jm[n, n] = -D.sum()
        rhs = -np.concatenate([Fa, [Fb]])
        try:
            step = np.linalg.solve(Jm, rhs)
        except np.linalg.LinAlgError:
            step = np.linalg.lstsq(Jm, rhs, rcond=None)[0]
        t = 1.0
        while True:
            J2, m2 = objective(a + t * step[:n], b + t * step[n])
            if J2 <= J + 1e-13 * abs(J) or t < 1e-6:
                break
            t *= 0.5
        a, b, J, m = a + t * step[:n], b + t * step[n], J2, m2
        if t == 1.0 and np.abs(step).max() <= tol:
            return a, float(b), it
    warnings.warn(f"the logistic CAV solve did not converge in {max_iter} Newton iterations (last update {np.abs(step).max():.3e}); "
                  "the last iterate is kept", UserWarning)
    return a, float(b), max_iter


class LogisticCAV:
    """The default concept classifier: the CONVERGED minimiser of the L2-regularised logistic loss
    ``(1/n) sum_i log(1 + exp(-y_i (w . x_i + b))) + (alpha / 2) ||w||^2`` (``b`` unpenalised), solved in the dual by damped
    Newton in float64 on the Gram matrix (``logistic_dual``); more than two concepts: one-vs-rest.

    This deliberately replaces Captum's ``DefaultClassifier``, ``SGDClassifier(alpha=0.01, max_iter=1000, tol=1e-3)`` with the
    hinge loss: that iterate depends on the shuffling of a stochastic solver stopped early and cannot be a parity target.  It is
    the stance ``linear_model.SkLearnLasso`` takes for Lime.  ``alpha`` keeps SGDClassifier's meaning and default."""

    def __init__(self, alpha: float = 0.01):
        if not (isinstance(alpha, (int, float)) and not isinstance(alpha, bool) and math.isfinite(alpha) and alpha > 0):
            raise ValueError(f"alpha must be a finite number > 0, not {alpha!r}")
        self.alpha = float(alpha)

    def settings(self) -> str:
        return f"logistic(alpha={self.alpha!r})"

    def dual(self, K: np.ndarray, y: np.ndarray) -> Tuple[np.ndarray, float]:
        a, b, _ = logistic_dual(K, y, self.alpha)
        return a, b


class MeanDifferenceCAV:
    """``w = mean(X_+) - mean(X_-)`` (the CAV of Martin & Weller-style mean differences), as dual coefficients ``+-1 / n_class``
    so that the same combine kernel builds it; ``b = -w . (mean_+ + mean_-) / 2`` puts the boundary midway."""

    def settings(self) -> str:
        return "mean_difference"

    def dual(self, K: np.ndarray, y: np.ndarray) -> Tuple[np.ndarray, float]:
        y = np.asarray(y, np.float64)
        pos, neg = y > 0, y < 0
        a = np.where(pos, 1.0 / pos.sum(), -1.0 / neg.sum())
        m = np.asarray(K, np.float64) @ a                                    # w . x_i
        return a, float(-0.5 * (m[pos].mean() + m[neg].mean()))


def split_rows(n: int, ratio: float, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(train, test)`` row indices: a seeded numpy permutation whose first ``int(ratio * n)`` rows are the test set."""
    perm = np.random.default_rng(seed).permutation(n)
    k = int(ratio * n)
    return perm[k:], perm[:k]


def fit_duals(classifier, K: np.ndarray, labels: np.ndarray, n_classes: int, train: np.ndarray, test: np.ndarray):
    """Fit on the Gram matrix ``K [n, n]`` of all rows: ``(A [C, n] dual coefficients, zero outside the training rows;
    b [C]; accuracy)``.  Two classes: one fit for class 1 and rows ``[-a, a]``; more: one-vs-rest.  The accuracy is measured on
    the test rows through the cross-Gram ``K[test][:, train]``, on the training rows if the test set is empty."""
    n = labels.shape[0]
    for c in range(n_classes):
        if not (labels[train] == c).any():
            raise ValueError(f"class {c} has no example in the training part of the split ({len(train)} of {n} rows): "
                             "lower test_split_ratio or add examples")
    Kt = K[np.ix_(train, train)]
    A, b = np.zeros((n_classes, n)), np.zeros(n_classes)
    if n_classes == 2:
        a, b1 = classifier.dual(Kt, np.where(labels[train] == 1, 1.0, -1.0))
        A[1, train], b[1] = a, b1
        A[0], b[0] = -A[1], -b1
    else:
        for c in range(n_classes):
            a, bc = classifier.dual(Kt, np.where(labels[train] == c, 1.0, -1.0))
            A[c, train], b[c] = a, bc
    ev = test if len(test) else train
    margins = K[np.ix_(ev, train)] @ A[:, train].T + b                       # [n_eval, C]
    pred = (margins[:, 1] > 0).astype(np.int64) if n_classes == 2 else margins.argmax(1)
    return A, b, float((pred == labels[ev]).mean())


def tcav_scores(scores: np.ndarray, magnitude: str = "mean") -> Tuple[np.ndarray, np.ndarray]:
    """``(sign_count [C], magnitude [C])`` of directional derivatives ``scores [B, C]`` (module docstring)."""
    s = np.asarray(scores, np.float64)
    sign = (s > 0).mean(0)
    if magnitude == "mean":
        return sign, s.mean(0)
    if magnitude == "normalized":
        return sign, np.abs(s * (s > 0)).sum(0) / np.abs(s).sum(0)
    raise ValueError(f"magnitude must be 'mean' or 'normalized', not {magnitude!r}")


def _student_t_sf2(t: float, df: float) -> float:
    """Two-sided tail ``P(|T_df| > |t|)`` through the regularised incomplete beta function (continued fraction, Lentz)."""
    x = df / (df + t * t)
    a, b = 0.5 * df, 0.5
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0

    def cf(a, b, x):
        tiny = 1e-300
        c, d = 1.0, 1.0 - (a + b) * x / (a + 1.0)
        d = 1.0 / (d if abs(d) > tiny else tiny)
        h = d
        for m in range(1, 500):
            for num in (m * (b - m) * x / ((a + 2 * m - 1) * (a + 2 * m)), -(a + m) * (a + b + m) * x / ((a + 2 * m) * (a + 2 * m + 1))):
                d = 1.0 + num * d
                d = 1.0 / (d if abs(d) > tiny else tiny)
                c = 1.0 + num / c
                c = c if abs(c) > tiny else tiny
                h *= d * c
            if abs(d * c - 1.0) < 1e-16:
                break
        return h

    lbeta = math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)
    front = math.exp(a * math.log(x) + b * math.log1p(-x) - lbeta)
    if x < (a + 1.0) / (a + b + 2.0):
        return min(1.0, front * cf(a, b, x) / a)
    return max(0.0, 1.0 - front * cf(b, a, 1.0 - x) / b)


def tcav_significance(concept_scores, random_scores) -> Tuple[float, float]:
    """Welch's two-sided t-test ``(t, p)`` (Kim et al. 2018, section 3.5): a concept's TCAV scores over several random
    counterparts against the scores of random-vs-random sets.  Host code, float64."""
    x, z = np.asarray(concept_scores, np.float64).reshape(-1), np.asarray(random_scores, np.float64).reshape(-1)
    if x.size < 2 or z.size < 2:
        raise ValueError("each sample needs at least two scores")
    vx, vz = x.var(ddof=1) / x.size, z.var(ddof=1) / z.size
    if vx + vz == 0.0:
        d = x.mean() - z.mean()
        return (float("nan"), float("nan")) if d == 0 else (math.copysign(math.inf, d), 0.0)
    t = (x.mean() - z.mean()) / math.sqrt(vx + vz)
    df = (vx + vz) ** 2 / (vx * vx / (x.size - 1) + vz * vz / (z.size - 1))
    return float(t), float(_student_t_sf2(t, df))


# ---------------------------------------------------------------------------------------------- the engine
class Concept:
    """``Concept(id, name, data)`` as in Captum: ``data`` is a ``[N, L]`` waveform tensor or an iterable of ``[n, L]`` batches
    (Captum's ``data_iter``)."""

    def __init__(self, id: int, name: str, data):
        if isinstance(id, bool) or not isinstance(id, int):
            raise ValueError(f"a concept id must be an int, not {id!r}")
        self.id, self.name, self.data = id, str(name), data
        self.data_iter = data                                                # Captum's attribute name

    @property
    def identifier(self) -> str:
        return f"{self.name}-{self.id}"

    def batches(self) -> Iterable[torch.Tensor]:
        d = self.data_iter
        for t in ([d] if torch.is_tensor(d) else d):
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] < 1 or not t.is_floating_point():
                raise ValueError(f"concept {self.identifier}: the data must be floating-point [n, L] waveform batches")
            yield t


def concepts_to_str(concepts: Sequence[Concept]) -> str:
    return "-".join(str(c.id) for c in concepts)


class CAV(NamedTuple):
    """``weights [C, F]`` device fp32 (row ``c`` is the CAV of concept ``classes[c]``), ``intercepts [C]``, ``classes`` (the
    concept ids) and ``accs`` (the accuracy on the held-out rows)."""
    weights: torch.Tensor
    classes: List[int]
    accs: float
    intercepts: np.ndarray


class Classifier:
    """Captum's ``captum.concept.Classifier`` protocol, for user classifiers (the slow path: they are handed a DataLoader over
    HOST copies of the activations)."""

    def train_and_eval(self, dataloader, **kwargs):
        raise NotImplementedError

    def weights(self) -> torch.Tensor:
        raise NotImplementedError

    def classes(self) -> List[int]:
        raise NotImplementedError


POOLS = ("none", "mean")
ATTR_METHODS = ("gradient", "gradient_x_activation", "integrated_gradients")


class HipTCAV:
    """TCAV over ``hidden_states[l]`` of a ``HipAttribution``'s classifier.  ``pool="none"``: the feature space is the flattened
    ``[T * H]`` activation (Captum), so the concept clips must give the inputs' frame count; ``pool="mean"``: the time mean
    ``[H]`` (``advh_concept_time_pool``; clip lengths may differ), for which the score is ``(sum_t g_t) . v``: the derivative of
    the logit when ``v`` is added to every frame, i.e. when the time mean moves along ``v``."""

    def __init__(self, attribution: HipAttribution, layers, classifier="logistic", alpha: float = 0.01, pool: str = "none",
                 test_split_ratio: float = 0.33, seed: int = 0, model_id: str = "default_model_id", save_path: Optional[str] = None,
                 internal_batch_size: Optional[int] = None, memory_budget: int = 8 << 30):
        if not isinstance(attribution, HipAttribution):
            raise TypeError("attribution must be a HipAttribution")
        nl = attribution.eg.emb.nl
        layers = [layers] if isinstance(layers, int) and not isinstance(layers, bool) else list(layers)
        if not layers:
            raise ValueError("layers must name at least one layer")
        self.layers = [check_layer(l, nl) for l in layers]
        if len(set(self.layers)) != len(self.layers):
            raise ValueError(f"layers repeats an entry: {layers}")
        if pool not in POOLS:
            raise ValueError(f"pool must be one of {POOLS}, not {pool!r}")
        if not (isinstance(test_split_ratio, (int, float)) and not isinstance(test_split_ratio, bool) and 0 <= test_split_ratio < 1):
            raise ValueError(f"test_split_ratio must lie in [0, 1), not {test_split_ratio!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or seed < 0:
            raise ValueError(f"seed must be a non-negative int, not {seed!r}")
        if classifier == "logistic":
            classifier = LogisticCAV(alpha)
        elif classifier == "mean_difference":
            classifier = MeanDifferenceCAV()
        elif not (hasattr(classifier, "dual") or all(hasattr(classifier, m) for m in ("train_and_eval", "weights", "classes"))):
            raise ValueError("classifier must be 'logistic', 'mean_difference', a LogisticCAV / MeanDifferenceCAV or an object with "
                             "Captum's Classifier protocol (train_and_eval, weights, classes)")
        self.att, self.classifier, self.pool = attribution, classifier, pool
        self.ratio, self.seed, self.model_id, self.save_path = float(test_split_ratio), seed, str(model_id), save_path
        self.chunk = 16 if internal_batch_size is None else _positive_int(internal_batch_size, "internal_batch_size")
        self.budget = _positive_int(memory_budget, "memory_budget")
        self._acts: Dict[int, Dict[int, torch.Tensor]] = {}                  # concept id -> layer -> [n, F] device fp32
        self._frames: Optional[int] = None
        self.cavs: Dict[str, Dict[int, CAV]] = {}

    # ------------------------------------------------------------------ activations
    def _features(self, T: int) -> int:
        H = self.att.eg.cfg.hidden_size
        return H if self.pool == "mean" else T * H

    def _concept_activations(self, concept: Concept) -> Dict[int, torch.Tensor]:
        """The concept's features per requested layer, ``[n, F]`` on the device; computed once per concept."""
        if concept.id in self._acts:
            return self._acts[concept.id]
        eg, top = self.att.eg, max(self.layers)
        parts: Dict[int, List[torch.Tensor]] = {l: [] for l in self.layers}
        held = sum(t.numel() * 4 for d in self._acts.values() for t in d.values())
        for batch in concept.batches():
            for r0 in range(0, batch.shape[0], self.chunk):
                x = self.att._prep(batch[r0:r0 + self.chunk])
                T = eg.forward(x, to_layer=top).shape[1]
                if self.pool == "none":
                    if self._frames is None:
                        self._frames = T
                    elif T != self._frames:
                        raise ValueError(f"pool='none' needs one frame count: concept {concept.identifier} gives {T} frames, earlier "
                                         f"clips gave {self._frames} (use clips of one length, or pool='mean')")
                held += len(self.layers) * x.shape[0] * self._features(T) * 4
                if held > self.budget:
                    raise MemoryError(f"the concept activations need more than memory_budget = {self.budget} bytes on the device "
                                      f"({held} after concept {concept.identifier}): fewer clips, fewer layers, pool='mean' or a larger budget")
                for l in self.layers:
                    h = eg.hidden(l)
                    parts[l].append(time_pool(h, mean=True) if self.pool == "mean" else h.view(h.shape[0], -1))
        if not parts[self.layers[0]]:
            raise ValueError(f"concept {concept.identifier} has no data")
        out = {l: (p[0] if len(p) == 1 else torch.cat(p)) for l, p in parts.items()}
        for l, t in out.items():
            self.att._checked(t, f"activations of concept {concept.identifier} at layer {l}", "the forward pass produced a non-finite activation")
        self._acts[concept.id] = out
        return out

    # ------------------------------------------------------------------ CAVs
    def _settings(self, concepts: Sequence[Concept], layer: int, n_rows: Sequence[int], F: int) -> str:
        cl = self.classifier.settings() if hasattr(self.classifier, "settings") else type(self.classifier).__name__
        return (f"classifier={cl};pool={self.pool};ratio={self.ratio!r};seed={self.seed};layer={layer};"
                f"concepts={[c.identifier for c in concepts]};rows={list(n_rows)};features={F};precision={self.att.precision}")

    def _cav_file(self, key: str, layer: int) -> Optional[str]:
        if self.save_path is None:
            return None
        return os.path.join(self.save_path, f"{self.model_id}_{key}_layer{layer}.npz")

    def _load(self, path: Optional[str], settings: str, dev) -> Optional[CAV]:
        if path is None or not os.path.exists(path):
            return None
        with np.load(path, allow_pickle=False) as z:
            if str(z["settings"]) != settings:
                return None
            return CAV(torch.from_numpy(z["weights"]).to(dev), [int(c) for c in z["classes"]], float(z["accs"]), z["intercepts"].copy())

    def _train(self, concepts: Sequence[Concept], layer: int) -> CAV:
        acts = [self._concept_activations(c)[layer] for c in concepts]
        X = torch.cat(acts)                                                  # [n, F]: the set's rows, concept after concept
        n, C = X.shape[0], len(concepts)
        labels = np.concatenate([np.full(a.shape[0], i) for i, a in enumerate(acts)])
        train, test = split_rows(n, self.ratio, self.seed)
        if hasattr(self.classifier, "dual"):
            K = gram(X).cpu().numpy()
            A, b, acc = fit_duals(self.classifier, K, labels, C, train, test)
            W = combine(torch.from_numpy(A).to(X.device, torch.float32), X)
            return CAV(W, [c.id for c in concepts], acc, b)
        return self._train_user(concepts, X, labels, train, test)

    def _train_user(self, concepts, X, labels, train, test) -> CAV:
        """A user classifier with Captum's protocol: a DataLoader over host copies of the training rows; the accuracy comes
        from its own ``train_and_eval`` (``{"accs": ...}``) when it returns one."""
        from torch.utils.data import DataLoader, TensorDataset
        ids = torch.tensor([concepts[i].id for i in labels[train]])
        stats = self.classifier.train_and_eval(DataLoader(TensorDataset(X[torch.from_numpy(train).to(X.device)].cpu(), ids), batch_size=len(train)))
        W = torch.as_tensor(self.classifier.weights(), dtype=torch.float32)
        if W.dim() != 2 or W.shape[1] != X.shape[1]:
            raise ValueError(f"the classifier's weights() must be [C, {X.shape[1]}], not {list(W.shape)}")
        acc = float(stats["accs"]) if isinstance(stats, dict) and "accs" in stats else float("nan")
        return CAV(W.to(X.device).contiguous(), [int(c) for c in self.classifier.classes()], acc, np.zeros(W.shape[0]))

    def _check_sets(self, experimental_sets) -> List[List[Concept]]:
        sets = [list(s) for s in experimental_sets]
        if not sets:
            raise ValueError("experimental_sets is empty")
        seen: Dict[int, Concept] = {}
        for s in sets:
            if len(s) < 2 or not all(isinstance(c, Concept) for c in s):
                raise ValueError("an experimental set is a list of at least two Concepts")
            if len({c.id for c in s}) != len(s):
                raise ValueError(f"experimental set {concepts_to_str(s)} repeats a concept")
            for c in s:
                if seen.setdefault(c.id, c) is not c:
                    raise ValueError(f"two different concepts share the id {c.id}")
        return sets

    def compute_cavs(self, experimental_sets, force_train: bool = False) -> Dict[str, Dict[int, CAV]]:
        """``{concepts_to_str(set): {layer: CAV}}``.  Activations: ``forward(x, to_layer=max(layers))`` in chunks of
        ``internal_batch_size`` clips, once per concept however many sets it appears in, kept on the device (MemoryError past
        ``memory_budget`` bytes).  Per (set, layer): the Gram matrix, the host solve, the combine kernel.  With ``save_path`` each
        CAV is one ``.npz`` (weights, intercepts, classes, accs and the settings that produced them; no pickle), reloaded unless
        ``force_train`` is set or the settings differ.  One engine keeps what it computed: a concept id stands for the same clips
        for the engine's lifetime, and a set it has trained is not trained again unless ``force_train`` is set."""
        sets = self._check_sets(experimental_sets)
        dev = self.att.emb.dev
        out: Dict[str, Dict[int, CAV]] = {}
        for s in sets:
            key = concepts_to_str(s)
            out[key] = {}
            for l in self.layers:
                if not force_train and l in self.cavs.get(key, {}):           # trained by an earlier call of this engine
                    out[key][l] = self.cavs[key][l]
                    continue
                path, cav, settings = self._cav_file(key, l), None, None
                if path is not None:
                    acts = [self._concept_activations(c)[l] for c in s]
                    settings = self._settings(s, l, [a.shape[0] for a in acts], acts[0].shape[1])
                    cav = None if force_train else self._load(path, settings, dev)
                if cav is None:
                    cav = self._train(s, l)
                    if path is not None:
                        os.makedirs(self.save_path, exist_ok=True)
                        np.savez(path, weights=cav.weights.cpu().numpy(), intercepts=np.asarray(cav.intercepts, np.float64),
                                 classes=np.asarray(cav.classes, np.int64), accs=np.float64(cav.accs), settings=np.str_(settings))
                out[key][l] = cav
        self.cavs.update(out)
        return out

    # ------------------------------------------------------------------ scores
    def _layer_attribution(self, waves, layer: int, attr_method: str, kw: dict) -> torch.Tensor:
        if attr_method == "gradient":
            return self.att.layer_gradient_x_activation(waves, layer, multiply_by_inputs=False)
        if attr_method == "gradient_x_activation":
            return self.att.layer_gradient_x_activation(waves, layer)
        return self.att.layer_integrated_gradients(waves, layer, baselines=kw.get("baselines"), n_steps=kw.get("n_steps", 50),
                                                   internal_batch_size=kw.get("internal_batch_size"))

    def _check_interpret(self, waves, target, attr_method, magnitude, kw):
        if target is not None:
            raise NotImplementedError("the classifier has a single output; target must be None")
        if not torch.is_tensor(waves) or waves.dim() != 2:
            raise ValueError("inputs must be a [B, L] waveform tensor")
        if attr_method not in ATTR_METHODS:
            raise ValueError(f"attr_method must be one of {ATTR_METHODS}, not {attr_method!r}")
        if magnitude not in ("mean", "normalized"):
            raise ValueError(f"magnitude must be 'mean' or 'normalized', not {magnitude!r}")
        extra = set(kw) - ({"baselines", "n_steps", "internal_batch_size"} if attr_method == "integrated_gradients" else set())
        if extra:
            raise TypeError(f"unexpected arguments for attr_method={attr_method!r}: {sorted(extra)}")

    def interpret(self, waves, experimental_sets, target=None, attr_method: str = "gradient", magnitude: str = "mean", **kw):
        """``{set: {layer: {"sign_count" [C], "magnitude" [C], "scores" [B, C]}}}`` (device fp32 tensors).  One layer attribution
        per layer -- ``"gradient"`` (default; Captum's default ``layer_attr_method``, LayerGradientXActivation with
        ``multiply_by_inputs=False``), ``"gradient_x_activation"`` or ``"integrated_gradients"`` (``baselines``, ``n_steps``,
        ``internal_batch_size`` forwarded) -- then ONE ``advh_concept_gram`` launch against the CAVs of all sets.
        ``scores[b, c] = <attr_b, w_c>``; ``sign_count = mean_b(scores > 0)``; ``magnitude="mean"`` is Captum 0.7's
        ``mean_b(scores)``, ``"normalized"`` the earlier Captum form ``sum|s * [s > 0]| / sum|s|``.  Parity with Captum is
        unpinned (captum is absent).  ``pool="mean"``: the attribution is summed over the frames first."""
        self._check_interpret(waves, target, attr_method, magnitude, kw)
        sets = self._check_sets(experimental_sets)
        cavs = self.compute_cavs(sets)
        out: Dict[str, Dict[int, dict]] = {concepts_to_str(s): {} for s in sets}
        for l in self.layers:
            g = self._layer_attribution(waves, l, attr_method, kw)           # [B, T, H]
            B, T, H = g.shape
            if self.pool == "none" and self._frames is not None and T != self._frames:
                raise ValueError(f"pool='none': the inputs give {T} frames, the concept clips gave {self._frames}")
            X = time_pool(g) if self.pool == "mean" else g.view(B, T * H)
            W = torch.cat([cavs[k][l].weights for k in out])                 # [sum C, F]
            S = gram(X, W).float()                                           # [B, sum C]
            host = S.cpu().numpy()                                           # the one synchronising copy of the layer
            stats, c0 = [], 0
            for k in out:
                C = cavs[k][l].weights.shape[0]
                stats.append(np.stack(tcav_scores(host[:, c0:c0 + C], magnitude)))
                c0 += C
            stats = torch.from_numpy(np.concatenate(stats, 1)).to(S.device, torch.float32)      # [2, sum C]: one upload
            c0 = 0
            for k in out:
                C = cavs[k][l].weights.shape[0]
                out[k][l] = {"sign_count": stats[0, c0:c0 + C].contiguous(), "magnitude": stats[1, c0:c0 + C].contiguous(),
                             "scores": S[:, c0:c0 + C].contiguous()}
                c0 += C
        return out

    def frame_sensitivity(self, waves, experimental_set, layer: int) -> torch.Tensor:
        """``s[b, c, t] = g[b, t, :] . v_c`` ``[B, C, T]`` for the ``pool="mean"`` CAVs ``v_c`` of one experimental set: where in
        the clip the concept pushes the logit.  Its sum over ``t`` is the ``pool="mean"`` score; each ``s[:, c]`` feeds
        ``HipAttribution.frames_to_wave``."""
        if self.pool != "mean":
            raise ValueError("frame_sensitivity needs pool='mean' (a CAV per frame feature)")
        l = check_layer(layer, self.att.eg.emb.nl)
        if l not in self.layers:
            raise ValueError(f"layer {l} is not one of this TCAV's layers {self.layers}")
        if not torch.is_tensor(waves) or waves.dim() != 2:
            raise ValueError("inputs must be a [B, L] waveform tensor")
        s = self._check_sets([experimental_set])[0]
        cav = self.compute_cavs([s])[concepts_to_str(s)][l]
        g = self.att.layer_gradient_x_activation(waves, l, multiply_by_inputs=False)
        B, T, H = g.shape
        S = gram(g.view(B * T, H), cav.weights).float()                      # [B * T, C]
        return S.view(B, T, -1).permute(0, 2, 1).contiguous()
