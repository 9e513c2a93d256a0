"""The interpretable models of Lime: Captum's ``SkLearnLasso``, ``SkLearnRidge`` and ``SkLearnLinearRegression`` (restated from
Captum 0.7's ``_utils/models/linear_model/{model,train}.py``: captum is absent), solved in float64 on the host without sklearn.

Captum's protocol: ``model.fit(DataLoader(TensorDataset(z, y, w)))`` concatenates the batches and fits
``sklearn.linear_model.<Model>(**kwargs).fit(z, y, sample_weight=w)``; ``representation()`` is the ``[1, K]`` fp32 weight and
``bias()`` the ``[1]`` fp32 intercept.  Here every fit centres ``z`` and ``y`` by their ``w``-weighted means (the free intercept,
``intercept = mean(y) - mean(z) . coef``) and solves the weighted problem on the centred data:

- ``SkLearnLasso(alpha)``: ``(1 / (2 sum w)) sum_s w_s (y_s - b - z_s . c)^2 + alpha ||c||_1``, sklearn >= 0.23's
  ``Lasso.fit(z, y, sample_weight=w)``.  Cyclic coordinate descent in float64 (``advh_lasso_cd``, a host function of the
  library) stopped on sklearn's duality gap at ``tol = 1e-10`` relative to ``||y||^2``, not sklearn's default ``1e-4``: Captum
  hands sklearn float32 data, which sklearn then fits in float32 with ``tol = 1e-4`` -- about 6e-5 from the converged minimiser on
  a 50 x 12 problem.  Reaching ``max_iter`` sweeps without convergence warns (UserWarning) and keeps the last iterate.
- ``SkLearnRidge(alpha=1.0)``: ``sum_s w_s (y_s - b - z_s . c)^2 + alpha ||c||^2`` (the weights unscaled, as sklearn's
  ``Ridge``), in closed form: the normal equations when K <= S, their dual ``c = Z^T (Z Z^T + alpha I)^-1 y`` otherwise.
- ``SkLearnLinearRegression()``: ``sum_s w_s (y_s - b - z_s . c)^2``, the min-norm least-squares solution of KernelShap's fit
  (``attribution.weighted_linear_fit``: the same arithmetic, bit for bit).
"""
from __future__ import annotations

import ctypes as C
import time
import warnings

import numpy as np
import torch

from . import _lib


def _weighted_centre(z: np.ndarray, y: np.ndarray, w: np.ndarray):
    """``(zc, yc, z_mean, y_mean)`` centred by the ``w``-weighted means."""
    zm = np.average(z, axis=0, weights=w)
    ym = np.average(y, weights=w)
    return z - zm, y - ym, zm, ym


def _check_data(z, y, w):
    z = np.asarray(z, np.float64)
    y = np.asarray(y, np.float64).reshape(-1)
    if z.ndim != 2 or z.shape[0] != y.shape[0] or z.shape[0] < 1:
        raise ValueError(f"the interpretable inputs must be [S, K] with S = len(y); got {list(z.shape)} and {y.shape[0]} outputs")
    w = np.ones(z.shape[0]) if w is None else np.asarray(w, np.float64).reshape(-1)
    if w.shape[0] != z.shape[0]:
        raise ValueError(f"{w.shape[0]} sample weights for {z.shape[0]} samples")
    if not (np.isfinite(z).all() and np.isfinite(y).all() and np.isfinite(w).all()):
        raise FloatingPointError("the interpretable model's data is not finite")
    if (w < 0).any() or w.sum() <= 0:
        raise ValueError("the sample weights must be >= 0 with a positive sum")
    return z, y, w


def lasso_fit(z, y, w=None, alpha: float = 1.0, tol: float = 1e-10, max_iter: int = 100_000):
    """sklearn's weighted Lasso in float64: ``(coef [K], intercept, gap, sweeps)``; the objective is in the module docstring."""
    z, y, w = _check_data(z, y, w)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not np.isfinite(alpha) or alpha < 0:
        raise ValueError(f"alpha must be a finite number >= 0, not {alpha!r}")
    zc, yc, zm, ym = _weighted_centre(z, y, w)
    sw = np.sqrt(w / w.sum())
    X = np.ascontiguousarray((zc * sw[:, None]).T)                       # [K][S]: one column per row of memory
    ys = np.ascontiguousarray(yc * sw)
    S, K = z.shape
    coef = np.zeros(K)
    gap, iters = C.c_double(0.0), C.c_int(0)
    dp = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.lib().advh_lasso_cd(dp(X), dp(ys), S, K, float(alpha), float(tol), int(max_iter), dp(coef), C.byref(gap),
                                        C.byref(iters)), "advh_lasso_cd")
    if iters.value >= max_iter and gap.value > tol * float(ys @ ys):
        warnings.warn(f"Lasso did not converge in {max_iter} sweeps (duality gap {gap.value:.3e}, tolerance "
                      f"{tol * float(ys @ ys):.3e}); the last iterate is kept", UserWarning)
    return coef, float(ym - zm @ coef), gap.value, iters.value


def ridge_fit(z, y, w=None, alpha: float = 1.0):
    """sklearn's weighted Ridge in float64: ``(coef [K], intercept)``."""
    z, y, w = _check_data(z, y, w)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not np.isfinite(alpha) or alpha < 0:
        raise ValueError(f"alpha must be a finite number >= 0, not {alpha!r}")
    zc, yc, zm, ym = _weighted_centre(z, y, w)
    sw = np.sqrt(w)
    X, ys = zc * sw[:, None], yc * sw
    S, K = X.shape
    if alpha == 0:
        coef = np.linalg.lstsq(X, ys, rcond=None)[0]
    elif K <= S:
        coef = np.linalg.solve(X.T @ X + alpha * np.eye(K), X.T @ ys)
    else:
        coef = X.T @ np.linalg.solve(X @ X.T + alpha * np.eye(S), ys)
    return coef, float(ym - zm @ coef)


def _loader_arrays(train_data):
    """Captum's ``sklearn_train_linear_model``: the batches of a DataLoader (or any iterable of ``(x, y[, w])``) concatenated."""
    xs, ys, ws = [], [], []
    for batch in train_data:
        if len(batch) not in (2, 3):
            raise ValueError("each batch must be (inputs, outputs) or (inputs, outputs, weights)")
        xs.append(torch.as_tensor(batch[0]).detach().cpu().reshape(len(batch[0]), -1))
        ys.append(torch.as_tensor(batch[1]).detach().cpu().reshape(-1))
        if len(batch) == 3:
            ws.append(torch.as_tensor(batch[2]).detach().cpu().reshape(-1))
    if not xs:
        raise ValueError("the training data is empty")
    z = torch.cat(xs).numpy()
    y = torch.cat(ys).numpy()
    w = torch.cat(ws).numpy() if ws else None
    return z, y, w


class _SkLearnModel:
    """What Captum's ``SkLearnLinearModel`` exposes: ``fit``, ``representation``, ``bias`` (and ``coef_`` / ``intercept_`` in
    float64)."""

    def __init__(self):
        self.coef_, self.intercept_ = None, None

    def fit(self, train_data, **kwargs):
        return self.fit_arrays(*_loader_arrays(train_data))

    def fit_arrays(self, z, y, w=None):
        """``fit`` on the arrays a DataLoader would concatenate (Lime calls it for these models: a DataLoader collates its
        batch one sample at a time)."""
        t0 = time.time()
        self.coef_, self.intercept_ = self._solve(z, y, w)
        return {"train_time": time.time() - t0}

    def representation(self) -> torch.Tensor:
        if self.coef_ is None:
            raise RuntimeError("fit the model first")
        return torch.from_numpy(self.coef_.astype(np.float32)).view(1, -1)

    def bias(self) -> torch.Tensor:
        if self.coef_ is None:
            raise RuntimeError("fit the model first")
        return torch.tensor([self.intercept_], dtype=torch.float32)


class SkLearnLasso(_SkLearnModel):
    def __init__(self, alpha: float = 1.0, tol: float = 1e-10, max_iter: int = 100_000):
        super().__init__()
        self.alpha, self.tol, self.max_iter = alpha, tol, max_iter
        self.gap_, self.n_iter_ = None, None

    def _solve(self, z, y, w):
        coef, icpt, self.gap_, self.n_iter_ = lasso_fit(z, y, w, self.alpha, self.tol, self.max_iter)
        return coef, icpt


class SkLearnRidge(_SkLearnModel):
    def __init__(self, alpha: float = 1.0):
        super().__init__()
        self.alpha = alpha

    def _solve(self, z, y, w):
        return ridge_fit(z, y, w, self.alpha)


class SkLearnLinearRegression(_SkLearnModel):
    def _solve(self, z, y, w):
        from .attribution import weighted_linear_fit
        z, y, w = _check_data(z, y, w)
        return weighted_linear_fit(z, y, w)
