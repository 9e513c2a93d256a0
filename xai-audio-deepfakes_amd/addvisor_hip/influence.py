"""Training-data influence (Captum 0.7's ``captum.influence``, restated: captum is absent) on the HIP chain: which TRAINING clips
made the classifier say so.

The classifier is a frozen wav2vec2 embedder followed by a logistic regression on time-pooled features, so everything after the
forward pass lives in the space of the pooled features ``phi [H]`` (augmented to ``[phi, 1]``: the bias column) or of one layer's
activations:

- ``HipInfluenceIndex``: the training set, embedded once (``EmbedderGrad.forward`` in chunks), kept on the device.
- ``HipSimilarityInfluence``: nearest training examples at a layer (cosine similarity or euclidean distance).
- ``HipTracInCPFast`` (Pruthi et al. 2020, last-layer form): ``sum_c lr_c grad l_c(test) . grad l_c(train)`` over the final linear
  layer, which for this model is the whole trainable part -- exact, not an approximation.
- ``HipLogisticInfluence`` (Koh & Liang 2017): ``grad l(test)^T H^-1 grad l(train)``; the objective is convex, so it is exact to
  first order.  The ``(H + 1) x (H + 1)`` Hessian is formed on the device (``advh_influence_moment``) and solved on the host in
  float64, the way TCAV's dual problem is.

Every product over rows is a HIP kernel (csrc/influence.hip, ``advh_concept_gram``); no torch op does arithmetic on activations.
Parity with Captum is unpinned: the formulas are restated from its source and the two papers.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .attribution import HipAttribution, _positive_int
from .concept import POOLS, _rows, gram, time_pool
from .embedder_grad import check_layer


def _st():
    return torch.cuda.current_stream().cuda_stream


def _sized(name: str, *args) -> int:
    n = getattr(_lib.lib(), name)(*args)
    if n < 0:
        raise _lib.AdvhError(f"{name}{args}: {_lib.ERRORS.get(n, n)}")
    return n


def _f64(t: torch.Tensor, shape: Tuple[int, ...], what: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype != torch.float64 or not t.is_cuda or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be a CUDA float64 tensor of shape {list(shape)}")
    return t.contiguous()


def _f32(t: torch.Tensor, shape: Tuple[int, ...], what: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be a CUDA fp32 tensor of shape {list(shape)}")
    return t.contiguous()


# ---------------------------------------------------------------------------------------------- the kernels
def moment_workspace(N: int, F: int) -> int:
    """Bytes of the partial buffer of ``moment`` (``advh_influence_moment_workspace``)."""
    return _sized("advh_influence_moment_workspace", N, F)


def sqdist_workspace(M: int, N: int, F: int) -> int:
    return _sized("advh_influence_sqdist_workspace", M, N, F)


def topk_workspace(M: int, N: int, k: int) -> int:
    return _sized("advh_influence_topk_workspace", M, N, k)


def moment(X: torch.Tensor, w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``Hm[f, g] = sum_i w[i] X[i, f] X[i, g]`` as a float64 ``[F, F]`` device tensor; ``w=None``: all ones."""
    N, F, ldx = _rows(X, "X")
    if w is not None:
        w = _f32(w, (N,), "w")
    ws = torch.empty(moment_workspace(N, F) // 4, dtype=torch.float32, device=X.device)
    Hm = torch.empty((F, F), dtype=torch.float64, device=X.device)
    _lib.check(_lib.lib().advh_influence_moment(X.data_ptr(), ldx, None if w is None else w.data_ptr(), N, F, ws.data_ptr(), Hm.data_ptr(),
                                                _st()), "advh_influence_moment")
    return Hm


def sqdist(X: torch.Tensor, Y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``D[i, j] = sum_f (X[i, f] - Y[j, f])^2`` as a float64 ``[M, N]`` device tensor; ``Y=None``: ``X`` against itself."""
    M, F, ldx = _rows(X, "X")
    N, Fy, ldy = (M, F, ldx) if Y is None else _rows(Y, "Y")
    if Fy != F:
        raise ValueError(f"X has {F} features, Y has {Fy}")
    ws = torch.empty(sqdist_workspace(M, N, F) // 4, dtype=torch.float32, device=X.device)
    D = torch.empty((M, N), dtype=torch.float64, device=X.device)
    _lib.check(_lib.lib().advh_influence_sqdist(X.data_ptr(), ldx, (X if Y is None else Y).data_ptr(), ldy, M, N, F, ws.data_ptr(),
                                                D.data_ptr(), _st()), "advh_influence_sqdist")
    return D


def sumsq(X: torch.Tensor) -> torch.Tensor:
    """``sum_f X[i, f]^2`` per row, float64 ``[M]``."""
    M, F, ldx = _rows(X, "X")
    out = torch.empty(M, dtype=torch.float64, device=X.device)
    _lib.check(_lib.lib().advh_influence_sumsq(X.data_ptr(), ldx, M, F, out.data_ptr(), _st()), "advh_influence_sumsq")
    return out


def residual(Z: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """``out[c, n] = sigma(Z[n, c]) - y[n]``, fp32 ``[C, N]``, from float64 logits ``Z [N, C]`` and fp32 labels ``y [N]``."""
    if not torch.is_tensor(Z) or Z.dim() != 2 or Z.numel() == 0:
        raise ValueError("Z must be a non-empty float64 [N, C] tensor")
    N, C = Z.shape
    Z, y = _f64(Z, (N, C), "Z"), _f32(y, (N,), "y")
    out = torch.empty((C, N), dtype=torch.float32, device=Z.device)
    _lib.check(_lib.lib().advh_influence_residual(Z.data_ptr(), y.data_ptr(), N, C, out.data_ptr(), _st()), "advh_influence_residual")
    return out


def _out(M: int, N: int, dev, out: Optional[torch.Tensor]) -> Tuple[torch.Tensor, int]:
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or tuple(out.shape) != (M, N) or (N > 1 and out.stride(1) != 1):
        raise ValueError(f"out must be an fp32 [{M}, {N}] tensor with contiguous rows")
    return out, (out.stride(0) if M > 1 else max(N, out.stride(0)))


def cosine(G: torch.Tensor, a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``G[m, n] / (sqrt(a[m]) sqrt(b[n]))``, 0 where a norm is zero; fp32 ``[M, N]``."""
    M, N = G.shape
    G, a, b = _f64(G, (M, N), "G"), _f64(a, (M,), "a"), _f64(b, (N,), "b")
    out, ldo = _out(M, N, G.device, out)
    _lib.check(_lib.lib().advh_influence_cosine(G.data_ptr(), a.data_ptr(), b.data_ptr(), M, N, out.data_ptr(), ldo, _st()),
               "advh_influence_cosine")
    return out


def root(D: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sqrt(D)`` in fp64, rounded once; fp32 ``[M, N]``."""
    M, N = D.shape
    D = _f64(D, (M, N), "D")
    out, ldo = _out(M, N, D.device, out)
    _lib.check(_lib.lib().advh_influence_root(D.data_ptr(), M, N, out.data_ptr(), ldo, _st()), "advh_influence_root")
    return out


def scale(G: torch.Tensor, rt: torch.Tensor, rn: torch.Tensor, lr: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``G[m, n] * sum_c lr[c] rt[c, m] rn[c, n]``, ``c`` ascending in fp64, rounded once; fp32 ``[M, N]``."""
    M, N = G.shape
    C = lr.shape[0]
    G, lr, rt, rn = _f64(G, (M, N), "G"), _f64(lr, (C,), "lr"), _f32(rt, (C, M), "rt"), _f32(rn, (C, N), "rn")
    out, ldo = _out(M, N, G.device, out)
    _lib.check(_lib.lib().advh_influence_scale(G.data_ptr(), rt.data_ptr(), rn.data_ptr(), lr.data_ptr(), C, M, N, out.data_ptr(), ldo, _st()),
               "advh_influence_scale")
    return out


def self_scale(ss: torch.Tensor, rn: torch.Tensor, lr: torch.Tensor) -> torch.Tensor:
    """``ss[n] * sum_c lr[c] rn[c, n]^2``, fp32 ``[N]``: the scale kernel's product on the diagonal."""
    C, N = rn.shape
    ss, lr, rn = _f64(ss, (N,), "ss"), _f64(lr, (C,), "lr"), _f32(rn, (C, N), "rn")
    out = torch.empty(N, dtype=torch.float32, device=rn.device)
    _lib.check(_lib.lib().advh_influence_self_scale(ss.data_ptr(), rn.data_ptr(), lr.data_ptr(), C, N, out.data_ptr(), _st()),
               "advh_influence_self_scale")
    return out


def topk(S: torch.Tensor, k: int, largest: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per row of fp32 ``S [M, N]`` the ``k`` extreme entries in order, ties to the lower index: ``(idx int32 [M, k], val fp32
    [M, k])``, equal to ``np.argsort(-+S[m], kind="stable")[:k]``.  The input must be finite."""
    M, N, lds = _rows(S, "S")
    k = _positive_int(k, "k")
    ws = torch.empty(topk_workspace(M, N, k) // 8, dtype=torch.int64, device=S.device)
    idx = torch.empty((M, k), dtype=torch.int32, device=S.device)
    val = torch.empty((M, k), dtype=torch.float32, device=S.device)
    _lib.check(_lib.lib().advh_influence_topk(S.data_ptr(), lds, M, N, k, int(bool(largest)), ws.data_ptr(), idx.data_ptr(), val.data_ptr(),
                                              _st()), "advh_influence_topk")
    return idx, val


# ---------------------------------------------------------------------------------------------- the index
def _labels(labels, n: int, dev) -> torch.Tensor:
    y = torch.as_tensor(labels)
    if y.dim() != 1 or y.shape[0] != n:
        raise ValueError(f"labels must be [{n}], one per clip; got {list(y.shape)}")
    y = y.to(dev, torch.float32)
    if not bool(((y == 0) | (y == 1)).all()):
        raise ValueError("labels must be 0 or 1")
    return y


class HipInfluenceIndex:
    """The training set, embedded once.  ``add(waves, labels)`` runs the forward in chunks of ``internal_batch_size`` clips and keeps

    - the pooled features -- exactly what the logistic regression sees: ``advh_pool_logreg``'s ``pooled`` output -- augmented as
      ``[phi, 1]`` in ``[N, H + 1]`` with the row stride rounded up to a multiple of 4 floats (16-byte loads in every kernel): the
      Gram matrix of augmented rows is ``phi . phi' + 1``, so the bias term of every gradient product comes for free;
    - for each layer in ``layers``, ``hidden_states[l]`` flattened (``pool="none"``: one frame count across all clips) or time-mean
      (``pool="mean"``, ``advh_concept_time_pool``), as ``HipTCAV`` does.

    Everything stays on the device; ``MemoryError`` past ``memory_budget`` bytes.  ``save`` / ``load``: one ``.npz`` without pickle,
    with the settings that produced it; a file whose settings differ is rejected."""

    def __init__(self, attribution: HipAttribution, layers=(), pool: str = "none", internal_batch_size: int = 16, memory_budget: int = 8 << 30):
        if not isinstance(attribution, HipAttribution):
            raise TypeError("attribution must be a HipAttribution")
        nl = attribution.eg.emb.nl
        layers = [layers] if isinstance(layers, int) and not isinstance(layers, bool) else list(layers)
        self.layers = [check_layer(l, nl) for l in layers]
        if len(set(self.layers)) != len(self.layers):
            raise ValueError(f"layers repeats an entry: {layers}")
        if pool not in POOLS:
            raise ValueError(f"pool must be one of {POOLS}, not {pool!r}")
        self.att, self.pool = attribution, pool
        self.chunk = _positive_int(internal_batch_size, "internal_batch_size")
        self.budget = _positive_int(memory_budget, "memory_budget")
        self.H = attribution.eg.cfg.hidden_size
        self.ld = (self.H + 1 + 3) // 4 * 4
        self._phi: List[torch.Tensor] = []                                   # [n, ld] chunks
        self._acts: Dict[int, List[torch.Tensor]] = {l: [] for l in self.layers}
        self._y: List[Optional[torch.Tensor]] = []
        self._frames: Optional[int] = None
        self._held = 0
        self._cache: dict = {}                                               # derived rows (norms), dropped by add / load
        self.version = 0                                                     # counts add / load: engines drop what they derived

    # ------------------------------------------------------------------ embedding
    def _features(self, T: int) -> int:
        return self.H if self.pool == "mean" else T * self.H

    def embed(self, waves: torch.Tensor, what: str = "the inputs") -> Tuple[torch.Tensor, Dict[int, torch.Tensor], int]:
        """``(phi [B, H + 1] augmented pooled features (row stride ``ld``), {layer: [B, F]}, bytes)`` of ``waves [B, L]``: one
        forward per chunk of ``internal_batch_size`` clips."""
        if not torch.is_tensor(waves) or waves.dim() != 2 or waves.shape[0] < 1 or not waves.is_floating_point():
            raise ValueError(f"{what} must be a floating-point [B, L] waveform tensor")
        eg, lib, H = self.att.eg, _lib.lib(), self.H
        B = waves.shape[0]
        dev = self.att.emb.dev
        phi = torch.zeros((B, self.ld), dtype=torch.float32, device=dev)
        phi[:, H] = 1.0
        acts: Dict[int, List[torch.Tensor]] = {l: [] for l in self.layers}
        for r0 in range(0, B, self.chunk):
            x = self.att._prep(waves[r0:r0 + self.chunk])
            eg.forward(x)
            h = eg.hidden(eg.emb.nl)                                         # the rows the pooling reads
            b, T = h.shape[0], h.shape[1]
            if self.pool == "none" and self.layers:
                if self._frames is None:
                    self._frames = T
                elif T != self._frames:
                    raise ValueError(f"pool='none' needs one frame count: {what} give {T} frames, earlier clips gave {self._frames} "
                                     "(use clips of one length, or pool='mean')")
            pooled = torch.empty((b, H), dtype=torch.float32, device=dev)
            scratch = torch.empty((2, b), dtype=torch.float32, device=dev)
            _lib.check(lib.advh_pool_logreg(h.data_ptr(), eg.emb.coef.data_ptr(), eg.emb.intercept, scratch[0].data_ptr(), scratch[1].data_ptr(),
                                            pooled.data_ptr(), b, T, H, _st()), "advh_pool_logreg")
            phi[r0:r0 + b, :H] = pooled
            for l in self.layers:
                hl = eg.hidden(l)
                acts[l].append(time_pool(hl, mean=True) if self.pool == "mean" else hl.view(b, -1))
        out = {l: (p[0] if len(p) == 1 else torch.cat(p)) for l, p in acts.items()}
        cause = "the forward pass produced a non-finite activation"
        self.att._checked(phi, f"pooled features of {what}", cause)
        for l, t in out.items():
            self.att._checked(t, f"activations of {what} at layer {l}", cause)
        return phi[:, :H + 1], out, phi.numel() * 4 + sum(t.numel() * 4 for t in out.values())

    def add(self, waves: torch.Tensor, labels=None) -> "HipInfluenceIndex":
        """Append clips (and their 0 / 1 labels, which TracIn and the influence functions need)."""
        if not torch.is_tensor(waves) or waves.dim() != 2 or waves.shape[0] < 1:
            raise ValueError("waves must be a [n, L] waveform tensor")
        if self._y and ((labels is None) != (self._y[0] is None)):
            raise ValueError("either every add() call gives labels or none does")
        y = None if labels is None else _labels(labels, waves.shape[0], self.att.emb.dev)
        for r0 in range(0, waves.shape[0], self.chunk):                      # chunk by chunk: the budget stops the loop early
            sl = slice(r0, r0 + self.chunk)
            phi, acts, nbytes = self.embed(waves[sl], "the training clips")
            self._held += nbytes
            if self._held > self.budget:
                raise MemoryError(f"the index needs more than memory_budget = {self.budget} bytes on the device ({self._held} after "
                                  f"{self.n + phi.shape[0]} clips): fewer clips, fewer layers, pool='mean' or a larger budget")
            self._phi.append(phi)
            for l in self.layers:
                self._acts[l].append(acts[l])
            self._y.append(None if y is None else y[sl])
        self._cache.clear()
        self.version += 1
        return self

    # ------------------------------------------------------------------ rows
    @property
    def n(self) -> int:
        return sum(p.shape[0] for p in self._phi)

    def _need(self):
        if not self._phi:
            raise ValueError("the index is empty: add() training clips first")

    def _joined(self, parts: List[torch.Tensor]) -> torch.Tensor:
        if len(parts) > 1:                                                   # join once; the parts are dropped
            ld = parts[0].stride(0) if parts[0].shape[0] > 1 else parts[0].shape[1]
            buf = torch.empty((sum(p.shape[0] for p in parts), max(ld, parts[0].shape[1])), dtype=torch.float32, device=parts[0].device)
            view = buf[:, :parts[0].shape[1]]
            r = 0
            for p in parts:
                view[r:r + p.shape[0]] = p
                r += p.shape[0]
            parts[:] = [view]
        return parts[0]

    @property
    def phi(self) -> torch.Tensor:
        """``[N, H + 1]`` augmented pooled features, row stride a multiple of 4 floats."""
        self._need()
        if len(self._phi) > 1:
            buf = torch.zeros((self.n, self.ld), dtype=torch.float32, device=self._phi[0].device)
            r = 0
            for p in self._phi:
                buf[r:r + p.shape[0], :self.H + 1] = p
                r += p.shape[0]
            self._phi = [buf[:, :self.H + 1]]
        return self._phi[0]

    def activations(self, layer: int) -> torch.Tensor:
        self._need()
        if layer not in self._acts:
            raise ValueError(f"layer {layer} is not one of this index's layers {self.layers}")
        return self._joined(self._acts[layer])

    @property
    def labels(self) -> torch.Tensor:
        self._need()
        if self._y[0] is None:
            raise ValueError("this method needs the training labels: pass labels to add()")
        if len(self._y) > 1:
            self._y = [torch.cat(self._y)]
        return self._y[0]

    def cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    # ------------------------------------------------------------------ files
    def _settings(self, n: int, frames) -> str:
        return (f"precision={self.att.precision};layers={self.layers};pool={self.pool};hidden={self.H};rows={n};frames={frames}")

    def save(self, path: str) -> None:
        self._need()
        arrays = {"phi": self.phi.cpu().numpy(), "settings": np.str_(self._settings(self.n, self._frames))}
        arrays["labels"] = self.labels.cpu().numpy() if self._y[0] is not None else np.zeros(0, np.float32)
        for l in self.layers:
            arrays[f"layer_{l}"] = self.activations(l).cpu().numpy()
        np.savez(path, **arrays)

    def load(self, path: str) -> "HipInfluenceIndex":
        """Replace the index's rows by the file's; ``ValueError`` if the file was written with other settings."""
        dev = self.att.emb.dev
        with np.load(path, allow_pickle=False) as z:
            phi = z["phi"]
            frames = None
            if self.pool == "none" and self.layers and f"layer_{self.layers[0]}" in z.files:
                frames = z[f"layer_{self.layers[0]}"].shape[1] // self.H
            want = self._settings(phi.shape[0], frames)
            if str(z["settings"]) != want:
                raise ValueError(f"{path} was written with other settings: {str(z['settings'])!r}, this index has {want!r}")
            buf = torch.zeros((phi.shape[0], self.ld), dtype=torch.float32, device=dev)
            buf[:, :self.H + 1] = torch.from_numpy(phi).to(dev)
            self._phi = [buf[:, :self.H + 1]]
            self._acts = {l: [torch.from_numpy(z[f"layer_{l}"]).to(dev)] for l in self.layers}
            y = z["labels"]
            self._y = [torch.from_numpy(y).to(dev) if y.shape[0] else None]
        self._frames = frames
        self._held = buf.numel() * 4 + sum(t[0].numel() * 4 for t in self._acts.values())
        self._cache.clear()
        self.version += 1
        return self


def _check_index(index) -> HipInfluenceIndex:
    if not isinstance(index, HipInfluenceIndex):
        raise TypeError("index must be a HipInfluenceIndex")
    return index


def _check_k(k, n: int, name: str = "k") -> Optional[int]:
    if k is None:
        return None
    k = _positive_int(k, name)
    if k > min(n, 256):
        raise ValueError(f"{name} must be at most min(N, 256) = {min(n, 256)}, not {k}")
    return k


def _ranked(S: torch.Tensor, k: Optional[int], largest: bool):
    if k is None:
        return S
    idx, val = topk(S, k, largest)
    return idx.long(), val


# ---------------------------------------------------------------------------------------------- similarity
METRICS = ("cosine", "euclidean")


class HipSimilarityInfluence:
    """Captum's ``SimilarityInfluence`` at one layer of the index: ``metric="cosine"`` is ``cosine_similarity`` (a zero row gives
    0, Captum's ``replace_nan=0``), ``"euclidean"`` is ``euclidean_distance`` (the distance itself, as Captum returns it);
    ``direction="max"`` ranks the largest values first, ``"min"`` the smallest."""

    def __init__(self, index: HipInfluenceIndex, layer: int, metric: str = "cosine", direction: str = "max"):
        self.index = _check_index(index)
        self.layer = check_layer(layer, index.att.eg.emb.nl)
        if self.layer not in index.layers:
            raise ValueError(f"layer {self.layer} is not one of the index's layers {index.layers}")
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, not {metric!r}")
        if direction not in ("max", "min"):
            raise ValueError(f"direction must be 'max' or 'min', not {direction!r}")
        self.metric, self.direction = metric, direction

    def influence(self, waves: torch.Tensor, top_k: Optional[int] = 1):
        """``(indices int64 [B, k], scores fp32 [B, k])``; ``top_k=None``: the full ``[B, N]`` matrix."""
        ix, l = self.index, self.layer
        Y = ix.activations(l)
        k = _check_k(top_k, Y.shape[0], "top_k")
        X = ix.embed(waves)[1][l]
        if X.shape[1] != Y.shape[1]:
            raise ValueError(f"the inputs give {X.shape[1]} features per clip, the index holds {Y.shape[1]}")
        if self.metric == "cosine":
            S = cosine(gram(X, Y), sumsq(X), ix.cached(("sumsq", l), lambda: sumsq(Y)))
        else:
            S = root(sqdist(X, Y))
        return _ranked(S, k, self.direction == "max")


# ---------------------------------------------------------------------------------------------- TracInCPFast
def _theta_rows(thetas: Sequence[Tuple], H: int, ld: int, dev) -> torch.Tensor:
    """``[C, H + 1]`` fp32 device rows ``[coef, intercept]`` with row stride ``ld``."""
    buf = np.zeros((len(thetas), ld), np.float32)
    for c, (coef, icpt) in enumerate(thetas):
        coef = np.asarray(coef.detach().cpu() if torch.is_tensor(coef) else coef, np.float64).reshape(-1)
        if coef.shape[0] != H or not np.isfinite(coef).all() or not math.isfinite(float(icpt)):
            raise ValueError(f"a coefficient vector must hold {H} finite numbers and the intercept must be finite")
        buf[c, :H], buf[c, H] = coef, float(icpt)
    return torch.from_numpy(buf).to(dev)[:, :H + 1]


class HipTracInCPFast:
    """``TracInCPFast`` (Pruthi et al. 2020): ``sum_c lr_c grad l_c(test) . grad l_c(train)`` over the final linear layer (weights
    and bias) with the per-sample loss BCE-with-logits, ``= (phi~_t . phi~_n) sum_c lr_c (p_c(t) - y_t) (p_c(n) - y_n)``.

    ``checkpoints``: a sequence of ``(coef [H], intercept, lr)``.  The embedder is frozen, so ONE forward per clip serves all
    checkpoints (Captum runs one per checkpoint): a checkpoint is a row of the logits Gram.  Unlike Captum there is no
    ``checkpoints_load_func`` and no ``loss_fn`` object: a checkpoint is its numbers, and the loss is the classifier's own."""

    def __init__(self, index: HipInfluenceIndex, checkpoints: Sequence[Tuple]):
        self.index = _check_index(index)
        cps = list(checkpoints)
        if not cps or not all(isinstance(c, (tuple, list)) and len(c) == 3 for c in cps):
            raise ValueError("checkpoints must be a non-empty sequence of (coef, intercept, lr)")
        lrs = [float(c[2]) for c in cps]
        if not all(math.isfinite(v) and v > 0 for v in lrs):
            raise ValueError("every checkpoint's learning rate must be a finite number > 0")
        dev = index.att.emb.dev
        self.W = _theta_rows([(c[0], c[1]) for c in cps], index.H, index.ld, dev)
        self.lr = torch.tensor(lrs, dtype=torch.float64, device=dev)
        self._rn = None

    def _train_residuals(self) -> torch.Tensor:
        ix = self.index
        if self._rn is None or self._rn[0] != ix.version:                    # the index grew since: its rows changed
            self._rn = (ix.version, residual(gram(ix.phi, self.W), ix.labels))
        return self._rn[1]

    def influence(self, waves: torch.Tensor, labels, k: Optional[int] = None, proponents: bool = True):
        """The ``[B, N]`` score matrix (``k=None``), or ``(indices int64 [B, k], scores fp32 [B, k])`` of the top-k proponents
        (largest scores) or opponents (smallest)."""
        ix = self.index
        Pn = ix.phi
        k = _check_k(k, Pn.shape[0])
        rn = self._train_residuals()
        Pt = ix.embed(waves)[0]
        rt = residual(gram(Pt, self.W), _labels(labels, Pt.shape[0], Pt.device))
        return _ranked(scale(gram(Pt, Pn), rt, rn, self.lr), k, bool(proponents))

    def self_influence(self) -> torch.Tensor:
        """``[N]`` fp32: ``|phi~_n|^2 sum_c lr_c (p_c(n) - y_n)^2``."""
        ix = self.index
        rn = self._train_residuals()
        return self_scale(sumsq(ix.phi), rn, self.lr)


# ---------------------------------------------------------------------------------------------- influence functions
class HipLogisticInfluence:
    """Influence functions (Koh & Liang 2017) of the logistic regression head at ``theta = (coef, intercept)`` (default: the
    attribution model's own) under the objective ``(1/N) sum_i BCE(theta . x~_i, y_i) + (l2 / 2) |coef|^2``:

    ``H = (1/N) sum_i p_i (1 - p_i) x~_i x~_i^T + l2 diag(1, ..., 1, 0) + damping I``.

    The first term is ``advh_influence_moment`` over the index with ``w = p (1 - p)`` (the N logits cross to the host for the
    weights), downloaded once as ``(H + 1)^2`` doubles; the Cholesky factorisation is float64 numpy, once per ``theta``.  Scores are
    ``+grad l(test)^T H^-1 grad l(train)``: Captum's sign, a positive score marks a proponent; ``-1 x`` Koh & Liang's
    ``I_up,loss``.  Influence functions assume that ``theta`` minimises the objective: ``fit()`` finds that minimiser."""

    def __init__(self, index: HipInfluenceIndex, l2: float, damping: float = 0.0, coef=None, intercept=None):
        self.index = _check_index(index)
        for name, v in (("l2", l2), ("damping", damping)):
            if not (isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v >= 0):
                raise ValueError(f"{name} must be a finite number >= 0, not {v!r}")
        self.l2, self.damping = float(l2), float(damping)
        emb = index.att.emb
        if (coef is None) != (intercept is None):
            raise ValueError("give both coef and intercept, or neither (the model's own)")
        self._set_theta(emb.coef if coef is None else coef, emb.intercept if intercept is None else intercept)

    def _set_theta(self, coef, intercept) -> None:
        ix = self.index
        self.W = _theta_rows([(coef, intercept)], ix.H, ix.ld, ix.att.emb.dev)
        self._linv, self._rn, self._version = None, None, ix.version

    def _reg(self) -> np.ndarray:
        d = np.full(self.index.H + 1, self.l2 + self.damping)
        d[-1] = self.damping
        return d

    def hessian(self) -> np.ndarray:
        """``H`` as float64 ``[H + 1, H + 1]`` numpy (one download)."""
        ix = self.index
        z = gram(ix.phi, self.W).cpu().numpy().reshape(-1)
        p = np.exp(-np.logaddexp(0.0, -z))
        w = torch.from_numpy((p * (1.0 - p)).astype(np.float32)).to(ix.phi.device)
        Hm = moment(ix.phi, w).cpu().numpy() / ix.n
        Hm[np.diag_indices_from(Hm)] += self._reg()
        return Hm

    def _factor(self) -> np.ndarray:
        if self._linv is None or self._version != self.index.version:
            self._version = self.index.version
            Hm = self.hessian()
            if not np.isfinite(Hm).all():
                raise FloatingPointError("the Hessian is not finite")
            try:
                Lc = np.linalg.cholesky(Hm)
                self._linv = np.linalg.solve(Lc, np.eye(len(Lc)))             # L^-1, once per theta: a query is two small products
            except np.linalg.LinAlgError:
                raise ValueError(f"the Hessian of {self.index.n} rows with l2 = {self.l2:g} is not positive definite: "
                                 f"raise damping (now {self.damping:g}) or l2") from None
        return self._linv

    def _solve(self, B: np.ndarray) -> np.ndarray:
        """``H^-1 B = L^-T (L^-1 B)`` for ``B [H + 1, m]`` through the inverse of the Cholesky factor ``H = L L^T``."""
        Li = self._factor()
        return Li.T @ (Li @ B)

    def influence(self, waves: torch.Tensor, labels, k: Optional[int] = None, proponents: bool = True):
        """``[B, N]`` scores (``k=None``) or the top-k proponents / opponents ``(indices int64 [B, k], scores fp32 [B, k])``.
        The host forms ``V = phi~_test H^-1`` (B rows); the device computes ``gram(V, phi~)`` and scales it by the residuals."""
        ix = self.index
        Pn = ix.phi
        k = _check_k(k, Pn.shape[0])
        yn = ix.labels
        Pt = ix.embed(waves)[0]
        yt = _labels(labels, Pt.shape[0], Pt.device)
        V = self._solve(Pt.cpu().numpy().astype(np.float64).T).T                                  # [B, H + 1]
        Vd = torch.zeros((V.shape[0], ix.ld), dtype=torch.float32, device=Pt.device)
        Vd[:, :ix.H + 1] = torch.from_numpy(V.astype(np.float32)).to(Pt.device)
        rt = residual(gram(Pt, self.W), yt)
        if self._rn is None or self._rn[0] != ix.version:
            self._rn = (ix.version, residual(gram(Pn, self.W), yn))
        rn = self._rn[1]
        one = torch.ones(1, dtype=torch.float64, device=Pt.device)
        return _ranked(scale(gram(Vd[:, :ix.H + 1], Pn), rt, rn, one), k, bool(proponents))

    def fit(self, max_iter: int = 50, tol: float = 1e-10) -> Tuple[np.ndarray, float, int]:
        """Newton's method for the minimiser of the objective on the index, from ``theta = 0``: per iteration the moment kernel
        (the Hessian) and a host solve; the gradient and the backtracking objective are float64 on a host copy of the
        ``[N, H + 1]`` features (a Newton fixed point is as accurate as its gradient).  Stops when the largest update is
        ``<= tol``.  Sets ``theta`` and returns ``(coef [H] float64, intercept, iterations)``."""
        max_iter = _positive_int(max_iter, "max_iter")
        ix = self.index
        X = ix.phi.cpu().numpy().astype(np.float64)
        y = ix.labels.cpu().numpy().astype(np.float64)
        reg = np.full(ix.H + 1, self.l2)
        reg[-1] = 0.0

        def objective(v):
            z = X @ v
            return float(np.mean(np.logaddexp(0.0, z) - y * z) + 0.5 * reg @ (v * v))

        v = np.zeros(ix.H + 1)
        J = objective(v)
        it = 0
        for it in range(1, max_iter + 1):
            self._set_theta(v[:-1], v[-1])
            p = np.exp(-np.logaddexp(0.0, -(X @ v)))
            grad = (p - y) @ X / len(y) + reg * v
            step = -self._solve(grad[:, None])[:, 0]
            t = 1.0
            while objective(v + t * step) > J + 1e-13 * abs(J) and t > 1e-6:
                t *= 0.5
            v = v + t * step
            J = objective(v)
            if t == 1.0 and np.abs(step).max() <= tol:
                break
        self._set_theta(v[:-1], v[-1])
        return v[:-1].copy(), float(v[-1]), it
