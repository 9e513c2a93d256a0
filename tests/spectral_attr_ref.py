"""CPU restatement of the time-frequency attributions (addvisor_hip/spectral_attribution.py) for
tests/test_spectral_attr_cpu.py and tests/test_gpu_spectral_attr.py, in torch autograd over ``oracle.signal_ref``
(``compute_stft``, ``embed_mask``, ``apply_mask``, ``compute_invert_stft``) and ``oracle.wav2vec2_ref`` (through
``oracle.attribution_ref.model_logit``):

    ``F(m)[b] = logit(embedder(istft(g(embed(m), |X_b|) e^{j angle X_b})))``, mask-in branch.

The method formulas follow the other ``*_ref.py`` files (Captum restated: captum is absent): path points ``b + alpha (m - b)``
step-major, GradientShap fed explicit draws, and the perturbation methods through ``ablation_ref`` / ``shapley_ref`` with this
file's forward plugged in (their rows are ``k * B + b`` / ``(p * K + j) * B + b``: row r belongs to clip ``r % B``).  The 2-D
occlusion is restated the way Captum computes it: one 0/1 mask per window, first dimension slowest, ``total += diff * mask;
weights += mask; total / weights``."""
import math

import numpy as np
import torch

import ablation_ref as AR
import attribution_baselines_ref as BR
import shapley_ref as SR
from oracle import attribution_ref as A
from oracle import signal_ref as S

NBIN = 513


class MaskModel:
    """``F`` over the clips ``waves [B, L]`` for the classifier ``model = (sd, cfg, coef, intercept)``."""

    def __init__(self, waves, model, domain="linear", sr=16000):
        self.model, self.domain = model, domain
        self.B, self.L = waves.shape
        self.al = self.L / sr
        self.X, self.mag, self.phase = S.compute_stft(waves.float(), audio_length=self.al, sr=sr)
        self.T = self.X.shape[-1]

    def waves(self, masks, clips):
        """``masks [R, Fm, Tm]`` applied to the spectrograms of ``clips [R]`` -> ``[R, L]``."""
        full = S.embed_mask(masks, NBIN, self.T)
        rel, _ = S.apply_mask(full, self.mag[clips], self.phase[clips], self.domain)
        return S.compute_invert_stft(rel, audio_length=self.al)

    def clips_of(self, R, clips=None):
        return torch.arange(R) % self.B if clips is None else torch.as_tensor(clips).long()

    def logit(self, masks, clips=None, per=16):
        """``[R]`` logits of the rows (row r of clip ``r % B`` unless ``clips`` says otherwise)."""
        c = self.clips_of(masks.shape[0], clips)
        with torch.no_grad():
            return torch.cat([A.model_logit(self.waves(masks[i:i + per], c[i:i + per]), *self.model).view(-1)
                              for i in range(0, masks.shape[0], per)])

    def gradient(self, masks, clips=None, per=8):
        """``dF/dm [R, Fm, Tm]`` by autograd."""
        c = self.clips_of(masks.shape[0], clips)
        out = []
        for i in range(0, masks.shape[0], per):
            with torch.enable_grad():
                m = masks[i:i + per].clone().detach().requires_grad_(True)
                f = A.model_logit(self.waves(m, c[i:i + per]), *self.model)
                (g,) = torch.autograd.grad(f.sum(), m)
            out.append(g)
        return torch.cat(out)

    def flat_forward(self, Fm, Tm):
        """``[rows, Fm * Tm] -> [rows]`` for ``ablation_ref`` / ``shapley_ref`` (rows ``... * B + b``)."""
        return lambda rows: self.logit(rows.view(-1, Fm, Tm))


def istft_adjoint(mm: MaskModel, masks, clips, g_wave):
    """``d <istft_rows(m), g_wave> / dm`` by autograd: the reference of advh_istft_masked_rows_bwd."""
    with torch.enable_grad():
        m = masks.clone().detach().requires_grad_(True)
        (g,) = torch.autograd.grad((mm.waves(m, torch.as_tensor(clips).long()) * g_wave).sum(), m)
    return g


def saliency(mm, m):
    return mm.gradient(m).abs()


def input_x_gradient(mm, m):
    return m * mm.gradient(m)


def integrated_gradients(mm, m, base, n_steps=50, method="gausslegendre", multiply_by_inputs=True, internal_batch=4):
    """IG along ``b + alpha (m - b)`` (``base [1 | B, Fm, Tm]``), step-major rows ``s * B + b``.  Returns ``(attr, delta [B])``,
    ``delta = sum attr - (F(m) - F(b))`` in float64, F(b) on each clip's own spectrogram."""
    B = m.shape[0]
    b = base.expand_as(m).to(m.dtype)
    alphas, steps = BR.approximation(method, n_steps)
    total = torch.zeros_like(m)
    for s0 in range(0, n_steps, internal_batch):
        a = torch.tensor(alphas[s0:s0 + internal_batch], dtype=m.dtype)
        pts = (b[None] + a[:, None, None, None] * (m - b)[None]).reshape(-1, *m.shape[1:])
        g = mm.gradient(pts).view(len(a), *m.shape)
        total += (g * torch.tensor(steps[s0:s0 + internal_batch], dtype=m.dtype)[:, None, None, None]).sum(0)
    attr = total * (m - b) if multiply_by_inputs else total
    f = mm.logit(torch.cat([m, b])).double()
    return attr, attr.double().flatten(1).sum(1) - (f[:B] - f[B:])


def gradient_shap(mm, m, base, idx, alpha, noise, sigma, S_, multiply_by_inputs=True):
    """GradientShap fed explicit draws (``attribution_baselines_ref.gradient_shap``): expanded rows ``g = b * S + s`` of clip
    ``g // S``, ``m~ = m_b + sigma noise[g]``, ``b_g = base[idx[g]]``, ``attr = mean_s (m~ - b) dF(b + alpha (m~ - b))``."""
    B = m.shape[0]
    clips = torch.arange(B * S_) // S_
    mt = m.repeat_interleave(S_, 0) + sigma * noise.to(m.dtype).view(B * S_, *m.shape[1:])
    bt = base.to(m.dtype)[torch.as_tensor(idx).long()]
    a = torch.as_tensor(alpha, dtype=m.dtype)[:, None, None]
    g = mm.gradient(bt + a * (mt - bt), clips)
    contrib = (mt - bt) * g if multiply_by_inputs else g
    return contrib.view(B, S_, *m.shape[1:]).sum(1) / S_


def occlusion2d_shifts(Fm, Tm, window, stride):
    return math.ceil((Fm - window[0]) / stride[0]) + 1, math.ceil((Tm - window[1]) / stride[1]) + 1


def occlusion2d_cover(Fm: int, Tm: int, window, stride):
    """The windows covering each bin by the closed form advh_occlusion2d_accumulate uses: per axis the inclusive range
    ``lo = max(0, ceil((p - w + 1) / s))``, ``hi = min(K - 1, p // s)``.  Returns ``(kf_lo, kf_hi [Fm], kt_lo, kt_hi [Tm])`` int64
    arrays; bin ``(f, t)`` is covered by the windows ``kf * Kt + kt`` of the two ranges, ``(kf_hi - kf_lo + 1) * (kt_hi - kt_lo +
    1)`` of them."""
    Kf, Kt = occlusion2d_shifts(Fm, Tm, window, stride)
    out = []
    for n, w, s, K in ((Fm, window[0], stride[0], Kf), (Tm, window[1], stride[1], Kt)):
        p = np.arange(n, dtype=np.int64)
        out += [np.where(p < w, 0, (p - w + s) // s), np.minimum(K - 1, p // s)]
    return tuple(out)


def occlusion2d_masks(Fm, Tm, window, stride):
    """``[Kf * Kt, Fm, Tm]`` float32 0/1 masks, Captum's ``_occlusion_mask`` for a 2-D input: ``ones(window)`` padded by the
    shift on the left / top and cropped at the far edges; window ``k = kf * Kt + kt`` (first dimension slowest)."""
    Kf, Kt = occlusion2d_shifts(Fm, Tm, window, stride)
    masks = np.zeros((Kf * Kt, Fm, Tm), np.float32)
    for kf in range(Kf):
        for kt in range(Kt):
            masks[kf * Kt + kt, kf * stride[0]:kf * stride[0] + window[0], kt * stride[1]:kt * stride[1] + window[1]] = 1
    return masks


def occlusion2d_rows(x, base, masks):
    """``[K * B, Fm, Tm]`` float32 numpy: row ``k * B + b`` = base inside window k, ``x[b]`` elsewhere."""
    K, B = masks.shape[0], x.shape[0]
    b = np.broadcast_to(base, x.shape)
    m = np.repeat(masks, B, 0) > 0
    return np.where(m, np.tile(b, (K, 1, 1)), np.tile(x, (K, 1, 1))).astype(np.float32)


def occlusion2d_accumulate(f0, fk, masks, B):
    """Captum's ``total += diff * mask; weights += mask; total / weights`` in float32, window by window: ``[B, Fm, Tm]``."""
    K = masks.shape[0]
    fk = np.asarray(fk, np.float32).reshape(K, B)
    f0 = np.asarray(f0, np.float32)
    total = np.zeros((B,) + masks.shape[1:], np.float32)
    weights = np.zeros_like(total)
    for k in range(K):
        diff = (f0 - fk[k]).astype(np.float32)
        total += diff[:, None, None] * masks[k][None]
        weights += masks[k][None]
    return total / weights


def occlusion(mm, m, base, window, stride):
    """Captum's Occlusion of ``m [B, Fm, Tm]`` (``base`` a number or ``[1 | B, Fm, Tm]``)."""
    B, Fm, Tm = m.shape
    masks = occlusion2d_masks(Fm, Tm, window, stride)
    b = np.full((1, Fm, Tm), base, np.float32) if isinstance(base, (int, float)) else base.numpy()
    rows = torch.from_numpy(occlusion2d_rows(m.numpy(), b, masks))
    return torch.from_numpy(occlusion2d_accumulate(mm.logit(m).numpy(), mm.logit(rows).numpy(), masks, B))


def _flat_base(base, B, Fm, Tm):
    return base if isinstance(base, (int, float)) else base.reshape(base.shape[0], Fm * Tm)


def feature_ablation(mm, m, base, feature_mask):
    B, Fm, Tm = m.shape
    attr, _ = AR.feature_ablation(m.reshape(B, -1), _flat_base(base, B, Fm, Tm), feature_mask.reshape(feature_mask.shape[0], -1),
                                  forward=mm.flat_forward(Fm, Tm))
    return attr.view(B, Fm, Tm)


def tf_pool(attr, bw, sw):
    """float64 box sums ``[B, ceil(Fm / bw), ceil(Tm / sw)]``, the last box of an axis cropped."""
    a = np.asarray(attr, np.float64)
    B, Fm, Tm = a.shape
    nb, ns = -(-Fm // bw), -(-Tm // sw)
    out = np.zeros((B, nb, ns))
    for i in range(nb):
        for j in range(ns):
            out[:, i, j] = a[:, i * bw:(i + 1) * bw, j * sw:(j + 1) * sw].sum((1, 2))
    return out


def shapley_value_sampling(mm, m, base, index, perm):
    """Captum's ShapleyValueSampling over the permutations ``perm [P, K]`` of the feature ranks ``index [1 | B, Fm * Tm]``."""
    B, Fm, Tm = m.shape
    return SR.shapley(m.reshape(B, -1), _flat_base(base, B, Fm, Tm), index, perm, forward=mm.flat_forward(Fm, Tm)).view(B, Fm, Tm)
