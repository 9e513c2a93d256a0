"""Plain float64 restatements (numpy) of the U-Net decoder's training kernels (csrc/unet_train.hip, csrc/unet_misc.hip):
training-mode BatchNorm2d around LeakyReLU with its running buffers and its backward, the gather / transpose index map
of ``advh_transpose_desc``, the mask head with its backward and its 33 sums, the 1-channel stem with its and the skip
channel's weight gradients, and ``pack_x``.  Nothing of the product is imported.  Two fp32 BatchNorms (two-pass and
one-pass) stand next to the fp64 one: the first sets the tolerance bars, the second shows that the bars are sharp.

Maps are channels-last ``[B][H + 2 PH][W + 2 PW][C]``; every function below takes the INTERIOR ``[B][H][W][C]``."""
import numpy as np

F32 = np.float32


def interior(m, PH, PW):
    return m[:, PH:m.shape[1] - PH, PW:m.shape[2] - PW, :]


def split_round(x):
    """The value a split-format plane pair holds for x (csrc/device_math.h): hi = fp16(x) (0 below 2^-14),
    lo = fp16((x - hi) * 2048), joined as the kernels join them: hi + lo / 2048 rounded to fp32."""
    x = np.asarray(x, np.float64)
    hi = x.astype(np.float16).astype(np.float64)
    hi = np.where(np.abs(x) < 2.0 ** -14, 0.0, hi)
    lo = ((x - hi) * 2048.0).astype(np.float16).astype(np.float64)
    return (hi + lo / 2048.0).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------ BatchNorm, fp64
def bn_forward(zi, gamma, beta, eps, slope):
    """-> coef [4][C] = [scale | shift | mean | invstd], biased variance, pre-activation y, activation lrelu(y)."""
    z = np.asarray(zi, np.float64)
    C = z.shape[-1]
    z2 = z.reshape(-1, C)
    mean = z2.mean(0)
    var = ((z2 - mean) ** 2).mean(0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    y = (z - mean) * invstd * gamma + beta
    return np.stack([scale, shift, mean, invstd]), var, y, np.where(y > 0, y, slope * y)


def bn_running(rmean, rvar, nbt, mean, var, n, momentum):
    """nn.BatchNorm2d's train() update: momentum on the batch value, unbiased variance, counter + 1."""
    unbiased = var * (n / max(n - 1.0, 1.0))
    return (1.0 - momentum) * rmean + momentum * mean, (1.0 - momentum) * rvar + momentum * unbiased, nbt + 1


def bn_backward(zi, g, coef, slope, inv_scale, positive=None):
    """The header's backward: dy^ = g * lrelu'(y), z^ = (z - mean) * invstd, coef_b = [k1 | m1 | m2] =
    [scale | mean dy^ | mean dy^ z^], dz = k1 (dy^ - m1 - z^ m2), dgamma = sum dy^ z^ * inv_scale, dbeta = sum dy^ * inv_scale.
    ``positive``: the LeakyReLU branch per element (default: the sign of the fp64 pre-activation)."""
    z, g = np.asarray(zi, np.float64), np.asarray(g, np.float64)
    scale, shift, mean, invstd = (np.asarray(r, np.float64) for r in coef)
    C = z.shape[-1]
    if positive is None:
        positive = scale * z + shift > 0
    dyh = g * np.where(positive, 1.0, slope)
    zh = (z - mean) * invstd
    s1, s2 = dyh.reshape(-1, C).sum(0), (dyh * zh).reshape(-1, C).sum(0)
    n = z.size // C
    coef_b = np.stack([scale, s1 / n, s2 / n])
    dz = coef_b[0] * (dyh - coef_b[1] - zh * coef_b[2])
    absum = np.stack([np.abs(dyh).reshape(-1, C).sum(0), np.abs(dyh * zh).reshape(-1, C).sum(0)])      # magnitudes of the two sums' terms
    terms = np.abs(coef_b[0]) * (np.abs(dyh) + np.abs(coef_b[1]) + np.abs(zh * coef_b[2]))              # ... and of dz's three terms
    return dict(sums=np.stack([s1, s2]), coef_b=coef_b, dz=dz, dgamma=s2 * inv_scale, dbeta=s1 * inv_scale, abs=absum, dz_terms=terms)


# ------------------------------------------------------------------------------------------------------ BatchNorm, fp32
def _f32_coef(mean, var, gamma, beta, eps):
    invstd = (F32(1.0) / np.sqrt(var + F32(eps))).astype(F32)
    scale = (gamma.astype(F32) * invstd).astype(F32)
    shift = (beta.astype(F32) - mean * scale).astype(F32)
    return np.stack([scale, shift, mean, invstd]).astype(F32)


def _f32_apply(z, coef, slope):
    y = (coef[0] * z + coef[1]).astype(F32)
    return np.where(y > 0, y, F32(slope) * y).astype(F32)


def _rows(a):
    """[...][C] -> contiguous [C][n], so that numpy's sum over the last axis is its pairwise one."""
    return np.ascontiguousarray(a.reshape(-1, a.shape[-1]).T)


def bn_forward_f32_two_pass(zi, gamma, beta, eps, slope):
    """Every operation in fp32 (numpy's pairwise sums): mean, then the sum of squared deviations from it."""
    z = np.asarray(zi, F32)
    z2 = _rows(z)
    n = F32(z2.shape[1])
    mean = (z2.sum(1, dtype=F32) / n).astype(F32)
    d = (z2 - mean[:, None]).astype(F32)
    var = ((d * d).sum(1, dtype=F32) / n).astype(F32)
    coef = _f32_coef(mean, var, gamma, beta, eps)
    return coef, var, _f32_apply(z, coef, slope)


def bn_forward_f32_one_pass(zi, gamma, beta, eps, slope):
    """Every operation in fp32: var = max(sum z^2 / n - mean^2, 0), the form the kernel had."""
    z = np.asarray(zi, F32)
    z2 = _rows(z)
    n = F32(z2.shape[1])
    mean = (z2.sum(1, dtype=F32) / n).astype(F32)
    var = np.maximum(((z2 * z2).sum(1, dtype=F32) / n).astype(F32) - mean * mean, F32(0)).astype(F32)
    coef = _f32_coef(mean, var, gamma, beta, eps)
    return coef, var, _f32_apply(z, coef, slope)


def bn_backward_f32(zi, g, coef, slope, inv_scale, positive):
    """bn_backward with every operation in fp32 (two-pass in the sense of the forward: mean and invstd are given)."""
    z, g = np.asarray(zi, F32), np.asarray(g, F32)
    scale, shift, mean, invstd = (np.asarray(r, F32) for r in coef)
    C = z.shape[-1]
    dyh = (g * np.where(positive, F32(1.0), F32(slope))).astype(F32)
    zh = ((z - mean) * invstd).astype(F32)
    s1, s2 = _rows(dyh).sum(1, dtype=F32), _rows((dyh * zh).astype(F32)).sum(1, dtype=F32)
    n = F32(z.size // C)
    coef_b = np.stack([scale, s1 / n, s2 / n]).astype(F32)
    dz = (coef_b[0] * (dyh - coef_b[1] - (zh * coef_b[2]).astype(F32))).astype(F32)
    return dict(sums=np.stack([s1, s2]), coef_b=coef_b, dz=dz, dgamma=(s2 * F32(inv_scale)).astype(F32), dbeta=(s1 * F32(inv_scale)).astype(F32))


# ------------------------------------------------------------------------------------------------------ transpose_gather
def transpose_gather(src, d, dst):
    """``src`` [B][Hs + 2 PHs][Ws + 2 PWs][Cs], ``d`` a dict with the fields of advh_transpose_desc, ``dst`` [rows][ld] (a copy
    is returned): dst[t*rpt + r0 + c][col0 + p] = src[b][PHs + y][PWs + x][c0 + c], p = (b*Hg + hg)*Wg + wg,
    (y, x) = (sy*(hg - GH) + oy[t], sx*(wg - GW) + ox[t]); zero where (y, x) lies outside the source interior."""
    dst = np.array(dst, copy=True)
    B, Hg, Wg = d["B"], d["Hg"], d["Wg"]
    b, hg, wg = np.meshgrid(np.arange(B), np.arange(Hg), np.arange(Wg), indexing="ij")
    p = ((b * Hg + hg) * Wg + wg).ravel()
    b, hg, wg = b.ravel(), hg.ravel(), wg.ravel()
    for t in range(d["ntap"]):
        y = d["sy"] * (hg - d["GH"]) + d["oy"][t]
        x = d["sx"] * (wg - d["GW"]) + d["ox"][t]
        ok = (y >= 0) & (y < d["Hs"]) & (x >= 0) & (x < d["Ws"])
        v = np.zeros((p.size, d["nC"]), src.dtype)
        v[ok] = src[b[ok], y[ok] + d["PHs"], x[ok] + d["PWs"], d["c0"]:d["c0"] + d["nC"]]
        r = t * d["rpt"] + d["r0"]
        dst[r:r + d["nC"], d["col0"] + p] = v.T
    return dst


# ------------------------------------------------------------------------------------------------------ head
def head(yi, w32, bias):
    """-> (mask, logits) [B][H][W]: sigmoid(sum_c y w + bias)."""
    logits = np.asarray(yi, np.float64) @ np.asarray(w32, np.float64) + bias
    return 1.0 / (1.0 + np.exp(-logits)), logits


def head_bwd(dmask, mask, w32, scale):
    """-> (dlogit [total], dy1 [total][32])."""
    dmask, mask = np.asarray(dmask, np.float64).ravel(), np.asarray(mask, np.float64).ravel()
    dlogit = dmask * mask * (1.0 - mask)
    return dlogit, scale * dlogit[:, None] * np.asarray(w32, np.float64)[None, :]


def head_wgrad(dlogit, y1):
    """The 33 sums: dw[c] = sum_i dlogit[i] y1[i][c], dw[32] = sum_i dlogit[i]."""
    dlogit, y1 = np.asarray(dlogit, np.float64).ravel(), np.asarray(y1, np.float64).reshape(-1, 32)
    return np.concatenate([dlogit @ y1, [dlogit.sum()]])


# ------------------------------------------------------------------------------------------------------ stem, skip, pack
def _windows(mag, H, W, KH, KW, sh, ph, pw):
    """The cropped magnitude's [B][Ho][W][KH*KW] windows of a (KH, KW) kernel, stride (sh, 1), zero padding (ph, pw)."""
    x = np.asarray(mag, np.float64)[:, :H, :W]
    xp = np.pad(x, ((0, 0), (ph, ph), (pw, pw)))
    Ho = (H + 2 * ph - KH) // sh + 1
    return np.stack([xp[:, kh:kh + sh * (Ho - 1) + 1:sh, kw:kw + W] for kh in range(KH) for kw in range(KW)], -1)


def stem(mag, H, W, wgt, bias, slope):
    """Conv2d(1, 32, (5, 3), stride (2, 1), padding (2, 1)) + LeakyReLU on the H x W crop -> [B][H/2][W][32]."""
    y = _windows(mag, H, W, 5, 3, 2, 2, 1) @ np.asarray(wgt, np.float64).reshape(32, 15).T + np.asarray(bias, np.float64)
    return np.where(y > 0, y, slope * y)


def stem_wgrad(dzi, mag, H, W):
    """dW[co][kh*3 + kw] = sum dz[b][ho][w][co] mag[b][2 ho + kh - 2][w + kw - 1]; dzi [B][H/2][W][32] -> [32][15]."""
    return np.einsum("bhwc,bhwk->ck", np.asarray(dzi, np.float64), _windows(mag, H, W, 5, 3, 2, 2, 1))


def skip_wgrad(dzi, mag, H, W):
    """dW[co][kh*3 + kw] = sum dz[b][h][w][co] mag[b][h + kh - 1][w + kw - 1]; dzi [B][H][W][32] -> [32][9]."""
    return np.einsum("bhwc,bhwk->ck", np.asarray(dzi, np.float64), _windows(mag, H, W, 3, 3, 1, 1, 1))


def pack_x(mag, H, W, cat, c0, PH, PW):
    """Channels [c0, c0 + 8) of the interior of ``cat`` <- (x, 1, 0, 0, 0, 0, 0, 0); everything else is kept."""
    cat = np.array(cat, np.float64, copy=True)
    it = interior(cat, PH, PW)
    it[..., c0:c0 + 8] = 0.0
    it[..., c0] = np.asarray(mag, np.float64)[:, :H, :W]
    it[..., c0 + 1] = 1.0
    return cat
