"""fp64 restatement of the embedder's row operations and waveform front end, for the kernel-level tests
(tests/test_gpu_rowops.py, tests/test_gpu_frontend.py, the attention tests of tests/test_gpu_split.py).

Plain torch, written from the call sites of oracle/wav2vec2_ref.py and from the formulas -- not from the kernels.  Every
function computes in float64 whatever dtype it is handed and is differentiable, so ``torch.autograd`` through it is the
reference of the backward kernels.  tests/test_embedder_ops_ref_cpu.py pins it against the fp32 oracle.
"""
import math

import torch
import torch.nn.functional as F

K0, S0 = 10, 5                      # kernel / stride of feature-encoder layer 0 (every wav2vec2 config)


def gelu(x):
    """Exact (erf) GELU: x * Phi(x)."""
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(z):
    """d/dz GELU(z) = Phi(z) + z * phi(z)."""
    z = z.double()
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def layernorm(x, gamma, beta, eps, add=None, act=False):
    """LayerNorm over the last dim of ``x (+ add)``: biased variance, eps inside the sqrt, affine, optional GELU."""
    x = x.double() if add is None else x.double() + add.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    return gelu(y) if act else y


def pool_logreg(h, coef, intercept):
    """h [B, T, H] -> (logit [B], prob [B], pooled [B, H]): time mean, Linear(H, 1), sigmoid."""
    pooled = h.double().mean(1)
    logit = pooled @ coef.double() + float(intercept)
    return logit, torch.sigmoid(logit), pooled


def pad_or_crop(wave, L):
    """[B, n] -> [B, L]: zero-pad the tail or crop."""
    n = wave.shape[-1]
    return wave[..., :L] if n >= L else F.pad(wave, (0, L - n))


def normalise(x, normalize=True):
    """(x - mean) / (std_unbiased + 1e-7) per clip, and what the kernel saves: (mean, 1 / (std + 1e-7)).  Identity when
    ``normalize`` is off (stats = (0, 1))."""
    x = x.double()
    if not normalize:
        return x, torch.zeros(x.shape[0], dtype=torch.float64), torch.ones(x.shape[0], dtype=torch.float64)
    mean = x.mean(-1, keepdim=True)
    std = torch.sqrt(((x - mean) ** 2).sum(-1, keepdim=True) / (x.shape[-1] - 1))
    rho = 1.0 / (std + 1e-7)
    return (x - mean) * rho, mean[:, 0], rho[:, 0]


def conv0(xhat, w0):
    """Conv1d(1 -> C0, k = 10, s = 5) without bias: [B, L] x [C0, 10] -> [B, T0, C0] (channels last)."""
    return F.conv1d(xhat.double()[:, None], w0.double().view(-1, 1, K0), stride=S0).transpose(1, 2)


def frontend_tail(z0, mode, gamma=None, beta=None, bias=None):
    """What follows the convolution.  mode 0: per-channel GroupNorm over the T0 frames (biased variance, eps 1e-5, affine) and
    GELU; mode 1: + bias (which may be absent).  Returns (out, mean_c, rstd_c); the last two are None in mode 1."""
    if mode == 1:
        return (z0 if bias is None else z0 + bias.double()), None, None
    mean_c = z0.mean(1, keepdim=True)
    var_c = ((z0 - mean_c) ** 2).mean(1, keepdim=True)
    rstd_c = 1.0 / torch.sqrt(var_c + 1e-5)
    return gelu((z0 - mean_c) * rstd_c * gamma.double() + beta.double()), mean_c[:, 0], rstd_c[:, 0]


def frontend(wave, L, w0, mode, normalize=True, gamma=None, beta=None, bias=None):
    """The waveform front end: pad / crop to L, clip normaliser, conv0, then ``frontend_tail``.
    Returns a dict: out [B, T0, C0], z0 (the convolution output), xhat, stats = (mean, 1 / (std + 1e-7)) [B, 2] and, in
    mode 0, mr = (mean_c, rstd_c) [B, C0, 2]."""
    x = pad_or_crop(wave.double(), L)
    xhat, mean, rho = normalise(x, normalize)
    z0 = conv0(xhat, w0)
    out, mean_c, rstd_c = frontend_tail(z0, mode, gamma, beta, bias)
    return {"out": out, "z0": z0, "xhat": xhat, "stats": torch.stack([mean, rho], -1),
            "mr": None if mean_c is None else torch.stack([mean_c, rstd_c], -1)}


def attention(q, k, v):
    """softmax(Q K^T / sqrt(d)) V on [..., T, d]; also returns the probabilities."""
    p = torch.softmax(q.double() @ k.double().transpose(-1, -2) / math.sqrt(q.shape[-1]), -1)
    return p @ v.double(), p
