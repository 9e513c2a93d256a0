"""CPU restatement of the baseline-aware attributions (IntegratedGradients with a baseline and a Riemann / Gauss-Legendre
rule, GradientShap) and of the counter-based noise generator, for tests/test_attribution_baselines_cpu.py and
tests/test_gpu_attribution_baselines.py.  Built on ``oracle.attribution_ref.input_gradient`` / ``model_logit`` (fp32
autograd on the CPU); parity with Captum is unpinned (captum is absent): the formulas are restated from Captum's
``approximation_methods.py``, ``IntegratedGradients``, ``GradientShap`` and from Salmon et al., SC'11 (Philox)."""
import numpy as np
import torch

from oracle import attribution_ref as A

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr: np.ndarray, k0: int, k1: int) -> np.ndarray:
    """Philox4x32-10 on ``ctr [N, 4]`` uint32 words, integer arithmetic in uint64."""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(k0 & MASK), np.uint64(k1 & MASK)
    for i in range(10):
        if i:
            k0, k1 = (k0 + np.uint64(W0)) & np.uint64(MASK), (k1 + np.uint64(W1)) & np.uint64(MASK)
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return np.stack(c, 1).astype(np.uint32)


def philox_words(seed: int, row0: int, rows: int, n: int) -> np.ndarray:
    """``[rows, ceil(n/4), 4]`` raw words of the counters (j/4, row lo, row hi, 0) under key (seed lo, seed hi)."""
    nq = -(-n // 4)
    g = np.repeat(np.arange(row0, row0 + rows, dtype=np.uint64), nq)
    q = np.tile(np.arange(nq, dtype=np.uint64), rows)
    ctr = np.stack([q & np.uint64(MASK), g & np.uint64(MASK), g >> np.uint64(32), np.zeros_like(g)], 1).astype(np.uint32)
    return philox4x32_10(ctr, seed & MASK, seed >> 32).reshape(rows, nq, 4)


def philox_normal(seed: int, row0: int, rows: int, n: int) -> np.ndarray:
    """float64 Box-Muller on the words: u = (2 (w >> 9) + 1) 2^-24, z = sqrt(-2 ln u_a) (cos, sin)(2 pi u_b)."""
    w = philox_words(seed, row0, rows, n)
    u = ((w >> np.uint32(9)).astype(np.float64) * 2 + 1) * 2.0 ** -24
    ra, rb = np.sqrt(-2 * np.log(u[..., 0])), np.sqrt(-2 * np.log(u[..., 2]))
    ta, tb = 2 * np.pi * u[..., 1], 2 * np.pi * u[..., 3]
    z = np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], -1)
    return z.reshape(rows, -1)[:, :n]


def approximation(method: str, n: int):
    """Captum's approximation tables, restated: (alphas, step sizes)."""
    if method == "gausslegendre":
        x, w = np.polynomial.legendre.leggauss(n)
        return 0.5 * (1 + x), 0.5 * w
    steps = np.full(n, 1.0 / n)
    if method == "riemann_trapezoid":
        steps[0] /= 2
        steps[-1] /= 2
        return np.linspace(0, 1, n), steps
    return {"riemann_left": np.linspace(0, 1 - 1 / n, n), "riemann_middle": np.linspace(1 / (2 * n), 1 - 1 / (2 * n), n),
            "riemann_right": np.linspace(1 / n, 1, n)}[method], steps


def integrated_gradients(x, base, model, n_steps=50, method="gausslegendre", multiply_by_inputs=True, internal_batch=8):
    """IG with a baseline ``[1, L]`` / ``[B, L]``: path points b + alpha (x - b) step-major, weighted gradient sum,
    times (x - b).  Returns ``(attr, delta [B])``, ``delta = sum attr - (F(x) - F(b))`` (float64)."""
    B, L = x.shape
    b = base.expand(B, L).to(x.dtype)
    alphas, steps = approximation(method, n_steps)
    total = torch.zeros_like(x)
    for s0 in range(0, n_steps, internal_batch):
        a = torch.tensor(alphas[s0:s0 + internal_batch], dtype=x.dtype)
        pts = (b[None] + a[:, None, None] * (x - b)[None]).reshape(-1, L)
        g = A.input_gradient(pts, *model).view(len(a), B, L)
        total += (g * torch.tensor(steps[s0:s0 + internal_batch], dtype=x.dtype)[:, None, None]).sum(0)
    attr = total * (x - b) if multiply_by_inputs else total
    with torch.no_grad():
        f = A.model_logit(torch.cat([x, b]), *model).double().view(-1)
    return attr, attr.double().sum(1) - (f[:B] - f[B:])


def gradient_shap(x, base, idx, alpha, noise, sigma, S, model, multiply_by_inputs=True, internal_batch=8):
    """GradientShap fed explicit draws: expanded rows g = b S + s, x~ = x_b + sigma noise[g], b_g = base[idx[g]],
    attr = mean_s (x~ - b) dF(b + alpha (x~ - b)).  Returns ``(attr, delta [B S])`` with
    ``delta[g] = sum_j (x~ - b)_j dF_j - (F(x~) - F(b))`` (float64)."""
    B, L = x.shape
    xt = x.repeat_interleave(S, 0) + sigma * noise.to(x.dtype)
    bt = base.to(x.dtype)[torch.as_tensor(idx).long()]
    a = torch.as_tensor(alpha, dtype=x.dtype)[:, None]
    pts = bt + a * (xt - bt)
    g = torch.cat([A.input_gradient(pts[i:i + internal_batch], *model) for i in range(0, B * S, internal_batch)])
    contrib = (xt - bt) * g
    attr = (contrib if multiply_by_inputs else g).view(B, S, L).sum(1) / S
    with torch.no_grad():
        fx = torch.cat([A.model_logit(xt[i:i + internal_batch], *model) for i in range(0, B * S, internal_batch)]).double().view(-1)
        fb = A.model_logit(base.to(x.dtype), *model).double().view(-1)[torch.as_tensor(idx).long()]
    return attr, contrib.double().sum(1) - (fx - fb)
