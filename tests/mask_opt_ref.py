"""CPU restatement, in float64 torch, of the per-clip optimised mask (addvisor_hip/mask_opt.py, csrc/mask_opt.hip) for
tests/test_mask_opt_cpu.py, tests/test_gpu_mask_opt_kernels.py and tests/test_gpu_mask_opt.py: ``U`` is ``F.interpolate``
(bilinear, ``align_corners=False``), the objective is written as the module docstring of mask_opt.py states it, the rank is a
stable ``argsort``, ``grad_theta`` comes from autograd, Adam / SGD are replayed in float64.  The engine-level functions drive
``spectral_attr_ref.MaskModel.logit`` / ``.gradient`` (the oracle's classifier over the oracle's ISTFT) with the rows
``[m_0, 1 - m_0, m_1, 1 - m_1, ...]`` of clips ``[0, 0, 1, 1, ...]``."""
import math

import torch
import torch.nn.functional as F

ADAM = (0.9, 0.999, 1e-8)


def upsample(p, Fm, Tm):
    """``m = U p``: ``[B, Fc, Tc] -> [B, Fm, Tm]``."""
    return F.interpolate(p[:, None], size=(Fm, Tm), mode="bilinear", align_corners=False)[:, 0]


def ranks(theta):
    """Ascending stable rank of each clip's cells, ``[B, K]`` int64 (ties to the lower index)."""
    order = torch.argsort(theta.flatten(1), dim=1, stable=True)
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(order.shape[1]).expand_as(order))
    return rank


def template(rank, K1):
    K = rank.shape[1]
    return (rank >= K - K1).double()


def regularisers(p, rank, K1):
    """``(A, mean p, TV) [B]`` of ``p [B, Fc, Tc]``."""
    K = p.shape[1] * p.shape[2]
    A = ((p.flatten(1) - template(rank, K1)) ** 2).sum(1) / K
    tv = ((p[:, 1:] - p[:, :-1]) ** 2).sum((1, 2)) + ((p[:, :, 1:] - p[:, :, :-1]) ** 2).sum((1, 2))
    return A, p.flatten(1).mean(1), tv / K


def reward(z, kind):
    return {"logit": lambda v: v, "prob": torch.sigmoid, "log_prob": F.logsigmoid}[kind](z)


def seeds_and_history(theta, logits, sign, lam, K1, kind):
    """From the rows' logits ``[2B]`` (``2b``: mask-in, ``2b + 1``: mask-out): ``(seeds [2B], history [B, 6])``, the seeds
    ``dJ / d logit`` by autograd, the history row ``(z_in, z_out, A, mean p, TV, J)``."""
    theta, sign = theta.double(), sign.double()
    A, P, TV = regularisers(torch.sigmoid(theta), ranks(theta), K1)
    with torch.enable_grad():
        lg = logits.double().clone().requires_grad_(True)
        z_in, z_out = sign * lg[0::2], sign * lg[1::2]
        data = -lam[0] * reward(z_in, kind) + lam[1] * reward(z_out, kind)
        (seeds,) = torch.autograd.grad(data.sum(), lg)
    J = data.detach() + lam[2] * A + lam[3] * P + lam[4] * TV
    return seeds, torch.stack([z_in.detach(), z_out.detach(), A, P, TV, J], 1)


def surrogate(theta, G, lam, K1, Fm, Tm):
    """``J = <G_in, m> + <G_out, 1 - m> + lam_area A + lam_l1 mean p + lam_tv TV`` per clip ``[B]``, the rank held constant:
    its gradient is the objective's when ``G [2B, Fm, Tm]`` is the chain's vector-Jacobian product of the rows."""
    p = torch.sigmoid(theta)
    m = upsample(p, Fm, Tm)
    A, P, TV = regularisers(p, ranks(theta.detach()), K1)
    return (G[0::2] * m).sum((1, 2)) + (G[1::2] * (1 - m)).sum((1, 2)) + lam[2] * A + lam[3] * P + lam[4] * TV


def grad_theta(theta, G, lam, K1):
    """``dJ / d theta [B, Fc, Tc]`` float64 by autograd through U, the sigmoid and the regularisers."""
    with torch.enable_grad():
        t = theta.double().clone().requires_grad_(True)
        (g,) = torch.autograd.grad(surrogate(t, G.double(), lam, K1, G.shape[1], G.shape[2]).sum(), t)
    return g


def adam_replay(theta, grads):
    """torch.optim.Adam's update (defaults, bias-corrected) in float64 over the list of gradients ``grads``: yields, per step,
    ``m_hat / (sqrt(v_hat) + eps)``, which the caller multiplies by ``lr`` and subtracts."""
    b1, b2, eps = ADAM
    m, v = torch.zeros_like(theta, dtype=torch.float64), torch.zeros_like(theta, dtype=torch.float64)
    for k, g in enumerate(grads, 1):
        g = g.double()
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        yield (m / (1 - b1 ** k)) / ((v / (1 - b2 ** k)).sqrt() + eps)


def replay(theta0, grads, optimizer, lr, momentum=0.9):
    """The thetas after each of ``len(grads)`` steps of the optimiser fed the gradients ``grads``, float64."""
    th, out = theta0.double().clone(), []
    if optimizer == "adam":
        for u in adam_replay(th, grads):
            th = th - lr * u
            out.append(th)
    else:
        v = torch.zeros_like(th)
        for g in grads:
            v = momentum * v + g.double()
            th = th - lr * v
            out.append(th)
    return out


def planted_box_run(G, theta0, K1, lam, lr, steps):
    """``steps`` Adam steps on the surrogate with fixed ``G`` (the rank recomputed every step): the final ``p [B, Fc, Tc]``."""
    th, grads, t0 = theta0.double().clone(), [], theta0.double().clone()
    for _ in range(steps):
        grads.append(grad_theta(th, G, lam, K1))
        th = replay(t0, grads, "adam", lr)[-1]
    return torch.sigmoid(th)


BOX = dict(Fm=64, Tm=32, cell=(8, 4), cells=(slice(2, 5), slice(3, 6)), area=9 / 64, lam=(1.0, 1.0, 10.0, 0.0, 0.0), lr=0.1, steps=30)


def planted(make_desc):
    """The planted box of tests/test_gpu_mask_opt_kernels.py: (64, 32) with cell (8, 4) is an 8 x 8 grid; the box is the 3 x 3
    cells [2, 5) x [3, 6) = the bins [16, 40) x [12, 24), its share 9 / 64 = area, K1 = 9; ``G_in = -1`` inside the box and +1
    outside, ``G_out = 0``; two clips from a start of 0.01 N(0, 1) around theta = 0.  ``make_desc`` builds the descriptor.
    Returns ``(desc, G [4, 64, 32], theta0 [2, 8, 8], the box's cells [8, 8] bool)``."""
    d = make_desc(BOX["Fm"], BOX["Tm"], BOX["cell"], lam=BOX["lam"], area=BOX["area"], optimizer="adam", lr=BOX["lr"], clips=2)
    G = torch.ones(4, BOX["Fm"], BOX["Tm"])
    G[0::2, 16:40, 12:24] = -1.0
    G[1::2] = 0.0
    theta0 = 0.01 * torch.randn((2, 8, 8), generator=torch.Generator().manual_seed(9))
    want = torch.zeros(8, 8, dtype=torch.bool)
    want[BOX["cells"]] = True
    return d, G, theta0, want


# ------------------------------------------------------------------------------------------------- over spectral_attr_ref.MaskModel
def rows_of(theta, Fm, Tm):
    """``[2B, Fm, Tm]`` float64: rows ``2b`` = m_b, ``2b + 1`` = 1 - m_b; and their clips."""
    m = upsample(torch.sigmoid(theta.double()), Fm, Tm)
    rows = torch.stack([m, 1 - m], 1).reshape(-1, Fm, Tm)
    return rows, torch.arange(rows.shape[0]) // 2


def model_step(mm, theta, sign, lam, K1, kind, Fm, Tm):
    """One evaluation at ``theta`` on the restated model: ``(grad_theta [B, Fc, Tc], seeds [2B], logits [2B], history [B, 6])``."""
    rows, clips = rows_of(theta, Fm, Tm)
    r32 = rows.float()
    logits = mm.logit(r32, clips).double()
    seeds, hist = seeds_and_history(theta, logits, sign, lam, K1, kind)
    G = seeds[:, None, None] * mm.gradient(r32, clips).double()
    return grad_theta(theta, G, lam, K1), seeds, logits, hist


def sgd_run(mm, theta0, sign, lam, K1, kind, Fm, Tm, lr, steps):
    """Free-running SGD (momentum 0): ``(thetas after each step, histories [steps, B, 6])``."""
    th, thetas, hist = theta0.double().clone(), [], []
    for _ in range(steps):
        g, _, _, h = model_step(mm, th, sign, lam, K1, kind, Fm, Tm)
        th = th - lr * g
        thetas.append(th)
        hist.append(h)
    return thetas, torch.stack(hist)


def ranked_cells(area, K):
    return int(math.floor(area * K + 0.5))
