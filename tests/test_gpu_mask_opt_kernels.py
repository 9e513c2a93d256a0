"""GPU: the three kernels of csrc/mask_opt.hip on their own operands (no embedder) against the float64 restatement of
tests/mask_opt_ref.py, at the smallest geometries that reach every branch:

    (513, 50), cell (16, 4)   -> grid (33, 13): a non-integer scale on both axes, the scalar body (Tm % 4 != 0)
    (512, 48), cell (64, 8)   -> grid (8, 6): an integer scale, the float4 body
    (16, 12),  cell (1, 1)    -> the identity
    (513, 50), cell (600, 60) -> one cell, Fc = Tc = 1 (one wavefront walks the whole map)
    B = 3 with b0 = 1, nb = 2 -> a clip subset;  an output pointer offset by one float -> the scalar body at Tm % 4 == 0."""
import pytest
import torch
import torch.nn.functional as F

import mask_opt_ref as R
from addvisor_hip import attribution as AT, mask_opt as MO

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

GEOS = {"noninteger": (513, 50, (16, 4)), "integer": (512, 48, (64, 8)), "identity": (16, 12, (1, 1)), "one_cell": (513, 50, (600, 60))}
B = 3
LAM_ALL = (1.5, 0.75, 3.0, 0.5, 2.0)
LAM_DATA = (1.0, 1.0, 0.0, 0.0, 0.0)


def make_desc(Fm, Tm, cell, lam=LAM_ALL, area=0.25, reward="log_prob", optimizer="sgd", lr=0.05, momentum=0.9, clips=B):
    Fc, Tc = MO.coarse_grid(Fm, Tm, cell)
    return MO.MaskOptDesc(clips, Fm, Tm, Fc, Tc, MO.ranked_cells(area, Fc * Tc), MO.REWARDS.index(reward), MO.OPTIMIZERS.index(optimizer),
                          *lam, lr, *MO.ADAM, momentum)


def draw(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def operands(d, dev, seed=0):
    """theta (a normal draw: no ties), G [2B, n], logits [2B] and signs [B] (both signs present)."""
    theta = draw((d.B, d.Fc, d.Tc), 100 + seed, 1.5)
    G = draw((2 * d.B, d.Fm * d.Tm), 200 + seed)
    logits = draw((2 * d.B,), 300 + seed, 2.0)
    sign = torch.tensor([1.0, -1.0, 1.0][:d.B])
    return tuple(t.to(dev).contiguous() for t in (theta, G, logits, sign))


def launch(d, theta, G, logits, sign, step=1, m1=None, m2=None, b0=0, nb=None):
    """rank -> terms -> step on the clips ``b0 .. b0 + nb - 1`` (``G`` / ``logits`` chunk-local): theta, m1, m2 updated in place;
    returns ``(grad_theta [B, K], p [B, K], seeds [2 nb], hist [B, 6])``."""
    nb = d.B if nb is None else nb
    K = d.Fc * d.Tc
    f32 = dict(dtype=torch.float32, device=theta.device)
    rank = AT.feature_rank(theta.view(d.B, K), False)
    p, seeds, hist, grad = torch.zeros((d.B, K), **f32), torch.zeros(2 * nb, **f32), torch.zeros((d.B, 6), **f32), torch.zeros((d.B, K), **f32)
    m1 = torch.zeros((d.B, K), **f32) if m1 is None else m1
    m2 = torch.zeros((d.B, K), **f32) if m2 is None else m2
    MO.mask_terms(d, theta, rank, sign, logits, b0, nb, p, seeds, hist)
    MO.mask_step(d, theta, p, rank, G, b0, nb, step, m1, m2, grad)
    return grad, p, seeds, hist


# ----------------------------------------------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("geo", list(GEOS))
def test_rows_against_the_restatement(gpu_device, geo):
    """<= 1e-6 absolute (values in [0, 1]; a sigmoid and six fp32 roundings); row 2j + 1 is 1 - row 2j bit for bit."""
    d = make_desc(*GEOS[geo])
    theta = operands(d, gpu_device)[0]
    rows = MO.mask_rows(d, theta, 0, B).cpu()
    ref, _ = R.rows_of(theta.cpu(), d.Fm, d.Tm)
    err = (rows.double() - ref.flatten(1)).abs().max().item()
    print(f"rows [{geo}]: max |err| = {err:.3e}")
    assert rows.shape == (2 * B, d.Fm * d.Tm) and err <= 1e-6
    assert torch.equal(rows[1::2], 1.0 - rows[0::2])
    if geo == "identity":                                                # U is exact there: the rows are the kernels' own sigmoid
        assert torch.equal(rows[0::2].view(B, d.Fc, d.Tc), MO.coarse_of(theta).cpu())


@pytest.mark.parametrize("geo", ["noninteger", "integer"])
def test_rows_of_a_clip_subset_and_of_an_unaligned_output(gpu_device, geo):
    """Clips 1 .. 2 of 3 give the bits of rows 2 .. 5 of the whole batch; an output offset by one float (the scalar body, also at
    Tm % 4 == 0) gives the bits of the aligned one."""
    d = make_desc(*GEOS[geo])
    theta = operands(d, gpu_device)[0]
    n = d.Fm * d.Tm
    full = MO.mask_rows(d, theta, 0, B)
    assert torch.equal(MO.mask_rows(d, theta, 1, 2), full[2:])
    buf = torch.full((4 * n + 2,), -7.0, device=gpu_device)
    off = buf[1:1 + 4 * n].view(4, n)
    assert off.data_ptr() % 16 == 4
    MO.mask_rows(d, theta, 1, 2, off)
    assert torch.equal(off, full[2:]) and float(buf[0]) == -7.0 and float(buf[-1]) == -7.0


# ------------------------------------------------------------------------------------------------------------------ the adjoint
@pytest.mark.parametrize("geo", list(GEOS))
def test_rows_and_step_are_adjoint(gpu_device, geo):
    """``<U p, G> = <p, U^T G>``: ``U p`` from the rows kernel, ``U^T G`` from ``grad_theta`` with the regularisers off and the
    factor ``p (1 - p)`` divided out on the host in float64; both sums in float64.  <= 1e-6 of ``sum |p . U^T G|``."""
    d = make_desc(*GEOS[geo], lam=LAM_DATA)
    theta, G, logits, sign = operands(d, gpu_device, 1)
    G[1::2] = 0                                                          # G_in - G_out = G_in
    Up = MO.mask_rows(d, theta, 0, B)[0::2].cpu().double()
    grad, p, _, _ = launch(d, theta.clone(), G, logits, sign)
    p = p.cpu().double()
    UtG = grad.cpu().double() / (p * (1 - p))
    lhs, rhs = (Up * G[0::2].cpu().double()).sum().item(), (p * UtG).sum().item()
    scale = (p * UtG).abs().sum().item()
    print(f"adjoint [{geo}]: <Up, G> = {lhs:.9e}, <p, UtG> = {rhs:.9e}, |diff| / scale = {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= 1e-6 * scale


# ----------------------------------------------------------------------------------------------------------------- grad_theta
@pytest.mark.parametrize("geo", list(GEOS))
def test_grad_theta_against_the_restatement(gpu_device, geo):
    """Every lambda non-zero: <= 1e-5 of max |ref| and cosine >= 0.999999 (an fp32 sum of at most 248 products and a tree at
    cell (16, 4)); the clip subset writes its own clips only."""
    d = make_desc(*GEOS[geo])
    theta, G, logits, sign = operands(d, gpu_device, 2)
    ref = R.grad_theta(theta.cpu(), G.cpu().view(2 * B, d.Fm, d.Tm), LAM_ALL, d.K1).flatten(1)
    grad = launch(d, theta.clone(), G, logits, sign)[0].cpu().double()
    err = ((grad - ref).abs().max() / ref.abs().max()).item()
    cos = F.cosine_similarity(grad.flatten(), ref.flatten(), dim=0).item()
    print(f"grad_theta [{geo}]: max err / max |ref| = {err:.3e}, cosine {cos:.9f}")
    assert err <= 1e-5 and cos >= 0.999999
    th = theta.clone()
    sub = launch(d, th, G[2:].contiguous(), logits[2:].contiguous(), sign, b0=1, nb=2)[0].cpu().double()
    assert torch.equal(sub[1:], grad[1:]) and not bool(sub[0].any()) and torch.equal(th[0], theta[0]) and not torch.equal(th[1:], theta[1:])


# ------------------------------------------------------------------------------------------------------------------ the update
@pytest.mark.parametrize("optimizer", MO.OPTIMIZERS)
@pytest.mark.parametrize("geo", ["noninteger", "integer"])
def test_update_replayed_from_the_device_gradient(gpu_device, geo, optimizer):
    """Three consecutive steps; the float64 replay is fed the device's own ``grad_theta`` (Adam's ``g / (sqrt(v) + eps)`` is a
    sign function where g ~ 0 and would amplify gradient noise otherwise): ``|theta' - ref| <= 1e-6 max(1, |ref|)``."""
    d = make_desc(*GEOS[geo], optimizer=optimizer, lr=0.05, momentum=0.9)
    theta, G, logits, sign = operands(d, gpu_device, 3)
    theta0, K = theta.cpu().clone(), d.Fc * d.Tc
    m1, m2 = torch.zeros((B, K), device=gpu_device), torch.zeros((B, K), device=gpu_device)
    grads, thetas = [], []
    for k in range(3):
        grads.append(launch(d, theta, G, logits, sign, k + 1, m1, m2)[0].cpu().view(B, d.Fc, d.Tc))
        thetas.append(theta.cpu().clone())
    worst = 0.0
    for k, ref in enumerate(R.replay(theta0, grads, optimizer, 0.05, 0.9)):
        excess = ((thetas[k].double() - ref).abs() / ref.abs().clamp(min=1)).max().item()
        worst = max(worst, excess)
        assert excess <= 1e-6, (k, excess)
        assert not torch.equal(thetas[k], theta0)
    print(f"{optimizer} [{geo}]: max |theta' - ref| / max(1, |ref|) over 3 steps = {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------------- the terms
@pytest.mark.parametrize("reward", MO.REWARDS)
@pytest.mark.parametrize("geo", ["noninteger", "one_cell"])
def test_terms_against_the_restatement(gpu_device, geo, reward):
    """The history row ``(z_in, z_out, A, mean p, TV, J)`` and the seeds: ``|err| <= 1e-6 max(1, |ref|)`` (means of values in
    [0, 1], logits and rewards of order one); both signs of s are among the three clips."""
    d = make_desc(*GEOS[geo], reward=reward)
    theta, G, logits, sign = operands(d, gpu_device, 4)
    _, p, seeds, hist = launch(d, theta.clone(), G, logits, sign)
    rs, rh = R.seeds_and_history(theta.cpu(), logits.cpu(), sign.cpu(), LAM_ALL, d.K1, reward)
    for name, ours, ref in (("history", hist.cpu().double(), rh), ("seeds", seeds.cpu().double(), rs),
                            ("p", p.cpu().double(), torch.sigmoid(theta.cpu().double()).flatten(1))):
        err = ((ours - ref).abs() / ref.abs().clamp(min=1)).max().item()
        print(f"terms [{geo}, {reward}] {name}: {err:.3e}")
        assert err <= 1e-6, (name, err)
    assert bool((sign.cpu() < 0).any()) and bool((sign.cpu() > 0).any()) and bool((rs != 0).all())


# ------------------------------------------------------------------------------------------------------------- the planted box
BOX = R.BOX


def planted_run(dev):
    d, G, theta0, _ = R.planted(make_desc)
    theta, G = theta0.to(dev).contiguous(), G.flatten(1).to(dev).contiguous()
    logits, sign = torch.tensor([1.0, -0.5, 2.0, 0.25], device=dev), torch.ones(2, device=dev)
    m1, m2 = torch.zeros((2, 64), device=dev), torch.zeros((2, 64), device=dev)
    for k in range(BOX["steps"]):
        MO.mask_rows(d, theta, 0, 2)
        launch(d, theta, G, logits, sign, k + 1, m1, m2)
    return theta


def test_planted_box_is_recovered_and_two_runs_are_bit_identical(gpu_device):
    """rank -> rows -> terms -> step on the planted box of ``mask_opt_ref.planted`` -- (64, 32) with cell (8, 4), the 3 x 3 cells
    [2, 5) x [3, 6), area 9 / 64, lam_area = 10, Adam at lr = 0.1, 30 steps, values for which the float64 restatement alone meets
    the condition (tests/test_mask_opt_cpu.py checks that): ``{p > 0.5}`` is the box's cells, the share of such cells is K1 / K
    exactly, and a second run gives the same bits."""
    d, _, _, want = R.planted(make_desc)
    theta = planted_run(gpu_device)
    p = MO.coarse_of(theta).cpu()
    assert all(torch.equal(p[b] > 0.5, want) for b in range(2))
    assert (p > 0.5).float().flatten(1).mean(1).tolist() == [d.K1 / 64] * 2
    assert torch.equal(theta, planted_run(gpu_device))
