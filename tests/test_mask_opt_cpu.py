"""CPU-only: the per-clip optimised mask (addvisor_hip/mask_opt.py, csrc/mask_opt.hip) -- the per-axis weight rule against
``F.interpolate``, the restatement's gradient (tests/mask_opt_ref.py) against central finite differences, every ValueError path
of ``check_mask_opt_args`` with CPU tensors and no device, and the ADVH_EINVAL contract of the three entry points (argument
validation happens before any HIP call, so it runs without a GPU)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import mask_opt_ref as R
from addvisor_hip import _lib, mask_opt as MO, spectral_attribution as SA

EINVAL = -1
GEOMETRIES = [((33, 13), (513, 50)), ((32, 12), (512, 48)), ((8, 6), (512, 48)), ((9, 7), (513, 50)), ((1, 1), (513, 50)),
              ((513, 50), (513, 50))]


def upsample_matrix(n, N):
    """The ``[N, n]`` float64 matrix of one axis of U from ``axis_weights``."""
    i0, i1, w1 = MO.axis_weights(n, N)
    U = torch.zeros(N, n, dtype=torch.float64)
    r = torch.arange(N)
    U.index_put_((r, i0), 1 - w1, accumulate=True)
    U.index_put_((r, i1), w1, accumulate=True)
    return U


@pytest.mark.parametrize("coarse,fine", GEOMETRIES, ids=[f"{c[0]}x{c[1]}" for c, _ in GEOMETRIES])
def test_axis_weights_are_torch_bilinear(coarse, fine):
    """``U_f p U_t^T`` from ``axis_weights`` equals ``F.interpolate(bilinear, align_corners=False)`` in float64 (rounding only)."""
    p = torch.rand(2, *coarse, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    Uf, Ut = upsample_matrix(coarse[0], fine[0]), upsample_matrix(coarse[1], fine[1])
    ours = Uf @ p @ Ut.T
    ref = F.interpolate(p[:, None], size=fine, mode="bilinear", align_corners=False)[:, 0]
    err = (ours - ref).abs().max().item()
    print(f"{coarse} -> {fine}: max |U p - interpolate| = {err:.2e}")
    assert err < 1e-13
    for n, N in zip(coarse, fine):
        i0, i1, w1 = MO.axis_weights(n, N)
        assert int(i0.min()) == 0 and int(i1.max()) == n - 1 and bool((i1 - i0 <= 1).all()) and bool(((w1 >= 0) & (w1 < 1)).all())
        assert sorted(set(i0.tolist()) | set(i1.tolist())) == list(range(n))       # every coarse point has a footprint
        if n == N:
            assert torch.equal(i0, torch.arange(N)) and not bool(w1.any())         # the identity is exact


def test_coarse_grid_and_ranked_cells():
    assert MO.coarse_grid(513, 199, (16, 4)) == (33, 50) and MO.coarse_grid(513, 50, (600, 60)) == (1, 1)
    assert MO.coarse_grid(16, 12, (1, 1)) == (16, 12)
    assert MO.ranked_cells(0.1, 1650) == 165 and MO.ranked_cells(0.5, 3) == 2 and MO.ranked_cells(None, 7) == 0
    assert MO.ranked_cells(0.1, 429) == R.ranked_cells(0.1, 429) == 43


@pytest.mark.parametrize("lam", [(1.0, 1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 3.0, 0.5, 2.0)], ids=["data", "all"])
def test_restatement_gradient_against_finite_differences(lam):
    """Central differences of the linear surrogate ``J = <G, rows(theta)> + regularisers`` in float64; theta is a normal draw (no
    exact ties, gaps far above the 1e-6 probe), so the rank is locally constant."""
    g = torch.Generator().manual_seed(11)
    B, Fc, Tc, Fm, Tm, K1 = 2, 4, 3, 37, 10, 5
    theta = torch.randn(B, Fc, Tc, dtype=torch.float64, generator=g)
    assert float((theta.flatten(1).sort(1).values.diff(dim=1)).min()) > 1e-4
    G = torch.randn(2 * B, Fm, Tm, dtype=torch.float64, generator=g)
    ours = R.grad_theta(theta, G, lam, K1)
    h, fd = 1e-6, torch.zeros_like(theta)
    for i in range(theta.numel()):
        e = torch.zeros(theta.numel(), dtype=torch.float64)
        e[i] = h
        e = e.view_as(theta)
        fd.view(-1)[i] = (R.surrogate(theta + e, G, lam, K1, Fm, Tm).sum() - R.surrogate(theta - e, G, lam, K1, Fm, Tm).sum()) / (2 * h)
    err = ((ours - fd).abs().max() / fd.abs().max()).item()
    print(f"autograd vs central differences: {err:.2e}")
    assert err < 1e-7


def test_restatement_seeds_are_the_closed_forms():
    """The seeds by autograd equal ``-lam_in s phi'(z_in)`` / ``lam_out s phi'(z_out)`` for the three rewards and both signs."""
    theta = torch.randn(2, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    lg, s = torch.tensor([1.5, -0.25, -2.0, 0.75], dtype=torch.float64), torch.tensor([1.0, -1.0], dtype=torch.float64)
    for kind, d in (("logit", lambda z: torch.ones_like(z)), ("prob", lambda z: torch.sigmoid(z) * (1 - torch.sigmoid(z))),
                    ("log_prob", lambda z: torch.sigmoid(-z))):
        seeds, hist = R.seeds_and_history(theta, lg, s, (2.0, 3.0, 1.0, 1.0, 1.0), 4, kind)
        assert torch.allclose(seeds[0::2], -2.0 * s * d(s * lg[0::2]), atol=1e-15), kind
        assert torch.allclose(seeds[1::2], 3.0 * s * d(s * lg[1::2]), atol=1e-15), kind
        assert hist.shape == (2, 6) and bool(torch.isfinite(hist).all())


def test_planted_box_inputs_satisfy_the_condition_in_float64():
    """The GPU test of the planted box (tests/test_gpu_mask_opt_kernels.py) states a condition on its inputs: with lam_area = 10,
    Adam at lr = 0.1 and 30 steps the float64 restatement alone must end with ``{p > 0.5}`` equal to the box's cells -- and far
    from the threshold, so that fp32 cannot flip a cell."""
    def make_desc(Fm, Tm, cell, lam, area, optimizer, lr, clips):
        Fc, Tc = MO.coarse_grid(Fm, Tm, cell)
        return MO.MaskOptDesc(clips, Fm, Tm, Fc, Tc, MO.ranked_cells(area, Fc * Tc), 2, 0, *lam, lr, *MO.ADAM, 0.9)
    d, G, theta0, want = R.planted(make_desc)
    assert (d.Fc, d.Tc, d.K1) == (8, 8, 9) and int(want.sum()) == 9
    p = R.planted_box_run(G.double(), theta0, d.K1, R.BOX["lam"], R.BOX["lr"], R.BOX["steps"])
    assert all(torch.equal(p[b] > 0.5, want) for b in range(2))
    margin = float((p - 0.5).abs().min())
    print(f"planted box: min |p - 0.5| after {R.BOX['steps']} steps = {margin:.3f}")
    assert margin > 0.3


# ------------------------------------------------------------------------------------------------------------- argument checks
def ok_args(**kw):
    a = dict(B=2, T=50, domain="linear")
    a.update(kw)
    return a


BAD = [dict(area=0.0), dict(area=1.0), dict(area=-0.1), dict(area=1.5), dict(area="10%"), dict(area=True), dict(area=None),
       dict(area=None, domain="log1p", lam_area=1.0),
       dict(cell=16), dict(cell=(16,)), dict(cell=(0, 4)), dict(cell=(16, 4.0)), dict(shape=(513,)), dict(shape=(514, 50)),
       dict(shape=(513, 51)), dict(shape=(0, 10)), dict(shape=513), dict(reward="probability"), dict(reward=None),
       dict(optimizer="lbfgs"), dict(target=1), dict(target=torch.tensor([0, 1, 1])), dict(target=torch.tensor([0, 2])),
       dict(target=torch.tensor([0.0, 1.0])), dict(target=torch.tensor([[0, 1]])),
       dict(init=torch.full((2, 33, 12), 0.5)), dict(init=torch.full((3, 33, 13), 0.5)), dict(init=torch.full((2, 513 * 50), 0.5)),
       dict(init=torch.ones(2, 33, 13, dtype=torch.long)), dict(init="unet"),
       dict(init=0.0), dict(init=1.0), dict(init=1.5), dict(init=torch.zeros(2, 33, 13)), dict(init=torch.ones(2, 513, 50)),
       dict(init=torch.full((2, 33, 13), float("nan"))),
       dict(steps=0), dict(steps=2.5), dict(lr=0.0), dict(lr=float("inf")), dict(lr=float("nan")), dict(momentum=1.0), dict(momentum=-0.1),
       dict(lam_in=-1.0), dict(lam_tv=float("nan")), dict(lam_area="big"), dict(init_noise=-1.0), dict(seed=-1), dict(seed=2 ** 64),
       dict(internal_batch_size=0), dict(trace=()), dict(B=65536), dict(B=0)]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(f"{k}={str(v)[:18]}" for k, v in kw.items()) for kw in BAD])
def test_check_mask_opt_args_value_errors(kw):
    with pytest.raises(ValueError):
        MO.check_mask_opt_args(**ok_args(**kw))


def test_the_linear_domain_error_says_why():
    with pytest.raises(ValueError, match="silent clip"):
        MO.check_mask_opt_args(2, 50, "linear", area=None)
    with pytest.raises(ValueError, match=r"open interval \(0, 1\)"):
        MO.check_mask_opt_args(2, 50, "linear", area=1.0)


def test_check_mask_opt_args_normalises():
    a = MO.check_mask_opt_args(2, 50, "linear", seed=5)
    assert (a.Fm, a.Tm, a.Fc, a.Tc, a.K1, a.K) == (513, 50, 33, 13, 43, 429) and a.sign is None and a.clips_per_chunk == 64
    assert a.lam == (1.0, 1.0, MO.DEFAULT_LAM_AREA, 0.0, 0.0) and (a.reward, a.optimizer) == (2, 0)
    assert a.theta0.shape == (2, 33, 13) and a.theta0.dtype == torch.float32
    assert 0 < float(a.theta0.std()) < 0.05 and len(set(a.theta0.flatten().tolist())) == a.theta0.numel()    # the noise breaks every tie
    assert torch.equal(a.theta0, MO.check_mask_opt_args(2, 50, "linear", seed=5).theta0)                     # seeded
    assert not torch.equal(a.theta0, MO.check_mask_opt_args(2, 50, "linear", seed=6).theta0)
    b = MO.check_mask_opt_args(2, 50, "log1p", area=None, lam_l1=0.1, init_noise=0.0, target=[1, 0], internal_batch_size=3,
                               optimizer="sgd", reward="logit")
    assert b.K1 == 0 and b.lam[2] == 0.0 and b.sign.tolist() == [1.0, -1.0] and b.clips_per_chunk == 1 and not bool(b.theta0.any())
    # a fine-grid init is box-averaged to the grid (the last boxes cropped), a coarse one is taken as it is
    fine = torch.rand(2, 513, 50, generator=torch.Generator().manual_seed(1)) * 0.8 + 0.1
    c = MO.check_mask_opt_args(2, 50, "linear", init=fine, init_noise=0.0)
    box = torch.stack([torch.stack([fine[:, i * 16:(i + 1) * 16, j * 4:(j + 1) * 4].double().mean((1, 2)) for j in range(13)], 1)
                       for i in range(33)], 1)
    assert torch.allclose(torch.sigmoid(c.theta0.double()), box, atol=1e-6)
    d = MO.check_mask_opt_args(2, 50, "linear", init=box, init_noise=0.0)
    assert torch.equal(c.theta0, d.theta0)


class _NoDevice:
    """Stands in for the engine's device state: any touch of it fails the test."""
    def __getattr__(self, name):
        raise AssertionError("a device call before the argument checks finished")


def test_optimize_mask_value_errors_fire_before_any_device_call():
    eng = SA.HipSpectralAttribution.__new__(SA.HipSpectralAttribution)
    eng.B, eng.T, eng.domain = 2, 50, "linear"
    eng._rows = eng.waves = _NoDevice()
    for kw in (dict(area=None), dict(area=1.0), dict(cell=(16,)), dict(reward="p"), dict(init=torch.zeros(2, 33, 13)), dict(shape=(513, 99))):
        with pytest.raises(ValueError):
            eng.optimize_mask(**kw)
    with pytest.raises(AssertionError, match="device call"):
        eng.optimize_mask(steps=1)
    with pytest.raises(NotImplementedError, match="optimize_mask"):
        eng.kernel_shap(None)


def test_explain_spectrogram_checks_mask_opt_first():
    import captum_saliency as cs
    assert "optimized_mask" in cs.SPECTRAL_METHODS
    x = torch.randn(2, 64)
    for kw in (dict(method="saliency", mask_opt={}), dict(method="optimized_mask", mask_opt=[("steps", 3)]),
               dict(method="optimized_mask", mask_opt=dict(shape=(4, 4))), dict(method="optimised_mask")):
        with pytest.raises(ValueError):
            cs.explain_spectrogram(None, x, **kw)


# ------------------------------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (C.c_float * 256)()
    yield C.addressof(buf)
    del buf


def desc(**kw):
    d = MO.MaskOptDesc(2, 16, 12, 4, 3, 3, 2, 0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.05, 0.9, 0.999, 1e-8, 0.9)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BAD_DESC = [dict(B=0), dict(B=-1), dict(B=65536), dict(Fm=0), dict(Tm=0), dict(Fc=0), dict(Tc=-2), dict(Fc=17), dict(Tc=13), dict(K1=-1),
            dict(K1=13), dict(reward=3), dict(reward=-1), dict(optimizer=2), dict(optimizer=-1), dict(lr=float("inf")), dict(lr=float("nan"))]


def entry_points(lib, p):
    """Each entry point as ``f(desc_ref, b0, nb, skip)`` with good operands, ``skip`` naming a pointer to null."""
    def arg(name, skip):
        return None if name == skip else p
    rows = lambda d, b0, nb, skip=None: lib.advh_mask_opt_rows(d, arg("theta", skip), b0, nb, arg("rows", skip), None)
    terms = lambda d, b0, nb, skip=None: lib.advh_mask_opt_terms(d, arg("theta", skip), arg("rank", skip), arg("sign", skip),
                                                                 arg("logits", skip), b0, nb, arg("p", skip), arg("seeds", skip),
                                                                 arg("hist", skip), None)
    step = lambda d, b0, nb, skip=None: lib.advh_mask_opt_step(d, arg("theta", skip), arg("p", skip), arg("rank", skip), arg("G", skip), b0, nb,
                                                               0.1, 0.001, arg("m1", skip), arg("m2", skip), arg("grad", skip), None)
    return {"rows": (rows, ("theta", "rows")), "terms": (terms, ("theta", "rank", "sign", "logits", "p", "seeds", "hist")),
            "step": (step, ("theta", "p", "rank", "G", "m1", "m2"))}


@pytest.mark.parametrize("name", ["rows", "terms", "step"])
def test_entry_points_return_einval_before_any_hip_call(lib, p, name):
    f, pointers = entry_points(lib, p)[name]
    assert f(None, 0, 2) == EINVAL
    for ptr in pointers:
        assert f(C.byref(desc()), 0, 2, ptr) == EINVAL, ptr
    for kw in BAD_DESC:
        assert f(C.byref(desc(**kw)), 0, 1) == EINVAL, kw
    for b0, nb in ((0, 0), (0, -1), (-1, 1), (1, 2), (2, 1), (0, 3)):                  # the clip range must lie inside [0, B)
        assert f(C.byref(desc()), b0, nb) == EINVAL, (b0, nb)


def test_step_bias_corrections_and_optional_pointers(lib, p):
    d = C.byref(desc())
    step = lib.advh_mask_opt_step
    for bc in ((0.0, 0.001), (0.1, 0.0), (-0.1, 0.001), (float("nan"), 0.001), (0.1, float("inf"))):
        assert step(d, p, p, p, p, 0, 2, bc[0], bc[1], p, p, None, None) == EINVAL, bc
    assert step(C.byref(desc(optimizer=1)), p, p, p, p, 0, 2, 0.0, 0.0, None, None, None, None) == EINVAL      # SGD still needs m1
    assert math.isclose(MO.bias_corrections(1)[0], 0.1) and math.isclose(MO.bias_corrections(1)[1], 0.001)
    assert MO.bias_corrections(3) == (1 - 0.9 ** 3, 1 - 0.999 ** 3)
