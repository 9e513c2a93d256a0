"""CPU-only: captum.robust (FGSM, PGD), the engine's argument checks and the numpy model of the attack kernels: names and
signatures, tests/robust_ref.py's ``step`` against the torch expressions of Captum's ``_perturb`` + ``_clip`` + ``bound`` bit for
bit, every argument check before any GPU work, the error contract of the three entry points, their resource usage, and the
ladder fold's host model on hand-made logits."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

import robust_ref as RR
from addvisor_hip import _lib, robust as RB
from test_build_resources import resources

INF = math.inf


def test_captum_names_and_signatures():
    import captum_saliency
    from captum.robust import FGSM, PGD
    assert captum_saliency.FGSM is FGSM and captum_saliency.PGD is PGD
    for cls in (FGSM, PGD):
        p = inspect.signature(cls.__init__).parameters
        assert list(p) == ["self", "forward_func", "loss_func", "lower_bound", "upper_bound"]
        assert [p[k].default for k in list(p)[2:]] == [None, -INF, INF]
    p = inspect.signature(FGSM.perturb).parameters
    assert list(p) == ["self", "inputs", "epsilon", "target", "additional_forward_args", "targeted", "mask"]
    assert [p[k].default for k in list(p)[4:]] == [None, False, None]
    p = inspect.signature(PGD.perturb).parameters
    assert list(p) == ["self", "inputs", "radius", "step_size", "step_num", "target", "additional_forward_args", "targeted",
                       "random_start", "norm", "mask"]
    assert [p[k].default for k in list(p)[6:]] == [None, False, False, "Linf", None]
    p = inspect.signature(captum_saliency.attack_waves).parameters
    assert list(p) == ["model", "waves", "labels", "attack", "explain", "attack_kwargs"]
    assert (p["attack"].default, p["explain"].default) == ("pgd", None)
    assert hasattr(captum_saliency.Wav2vec2LogReg, "hip_robust")
    assert [f[0] for f in RB.RobustDesc._fields_] == ["x0", "x", "grad", "seed", "mask", "eps", "n", "B", "p", "x_rows", "grad_rows",
                                                      "mask_rows", "targeted", "norm", "radius", "lo", "hi"]


def _data(R=5, n=1001, seed=0, away=False):
    """``away``: |x0| >= 0.2, so that no element of x0 + d cancels (a bar relative to the output element then measures the norm's
    error, which enters through d, and not the cancellation)."""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-1, 1, (R, n)).astype(np.float32)
    if away:
        x0 = (np.sign(x0) * (0.2 + 0.8 * np.abs(x0))).astype(np.float32)
    x = (x0 + rng.uniform(-0.02, 0.02, (R, n))).astype(np.float32)
    g = (rng.standard_normal((R, n)) * 10.0 ** rng.uniform(-8, 0, (R, n))).astype(np.float32)
    plant = np.array([0.0, -0.0, 1e-6, -1e-6, 1.0000001e-6, -1.0000001e-6, 9.9999e-7, np.float32(1e-6) * 2], np.float32)
    g[:, :plant.size] = plant
    g[1, 100:108] = plant[::-1]
    mask = (rng.uniform(0, 1, (R, n)) > 0.3).astype(np.float32)
    mask[:, 50:60] = 0.5                                                  # a fractional mask scales the step
    return x0, x, g, mask


@pytest.mark.parametrize("norm,name", [(0, None), (1, "Linf")])
def test_step_model_equals_the_torch_expression_bit_for_bit(norm, name):
    x0, x, g, mask = _data()
    t = torch.from_numpy
    for mult in (1, -1):
        for m in (None, mask, mask[:1]):
            for lo, hi in ((-INF, INF), (-0.5, 0.7), (-INF, 0.1)):
                for eps, radius in ((0.01, 0.02), (1e-3, 1e-3), (0.3, 0.05), (0.0, 0.0)):
                    ours = RR.step(x0, x, g, None, m, eps, mult, radius, norm, lo, hi)
                    ref = RR.torch_step(t(x0), t(x), t(g), eps, mult, radius, name, lo, hi, None if m is None else t(m)).numpy()
                    assert ours.dtype == np.float32
                    assert np.array_equal(ours.view(np.uint32), ref.view(np.uint32)), (norm, mult, lo, hi, eps)
    # a per-row seed is a product rounded in fp32 before the sign and the threshold: the same as handing torch seed * g
    seed = np.array([0.3, -0.7, 0.0, 1e-3, -1.0], np.float32)
    ours = RR.step(x0, x, g, seed, mask, 0.01, 1, 0.02, norm, -1.0, 1.0)
    ref = RR.torch_step(t(x0), t(x), t(seed)[:, None] * t(g), 0.01, 1, 0.02, name, -1.0, 1.0, t(mask)).numpy()
    assert np.array_equal(ours.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(ours[2], np.clip(x[2] if norm == 0 else x0[2] + np.clip(x[2] - x0[2], np.float32(-0.02), np.float32(0.02)),
                                           -1, 1))                        # seed 0: no step at all
    # the threshold: 0, +-1e-6 (= float32(1e-6)) and 9.9999e-7 do not move, +-1.0000001e-6 (the next float32) and 2e-6 do
    plain = RR.step(None, x, g, None, None, 0.01, 1, 0.0, 0, -INF, INF)
    assert np.array_equal(plain[0, :4], x[0, :4]) and plain[0, 6] == x[0, 6]
    assert np.all(plain[0, [4, 5, 7]] != x[0, [4, 5, 7]])
    # per-row step sizes (the ladder)
    eps = np.array([1e-3, 2e-3, 4e-3, 8e-3, 0.5])
    ours = RR.step(x0, x, g, None, None, eps, -1, 0.02, norm, -INF, INF)
    for r in range(5):
        ref = RR.torch_step(t(x0[r:r + 1]), t(x[r:r + 1]), t(g[r:r + 1]), float(eps[r]), -1, 0.02, name, -INF, INF).numpy()
        assert np.array_equal(ours[r:r + 1].view(np.uint32), ref.view(np.uint32))


def test_step_model_l2_against_renorm():
    x0, x, g, mask = _data(away=True)
    t = torch.from_numpy
    for radius in (0.05, 0.5, 10.0):                                      # 10: every row inside the ball (factor exactly 1)
        d = (x - x0) * np.float32(3)
        rn, ref = RR.renorm(d, radius), torch.renorm(t(d), 2, 0, radius).numpy()
        assert np.all(np.abs(rn.astype(np.float64) - ref) <= 1e-6 * np.abs(ref)), radius
        for eps in (0.01, 0.1):
            ours = RR.step(x0, x, g, None, mask, eps, 1, radius, 2, -INF, INF)
            ref = RR.torch_step(t(x0), t(x), t(g), eps, 1, radius, "L2", -INF, INF, t(mask)).numpy()
            assert np.all(np.abs(ours.astype(np.float64) - ref) <= 1e-6 * np.abs(ref)), (radius, eps)
            dist = np.sqrt(((ours.astype(np.float64) - x0) ** 2).sum(1))
            assert np.all(dist <= radius * (1 + 1e-5))
    inside = RR.step(x0, x, g, None, None, 0.01, 1, 10.0, 2, -INF, INF)
    v = RR.step(None, x, g, None, None, 0.01, 1, 0.0, 0, -INF, INF)
    assert np.array_equal(inside, x0 + (v - x0))                         # factor 1: x0 + (v - x0) * 1, Captum's own rounding


class _NoEngine:
    def hip_robust(self):
        raise AssertionError("the front end reached the engine before rejecting its arguments")


def test_front_end_validates_before_gpu_work():
    from captum.robust import FGSM, PGD
    x = torch.zeros(2, 100)
    m = _NoEngine()
    ok_f = dict(inputs=x, epsilon=0.01, target=1)
    bad_common = [dict(inputs=x[0]), dict(inputs=torch.zeros(2, 3, 4)), dict(inputs=x.numpy()), dict(inputs=x.long()),
                  dict(inputs=torch.zeros(0, 100)), dict(target=2), dict(target=-1), dict(target=True), dict(target=0.5),
                  dict(target=None), dict(target=torch.tensor([0, 1, 1])), dict(target=torch.tensor([0.0, 0.5])),
                  dict(target=torch.zeros(2, 2)), dict(mask=torch.ones(3, 100)), dict(mask=torch.ones(2, 99)),
                  dict(mask=torch.ones(2, 2, 50)), dict(mask=np.ones((2, 100))), dict(mask=1)]
    for b in bad_common + [dict(epsilon=-0.1), dict(epsilon=INF), dict(epsilon=float("nan")), dict(epsilon="a"), dict(epsilon=None)]:
        kw = dict(ok_f)
        kw.update(b)
        with pytest.raises(ValueError):
            FGSM(m).perturb(**kw)
    ok_p = dict(inputs=x, radius=0.02, step_size=0.005, step_num=3, target=torch.tensor([0, 1]))
    for b in bad_common + [dict(radius=-1.0), dict(radius=INF), dict(step_size=float("nan")), dict(step_size=-1e-3),
                           dict(step_num=-1), dict(step_num=2.0), dict(step_num=True), dict(norm="L1"), dict(norm="linf"),
                           dict(norm=2), dict(norm=None)]:
        kw = dict(ok_p)
        kw.update(b)
        with pytest.raises(ValueError):
            PGD(m).perturb(**kw)
    for cls, ok in ((FGSM, ok_f), (PGD, ok_p)):
        for bounds in ((1.0, -1.0), (float("nan"), 1.0), (-1.0, float("nan")), ("a", 1.0), (None, 1.0)):
            with pytest.raises(ValueError):
                cls(m, lower_bound=bounds[0], upper_bound=bounds[1]).perturb(**ok)
        with pytest.raises(ValueError):
            cls(m, loss_func="bce").perturb(**ok)
        with pytest.raises(TypeError):
            cls(torch.nn.Linear(100, 1)).perturb(**ok)
        with pytest.raises(NotImplementedError):
            cls(m).perturb(additional_forward_args=(1,), **ok)
        with pytest.raises(AssertionError):                              # valid arguments go on to the engine
            cls(m, lower_bound=-1.0, upper_bound=1.0).perturb(mask=torch.ones(1, 100), targeted=True, **ok)
        with pytest.raises(AssertionError):                              # a callable loss takes any target
            cls(m, loss_func=lambda out, t: out.sum()).perturb(**dict(ok, target="anything"))


class _Stub(RB.HipRobust):
    """The engine's methods up to their first GPU step."""

    def __init__(self):
        class Att:
            loss_scale = 4096.0

            def _prep(self, waves):
                raise AssertionError("the engine touched the clips before rejecting its arguments")
        self.att = Att()


def test_engine_checks_before_gpu_work():
    eng = _Stub()
    x = torch.zeros(2, 64)
    for bad in (dict(epsilons=[]), dict(epsilons=[1e-3, 1e-3]), dict(epsilons=[2e-3, 1e-3]), dict(epsilons=[0.0, 1e-3]),
                dict(epsilons=[-1e-3, 1e-3]), dict(epsilons=[1e-3, INF]), dict(epsilons=[1e-3, float("nan")]), dict(epsilons=1e-3),
                dict(epsilons=[1e-3, "a"]), dict(epsilons=[1e-3 * (k + 1) for k in range(RB.MAX_P + 1)]),
                dict(epsilons=[1.0, 1.0 + 1e-12]), dict(internal_batch_size=0), dict(target=3), dict(mask=torch.ones(2, 3)),
                dict(lower_bound=1.0, upper_bound=0.0)):
        kw = dict(waves=x, epsilons=[1e-3, 2e-3], target=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            eng.fgsm_min_epsilon(**kw)
    with pytest.raises(AssertionError):
        eng.fgsm_min_epsilon(x, torch.tensor([1e-3, 2e-3]), 1, internal_batch_size=1)
    for bad in (dict(trace=()), dict(trace={}), dict(seed=-1, random_start=True), dict(seed=2 ** 64, random_start=True),
                dict(norm="L3")):
        kw = dict(waves=x, radius=0.02, step_size=0.005, step_num=2, target=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            eng.pgd(**kw)
    with pytest.raises(AssertionError):
        eng.pgd(x, 0.02, 0.005, 2, 0, trace=[], norm="L2", random_start=True, seed=5)
    with pytest.raises(ValueError):
        eng.fgsm(x, -1.0, 0)
    with pytest.raises(AssertionError):
        eng.fgsm(x, 0.0, torch.tensor([[1], [0]]))
    assert RB.check_target(torch.tensor([[1], [0]]), 2).tolist() == [1.0, 0.0]
    assert RB.check_mask(torch.ones(64), 2, 64).shape == (1, 64)
    # host tensors never reach a kernel
    f = torch.zeros(2, 8)
    for call in (lambda: RB.robust_step(f, f, f, None, None, [0.1], False, 1, 0.1, -1.0, 1.0, f),
                 lambda: RB.random_point(f, 1, 1, 0.1, -1.0, 1.0),
                 lambda: RB.first_flip_rows(torch.zeros(4), torch.zeros(2), torch.zeros(2))):
        with pytest.raises(ValueError):
            call()


def test_loss_seed_on_the_host():
    """The default seed is prob - target; a callable loss is differentiated over the logit leaf alone."""
    eng = _Stub()
    logit = torch.tensor([[0.3], [-1.2], [2.0]])
    prob = torch.sigmoid(logit)
    t = torch.tensor([1.0, 0.0, 1.0])
    assert torch.equal(eng.loss_seed(logit, prob, t, None), prob.view(-1) - t)
    assert torch.equal(eng.loss_seed(logit, prob, 1, None), prob.view(-1) - 1.0)
    bce = lambda out, tgt: torch.nn.functional.binary_cross_entropy_with_logits(out, tgt.view(-1, 1), reduction="sum")
    with torch.no_grad():                                                # the engine enables grad on its own
        s = eng.loss_seed(logit, prob, t, bce)
    assert s.shape == (3,) and torch.allclose(s, prob.view(-1) - t, rtol=0, atol=1e-6)
    assert torch.equal(eng.loss_seed(logit, prob, None, lambda out, tgt: (out * out).sum()), 2 * logit.view(-1))
    with pytest.raises(ValueError):
        eng.loss_seed(logit, prob, t, lambda out, tgt: torch.zeros(3))
    with pytest.raises(ValueError):
        eng.loss_seed(logit, prob, t, lambda out, tgt: 1.0)


def test_first_flip_host_model():
    eps = [1e-3, 2e-3, 4e-3, 8e-3]
    clean = np.array([1.5, 1.5, -0.2, -0.2, 0.0, 0.0, 3.0], np.float32)
    logits = np.array([[-1, -1, -1, -1],        # a flip at k = 0
                       [1, 1, 1, -1e-9],        # a flip at the last k
                       [-1, -2, -3, -4],        # no flip
                       [-1, 0.0, 1, 1],         # a logit of exactly 0 is "not > 0": no flip at k = 1, the flip is at k = 2
                       [0.0, 0.0, -1, 1e-9],    # a clean logit of exactly 0 is negative: the flip is at k = 3
                       [-5, -5, -5, -5],
                       [2, 0.0, 5, -1]], np.float32)   # exactly 0 against a positive clean logit flips
    out, first = RB.first_flip(logits, clean, eps)
    assert first.tolist() == [0, 3, 4, 2, 3, 4, 1] and first.dtype == np.int32
    want = np.array([1e-3, 8e-3, np.inf, 4e-3, 8e-3, np.inf, 2e-3], np.float32)
    assert out.dtype == np.float32 and np.array_equal(out, want)


def test_argument_errors_of_the_robust_entry_points():
    """include/addvisor_hip.h error contract (negative return, nothing launched): validation happens before any HIP call, so it
    runs without a GPU."""
    lib = _lib.lib()
    EINVAL = -1
    fb = (C.c_float * 256)()
    ib = (C.c_int * 16)()
    pf, pi = C.addressof(fb), C.addressof(ib)
    nan = float("nan")

    def step(row0=0, rows=6, out=pf, eps=(1e-3, 2e-3, 3e-3), **f):
        arr = (C.c_double * max(1, len(eps)))(*eps) if eps is not None else None
        d = dict(x0=pf, x=pf, grad=pf, seed=None, mask=None, eps=None if arr is None else C.addressof(arr), n=8, B=2, p=3, x_rows=2,
                 grad_rows=6, mask_rows=1, targeted=0, norm=1, radius=0.1, lo=-1.0, hi=1.0)
        d.update(f)
        return lib.advh_robust_step(C.byref(RB.RobustDesc(**d)), row0, rows, out, None)

    for bad in (dict(x=None), dict(grad=None), dict(eps=None), dict(out=None), dict(x0=None), dict(norm=2, x0=None), dict(n=0),
                dict(n=-4), dict(B=0), dict(p=0), dict(p=RB.MAX_P + 1), dict(norm=3), dict(norm=-1), dict(targeted=2),
                dict(radius=-0.1), dict(radius=nan), dict(radius=INF), dict(eps=(1e-3, -1e-3, 1e-3)), dict(eps=(1e-3, nan, 1e-3)),
                dict(eps=(INF, 1e-3, 1e-3)), dict(lo=1.0, hi=-1.0), dict(lo=nan), dict(hi=nan), dict(x_rows=3), dict(x_rows=0),
                dict(grad_rows=4), dict(mask=pf, mask_rows=3), dict(mask=pf, mask_rows=0), dict(row0=-1), dict(rows=0),
                dict(rows=7), dict(row0=4, rows=3), dict(row0=6, rows=1), dict(B=1 << 27, p=32, x_rows=1 << 27, grad_rows=1 << 27)):
        assert step(**bad) == EINVAL, bad
    assert lib.advh_robust_step(None, 0, 1, pf, None) == EINVAL
    rs = lambda x0=pf, B=2, n=8, norm=1, radius=0.1, lo=-1.0, hi=1.0, out=pf: lib.advh_robust_random_start(x0, B, n, 7, norm, radius,
                                                                                                         lo, hi, out, None)
    for bad in (dict(x0=None), dict(out=None), dict(B=0), dict(n=0), dict(norm=0), dict(norm=3), dict(radius=-1.0), dict(radius=nan),
                dict(radius=INF), dict(lo=1.0, hi=0.0), dict(lo=nan), dict(hi=nan)):
        assert rs(**bad) == EINVAL, bad
    ff = lambda lg=pf, cl=pf, eps=pf, B=2, K=3, out=pf, first=pi: lib.advh_robust_first_flip(lg, cl, eps, B, K, out, first, None)
    for bad in (dict(lg=None), dict(cl=None), dict(eps=None), dict(out=None), dict(first=None), dict(B=0), dict(K=0), dict(K=-1),
                dict(B=1 << 16, K=1 << 16)):
        assert ff(**bad) == EINVAL, bad


def test_robust_kernels_do_not_spill():
    res = resources("attribution_robust.hip")
    for nm, count in (("robust_step_kernel", 4), ("robust_random_start_kernel", 4), ("robust_first_flip_kernel", 1)):
        hit = {k: v for k, v in res.items() if nm in k}
        assert len(hit) == count, (nm, sorted(res))
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
