"""CPU-only: captum.metrics (infidelity, sensitivity_max, infidelity_perturb_func_decorator) and the engine's metric loops: names
and signatures, the chunk plan against Captum's ``_divide_and_aggregate_metrics`` (tests/metrics_ref.py), the decorator and
safe_div on a hand-computed case, the fp64 fold and normalisation against a numpy model, the uniform rows' bit patterns, every
argument check before any GPU work, the error contract of the new entry points and their resource usage."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

import metrics_ref as MR
from addvisor_hip import _lib, attribution as AT
from metrics_ref import fold_model
from test_build_resources import resources

TRIPLES = [(2, 4, None), (2, 4, 2), (2, 4, 4), (2, 4, 6), (2, 4, 8), (3, 10, 9), (3, 10, 7), (1, 5, 2), (4, 7, 100), (2, 6, 3)]


def test_captum_names_and_signatures():
    import captum_saliency
    from captum.metrics import NoisyPerturbation, default_perturb_func, infidelity, infidelity_perturb_func_decorator, sensitivity_max
    assert captum_saliency.infidelity is infidelity and captum_saliency.sensitivity_max is sensitivity_max
    p = inspect.signature(infidelity).parameters
    assert list(p) == ["forward_func", "perturb_func", "inputs", "attributions", "baselines", "additional_forward_args", "target",
                       "n_perturb_samples", "max_examples_per_batch", "normalize"]
    assert [p[k].default for k in list(p)[4:]] == [None, None, None, 10, None, False]
    p = inspect.signature(sensitivity_max).parameters
    assert list(p) == ["explanation_func", "inputs", "perturb_func", "perturb_radius", "n_perturb_samples", "norm_ord",
                       "max_examples_per_batch", "kwargs"]
    assert [p[k].default for k in list(p)[2:7]] == [default_perturb_func, 0.02, 10, "fro", None]
    assert list(inspect.signature(infidelity_perturb_func_decorator).parameters) == ["multiply_by_inputs"]
    assert inspect.signature(infidelity_perturb_func_decorator).parameters["multiply_by_inputs"].default is True
    n = NoisyPerturbation(0.05)
    assert (n.stdevs, n.multiply_by_inputs) == (0.05, False) and callable(n)
    p = inspect.signature(captum_saliency.compute_camptum_saliency_metrics).parameters
    assert p["explanation_metrics"].default is False
    assert inspect.signature(captum_saliency.score_explanations).parameters["stdevs"].default == 0.01


@pytest.mark.parametrize("B,S,mex", TRIPLES)
def test_chunk_plan_matches_captum(B, S, mex):
    ours = AT.metric_partitions(B, S, mex)
    sizes = MR.chunk_sizes(B, S, mex)
    assert [n for _, n in ours] == sizes
    assert [s0 for s0, _ in ours] == list(np.cumsum([0] + sizes[:-1]))
    assert sum(sizes) == S
    m = S if mex is None else mex // B
    if m < S:
        assert sizes == [m] * (S // m) + ([S % m] if S % m else [])


def test_chunk_plan_rejects_a_batch_below_the_clip_count():
    with pytest.raises(ValueError):
        AT.metric_partitions(4, 10, 3)
    with pytest.raises(AssertionError):                                # Captum asserts
        MR.chunk_sizes(4, 10, 3)
    assert AT.metric_partitions(4, 2, 4) == [(0, 1), (1, 1)]


def test_decorator_and_safe_div_hand_computed():
    from captum.metrics import infidelity_perturb_func_decorator
    x = torch.tensor([[2.0, 0.0, -1.0, 4.0]])
    xt = torch.tensor([[1.0, 0.5, -1.0, 3.0]])
    base = torch.tensor([[0.0, 1.0, -1.0, 2.0]])
    f = infidelity_perturb_func_decorator(True)(lambda inputs, baselines=None: xt)
    pert, got = f(x)
    assert got is xt
    assert pert.tolist() == [[0.5, -0.5, 0.0, 0.25]]                 # (x - x~) / x, x = 0 -> divided by 1
    pert, _ = f(x, base)
    assert pert.tolist() == [[0.5, 0.5, 0.0, 0.5]]                   # (x - x~) / (x - b): x - b = 2, -1, 0 (-> 1), 2
    pert, _ = infidelity_perturb_func_decorator(False)(lambda inputs: xt)(x)
    assert pert.tolist() == [[1.0, -0.5, 0.0, 1.0]]
    from captum.metrics import safe_div
    assert safe_div(torch.tensor([3.0]), 0).item() == 3.0 and safe_div(torch.tensor([3.0]), 2).item() == 1.5
    assert safe_div(torch.tensor([3.0, 3.0]), torch.tensor([0.0, 4.0]), 2.0).tolist() == [1.5, 0.75]


def test_fold_and_normalisation_arithmetic():
    rng = np.random.default_rng(3)
    B, S = 3, 10
    a = rng.standard_normal((B, S)).astype(np.float32).astype(np.float64)
    d = rng.standard_normal((B, S)).astype(np.float32).astype(np.float64)
    for normalize in (False, True):
        whole = fold_model(a, d, AT.metric_partitions(B, S), normalize)
        for mex in (3, 6, 12):                                             # sample-order fp64 sums: the chunking changes nothing
            assert np.array_equal(fold_model(a, d, AT.metric_partitions(B, S, mex), normalize), whole)
        # Captum's loop over the same (a, d) (metrics_ref's chunk tensors in float64)
        it = iter(range(S))

        def metric(n):
            idx = [next(it) for _ in range(n)]
            aa, dd = torch.from_numpy(a[:, idx]), torch.from_numpy(d[:, idx])
            return (aa.pow(2).sum(-1), (aa * dd).sum(-1), dd.pow(2).sum(-1)) if normalize else ((aa - dd).pow(2).sum(-1),)
        agg = MR.divide_and_aggregate(B, S, metric, lambda x, y: tuple(p + q for p, q in zip(x, y)), 2 * B)
        if normalize:
            beta = MR.safe_div(agg[1], agg[0])
            ref = (beta ** 2 * agg[0] - 2 * beta * agg[1] + agg[2]) / S
        else:
            ref = agg[0] / S
        assert np.allclose(whole, ref.numpy(), rtol=1e-6, atol=0)
    # normalised <= plain, and a 2^k scale of the attribution leaves the normalised value bit-identical
    plain, norm = fold_model(a, d, [(0, S)], False), fold_model(a, d, [(0, S)], True)
    assert np.all(norm <= plain * (1 + 1e-12))
    for k in (-3, 5):
        assert np.array_equal(fold_model(a * 2.0 ** k, d, [(0, S)], True), norm)
    assert np.array_equal(fold_model(np.zeros_like(a), d, [(0, S)], True), (np.sum(d * d, 1) / S).astype(np.float32))


def test_uniform_rows_bit_patterns():
    """2u - 1 is exact in float32 (so the rows are x + r * t with two roundings), symmetric inside (-1, 1); the bit patterns
    of seed 0x5EED, rows 5-6 are pinned (the device must reproduce them, tests/test_gpu_metrics.py)."""
    t = MR.uniform(0x5EED, 5, 2, 6)
    w = MR.R.philox_words(0x5EED, 5, 2, 6).reshape(2, -1)[:, :6]
    t64 = 2.0 * (((w >> 9).astype(np.float64) * 2 + 1) * 2.0 ** -24) - 1.0
    assert t.dtype == np.float32 and np.array_equal(t.astype(np.float64), t64)
    assert np.all(np.abs(t) < 1)
    assert t.view(np.uint32).tolist() == PINNED
    x = np.linspace(-0.5, 0.5, 12, dtype=np.float32).reshape(2, 6)
    rows = MR.uniform_rows(x, 0x5EED, 4, 1, 2, 0.02)                  # clip b's rows are global rows b * 4 + 1, b * 4 + 2
    for b in range(2):
        want = x[b] + np.float32(0.02) * MR.uniform(0x5EED, b * 4 + 1, 2, 6)
        assert np.array_equal(rows[2 * b:2 * b + 2].view(np.uint32), want.view(np.uint32))


PINNED = [[1054808284, 1058061306, 3191293448, 3187665168, 3196856548, 3209879394],
          [3208967498, 3153058048, 3206824710, 3120601088, 3204672242, 3205326186]]


def test_pinned_words_have_a_known_answer():
    # Philox4x32-10 known-answer vector (Salmon et al., Random123 kat_vectors): counter 0, key 0
    ctr = np.zeros((1, 4), np.uint32)
    assert MR.R.philox4x32_10(ctr, 0, 0)[0].tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


class _NoEngine:
    def hip_attribution(self):
        raise AssertionError("the front end reached the engine before rejecting its arguments")


def _never(*a, **k):
    raise AssertionError("the explanation ran before the arguments were rejected")


def test_front_end_validates_before_gpu_work():
    from captum.metrics import NoisyPerturbation, infidelity, sensitivity_max
    x, a = torch.zeros(2, 100), torch.zeros(2, 100)
    m, nz = _NoEngine(), NoisyPerturbation(0.01)
    bad_infid = [dict(target=0), dict(additional_forward_args=(1,)), dict(inputs=x[0]), dict(inputs=torch.zeros(2, 3, 4)),
                 dict(inputs=x.numpy()), dict(attributions=a[:, :99]), dict(attributions=a[:1]), dict(attributions=None),
                 dict(n_perturb_samples=0), dict(n_perturb_samples=2.5), dict(max_examples_per_batch=1),
                 dict(max_examples_per_batch=0), dict(baselines=torch.zeros(3, 100)), dict(baselines=torch.zeros(2, 99)),
                 dict(perturb_func=None)]
    for b in bad_infid:
        kw = dict(forward_func=m, perturb_func=nz, inputs=x, attributions=a)
        kw.update(b)
        with pytest.raises(ValueError):
            infidelity(**kw)
    with pytest.raises(TypeError):
        infidelity(torch.nn.Linear(100, 1), nz, x, a)
    with pytest.raises(AssertionError):                                  # valid arguments go on to the engine
        infidelity(m, nz, x, a, baselines=torch.zeros(2, 100), max_examples_per_batch=2, normalize=True)
    bad_sens = [dict(target=0), dict(additional_forward_args=(1,)), dict(inputs=x[0]), dict(n_perturb_samples=0),
                dict(max_examples_per_batch=1), dict(norm_ord=3), dict(norm_ord="nuc"), dict(norm_ord=None), dict(norm_ord=True),
                dict(perturb_radius=-0.1), dict(perturb_radius=float("nan")), dict(perturb_radius=float("inf")),
                dict(explanation_func=None)]
    for b in bad_sens:
        kw = dict(explanation_func=_never, inputs=x)
        kw.update(b)
        with pytest.raises(ValueError):
            sensitivity_max(**kw)
    for ok in ("fro", 2, 1, math.inf, float("inf"), np.inf, 2.0):
        assert AT.check_norm_ord(ok) == {"fro": 0, 2: 0, 1: 1}.get(ok if isinstance(ok, str) else float(ok), 2)


class _Stub(AT.HipAttribution):
    """The engine's loop up to its first forward: the perturbation is validated before any GPU work."""

    def __init__(self):
        class Emb:
            def forward(self, *a, **k):
                raise AssertionError("the engine ran the forward before rejecting the perturbation")
        self.eg = type("EG", (), {"emb": Emb()})()

    def _prep(self, waves):
        return waves.float().contiguous()


def test_engine_checks_the_perturbation_before_gpu_work():
    eng = _Stub()
    x, a = torch.zeros(2, 16), torch.ones(2, 16)
    bad = [lambda xe: (xe, xe[:, :8]), lambda xe: (xe[1:], xe), lambda xe: xe, lambda xe: (xe, xe, xe), lambda xe: ("a", xe)]
    for pf in bad:
        with pytest.raises(ValueError):
            eng.infidelity(x, pf, a, n_perturb_samples=3, seed=1)
    with pytest.raises(AssertionError):
        eng.infidelity(x, lambda xe: (xe, xe), a, n_perturb_samples=3, seed=1)
    seen = []
    with pytest.raises(AssertionError):                                  # baselines [B, L] arrive repeat_interleaved
        eng.infidelity(x, lambda xe, be: seen.append(be[:, 0].tolist()) or (xe, xe), a, n_perturb_samples=3, seed=1,
                       baselines=torch.arange(2.0)[:, None].expand(2, 16))
    assert seen == [[0, 0, 0, 1, 1, 1]]
    for pf in (lambda xe: xe[:, :8], lambda xe: (xe, xe), lambda xe, r: xe[1:]):
        with pytest.raises(ValueError):
            AT.sensitivity_max(_never, x, "cpu", perturb_func=pf, n_perturb_samples=2, seed=1)
    radius = []
    with pytest.raises(AssertionError):                                  # two parameters: the radius is passed
        AT.sensitivity_max(_never, x, "cpu", perturb_func=lambda xe, r: radius.append(r) or xe, perturb_radius=0.125,
                           n_perturb_samples=2, seed=1)
    assert radius == [0.125]


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached with a host tensor")


class _Drawn(Exception):
    pass


def test_host_tensors_never_reach_a_kernel(monkeypatch):
    """The metric kernel wrappers and philox_normal reject host tensors with ValueError before the library is touched, and
    NoisyPerturbation draws a host tensor's noise on a GPU (metric_device), never into host memory."""
    monkeypatch.setattr(_lib, "lib", lambda: _NoLib())
    x, f64 = torch.zeros(2, 8), torch.zeros(2, dtype=torch.float64)
    d = AT.metric_desc(x, 1, 3, 0, 2, AT.MR_GAUSS, 0.1, x)
    calls = [lambda: AT.philox_normal(1, 0, 2, 8, "cpu"), lambda: AT.philox_normal(1, 0, 2, 8, x.device),
             lambda: AT.metric_rows(d, 0, 4, torch.zeros(4, 8), torch.zeros(4)), lambda: AT.uniform_rows(x, 1, 3, 0, 2, 0.02),
             lambda: AT.metric_row_dot(torch.zeros(4, 8), x, 2),
             lambda: AT.infidelity_fold(torch.zeros(4), torch.zeros(2), torch.zeros(4), 2, 2, False, f64),
             lambda: AT.infidelity_finalize(f64, 2, 3, False), lambda: AT.row_norm(x, 0),
             lambda: AT.sensitivity_fold(x, torch.zeros(4, 8), torch.ones(2), 2, 0, torch.zeros(2)),
             lambda: AT.sensitivity_max(lambda w: w, x, "cpu", n_perturb_samples=2, seed=1)]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    seen = []

    def record(seed, row0, rows, n, device, raw=False):
        seen.append(torch.device(device))
        raise _Drawn()
    monkeypatch.setattr(AT, "philox_normal", record)
    for mul, b in ((False, None), (True, None), (True, torch.ones(2, 8))):
        with pytest.raises(_Drawn):
            AT.NoisyPerturbation(0.1, mul)(x, b)
    assert len(seen) == 3 and all(dv.type == "cuda" for dv in seen)
    with pytest.raises(ValueError):
        AT.NoisyPerturbation(0.1)(x[0])


class _Reached(Exception):
    pass


def test_sensitivity_does_not_pass_target_on():
    """target / additional_forward_args are checked as None and dropped: an explanation that does not take them runs."""
    def explain(w):
        raise _Reached()
    for kw in (dict(target=None), dict(additional_forward_args=None), dict(target=None, additional_forward_args=None)):
        with pytest.raises(_Reached):
            AT.sensitivity_max(explain, torch.zeros(2, 8), "cpu", perturb_func=lambda xe: xe, n_perturb_samples=2, seed=1, **kw)


def test_sensitivity_kwargs_expansion():
    B, L = 2, 4
    base = torch.arange(2.0)[:, None].expand(B, L)
    mask = torch.zeros(B, L, dtype=torch.int64)
    kw = AT.sensitivity_kwargs({"baselines": base, "feature_mask": mask, "n_steps": 3}, B, L, 3)
    assert kw["baselines"][:, 0].tolist() == [0, 0, 0, 1, 1, 1]
    assert kw["feature_mask"] is mask and kw["n_steps"] == 3               # feature_mask passes unchanged (unlike NoiseTunnel)
    one = torch.zeros(1, L)
    assert AT.sensitivity_kwargs({"baselines": one}, B, L, 3)["baselines"] is one
    assert AT.sensitivity_kwargs({"baselines": 0.5}, B, L, 3)["baselines"] == 0.5
    assert AT.sensitivity_kwargs({"baselines": base[:, :3]}, B, L, 3)["baselines"].shape == (B, 3)
    assert AT.expand_metric_baselines(base[:1], 1, L, 4).shape == (1, L)


def test_argument_errors_of_the_metric_entry_points():
    """include/addvisor_hip.h error contract (negative return, nothing launched): validation happens before any HIP call, so it
    runs without a GPU."""
    lib = _lib.lib()
    EINVAL = -1
    fb = (C.c_float * 256)()
    db = (C.c_double * 64)()
    pf, pd = C.addressof(fb), C.addressof(db)

    def rows(row0=0, n_rows=2, out=pf, dot=None, **f):
        d = dict(x=pf, attr=None, base=None, n=8, seed=1, B=2, S=3, s0=0, p=2, base_rows=1, mode=0, mul=0, scale=0.02)
        d.update(f)
        return lib.advh_metric_rows(C.byref(AT.MetricDesc(**d)), row0, n_rows, out, dot, None)

    for bad in (dict(x=None), dict(out=None), dict(n=0), dict(B=0), dict(S=0), dict(p=0), dict(s0=-1), dict(s0=2), dict(p=4),
                dict(row0=-1), dict(n_rows=0), dict(row0=3, n_rows=2), dict(n_rows=5), dict(scale=-1.0), dict(scale=float("nan")),
                dict(scale=float("inf")), dict(mode=2), dict(mode=-1), dict(dot=pf), dict(mul=1), dict(mode=1, attr=pf),
                dict(mode=1, dot=pf), dict(mode=1, attr=pf, dot=pf, mul=2), dict(mode=1, attr=pf, dot=pf, mul=1, base=pf,
                                                                                 base_rows=3)):
        assert rows(**bad) == EINVAL, bad
    rp = lambda q=pf, a=pf, B=2, p=2, n=8, o=pf: lib.advh_metric_row_dot(q, a, B, p, n, o, None)
    for bad in (dict(q=None), dict(a=None), dict(o=None), dict(B=0), dict(p=0), dict(n=0), dict(B=1 << 16, p=1 << 16)):
        assert rp(**bad) == EINVAL, bad
    fold = lambda dt=pf, f0=pf, fk=pf, B=2, p=2, nz=0, acc=pd: lib.advh_infidelity_fold(dt, f0, fk, B, p, nz, acc, None)
    for bad in (dict(dt=None), dict(f0=None), dict(fk=None), dict(acc=None), dict(B=0), dict(p=-1), dict(nz=2), dict(nz=-1)):
        assert fold(**bad) == EINVAL, bad
    fin = lambda acc=pd, B=2, S=3, nz=0, out=pf: lib.advh_infidelity_finalize(acc, B, S, nz, out, None)
    for bad in (dict(acc=None), dict(out=None), dict(B=0), dict(S=0), dict(S=-2), dict(nz=3)):
        assert fin(**bad) == EINVAL, bad
    nrm = lambda v=pf, r=2, n=8, o=0, out=pf: lib.advh_row_norm(v, r, n, o, out, None)
    for bad in (dict(v=None), dict(out=None), dict(r=0), dict(n=0), dict(o=-1), dict(o=3)):
        assert nrm(**bad) == EINVAL, bad
    sf = lambda e=pf, et=pf, en=pf, B=2, p=2, n=8, o=0, ratio=pf, smax=pf: lib.advh_sensitivity_fold(e, et, en, B, p, n, o, ratio,
                                                                                                    smax, None)
    for bad in (dict(e=None), dict(et=None), dict(en=None), dict(ratio=None), dict(smax=None), dict(B=0), dict(p=0), dict(n=-1),
                dict(o=5)):
        assert sf(**bad) == EINVAL, bad


def test_metric_kernels_do_not_spill():
    res = resources("attribution_metrics.hip")
    for nm in ("metric_rows_kernel", "row_dot_kernel", "row_norm_kernel", "max_fold_kernel", "infidelity_fold_kernel",
               "infidelity_finalize_kernel"):
        hit = {k: v for k, v in res.items() if nm in k}
        assert hit, (nm, sorted(res))
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
