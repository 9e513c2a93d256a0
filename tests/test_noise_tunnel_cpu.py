"""CPU-only: NoiseTunnel's front end and partition loop: names and signatures, the partition plan, the noise rows and the
delta order against a literal restatement of Captum's loop (tests/noise_tunnel_ref.py), the keyword expansion and the baseline
draws, argument checking before any GPU work, the error contract of advh_nt_fold / advh_nt_finalize, and their resource usage."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import noise_tunnel_ref as NR
from addvisor_hip import _lib, attribution as AT
from test_build_resources import resources

CASES = [(5, None), (6, 4), (6, 1), (7, 10)]


def captum_plan(S, batch):
    """Captum's loop, literally, over B clips: per partition ``(s0, size, [global (clip, sample) index of each row])``."""
    plan, s0 = [], 0
    for n in NR.partitions(S, batch):
        plan.append((s0, n, [b * S + s0 + s for b in range(3) for s in range(n)]))
        s0 += n
    return plan


def test_captum_names_and_signature():
    from captum.attr import NoiseTunnel
    import captum_saliency
    assert captum_saliency.NoiseTunnel is NoiseTunnel
    p = inspect.signature(NoiseTunnel.attribute).parameters
    assert list(p) == ["self", "inputs", "nt_type", "nt_samples", "nt_samples_batch_size", "stdevs", "draw_baseline_from_distrib",
                       "kwargs"]
    assert (p["nt_type"].default, p["nt_samples"].default, p["nt_samples_batch_size"].default, p["stdevs"].default,
            p["draw_baseline_from_distrib"].default) == ("smoothgrad", 5, None, 1.0, False)
    assert p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    p = inspect.signature(captum_saliency.explain_waves).parameters
    assert (p["method"].default, p["nt_type"].default, p["nt_samples"].default) == ("input_x_gradient", None, 5)
    assert AT.NT_TYPES == ("smoothgrad", "smoothgrad_sq", "vargrad")


@pytest.mark.parametrize("S,batch", CASES)
def test_partition_plan_matches_captum(S, batch):
    ours = AT.noise_tunnel_partitions(*AT.check_noise_tunnel_args("smoothgrad", S, batch)[:2])
    plan = captum_plan(S, batch)
    assert [(s0, n) for s0, n, _ in plan] == ours
    for (s0, n, rows) in plan:
        assert AT.noise_tunnel_rows(3, S, s0, n).tolist() == rows
    # every (clip, sample) is noised exactly once, whatever the partitioning
    assert sorted(g for _, _, rows in plan for g in rows) == list(range(3 * S))


class _FakeEngine(AT.HipAttribution):
    """The engine's partition loop on the CPU: the noisy rows hold their global (clip, sample) index (plus x), the fold and the
    finalize are numpy, nothing else of the engine is touched."""

    def __init__(self):
        pass

    def _prep(self, waves):
        return waves

    def _checked(self, out, what="", cause=None):
        return out


@pytest.fixture
def cpu_loop(monkeypatch):
    def rows(x, seed, S, s0, pp, stdevs, out=None):
        B, L = x.shape
        g = torch.from_numpy(AT.noise_tunnel_rows(B, S, s0, pp)).double()
        return x.repeat_interleave(pp, 0) + stdevs * g[:, None].expand(B * pp, L)

    def fold(attr, B, pp, total, total_sq):
        a = attr.double().view(B, pp, -1)
        for s in range(pp):
            total += a[:, s]
            total_sq += a[:, s] * a[:, s]

    def finalize(total, total_sq, S, nt_type):
        m, m2 = total / S, total_sq / S
        return {"smoothgrad": m, "smoothgrad_sq": m2, "vargrad": m2 - m * m}[nt_type].float()

    monkeypatch.setattr(AT, "nt_noisy_rows", rows)
    monkeypatch.setattr(AT, "nt_fold", fold)
    monkeypatch.setattr(AT, "nt_finalize", finalize)
    return _FakeEngine()


@pytest.mark.parametrize("S,batch", CASES)
def test_loop_rows_kwargs_and_delta_order(cpu_loop, S, batch):
    """The engine's loop: the rows it attributes, the kwargs each partition gets and the delta order are Captum's; the moments
    equal the restatement's given the same rows."""
    B, L = 3, 8
    x = torch.zeros(B, L, dtype=torch.float64)
    base = torch.arange(B, dtype=torch.float64)[:, None].expand(B, L).contiguous()
    seen = []

    def attribute(rows, baselines=None, feature_mask=None, n_steps=None, return_convergence_delta=False):
        seen.append((rows[:, 0].long().tolist(), baselines[:, 0].long().tolist(), feature_mask.shape, n_steps))
        a = torch.sin(rows + 0.5).float()
        return (a, rows[:, 0].clone()) if return_convergence_delta else a

    mask = torch.zeros(B, L, dtype=torch.int64)
    out, delta = cpu_loop.noise_tunnel(x, attribute, "vargrad", S, batch, 1.0, seed=5, return_convergence_delta=True,
                                       baselines=base, feature_mask=mask, n_steps=7)
    plan = captum_plan(S, batch)
    assert len(seen) == len(plan)
    for (rows, bl, fm, ns), (s0, n, want) in zip(seen, plan):
        assert rows == want                                                # row b * n + s' is (clip b, sample s0 + s')
        assert bl == [b for b in range(B) for _ in range(n)]              # [B, L] baselines repeat_interleaved
        assert tuple(fm) == (B * n, L) and ns == 7
    assert delta.long().tolist() == [g for _, _, rows in plan for g in rows]
    z = torch.arange(B * S, dtype=torch.float64).view(B, S, 1).expand(B, S, L)
    ref = NR.noise_tunnel(x, lambda w, **kw: torch.sin(w + 0.5).float(), "all", S, batch, 1.0, z=z)
    for nt, want in zip(AT.NT_TYPES, ref):
        got = cpu_loop.noise_tunnel(x, attribute, nt, S, batch, 1.0, seed=5, baselines=base, feature_mask=mask)
        assert torch.equal(got, want), nt


def test_loop_draws_baselines_from_the_distribution(cpu_loop):
    B, S, L, seed = 3, 6, 4, 123
    dist = torch.arange(5, dtype=torch.float64)[:, None].expand(5, L).contiguous()
    seen = []

    def attribute(rows, baselines=None):
        seen.append(baselines[:, 0].long().tolist())
        return rows

    cpu_loop.noise_tunnel(torch.zeros(B, L, dtype=torch.float64), attribute, "smoothgrad", S, 4, 0.0, True, seed=seed,
                          baselines=dist)
    idx = AT.noise_tunnel_baseline_draws(seed, B, S, 5)
    assert seen == [idx[AT.noise_tunnel_rows(B, S, s0, n)].tolist() for s0, n in ((0, 4), (4, 2))]
    assert seen[0] == [idx[b * S + s] for b in range(B) for s in range(4)]


def test_expansion_rules_and_draws_have_known_answers():
    L = 3
    b2 = torch.tensor([[1.0] * L, [2.0] * L])
    kw = AT.noise_tunnel_kwargs({"baselines": b2, "feature_mask": torch.tensor([[0, 0, 1], [1, 1, 0]]), "n_steps": 4,
                                 "method": "riemann_left", "sliding_window_shapes": (2,)}, 2, 3)
    assert kw["baselines"][:, 0].tolist() == [1, 1, 1, 2, 2, 2]
    assert kw["feature_mask"].tolist() == [[0, 0, 1]] * 3 + [[1, 1, 0]] * 3
    assert (kw["n_steps"], kw["method"], kw["sliding_window_shapes"]) == (4, "riemann_left", (2,))
    one, m1 = torch.ones(1, L), torch.zeros(1, L, dtype=torch.int64)
    for B in (1, 2):                                                      # [1, L] and numbers pass unchanged
        kw = AT.noise_tunnel_kwargs({"baselines": one, "feature_mask": m1}, B, 3)
        assert kw["baselines"] is one and kw["feature_mask"] is m1
        assert AT.noise_tunnel_kwargs({"baselines": 0.5}, B, 3)["baselines"] == 0.5
    assert AT.noise_tunnel_kwargs({"baselines": b2}, 3, 2)["baselines"] is b2         # first dimension != B: unchanged
    assert AT.noise_tunnel_kwargs({"feature_mask": None}, 2, 2)["feature_mask"] is None
    assert AT.noise_tunnel_kwargs({"baselines": b2[:1]}, 1, 4)["baselines"].shape == (1, L)     # B = 1: not expanded
    dist = torch.arange(5.0)[:, None].expand(5, L)
    kw = AT.noise_tunnel_kwargs({"baselines": dist}, 2, 2, drawn_rows=np.array([4, 0, 2, 2]))
    assert kw["baselines"][:, 0].tolist() == [4, 0, 2, 2]
    # numpy.random.Generator(PCG64(seed)).integers(0, N_b, B * S)
    assert AT.noise_tunnel_baseline_draws(7, 2, 4, 3).tolist() == [2, 1, 2, 2, 1, 2, 2, 0]
    assert AT.noise_tunnel_baseline_draws(123, 3, 3, 5).tolist() == [0, 3, 2, 0, 4, 1, 1, 0, 1]
    assert NR.baseline_draws(7, 2, 4, 3).tolist() == [2, 1, 2, 2, 1, 2, 2, 0]


def test_argument_checks():
    assert AT.check_noise_tunnel_args("vargrad", 6, 4, (0.25,)) == (6, 4, 0.25)
    assert AT.check_noise_tunnel_args("smoothgrad", 3, 10, 0) == (3, 3, 0.0)
    assert AT.check_noise_tunnel_args("smoothgrad_sq", np.int64(2), None, np.float32(0.5)) == (2, 2, 0.5)
    bad = [dict(nt_type="smoothgrad_abs"), dict(nt_type=None), dict(nt_samples=0), dict(nt_samples=-1), dict(nt_samples=2.0),
           dict(nt_samples=True), dict(nt_samples_batch_size=0), dict(nt_samples_batch_size=1.5), dict(stdevs=-0.1),
           dict(stdevs=float("inf")), dict(stdevs=float("nan")), dict(stdevs=(0.1, 0.2)), dict(stdevs=()), dict(stdevs="0.1"),
           dict(stdevs=True), dict(target=0)]
    for b in bad:
        args = dict(nt_type="smoothgrad", nt_samples=5, nt_samples_batch_size=None, stdevs=1.0, target=None)
        args.update(b)
        with pytest.raises(ValueError):
            AT.check_noise_tunnel_args(**args)


class _NoEngine:
    def hip_attribution(self):
        raise AssertionError("the front end reached the engine before rejecting its arguments")


def test_front_end_validates_before_gpu_work():
    from captum.attr import (FeatureAblation, GradientShap, InputXGradient, IntegratedGradients, KernelShap, NoiseTunnel, Occlusion,
                             Saliency, ShapleyValueSampling, ShapleyValues)
    x = torch.zeros(2, 100)
    m = _NoEngine()
    sal, ig, gs = NoiseTunnel(Saliency(m)), NoiseTunnel(IntegratedGradients(m)), NoiseTunnel(GradientShap(m))
    calls = []
    for nt in (sal, ig, NoiseTunnel(Occlusion(m)), NoiseTunnel(KernelShap(m))):
        calls += [lambda nt=nt: nt.attribute(x, nt_type="smoothgrad_abs"), lambda nt=nt: nt.attribute(x, nt_samples=0),
                  lambda nt=nt: nt.attribute(x, nt_samples=2.5), lambda nt=nt: nt.attribute(x, nt_samples_batch_size=0),
                  lambda nt=nt: nt.attribute(x, stdevs=-1.0), lambda nt=nt: nt.attribute(x, stdevs=float("nan")),
                  lambda nt=nt: nt.attribute(x, stdevs=float("inf")), lambda nt=nt: nt.attribute(x, stdevs=(0.1, 0.1)),
                  lambda nt=nt: nt.attribute(x, target=0), lambda nt=nt: nt.attribute(x[0])]
    calls += [lambda: sal.attribute(x, return_convergence_delta=True),
              lambda: NoiseTunnel(Occlusion(m)).attribute(x, sliding_window_shapes=(10,), return_convergence_delta=True),
              lambda: ig.attribute(x, draw_baseline_from_distrib=True),                           # no distribution
              lambda: ig.attribute(x, draw_baseline_from_distrib=True, baselines=0.5),
              lambda: ig.attribute(x, draw_baseline_from_distrib=True, baselines=torch.zeros(3, 99)),
              lambda: gs.attribute(x, draw_baseline_from_distrib=True, baselines=torch.zeros(3, 100, dtype=torch.int64))]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    for call in (lambda: sal.attribute(x), lambda: ig.attribute(x, return_convergence_delta=True, n_steps=4),
                 lambda: gs.attribute(x, baselines=torch.zeros(3, 100), draw_baseline_from_distrib=True, stdevs=(0.1,)),
                 lambda: NoiseTunnel(InputXGradient(m)).attribute(x, nt_type="vargrad", nt_samples_batch_size=2),
                 lambda: NoiseTunnel(FeatureAblation(m)).attribute(x, stdevs=0),
                 lambda: NoiseTunnel(ShapleyValueSampling(m)).attribute(x, nt_samples=1),
                 lambda: NoiseTunnel(ShapleyValues(m)).attribute(x, nt_type="smoothgrad_sq")):
        with pytest.raises(AssertionError):                               # valid arguments go on to the engine
            call()
    for bad in (object(), sal, Saliency, None):
        with pytest.raises(TypeError):
            NoiseTunnel(bad)
    assert ig.has_convergence_delta() and gs.is_delta_supported and not sal.has_convergence_delta()


def test_engine_validates_before_gpu_work():
    class Stub(AT.HipAttribution):
        def __init__(self):
            pass

        def _prep(self, waves):
            raise AssertionError("the engine reached the device before rejecting its arguments")

    eng = Stub()
    x = torch.zeros(2, 100)
    for kw in (dict(nt_type="x"), dict(nt_samples=0), dict(nt_samples_batch_size=-2), dict(stdevs=-1.0), dict(stdevs=(1.0, 2.0)),
               dict(seed=-1), dict(seed=2 ** 64), dict(draw_baseline_from_distrib=True),
               dict(draw_baseline_from_distrib=True, baselines=torch.zeros(2, 50))):
        with pytest.raises(ValueError):
            eng.noise_tunnel(x, eng.saliency, **kw)
    with pytest.raises(ValueError):                                       # saliency has no delta
        eng.noise_tunnel(x, eng.saliency, return_convergence_delta=True)
    with pytest.raises(ValueError):
        eng.noise_tunnel(torch.zeros(2, 3, 4), eng.saliency)
    for ok in (dict(), dict(return_convergence_delta=True)):
        with pytest.raises(AssertionError):
            eng.noise_tunnel(x, eng.integrated_gradients, **ok)


def test_argument_errors_of_the_noise_tunnel_entry_points():
    """include/addvisor_hip.h error contract (negative return, nothing launched): validation happens before any HIP call, so it
    runs without a GPU."""
    lib = _lib.lib()
    EINVAL = -1
    fb = (C.c_float * 64)()
    db = (C.c_double * 64)()
    pf, pd = C.addressof(fb), C.addressof(db)
    fold = lambda attr=pf, B=2, p=3, n=8, s=pd, q=pd: lib.advh_nt_fold(attr, B, p, n, s, q, None)
    fin = lambda s=pd, q=pd, B=2, n=8, S=3, t=0, out=pf: lib.advh_nt_finalize(s, q, B, n, S, t, out, None)
    for bad in (dict(attr=None), dict(s=None), dict(q=None), dict(B=0), dict(B=-1), dict(p=0), dict(p=-3), dict(n=0), dict(n=-8)):
        assert fold(**bad) == EINVAL, bad
    for bad in (dict(s=None), dict(q=None), dict(out=None), dict(B=0), dict(n=0), dict(n=-1), dict(S=0), dict(S=-2), dict(t=-1),
                dict(t=3)):
        assert fin(**bad) == EINVAL, bad


def test_noise_tunnel_kernels_do_not_spill():
    res = resources("attribution_paths.hip")
    for nm in ("nt_fold_kernel", "nt_finalize_kernel", "path_points_kernel"):
        hit = {k: v for k, v in res.items() if nm in k}
        assert hit, (nm, sorted(res))
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
