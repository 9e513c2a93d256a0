"""GPU: Captum's FGSM and PGD (captum.robust, HipRobust.fgsm / pgd / fgsm_min_epsilon) against tests/robust_ref.py: the step
kernel's bits against the numpy model (float4 and scalar forms, row windows, in place), the random start against the Philox
model, a replay of every step of a device trace, one-step parity and multi-step outcome against the oracle's attack, the
epsilon ladder, the front ends and wav2vec2-base at 4 s."""
import math
import os

import numpy as np
import pytest
import torch

import robust_ref as RR
from addvisor_hip import attribution as AT, robust as RB, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.robust import HipRobust
from oracle import attribution_ref as A

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": 1e-4, "f16": 3e-2}                # the attribution bars (max |err| / max |ref|) of the attribution tests
# Measured on the MI355X (tiny config, 2 clips x 1 s): the step kernel and the Linf random start equal the numpy model bit for bit,
# every Linf trace replays bit for bit and every L2 one inside the bar; one FGSM step (f32): 0 of 32 000 elements differ from the
# oracle's (exempt share 0.25 %); PGD of 5 steps of 5e-4, the oracle's logit at the device's clip against its logit at its own,
# |delta| / |shift|: f32 0 (Linf) and 8.4e-6 (L2) against a bar of 3e-3, f16 6.8e-5 (Linf) and 5.4e-4 (L2) against 1.2 / 0.71 (ten
# times the CPU emulation at the f16 attribution bar); the L2 random start's distance within 4e-7 relative of radius * u^(1/n);
# wav2vec2-base at 4 s: the device's logit at its adversarial clip within 8.3e-7 of the oracle's.
INF = math.inf
B, L = 2, 16000
L2_REL, L2_ABS = 1e-5, 1e-12
# The L2 bar: a 256-thread tree over <= 5000 squares has at most 20 serial adds plus 8 tree levels, ~30 * 2^-24 ~ 2e-6 relative
# on the norm; the bar is 5 x that, relative to the output element (+ 1e-12 absolute).

_CACHE = {}


def setup(dev, precision, cfg_name="tiny"):
    key = (cfg_name, precision)
    if key not in _CACHE:
        cfg = syn.tiny_config(False) if cfg_name == "tiny" else syn.base_config()
        sd = syn.embedder_weights(cfg)
        coef, icpt = syn.logreg_weights(cfg.hidden_size)
        att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision))
        _CACHE[key] = (HipRobust(att), (sd, cfg, coef, icpt))
    return _CACHE[key]


def clips(length=L, seed=41, n=B):
    return syn.make_clips(n, length, seed=seed)


def lifted(w):
    """Clips moved off zero, into [0.05, 0.95].  The L2 bar is relative to the output element x0 + d * factor while the norm's
    error enters through d * factor: where x0 + d cancels, the bar would measure the cancellation.  With |x0| >= 0.05 and
    ||d|| <= 5e-2 over 16000 samples no element cancels."""
    return 0.5 + 0.45 * w / w.abs().max()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _step_data(n, Bx, p, away):
    rng = np.random.default_rng(n + p)
    x0 = rng.uniform(-1, 1, (Bx, n)).astype(np.float32)
    if away:                                              # see lifted()
        x0 = (np.sign(x0) * (0.2 + 0.8 * np.abs(x0))).astype(np.float32)
    x0e = np.repeat(x0, p, 0)
    xe = (x0e + rng.uniform(-0.04, 0.04, (Bx * p, n))).astype(np.float32)
    xe[:p] = x0e[:p]                                      # clip 0 starts at its clean clip: inside the L2 ball after a small step
    ge = (rng.standard_normal((Bx * p, n)) * 10.0 ** rng.uniform(-8, 0, (Bx * p, n))).astype(np.float32)
    plant = np.array([0.0, -0.0, 1e-6, -1e-6, 1.0000001e-6, -1.0000001e-6], np.float32)
    ge[:, 7:7 + plant.size] = plant
    ge[:, n - plant.size:] = plant[::-1]
    mask = (rng.uniform(0, 1, (Bx, n)) > 0.3).astype(np.float32)
    mask[:, 20:30] = 0.5
    return x0, x0e, xe, ge, mask


def _offset(t, dev, misalign):
    """``t`` on the device, contiguous; ``misalign``: its base pointer one float past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(t))
    if not misalign:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


STEP_CASES = [  # p, expanded x / grad rows, mask, seed, targeted, (lo, hi), misaligned
    (1, True, None, None, False, (-INF, INF), False),
    (1, True, "1", "mixed", True, (-0.5, 0.7), False),
    (1, True, "B", "mixed", False, (-INF, 0.4), True),
    (3, False, None, "mixed", False, (-0.9, INF), False),
    (3, True, "B", None, True, (-INF, INF), False),
    (3, False, "1", "mixed", True, (-0.5, 0.7), True),
]


@pytest.mark.parametrize("n", [1000, 1001, 5000])
def test_step_kernel_bits(gpu_device, n):
    dev = gpu_device
    Bx, radius = 3, 0.35
    for p, expanded, mk, sk, targeted, (lo, hi), mis in STEP_CASES:
        eps = [1e-3, 2e-3, 4e-3][:p]
        seed = None if sk is None else np.array([0.37, 0.0, -0.64], np.float32)
        for norm in (0, 1, 2):
            x0, x0e, xe, ge, mask = _step_data(n, Bx, p, away=norm == 2)
            m = None if mk is None else (mask[:1] if mk == "1" else mask)
            R = Bx * p
            xs, gs = (xe, ge) if expanded else (xe[::p], ge[::p])           # B rows: each clip's first row
            xm, gm = (xe, ge) if expanded else (np.repeat(xs, p, 0), np.repeat(gs, p, 0))
            want = RR.step(x0e, xm, gm, None if seed is None else np.repeat(seed, p), None if m is None else np.repeat(m, p, 0) if
                           m.shape[0] == Bx else m, np.tile(eps, Bx), -1 if targeted else 1, radius, norm, lo, hi)
            tx0, tx, tg = _offset(x0, dev, mis), _offset(xs, dev, mis), _offset(gs, dev, mis)
            ts = None if seed is None else torch.from_numpy(seed).to(dev)
            tm = None if m is None else _offset(m, dev, mis)
            call = lambda out, row0=0, rows=None, x=tx: RB.robust_step(None if norm == 0 else tx0, x, tg, ts, tm, eps, targeted, norm,
                                                                       radius, lo, hi, out, row0, rows, B=Bx)
            one = call(_offset(np.zeros((R, n), np.float32), dev, mis)).cpu().numpy()
            two = torch.full((R, n), 7.0, device=dev)
            h = R // 2 + 1 if R > 2 else 1
            call(two[:h], 0, h)
            call(two[h:], h, R - h)
            assert np.array_equal(bits(one), bits(two.cpu().numpy())), (n, p, norm, "row window")
            if expanded:                                                   # in place: out is the rows of x
                xin = _offset(xs, dev, mis)
                call(xin, x=xin)
                assert np.array_equal(bits(one), bits(xin.cpu().numpy())), (n, p, norm, "in place")
            tag = (n, p, expanded, mk, sk, targeted, lo, hi, mis, norm)
            if norm != 2:
                assert np.array_equal(bits(one), bits(want)), tag
                continue
            err = np.abs(one.astype(np.float64) - want)
            assert np.all(err <= L2_REL * np.abs(want) + L2_ABS), (tag, err.max())
            v = RR.step(None, xm, gm, None if seed is None else np.repeat(seed, p), None if m is None else np.repeat(m, p, 0) if
                        m.shape[0] == Bx else m, np.tile(eps, Bx), -1 if targeted else 1, 0.0, 0, -INF, INF)
            s = np.sqrt(((v - x0e).astype(np.float64) ** 2).sum(1))
            inside = s <= radius * (1 - 1e-4)
            assert inside[:p].all() and not inside[p:].any(), (tag, s)     # clip 0 inside the ball, the others outside
            # inside the ball the factor is exactly 1: the row is the unprojected v through Captum's own x0 + (v - x0), bit for bit
            assert np.array_equal(bits(one[inside]), bits(want[inside])), tag
            if lo == -INF and hi == INF:
                assert np.array_equal(bits(one[inside]), bits(x0e[inside] + (v[inside] - x0e[inside]))), tag
                dist = np.sqrt(((one.astype(np.float64) - x0e) ** 2).sum(1))
                assert np.all(dist <= radius * (1 + 1e-5)), (tag, dist)
                assert np.all(dist[~inside] >= radius * (1 - 1e-5)), (tag, dist)


def test_random_start(gpu_device):
    dev = gpu_device
    seed, radius = 0x5EED_0123_4567, 0.02
    for n in (1000, 1001):
        x = clips(n, n=3)
        xn, xd = x.numpy(), x.to(dev)
        for lo, hi in ((-INF, INF), (-0.05, 0.05)):
            got = RB.random_point(xd, seed, 1, radius, lo, hi)
            assert np.array_equal(bits(got.cpu().numpy()), bits(RR.random_start(xn, seed, 1, radius, lo, hi))), (n, lo)
            rows = AT.uniform_rows(xd, seed, 1, 0, 1, radius)
            assert torch.equal(got, rows.clamp(min=lo, max=hi)), (n, lo)
            assert torch.equal(got, RB.random_point(xd, seed, 1, radius, lo, hi))
            assert not torch.equal(got, RB.random_point(xd, seed + 1, 1, radius, lo, hi))
            got2 = RB.random_point(xd, seed, 2, radius, lo, hi)
            want, r = RR.random_start(xn, seed, 2, radius, lo, hi)
            assert np.all(np.abs(got2.cpu().double().numpy() - want) <= 2e-6 * (1 + np.abs(want))), (n, lo)
            assert torch.equal(got2, RB.random_point(xd, seed, 2, radius, lo, hi))
            assert not torch.equal(got2, RB.random_point(xd, seed + 1, 2, radius, lo, hi))
            if lo == -INF:
                dist = np.sqrt(((got2.cpu().double().numpy() - xn.astype(np.float64)) ** 2).sum(1))
                print(f"L2 random start n={n}: distance {dist.tolist()} vs radius * u^(1/n) {r.tolist()}")
                assert np.all(np.abs(dist - r) <= 1e-5 * r) and np.all(r < radius) and np.all(r > 0.9 * radius)
                lin = (got.cpu() - x).abs().max().item()
                assert 0.9 * radius < lin <= radius * (1 + 1e-6)


def _mask(length=L):
    m = torch.ones(1, length)
    m[:, 1000:3000] = 0.0
    m[:, 9000:9500] = 0.5
    return m


def _replay(x0, trace, final, mask, step_size, targeted, radius, norm, lo, hi):
    """Every step of a device trace through the numpy model: the next iterate bit for bit (Linf) or at the L2 bar."""
    code = RB.NORMS[norm]
    for k, (xk, gk, sk) in enumerate(trace):
        nxt = (trace[k + 1][0] if k + 1 < len(trace) else final).cpu().numpy()
        want = RR.step(x0.numpy(), xk.cpu().numpy(), gk.cpu().numpy(), sk.cpu().numpy(), None if mask is None else mask.numpy(),
                       step_size, -1 if targeted else 1, radius, code, lo, hi)
        if code == 1:
            assert np.array_equal(bits(nxt), bits(want)), (norm, targeted, k)
        else:
            err = np.abs(nxt.astype(np.float64) - want)
            assert np.all(err <= L2_REL * np.abs(want) + L2_ABS), (norm, targeted, k, err.max())


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_trace_replay(gpu_device, precision):
    rob, _ = setup(gpu_device, precision)
    dev = gpu_device
    mask = _mask()
    tgt = torch.tensor([1, 0])
    bce = lambda out, t: torch.nn.functional.binary_cross_entropy_with_logits(out, t.view(-1, 1).float(), reduction="sum")
    for norm, radius, x0 in (("Linf", 2e-3, clips()), ("L2", 5e-2, lifted(clips()))):
        for targeted in (False, True):
            trace = []
            out = rob.pgd(x0.to(dev), radius, 5e-4, 4, tgt, targeted=targeted, random_start=True, norm=norm, mask=mask,
                          lower_bound=-1.0, upper_bound=1.0, seed=77, trace=trace)
            assert len(trace) == 4 and out.shape == (B, L)
            start = RB.random_point(x0.to(dev), 77, RB.NORMS[norm], radius, -1.0, 1.0)
            assert torch.equal(trace[0][0], start)
            _replay(x0, trace, out, mask, 5e-4, targeted, radius, norm, -1.0, 1.0)
            for xk, _, sk in trace:                                    # the default loss's seed: prob - target
                prob = rob.eg.forward(xk)[1].view(-1)
                assert torch.equal(sk, prob - tgt.to(dev).float()), (norm, targeted)
            assert float(out.max()) <= 1.0 and float(out.min()) >= -1.0
        trace2 = []
        rob.pgd(x0.to(dev), radius, 5e-4, 1, tgt, loss_func=bce, random_start=True, norm=norm, mask=mask, lower_bound=-1.0,
                upper_bound=1.0, seed=77, trace=trace2)
        assert torch.equal(trace2[0][0], trace[0][0])
        err = (trace2[0][2] - trace[0][2]).abs().max().item()
        print(f"[{precision}] {norm}: callable BCE seed vs default, max |err| {err:.3e}")
        assert err <= 1e-6


def test_one_step_parity_against_the_oracle(gpu_device):
    """f32, FGSM, epsilon 1e-3: outside the elements whose sign or threshold the f32 attribution bar cannot decide, the device's
    adversarial clip equals the oracle's bit for bit.  The exempt share is capped at 1 % (the oracle alone: 0.25 % for these
    inputs and targets, computed on the CPU)."""
    rob, model = setup(gpu_device, "f32")
    x = clips()
    tgt = torch.tensor([1, 0])
    g = RR.loss_gradient(x, tgt, model)
    band = TOL["f32"] * g.abs().max()
    exempt = (g.abs() < band) | ((g.abs() - 1e-6).abs() < band)
    share = exempt.float().mean().item()
    for targeted in (False, True):
        ours = rob.fgsm(x.to(gpu_device), 1e-3, tgt, targeted=targeted).cpu()
        ref = RR.fgsm(x, 1e-3, tgt, model, targeted=targeted)
        diff = (ours.view(torch.int32) != ref.view(torch.int32))
        print(f"FGSM one step (targeted={targeted}): {int(diff.sum())} elements differ, {int((diff & ~exempt).sum())} outside the exempt "
              f"set; exempt share {share:.4%}")
        assert share <= 0.01
        assert not bool((diff & ~exempt).any())
        step = (ours.double() - x.double()).abs().max().item()          # epsilon, to the rounding of x + e (|x| < 1: half an ulp <= 2^-25)
        assert 0.9e-3 < step <= float(np.float32(1e-3)) + 2.0 ** -25


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_multi_step_outcome_against_the_oracle(gpu_device, precision):
    """PGD Linf (radius 2e-3) and L2 (radius 5e-2), 5 steps of 5e-4: the oracle's logit at the device's adversarial clip against
    its logit at its own.  On the CPU, the oracle's attack with a Gaussian gradient error of 1e-4 max|g| per step moves the final
    logit by <= 1.4e-4 against a shift of 0.19 - 0.97: the f32 bar is |delta logit| <= 3e-3 |shift|; the f16 bar is 10 x the same
    emulation at 3e-2 max|g|, computed here.
    Measured on the MI355X, |delta logit| / |shift|: f32 0 (Linf), 8.4e-6 (L2); f16 6.8e-5 (Linf), 5.4e-4 (L2), against f16 bars of
    1.2 and 0.71 from the emulation."""
    rob, model = setup(gpu_device, precision)
    dev = gpu_device
    x = clips()
    tgt = torch.tensor([1, 0])
    z0 = A.model_logit(x, *model).view(-1)
    for norm, radius in (("Linf", 2e-3), ("L2", 5e-2)):
        ref = RR.pgd(x, radius, 5e-4, 5, tgt, model, norm=norm)
        zr = A.model_logit(ref, *model).view(-1)
        shift = (zr - z0).abs()
        if precision == "f32":
            rel = 3e-3
        else:
            gen = torch.Generator().manual_seed(3)

            def noisy(k, cur):
                gg = RR.loss_gradient(cur, tgt, model)
                return gg + TOL["f16"] * gg.abs().max() * torch.randn(gg.shape, generator=gen)
            zn = A.model_logit(RR.pgd(x, radius, 5e-4, 5, tgt, model, norm=norm, grad_fn=noisy), *model).view(-1)
            rel = 10 * ((zn - zr).abs() / shift).max().item()
        ours = rob.pgd(x.to(dev), radius, 5e-4, 5, tgt, norm=norm).cpu()
        zd = A.model_logit(ours, *model).view(-1)
        ratio = ((zd - zr).abs() / shift).max().item()
        print(f"PGD {norm} [{precision}]: oracle logit at the device's clip vs at its own, |delta| / |shift| = {ratio:.3e} "
              f"(bar {rel:.3e}; shift {shift.tolist()})")
        assert ratio <= rel, (norm, ratio, rel)
        # properties
        base = RR.bce(x, tgt, model)
        assert bool((RR.bce(ours, tgt, model) > base).all()), norm
        assert bool((RR.bce(rob.pgd(x.to(dev), radius, 5e-4, 5, tgt, targeted=True, norm=norm).cpu(), tgt, model) < base).all()), norm
        mask = _mask()
        tg = rob.pgd(x.to(dev), radius, 5e-4, 5, tgt, targeted=True, norm=norm, mask=mask, lower_bound=-0.5, upper_bound=0.5).cpu()
        assert float(tg.max()) <= 0.5 and float(tg.min()) >= -0.5 and float(x.abs().max()) > 0.5      # the bounds hold, and bind
        xc = x.clamp(-0.5, 0.5)
        off = (mask[0] == 0)
        assert torch.equal(tg[:, off], xc[:, off])                    # masked-out samples: the (bounded) clean clip
        free = rob.pgd(x.to(dev), radius, 5e-4, 5, tgt, norm=norm, mask=mask).cpu()
        assert torch.equal(free[:, off], x[:, off])
        for adv in (ours, free):
            d = adv.double() - x.double()
            if norm == "Linf":
                ulp = torch.from_numpy(np.spacing(np.abs(adv.numpy()))).double()
                assert bool((d.abs() <= float(np.float32(radius)) + ulp).all())
            else:
                assert bool((d.pow(2).sum(1).sqrt() <= radius * (1 + 1e-5)).all())
        assert torch.equal(rob.pgd(x.to(dev), radius, 5e-4, 0, tgt, norm=norm).cpu(), x)
        alone = rob.pgd(x[:1].to(dev), radius, 5e-4, 5, tgt[:1], norm=norm).cpu()
        assert torch.equal(alone[0], ours[0]), norm                    # the result does not depend on the batch


def test_ladder(gpu_device):
    rob, _ = setup(gpu_device, "f32")
    dev = gpu_device
    x = clips().to(dev)
    eps = [2.5e-4, 5e-4, 1e-3, 2e-3, 4e-3, 8e-3]
    K = len(eps)
    mask = _mask().to(dev)
    rec = {}
    eps_min, adv = rob.fgsm_min_epsilon(x, eps, 0, mask=mask, lower_bound=-1.0, upper_bound=1.0, record=rec)
    assert eps_min.shape == (B,) and adv.shape == (B, L) and rec["ladder"].shape == (B, K, L)
    for k, e in enumerate(eps):
        assert torch.equal(rec["ladder"][:, k], rob.fgsm(x, e, 0, mask=mask, lower_bound=-1.0, upper_bound=1.0)), k
    want, first = RB.first_flip(rec["logits"].cpu().numpy(), rec["clean_logits"].cpu().numpy(), eps)
    print(f"ladder: eps_min {eps_min.tolist()}, first {rec['first'].tolist()}, logits {rec['logits'].tolist()}")
    assert np.array_equal(bits(eps_min.cpu().numpy()), bits(want)) and np.array_equal(rec["first"].cpu().numpy(), first)
    assert np.isfinite(want).any()
    for b in range(B):
        assert torch.equal(adv[b], rec["ladder"][b, first[b]] if first[b] < K else x[b])
    rec2 = {}
    eps2, adv2 = rob.fgsm_min_epsilon(x, eps, 0, mask=mask, lower_bound=-1.0, upper_bound=1.0, internal_batch_size=K, record=rec2)
    assert torch.equal(eps2, eps_min) and torch.equal(adv2, adv) and torch.equal(rec2["logits"], rec["logits"])
    tiny, same = rob.fgsm_min_epsilon(x, [1e-9, 2e-9], 0)
    assert bool(torch.isinf(tiny).all()) and torch.equal(same, x)
    # targeted towards the current decision never flips it
    keep, _ = rob.fgsm_min_epsilon(x, eps[:3], 0, targeted=True)
    assert bool(torch.isinf(keep).all())


@pytest.fixture
def tiny_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_captum_front_end_and_attack_waves(gpu_device, tiny_runtime):
    import captum_saliency as cs
    from captum.robust import FGSM, PGD
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(gpu_device)
    eng = model.hip_robust()
    assert eng is model.hip_robust() and eng.att is model.hip_attribution()
    x = clips(seed=45).to(gpu_device)
    tgt = torch.tensor([0, 1])
    a = FGSM(model, lower_bound=-1.0, upper_bound=1.0).perturb(x, 1e-3, tgt, targeted=True)
    assert torch.equal(a, eng.fgsm(x, 1e-3, tgt, targeted=True, lower_bound=-1.0, upper_bound=1.0))
    torch.manual_seed(5)
    p1 = PGD(model).perturb(x, 2e-3, 5e-4, 2, tgt, random_start=True, norm="L2")
    torch.manual_seed(5)
    assert torch.equal(p1, eng.pgd(x, 2e-3, 5e-4, 2, tgt, random_start=True, norm="L2"))
    assert not torch.equal(p1, PGD(model).perturb(x, 2e-3, 5e-4, 2, tgt, random_start=True, norm="L2"))
    assert torch.equal(PGD(model).perturb(x, 2e-3, 5e-4, 2, tgt), eng.pgd(x, 2e-3, 5e-4, 2, tgt))
    for attack, kw in (("pgd", dict(step_num=2)), ("fgsm", dict(epsilon=5e-4, lower_bound=-1.0, upper_bound=1.0))):
        out = cs.attack_waves(model, x, tgt, attack=attack, explain="saliency", **kw)
        assert set(out) == {"predictions", "adversarial_predictions", "adversarial", "explanation_shift"}
        assert out["predictions"].shape == (B, 1) and out["adversarial_predictions"].shape == (B, 1)
        assert out["adversarial"].shape == (B, L) and out["explanation_shift"].shape == (B,)
        att = model.hip_attribution()
        e, et = att.saliency(x), att.saliency(out["adversarial"])
        shift = torch.zeros(B, device=gpu_device)
        AT.sensitivity_fold(e, et, AT.row_norm(e, 0), 1, 0, shift)
        assert torch.equal(out["explanation_shift"], shift)
        ref = ((et.double() - e.double()).norm(dim=1) / e.double().norm(dim=1)).cpu()
        print(f"attack_waves({attack}): explanation_shift {shift.tolist()}, predictions {out['predictions'].view(-1).tolist()} -> "
              f"{out['adversarial_predictions'].view(-1).tolist()}")
        assert bool(((shift.cpu().double() - ref).abs() <= 1e-5 * ref).all())
    assert set(cs.attack_waves(model, x, tgt, attack="fgsm")) == {"predictions", "adversarial_predictions", "adversarial"}
    with pytest.raises(ValueError):
        cs.attack_waves(model, x, tgt, attack="cw")


def test_base_4s(gpu_device):
    """wav2vec2-base, 2 clips x 4 s, f32: PGD Linf, 2 steps; the trace replays bit for bit, the result is finite, and the oracle's
    logit at the device's adversarial clip is within the forward's logit bar (1e-4) of the device's own logit there."""
    rob, model = setup(gpu_device, "f32", "base")
    x = syn.make_clips(2, 64000)
    tgt = torch.tensor([0, 1])
    trace = []
    out = rob.pgd(x.to(gpu_device), 2e-3, 1e-3, 2, tgt, trace=trace)
    assert len(trace) == 2 and bool(torch.isfinite(out).all())
    _replay(x, trace, out, None, 1e-3, False, 2e-3, "Linf", -INF, INF)
    zd = rob.att.logits(out).cpu()
    zo = A.model_logit(out.cpu(), *model).view(-1)
    err = (zd - zo).abs().max().item()
    print(f"base 4 s PGD: device logit {zd.tolist()} vs oracle at the same clip {zo.tolist()}, |err| {err:.3e}")
    assert err <= 1e-4
