"""GPU: Captum's infidelity and sensitivity_max (captum.metrics, HipAttribution.infidelity / sensitivity_max) against the
Captum-style restatement of tests/metrics_ref.py: the device rows (uniform bit for bit against numpy, Gaussian within the
generator's bar, fused = generic bit for bit), infidelity over Saliency / InputXGradient / IG attributions, sensitivity_max
over Saliency / IG / NoiseTunnel(Saliency) in three norms, the metrics' properties, the chunkings, the front ends and
wav2vec2-base at 4 s."""
import math
import os

import numpy as np
import pytest
import torch

import attribution_baselines_ref as R
import metrics_ref as MR
import noise_tunnel_ref as NR
from addvisor_hip import attribution as AT, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution, NoisyPerturbation
from addvisor_hip.embedder import HipEmbedder

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": 1e-4, "f16": 3e-2}                # the attribution bars (max |err| / max |ref|) of the attribution tests
TOL_LOGIT = {"f32": 1e-4, "f16": 1e-2}          # the perturbation methods' logit parity (tests/test_gpu_ablation.py)
RADIUS = {"f32": 0.02, "f16": 0.1}              # f16: a larger radius keeps the metric well above its error
# Measured on the MI355X (tiny config, 2 clips x 1 s, S = 4): infidelity within 2.7e-7 of the restatement in f32 (Saliency,
# 1/200 of its propagated bound) and 1.8e-4 in f16 (1/30 of the bound); sensitivity_max within 1.3e-6 (f32, NoiseTunnel(Saliency))
# and 6.4e-3 (f16, IG, max norm) against a bar of 2e-4 / 6e-2, metric values 0.08 - 0.25 (f32) and 0.37 - 1.2 (f16); the device
# uniform rows equal numpy's bit for bit and the fused Gaussian rows and dots equal the generic path's bit for bit; every chunking
# of both metrics was bit-identical; wav2vec2-base at 4 s: infidelity 7.6e-9 (bound 8.2e-6), sensitivity_max 1.1e-8.  The
# fold and finalize kernels equal tests/metrics_ref.py's numpy model bit for bit over every chunk plan.
B, L, S, SIGMA = 2, 16000, 4, 0.01

_CACHE = {}


def setup(dev, precision, cfg_name="tiny"):
    key = (cfg_name, precision)
    if key not in _CACHE:
        cfg = syn.tiny_config(False) if cfg_name == "tiny" else syn.base_config()
        sd = syn.embedder_weights(cfg)
        coef, icpt = syn.logreg_weights(cfg.hidden_size)
        _CACHE[key] = (HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision)), (sd, cfg, coef, icpt))
    return _CACHE[key]


def clips(length=L, seed=41, n=B):
    return syn.make_clips(n, length, seed=seed)


def baseline(n, length, seed):
    return 0.05 * torch.randn(n, length, generator=torch.Generator().manual_seed(seed))


class DeviceNoisy:
    """A Python perturb_func built from philox_normal on the device: its calls take the chunks in order, chunk ``[s0, s0 + n)``
    getting ``(sigma N(seed, b * S + s0 + s', :), x - sigma N)``, or the decorator's perturbation when ``mul`` -- the generic
    path's twin of NoisyPerturbation's fused rows."""

    def __init__(self, seed, Bx, S_, sigma, mul=False, s0=0):
        self.seed, self.B, self.S, self.sigma, self.mul, self.s0 = seed, Bx, S_, sigma, mul, s0

    def __call__(self, xe, be=None):
        n = xe.shape[0] // self.B
        z = torch.cat([AT.philox_normal(self.seed, b * self.S + self.s0, n, xe.shape[1], xe.device) for b in range(self.B)])
        self.s0 += n
        noise = self.sigma * z
        xt = xe - noise
        if not self.mul:
            return noise, xt
        den = xe if be is None else xe - be
        return (xe - xt) / torch.where(den != 0, den, torch.ones_like(den)), xt


def test_rows_against_numpy_and_the_generic_path(gpu_device):
    dev = gpu_device
    seed = 0x5EED_0123_4567
    for length in (1000, 1001):                                       # float4 and scalar forms
        x = clips(length).to(dev)
        xn = x.cpu().numpy()
        attr = torch.randn(B, length, generator=torch.Generator().manual_seed(3)).to(dev)
        base = baseline(B, length, 4).to(dev)
        for s0, pp in AT.metric_partitions(B, 5, 2 * B) + [(0, 5)]:
            u = AT.uniform_rows(x, seed, 5, s0, pp, 0.02)
            want = MR.uniform_rows(xn, seed, 5, s0, pp, 0.02)
            assert np.array_equal(u.cpu().numpy().view(np.uint32), want.view(np.uint32)), (length, s0, pp)
            R_ = B * pp
            zero = torch.zeros_like(x)
            rows, dot = torch.empty(R_, length, device=dev), torch.empty(R_, device=dev)
            AT.metric_rows(AT.metric_desc(zero, seed, 5, s0, pp, AT.MR_GAUSS, 1.0, attr), 0, R_, rows, dot)
            z = torch.cat([AT.philox_normal(seed, b * 5 + s0, pp, length, dev) for b in range(B)])
            assert torch.equal(-rows, z)                              # 0 - 1 * z
            zr = np.concatenate([R.philox_normal(seed, b * 5 + s0, pp, length) for b in range(B)])
            assert np.all(np.abs(-rows.cpu().double().numpy() - zr) <= 2e-6 * (1 + np.abs(zr)))
            for mul, bb in ((False, None), (True, None), (True, base), (True, base[:1])):
                rows, dot = torch.empty(R_, length, device=dev), torch.empty(R_, device=dev)
                d = AT.metric_desc(x, seed, 5, s0, pp, AT.MR_GAUSS, SIGMA, attr, bb, mul)
                half = R_ // 2                                        # two launches: rows [0, half), [half, R_)
                AT.metric_rows(d, 0, half, rows[:half], dot)
                AT.metric_rows(d, half, R_ - half, rows[half:], dot)
                gen = DeviceNoisy(seed, B, 5, SIGMA, mul, s0)
                be = None if bb is None else AT.expand_metric_baselines(bb, B, length, pp)
                pert, xt = gen(x.repeat_interleave(pp, 0), be)
                assert torch.equal(rows, xt), (length, s0, mul)
                assert torch.equal(dot, AT.metric_row_dot(pert.contiguous(), attr, pp)), (length, s0, mul, bb is None)


def test_fold_and_finalize_bits(gpu_device):
    """advh_infidelity_fold / advh_infidelity_finalize against tests/metrics_ref.py's fold_model bit for bit: fixed (dot, f0, fk),
    d = f0 - fk in fp32, several chunk plans, both modes, and a clip whose attribution sums are zero (beta's denominator 1)."""
    dev = gpu_device
    rng = np.random.default_rng(5)
    Bx, Sx = 3, 10
    dot = rng.standard_normal((Bx, Sx)).astype(np.float32)
    dot[2] = 0.0
    f0 = rng.standard_normal(Bx).astype(np.float32)
    fk = rng.standard_normal((Bx, Sx)).astype(np.float32)
    d = (f0[:, None] - fk).astype(np.float32)
    f0t = torch.from_numpy(f0).to(dev)
    for normalize in (False, True):
        outs = []
        for mex in (None, 3 * Bx, 4 * Bx, 7 * Bx, Bx):
            plan = AT.metric_partitions(Bx, Sx, mex)
            acc = torch.zeros(3 * Bx if normalize else Bx, dtype=torch.float64, device=dev)
            for s0, pp in plan:
                dc = torch.from_numpy(np.ascontiguousarray(dot[:, s0:s0 + pp]).reshape(-1)).to(dev)
                fc = torch.from_numpy(np.ascontiguousarray(fk[:, s0:s0 + pp]).reshape(-1)).to(dev)
                AT.infidelity_fold(dc, f0t, fc, Bx, pp, normalize, acc)
            out = AT.infidelity_finalize(acc, Bx, Sx, normalize).cpu().numpy()
            want = MR.fold_model(dot.astype(np.float64), d.astype(np.float64), plan, normalize)
            assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (normalize, mex, out, want)
            outs.append(out)
        assert all(np.array_equal(o.view(np.uint32), outs[0].view(np.uint32)) for o in outs)


def _bound(rec, beta, precision, fmax):
    """|infidelity - ref| bound: the row's d carries two logits (2 TOL_LOGIT max(1, |F|)), its a the fp32 row tree (1e-6 of
    sum |pert . attr|); a squared residual r = beta a - d moves by at most 2 |r| e + e^2."""
    e = 2 * TOL_LOGIT[precision] * max(1.0, fmax) + max(1.0, abs(beta)) * 1e-6 * rec["abs"].max().item()
    r = (beta * rec["a"] - rec["d"]).abs().max().item()
    return 2 * r * e + e * e


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_infidelity_against_the_restatement(gpu_device, precision):
    att, model = setup(gpu_device, precision)
    dev = gpu_device
    x = clips()
    nb = baseline(B, L, 5)
    fwd = MR.model_forward(model)
    attrs = {"Saliency": att.saliency(x.to(dev)), "InputXGradient": att.input_x_gradient(x.to(dev)),
             "IG": att.integrated_gradients(x.to(dev), n_steps=4, baselines=nb.to(dev))}
    cases = [("Saliency", False, False, None, None), ("Saliency", True, False, None, 2 * B),
             ("InputXGradient", False, True, None, None), ("InputXGradient", True, True, None, None),
             ("IG", False, True, nb, None), ("IG", True, True, nb, 3 * B)]
    for k, (name, normalize, mul, bl, mex) in enumerate(cases):
        seed = 100 + k
        a = attrs[name]
        ours = att.infidelity(x.to(dev), NoisyPerturbation(SIGMA, mul), a, baselines=None if bl is None else bl.to(dev),
                              n_perturb_samples=S, max_examples_per_batch=mex, normalize=normalize, seed=seed)
        if normalize:
            plain = att.infidelity(x.to(dev), NoisyPerturbation(SIGMA, mul), a, baselines=None if bl is None else bl.to(dev),
                                   n_perturb_samples=S, max_examples_per_batch=mex, seed=seed)
            assert bool((ours <= plain * (1 + 1e-12)).all()), (name, ours, plain)
        rec = {}
        ref = MR.infidelity(fwd, MR.NoisyChunks(seed, B, S, SIGMA, mul, mex), x, a.cpu(), baselines=bl, n_perturb_samples=S,
                            max_examples_per_batch=mex, normalize=normalize, record=rec)
        fmax = fwd(x).abs().max().item() + rec["d"].abs().max().item()
        for b in range(B):
            beta = 1.0
            if normalize:
                aa, dd = rec["a"][b], rec["d"][b]
                beta = ((aa * dd).sum() / ((aa * aa).sum() if (aa * aa).sum() != 0 else 1.0)).item()
            sub = {key: v[b:b + 1] for key, v in rec.items()}
            bound = _bound(sub, beta, precision, fmax)
            err = abs(ours[b].item() - ref[b].item())
            print(f"infidelity({name}, normalize={normalize}, mul={mul}) [{precision}] clip {b}: {ours[b].item():.6e} vs "
                  f"{ref[b].item():.6e}, |err| {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (name, normalize, mul, b, err, bound)


def _seeded(fn, seeds):
    """``fn(w, seed=...)`` with the seeds of ``seeds`` in call order (the same order for every call of the metric)."""
    it = iter(seeds)
    return lambda w, **kw: fn(w, seed=next(it), **kw)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_sensitivity_against_the_restatement(gpu_device, precision):
    att, model = setup(gpu_device, precision)
    dev = gpu_device
    x = clips(seed=42)
    nb = baseline(B, L, 6)
    r = RADIUS[precision]
    nt_seeds = [31, 32]                                                 # e, then the single chunk
    cases = [("Saliency", lambda: att.saliency, NR.saliency(model), {}, {}),
             ("IG", lambda: lambda w, **k: att.integrated_gradients(w, n_steps=4, **k), NR.integrated_gradients(model, 4),
              dict(baselines=nb.to(dev)), dict(baselines=nb)),
             ("NoiseTunnel(Saliency)", lambda: _seeded(lambda w, seed: att.noise_tunnel(w, att.saliency, "smoothgrad", 2, None,
                                                                                         SIGMA, seed=seed), nt_seeds),
              None, {}, {})]
    ords = ("fro", 1, math.inf)
    for k, (name, make, ref_fn, kw, ref_kw) in enumerate(cases):
        seed = 200 + k
        ours = torch.stack([att.sensitivity_max(make(), x.to(dev), perturb_radius=r, n_perturb_samples=S, norm_ord=o, seed=seed,
                                                **kw) for o in ords])
        if ref_fn is None:
            it = iter(nt_seeds)
            ref_fn = lambda w: NR.noise_tunnel(w, NR.saliency(model), "smoothgrad", 2, None, SIGMA, seed=next(it))
        ref = MR.sensitivity_max(ref_fn, x, MR.default_rows(seed, B, S, r), S, ords, **ref_kw)
        err = (ours.cpu().double() - ref).abs().max().item()
        print(f"sensitivity_max({name}) [{precision}] (fro, 1, inf): {ours.cpu().tolist()} vs {ref.tolist()}, max |err| {err:.3e}")
        assert err <= 2 * TOL[precision], (name, err)


def test_properties(gpu_device):
    att, _ = setup(gpu_device, "f32")
    dev = gpu_device
    x = clips(seed=43).to(dev)
    a = att.input_x_gradient(x)
    nb = baseline(B, L, 7).to(dev)
    np_ = NoisyPerturbation(SIGMA)
    base_v = att.infidelity(x, np_, a, n_perturb_samples=S, normalize=True, seed=5)
    for k in (-4, 3):                                                   # a 2^k scale of the attribution: bit-identical
        assert torch.equal(att.infidelity(x, np_, a * 2.0 ** k, n_perturb_samples=S, normalize=True, seed=5), base_v)
    for mul, bl in ((False, None), (True, None), (True, nb)):           # fused = generic at the same chunking, bit for bit
        for mex in (None, 2 * B):
            for normalize in (False, True):
                fused = att.infidelity(x, NoisyPerturbation(SIGMA, mul), a, baselines=bl, n_perturb_samples=S,
                                       max_examples_per_batch=mex, normalize=normalize, seed=9)
                gen = att.infidelity(x, DeviceNoisy(9, B, S, SIGMA, mul), a, baselines=bl, n_perturb_samples=S,
                                     max_examples_per_batch=mex, normalize=normalize, seed=9)
                assert torch.equal(fused, gen), (mul, bl is None, mex, normalize, fused, gen)
    torch.manual_seed(11)
    v1 = att.infidelity(x, np_, a, n_perturb_samples=S)
    s1 = att.sensitivity_max(att.saliency, x, n_perturb_samples=2)
    torch.manual_seed(11)
    assert torch.equal(v1, att.infidelity(x, np_, a, n_perturb_samples=S))
    assert torch.equal(s1, att.sensitivity_max(att.saliency, x, n_perturb_samples=2))
    assert not torch.equal(v1, att.infidelity(x, np_, a, n_perturb_samples=S))
    z = att.sensitivity_max(att.saliency, x, perturb_radius=0.0, n_perturb_samples=2, seed=3)
    print(f"sensitivity_max at radius 0: {z.tolist()}")                 # measured 0 (the chain is deterministic)
    assert float(z.max()) < 1e-6
    const = att.sensitivity_max(lambda w: torch.ones_like(w), x, n_perturb_samples=3, seed=3)
    assert torch.equal(const, torch.zeros(B, device=dev))
    # the identity explanation with the max norm: max_s ||x_b - x~_s||_inf / ||x_b||_inf from the numpy rows, to 1 ulp
    ident = att.sensitivity_max(lambda w: w.clone(), x, n_perturb_samples=S, norm_ord=math.inf, seed=17,
                                max_examples_per_batch=3 * B)
    xn = x.cpu().numpy()
    rows = np.concatenate([MR.uniform_rows(xn, 17, S, s0, pp, 0.02).reshape(B, pp, L) for s0, pp in AT.metric_partitions(B, S, 3 * B)],
                          1)
    want = np.array([np.max([np.max(np.abs(xn[b] - rows[b, s])) for s in range(S)]) / np.max(np.abs(xn[b])) for b in range(B)],
                    np.float32)
    ulp = np.abs(ident.cpu().numpy().view(np.int32) - want.view(np.int32))
    print(f"identity explanation, max norm: {ident.tolist()} vs {want.tolist()} ({ulp.max()} ulp)")
    assert ulp.max() <= 1
    # non-finite logits, attributions or explanations raise instead of returning NaN
    def nan_rows(xe):
        xt = xe.clone()
        xt[1, 5] = float("inf")
        return xe - xt, xt
    with pytest.raises(FloatingPointError):
        att.infidelity(x, nan_rows, a, n_perturb_samples=2, seed=1)
    bad = a.clone()
    bad[0, 7] = float("inf")
    with pytest.raises(FloatingPointError):
        att.infidelity(x, np_, bad, n_perturb_samples=2, seed=1)
    with pytest.raises(FloatingPointError):
        att.sensitivity_max(lambda w: w * float("inf"), x, n_perturb_samples=2, seed=1)


def test_chunkings_agree(gpu_device):
    att, _ = setup(gpu_device, "f32")
    dev = gpu_device
    x = clips(seed=44).to(dev)
    a = att.saliency(x)
    for normalize in (False, True):
        outs = {(mex, ibs): att.infidelity(x, NoisyPerturbation(SIGMA), a, n_perturb_samples=S, max_examples_per_batch=mex,
                                           normalize=normalize, seed=21, internal_batch_size=ibs)
                for mex in (None, B, 3 * B) for ibs in (None, 3)}
        ref = outs[(None, None)]
        for key, v in outs.items():
            err = ((v - ref).abs() / ref.abs()).max().item()
            print(f"infidelity normalize={normalize} max_examples_per_batch, internal_batch_size = {key}: rel err {err:.3e}, "
                  f"bit-identical {torch.equal(v, ref)}")
            assert err <= 1e-3, (key, err)
    sens = {mex: att.sensitivity_max(att.saliency, x, n_perturb_samples=S, max_examples_per_batch=mex, seed=22)
            for mex in (None, B, 3 * B)}
    for mex, v in sens.items():
        err = (v - sens[None]).abs().max().item()
        print(f"sensitivity_max max_examples_per_batch={mex}: max |err| {err:.3e}, bit-identical {torch.equal(v, sens[None])}")
        assert err <= 2 * TOL["f32"]


@pytest.fixture
def tiny_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_captum_front_end_and_score_explanations(gpu_device, tiny_runtime):
    import captum_saliency as cs
    from captum.attr import FeatureAblation, NoiseTunnel, Saliency
    from captum.metrics import infidelity, infidelity_perturb_func_decorator, sensitivity_max
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(gpu_device)
    eng = model.hip_attribution()
    x = clips(seed=45).to(gpu_device)
    a = Saliency(model).attribute(x)
    torch.manual_seed(5)
    v = infidelity(model, NoisyPerturbation(SIGMA), x, a, n_perturb_samples=3, normalize=True)
    torch.manual_seed(5)
    assert v.shape == (B,) and torch.equal(v, eng.infidelity(x, NoisyPerturbation(SIGMA), a, n_perturb_samples=3, normalize=True))
    # a decorated Python perturb_func (generic path) runs end to end
    pf = infidelity_perturb_func_decorator(True)(lambda inputs: inputs - 0.01 * torch.randn_like(inputs))
    w = infidelity(model, pf, x, a, n_perturb_samples=3, max_examples_per_batch=2 * B)
    assert w.shape == (B,) and torch.isfinite(w).all()
    torch.manual_seed(6)
    s = sensitivity_max(Saliency(model).attribute, x, n_perturb_samples=3)
    torch.manual_seed(6)
    assert torch.equal(s, eng.sensitivity_max(eng.saliency, x, n_perturb_samples=3))
    torch.manual_seed(6)                                                # target / additional_forward_args None: not passed on
    assert torch.equal(s, sensitivity_max(eng.saliency, x, n_perturb_samples=3, target=None, additional_forward_args=None))
    # host inputs: the perturbations are drawn on the GPU and come back on the host, equal to the same call on the GPU
    from captum.metrics import default_perturb_func
    for pf in (NoisyPerturbation(SIGMA), NoisyPerturbation(SIGMA, True)):
        torch.manual_seed(7)
        host = pf(x.cpu())
        torch.manual_seed(7)
        dev_ = pf(x)
        assert all(h.device.type == "cpu" and torch.equal(h, g.cpu()) for h, g in zip(host, dev_))
    torch.manual_seed(8)
    host = default_perturb_func(x.cpu())
    torch.manual_seed(8)
    assert host.device.type == "cpu" and torch.equal(host, default_perturb_func(x).cpu())
    s = sensitivity_max(NoiseTunnel(Saliency(model)).attribute, x, n_perturb_samples=2, nt_samples=2, stdevs=SIGMA)
    assert s.shape == (B,) and torch.isfinite(s).all()
    seg = (torch.arange(L, device=gpu_device) * 2 // L)
    fa = FeatureAblation(model).attribute
    assert torch.isfinite(sensitivity_max(fa, x, n_perturb_samples=2, feature_mask=seg[None])).all()
    with pytest.raises(ValueError):                                     # a per-clip mask is not expanded: the method's own check
        sensitivity_max(fa, x, n_perturb_samples=2, feature_mask=seg[None].expand(B, L).contiguous())
    for method in ("saliency", "input_x_gradient"):
        sc = cs.score_explanations(model, x, method, n_perturb_samples=3)
        print(f"score_explanations({method}): {({k: t.tolist() for k, t in sc.items()})}")
        assert set(sc) == {"infidelity", "sensitivity_max"}
        assert all(t.shape == (B,) and torch.isfinite(t).all() for t in sc.values())


def test_base_4s(gpu_device):
    """wav2vec2-base, 1 clip x 4 s, f32: infidelity of InputXGradient (4 noisy samples) and sensitivity_max of Saliency (2
    samples) against the restatement."""
    att, model = setup(gpu_device, "f32", "base")
    w = syn.make_clips(1, 64000)
    a = att.input_x_gradient(w.to(gpu_device))
    ours = att.infidelity(w.to(gpu_device), NoisyPerturbation(SIGMA), a, n_perturb_samples=4, seed=51)
    rec = {}
    fwd = MR.model_forward(model, 2)
    ref = MR.infidelity(fwd, MR.NoisyChunks(51, 1, 4, SIGMA), w, a.cpu(), n_perturb_samples=4, record=rec)
    bound = _bound(rec, 1.0, "f32", fwd(w).abs().max().item() + rec["d"].abs().max().item())
    err = abs(ours.item() - ref.item())
    print(f"base 4 s infidelity(InputXGradient): {ours.item():.6e} vs {ref.item():.6e}, |err| {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    s = att.sensitivity_max(att.saliency, w.to(gpu_device), n_perturb_samples=2, seed=52)
    sref = MR.sensitivity_max(NR.saliency(model, 2), w, MR.default_rows(52, 1, 2, 0.02), 2)
    err = (s.cpu().double() - sref).abs().max().item()
    print(f"base 4 s sensitivity_max(Saliency): {s.item():.6e} vs {sref.item():.6e}, |err| {err:.3e}")
    assert err <= 2 * TOL["f32"]
