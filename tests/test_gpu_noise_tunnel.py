"""GPU: NoiseTunnel (SmoothGrad, SmoothGrad-squared, VarGrad) over the HIP attribution methods, against the Captum-style
restatement of tests/noise_tunnel_ref.py: every wrapped method and mode, drawn baselines and convergence deltas, the noisy rows
of every partitioning against the single partition and the numpy Philox, the fold against a hand-written loop bit for bit,
stdevs = 0, determinism, overflow reporting, the captum.attr front end, explain_waves and wav2vec2-base at 4 s."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attribution_baselines_ref as R
import noise_tunnel_ref as NR
from addvisor_hip import attribution as AT, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
from oracle import attribution_ref as A

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# The bars of tests/test_gpu_attribution_baselines.py (max |err| / max |ref|, cosine) for every mode; VarGrad's error is measured
# against max |E[a^2]_ref| (its own scale cancels).  Measured on the MI355X (tiny config, 2 clips x 3 samples, stdevs 0.05), worst
# over Saliency, InputXGradient, IG (Gauss-Legendre, riemann_middle) and GradientShap: f32 2.7e-6 (smoothgrad_sq of InputXGradient),
# cosine 1.00000000; f16 5.6e-3 (smoothgrad_sq of IG riemann_middle), cosine >= 0.99997545 (vargrad of Saliency).
TOL = {"f32": (1e-4, 0.999999), "f16": (3e-2, 0.999)}
DELTA_TOL = {"f32": (1e-3, 1e-4), "f16": (3e-2, 1e-2)}
TOL_LOGIT = {"f32": 1e-4, "f16": 1e-2}          # the perturbation methods' logit parity (tests/test_gpu_ablation.py)
# Measured: the IG deltas (drawn baselines) within 5.2e-6 (f32) / 6.7e-3 (f16) of the restatement's, |F(x~) - F(b)| up to 2.6;
# Occlusion / FeatureAblation / ShapleyValues at most 1/40 of their propagated bound in f32 (4.2e-6 on E[a^2] of FeatureAblation
# [1, L]) and 1/4 in f16 (1.1e-2 on E[a^2] of Occlusion, bound 5.9e-2); wav2vec2-base at 4 s 1.4e-6 (InputXGradient) and 9.7e-7
# (IG), cosine 1.00000000.
B, L, S, SIGMA = 2, 16000, 3, 0.05

_CACHE, _REF = {}, {}


def setup(dev, precision, cfg_name="tiny"):
    key = (cfg_name, precision)
    if key not in _CACHE:
        cfg = syn.tiny_config(False) if cfg_name == "tiny" else syn.base_config()
        sd = syn.embedder_weights(cfg)
        coef, icpt = syn.logreg_weights(cfg.hidden_size)
        _CACHE[key] = (HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision)), (sd, cfg, coef, icpt))
    return _CACHE[key]


def noise_baseline(n, length, seed):
    return 0.05 * torch.randn(n, length, generator=torch.Generator().manual_seed(seed))


def clips(length=L, seed=31):
    return syn.make_clips(B, length, seed=seed)


def close_modes(ours, ref, precision, what):
    """``ours`` / ``ref``: the three modes (smoothgrad, smoothgrad_sq, vargrad)."""
    tol, cmin = TOL[precision]
    for nt, o, r in zip(AT.NT_TYPES, ours, ref):
        scale = ref[1] if nt == "vargrad" else r
        err = ((o.cpu() - r).abs().max() / (scale.abs().max() + 1e-30)).item()
        cos = F.cosine_similarity(o.cpu().double().flatten(), r.double().flatten(), dim=0).item()
        print(f"{what} {nt} [{precision}]: max err / max ref {err:.3e}, cosine {cos:.8f}")
        assert err < tol and cos > cmin, (what, nt, err, cos)


def run_modes(att, x, fn, **kw):
    return [att.noise_tunnel(x, fn, nt_type=nt, **kw) for nt in AT.NT_TYPES]


def gradient_cases(att, model, dev):
    """(name, engine callable, oracle callable, kwargs): NoiseTunnel's kwargs as the engine and the restatement take them."""
    nb = noise_baseline(B, L, 3)
    dist = noise_baseline(3, L, 4)
    return [("Saliency", att.saliency, NR.saliency(model), {}, {}),
            ("InputXGradient", att.input_x_gradient, NR.input_x_gradient(model), {}, {}),
            ("IG gausslegendre [B,L] baseline", att.integrated_gradients, NR.integrated_gradients(model, 4),
             dict(n_steps=4, baselines=nb.to(dev)), dict(baselines=nb)),
            ("IG riemann_middle", lambda w, **k: att.integrated_gradients(w, method="riemann_middle", **k),
             NR.integrated_gradients(model, 4, "riemann_middle"), dict(n_steps=4, baselines=nb.to(dev)), dict(baselines=nb)),
            ("GradientShap", lambda w, **k: att.gradient_shap(w, n_samples=2, seed=77, **k), NR.gradient_shap(model, 2, 0.0, 77),
             dict(baselines=dist.to(dev)), dict(baselines=dist))]


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_gradient_methods_against_the_oracle(gpu_device, precision):
    att, model = setup(gpu_device, precision)
    x = clips()
    for name, fn, ref_fn, kw, ref_kw in gradient_cases(att, model, gpu_device):
        batch = 2 if name.startswith("IG") else None                     # IG over two partitions (2 + 1 samples)
        ours = run_modes(att, x.to(gpu_device), fn, nt_samples=S, nt_samples_batch_size=batch, stdevs=SIGMA, seed=5, **kw)
        if name not in _REF:
            _REF[name] = NR.noise_tunnel(x, ref_fn, "all", S, batch, SIGMA, seed=5, **ref_kw)
        close_modes(ours, _REF[name], precision, f"NoiseTunnel({name})")


def delta_bound_ok(delta, ref_delta, ref_df, precision):
    rel, ab = DELTA_TOL[precision]
    return bool(((delta.double().cpu() - ref_delta).abs() <= rel * ref_df.abs() + ab).all())


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_ig_drawn_baselines_and_deltas(gpu_device, precision):
    att, model = setup(gpu_device, precision)
    x = clips()
    dist = noise_baseline(4, L, 6)
    seed = 9
    ours = []
    for nt in AT.NT_TYPES:
        a, delta = att.noise_tunnel(x.to(gpu_device), att.integrated_gradients, nt, S, None, SIGMA, True, seed=seed,
                                    return_convergence_delta=True, n_steps=4, baselines=dist.to(gpu_device))
        ours.append(a)
    key = "IG drawn"
    if key not in _REF:
        _REF[key] = NR.noise_tunnel(x, NR.integrated_gradients(model, 4), "all", S, None, SIGMA, seed=seed,
                                    draw_baseline_from_distrib=True, return_convergence_delta=True, baselines=dist)
    ref, ref_delta = _REF[key]
    close_modes(ours, ref, precision, "NoiseTunnel(IG, drawn baselines)")
    # one partition: delta[b * S + s] of noisy row (b, s) with baseline dist[idx[b * S + s]]
    assert delta.shape == (B * S,)
    rows = (x[:, None] + SIGMA * NR.noise(seed, B, S, L)).reshape(B * S, L)
    idx = NR.baseline_draws(seed, B, S, 4)
    ref_df = (A.model_logit(rows, *model).double() - A.model_logit(dist[torch.as_tensor(idx)], *model).double()).view(-1)
    err = (delta.double().cpu() - ref_delta).abs().max().item()
    print(f"NoiseTunnel(IG) delta [{precision}]: max |delta - ref| {err:.3e}, |F(x~) - F(b)| up to {ref_df.abs().max().item():.3f}")
    assert delta_bound_ok(delta, ref_delta, ref_df, precision), (delta, ref_delta)


def perturbation_bound(ours, ref, e, amax, precision, what):
    """The wrapped method's elementwise bound e on a propagates to e (E[a]), e (2 max|a| + e) (E[a^2]) and twice that (VarGrad)."""
    for nt, o, r, bound in zip(AT.NT_TYPES, ours, ref, (e, e * (2 * amax + e), 2 * e * (2 * amax + e))):
        err = (o.cpu() - r).abs().max().item()
        print(f"{what} {nt} [{precision}]: max |err| {err:.3e} (bound {bound:.3e}), max |ref| {r.abs().max().item():.3e}")
        assert err <= bound, (what, nt, err, bound)


class _MaxAbs:
    """Wraps a restatement callable and keeps max |a| over every sample it attributed."""

    def __init__(self, fn):
        self.fn, self.amax = fn, 0.0

    def __call__(self, w, **kw):
        a = self.fn(w, **kw)
        self.amax = max(self.amax, a.abs().max().item())
        return a


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_perturbation_methods_against_the_oracle(gpu_device, precision):
    att, model = setup(gpu_device, precision)
    x = clips(seed=32)
    dev = gpu_device
    seg1 = (torch.arange(L) * 5 // L)[None]                                          # [1, L], 5 segments
    segB = torch.stack([seg1[0], (torch.arange(L) * 4 // L)])                        # [B, L], 5 / 4 segments
    seg3 = (torch.arange(L) * 3 // L)[None]
    base = noise_baseline(1, L, 12)
    cases = [("Occlusion", lambda w, **k: att.occlusion(w, 4000, 2000, **k), NR.occlusion(model, 4000, 2000), {}),
             ("FeatureAblation [1,L]", att.feature_ablation, NR.feature_ablation(model), dict(feature_mask=seg1, baselines=base)),
             ("FeatureAblation [B,L]", att.feature_ablation, NR.feature_ablation(model), dict(feature_mask=segB)),
             ("ShapleyValues", att.shapley_values, NR.shapley_values(model), dict(feature_mask=seg3, baselines=base))]
    rows = (x[:, None] + SIGMA * NR.noise(8, B, S, L)).reshape(B * S, L)
    fmax = A.model_logit(torch.cat([rows, base]), *model).abs().max().item()
    e = 2 * TOL_LOGIT[precision] * max(1.0, fmax)
    for name, fn, ref_fn, kw in cases:
        dkw = {k: v.to(dev) for k, v in kw.items()}
        ours = run_modes(att, x.to(dev), fn, nt_samples=S, nt_samples_batch_size=2, stdevs=SIGMA, seed=8, **dkw)
        if name not in _REF:
            rec = _MaxAbs(ref_fn)
            _REF[name] = (NR.noise_tunnel(x, rec, "all", S, 2, SIGMA, seed=8, **kw), rec.amax)
        ref, amax = _REF[name]
        perturbation_bound(ours, ref, e, amax, precision, f"NoiseTunnel({name})")


def hand_loop(att, method, x, seeds, nt_type, S, batch, sigma, **kw):
    """A literal partition loop over the engine's method: noisy rows of ``seeds[0]``, inner seeds ``seeds[1:]`` in partition
    order, fp64 sums on the device added in sample order, the mode in fp64, one rounding to fp32."""
    Bx, Lx = x.shape
    tot = torch.zeros(Bx, Lx, dtype=torch.float64, device=x.device)
    sq = torch.zeros_like(tot)
    for (s0, pp), inner in zip(AT.noise_tunnel_partitions(S, batch), seeds[1:]):
        rows = AT.nt_noisy_rows(x, seeds[0], S, s0, pp, sigma)
        a = method(rows, seed=inner, **kw).view(Bx, pp, Lx).double()
        for s in range(pp):
            tot += a[:, s]
            sq += a[:, s] * a[:, s]
    div = torch.full_like(tot, S)                                        # a true division (not times the reciprocal)
    m, m2 = tot / div, sq / div
    return {"smoothgrad": m, "smoothgrad_sq": m2, "vargrad": m2 - m * m}[nt_type].float()


def test_sampled_methods_reproduce_and_equal_a_hand_written_loop(gpu_device):
    att, _ = setup(gpu_device, "f32")
    x = clips(seed=33).to(gpu_device)
    seg = (torch.arange(L, device=gpu_device) * 4 // L)[None]
    for name, method, kw in (("ShapleyValueSampling", att.shapley_value_sampling, dict(feature_mask=seg, n_samples=3)),
                             ("KernelShap", att.kernel_shap, dict(feature_mask=seg, n_samples=6))):
        for nt in ("smoothgrad", "vargrad"):
            torch.manual_seed(21)
            a = att.noise_tunnel(x, method, nt, S, 2, SIGMA, **kw)
            torch.manual_seed(21)
            assert torch.equal(a, att.noise_tunnel(x, method, nt, S, 2, SIGMA, **kw)), (name, nt)
            torch.manual_seed(21)
            seeds = [AT.draw_seed() for _ in range(3)]                   # NoiseTunnel's, then one per partition (2 + 1 samples)
            h = hand_loop(att, method, x, seeds, nt, S, 2, SIGMA, **kw)
            print(f"NoiseTunnel({name}) {nt}: max |engine - hand loop| {(a - h).abs().max().item():.3e}")
            assert torch.equal(a, h), (name, nt)
        torch.manual_seed(22)
        assert not torch.equal(a, att.noise_tunnel(x, method, "vargrad", S, 2, SIGMA, **kw))


def test_partitions_share_the_noise(gpu_device):
    att, model = setup(gpu_device, "f32")
    seed, S6 = 0x5EED_0123_4567, 6
    for length in (1000, 1001):                                          # float4 and scalar forms of the path-point kernel
        x = clips(length).to(gpu_device)
        zero = torch.zeros_like(x)
        full = AT.nt_noisy_rows(x, seed, S6, 0, S6, SIGMA).view(B, S6, length)
        zfull = AT.nt_noisy_rows(zero, seed, S6, 0, S6, 1.0).view(B, S6, length)
        for batch in (None, 4, 1):
            for s0, pp in AT.noise_tunnel_partitions(*AT.check_noise_tunnel_args("smoothgrad", S6, batch)[:2]):
                part = AT.nt_noisy_rows(x, seed, S6, s0, pp, SIGMA).view(B, pp, length)
                assert torch.equal(part, full[:, s0:s0 + pp]), (length, batch, s0)
                zpart = AT.nt_noisy_rows(zero, seed, S6, s0, pp, 1.0).view(B, pp, length)   # x = 0, stdevs = 1: the normals
                assert torch.equal(zpart, zfull[:, s0:s0 + pp])
                for b in range(B):
                    assert torch.equal(zpart[b], AT.philox_normal(seed, b * S6 + s0, pp, length, gpu_device))
                    rz = R.philox_normal(seed, b * S6 + s0, pp, length)
                    assert np.all(np.abs(zpart[b].cpu().double().numpy() - rz) <= 2e-6 * (1 + np.abs(rz)))
    x = clips().to(gpu_device)
    # measured bit-identical across the three partitionings (the chain's rows do not interact), but not required
    outs = [att.noise_tunnel(x, att.input_x_gradient, "smoothgrad_sq", S6, batch, SIGMA, seed=seed) for batch in (None, 4, 1)]
    for o in outs[1:]:
        err = ((o - outs[0]).abs().max() / outs[0].abs().max()).item()
        print(f"NoiseTunnel(InputXGradient) across nt_samples_batch_size: max err / max {err:.3e}")
        assert err < 2 * TOL["f32"][0]


def test_zero_stdevs(gpu_device):
    att, _ = setup(gpu_device, "f32")
    x = clips(seed=34).to(gpu_device)
    nb = noise_baseline(B, L, 13).to(gpu_device)
    for name, fn, kw in (("InputXGradient", att.input_x_gradient, {}),
                         ("IG", att.integrated_gradients, dict(n_steps=4, baselines=nb))):
        plain = fn(x, **kw)
        sg = att.noise_tunnel(x, fn, "smoothgrad", 4, None, 0.0, seed=1, **kw)
        sq = att.noise_tunnel(x, fn, "smoothgrad_sq", 4, None, 0.0, seed=1, **kw)
        vg = att.noise_tunnel(x, fn, "vargrad", 4, None, 0.0, seed=1, **kw)
        err = ((sg - plain).abs().max() / plain.abs().max()).item()      # measured 0 (bit-identical) for both; 1e-5 required
        v = (vg.abs().max() / sq.abs().max()).item()                     # measured 0
        print(f"stdevs = 0, {name}: |smoothgrad - plain| / max {err:.3e}, max |vargrad| / max smoothgrad_sq {v:.3e}")
        assert err <= 1e-5 and v <= 1e-6


def test_determinism(gpu_device):
    att, _ = setup(gpu_device, "f32")
    x = clips(seed=35).to(gpu_device)
    dist = noise_baseline(3, L, 14).to(gpu_device)
    for fn, kw in ((att.saliency, {}), (lambda w, **k: att.gradient_shap(w, n_samples=2, seed=3, **k), dict(baselines=dist))):
        a = att.noise_tunnel(x, fn, "vargrad", 4, 3, SIGMA, seed=41, **kw)
        assert torch.equal(a, att.noise_tunnel(x, fn, "vargrad", 4, 3, SIGMA, seed=41, **kw))
        assert not torch.equal(a, att.noise_tunnel(x, fn, "vargrad", 4, 3, SIGMA, seed=42, **kw))


def test_overflow_raises(gpu_device):
    cfg = syn.tiny_config(False)
    sd = syn.embedder_weights(cfg)
    coef, icpt = syn.logreg_weights(cfg.hidden_size)
    w = syn.make_clips(1, L, seed=5).to(gpu_device)
    for precision in ("f32", "f16"):
        att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, gpu_device, precision=precision), loss_scale=2.0 ** 40)
        with pytest.raises(FloatingPointError):
            att.noise_tunnel(w, att.input_x_gradient, "smoothgrad", 2, None, SIGMA, seed=1)
        with pytest.raises(FloatingPointError):
            att.noise_tunnel(w, att.integrated_gradients, "vargrad", 2, 1, SIGMA, seed=1, n_steps=4,
                             baselines=noise_baseline(1, L, 2).to(gpu_device))


@pytest.fixture
def tiny_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_captum_front_end_and_explain_waves(gpu_device, tiny_runtime):
    import captum_saliency as cs
    from captum.attr import GradientShap, InputXGradient, IntegratedGradients, NoiseTunnel, Occlusion
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(gpu_device)
    eng = model.hip_attribution()
    x = clips(seed=36).to(gpu_device)
    torch.manual_seed(5)
    a = NoiseTunnel(InputXGradient(model)).attribute(x, nt_samples=3, stdevs=SIGMA)
    torch.manual_seed(5)
    assert a.shape == x.shape and torch.equal(a, eng.noise_tunnel(x, eng.input_x_gradient, nt_samples=3, stdevs=SIGMA))
    b = noise_baseline(B, L, 15).to(gpu_device)
    torch.manual_seed(6)
    ig, d = NoiseTunnel(IntegratedGradients(model)).attribute(x, nt_type="vargrad", nt_samples=3, nt_samples_batch_size=2,
                                                              stdevs=SIGMA, baselines=b, n_steps=4, return_convergence_delta=True)
    torch.manual_seed(6)
    ig2, d2 = eng.noise_tunnel(x, eng.integrated_gradients, "vargrad", 3, 2, SIGMA, baselines=b, n_steps=4,
                               return_convergence_delta=True)
    assert d.shape == (B * 3,) and torch.equal(ig, ig2) and torch.equal(d, d2)
    dist = noise_baseline(3, L, 16).to(gpu_device)
    torch.manual_seed(7)                                                 # GradientShap draws its own seed after NoiseTunnel's
    g, gd = NoiseTunnel(GradientShap(model)).attribute(x, nt_samples=2, stdevs=SIGMA, baselines=dist, n_samples=3,
                                                       return_convergence_delta=True)
    torch.manual_seed(7)
    nt_seed, inner = AT.draw_seed(), AT.draw_seed()
    g2, gd2 = eng.noise_tunnel(x, lambda w, **k: eng.gradient_shap(w, seed=inner, **k), nt_samples=2, stdevs=SIGMA, seed=nt_seed,
                               baselines=dist, n_samples=3, return_convergence_delta=True)
    assert gd.shape == (B * 2 * 3,) and torch.equal(g, g2) and torch.equal(gd, gd2)
    o = NoiseTunnel(Occlusion(model)).attribute(x, nt_samples=2, stdevs=SIGMA, sliding_window_shapes=(4000,), strides=(4000,))
    assert o.shape == x.shape and torch.isfinite(o).all()
    with pytest.raises(ValueError):
        NoiseTunnel(Occlusion(model)).attribute(x, sliding_window_shapes=(4000,), return_convergence_delta=True)
    # explain_waves: NoiseTunnel(InputXGradient) -> time mask -> three classifier passes
    torch.manual_seed(8)
    p, t, m = cs.explain_waves(model, x, nt_type="smoothgrad", nt_samples=3)
    torch.manual_seed(8)
    attr = eng.noise_tunnel(x, eng.input_x_gradient, "smoothgrad", 3, stdevs=0.01)
    _, w_rel, w_irr = eng.time_mask(attr, x)
    _, _, probs = runtime.hip_embedder().forward(torch.cat([x, w_rel, w_irr], 0), want_hidden=False)
    assert torch.equal(p, probs[:B]) and torch.equal(t, probs[B:2 * B]) and torch.equal(m, probs[2 * B:])


def test_base_4s(gpu_device):
    """wav2vec2-base, 1 clip x 4 s, f32: NoiseTunnel over InputXGradient (4 samples) and over IntegratedGradients (4 samples x
    8 steps, noise baseline) against the restatement."""
    att, model = setup(gpu_device, "f32", "base")
    w = syn.make_clips(1, 64000)
    base = noise_baseline(1, 64000, 17)
    ours = {"ixg": att.noise_tunnel(w.to(gpu_device), att.input_x_gradient, "smoothgrad", 4, None, SIGMA, seed=23),
            "ig": att.noise_tunnel(w.to(gpu_device), att.integrated_gradients, "smoothgrad", 4, None, SIGMA, seed=24, n_steps=8,
                                   baselines=base.to(gpu_device))}
    ref = {"ixg": NR.noise_tunnel(w, NR.input_x_gradient(model, 4), "smoothgrad", 4, None, SIGMA, seed=23),
           "ig": NR.noise_tunnel(w, NR.integrated_gradients(model, 8, internal_batch=2), "smoothgrad", 4, None, SIGMA, seed=24,
                                 baselines=base)}
    tol, cmin = TOL["f32"]
    for k in ours:
        err = ((ours[k].cpu() - ref[k]).abs().max() / ref[k].abs().max()).item()
        cos = F.cosine_similarity(ours[k].cpu().double().flatten(), ref[k].double().flatten(), dim=0).item()
        print(f"base 4 s NoiseTunnel {k} [f32]: max err / max ref {err:.3e}, cosine {cos:.8f}")
        assert err < tol and cos > cmin, (k, err, cos)
