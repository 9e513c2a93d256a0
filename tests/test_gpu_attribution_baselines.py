"""GPU: IntegratedGradients with baselines / Riemann rules / convergence deltas and GradientShap on the HIP path
(csrc/attribution_paths.hip) vs the CPU restatement of tests/attribution_baselines_ref.py, the counter-based noise
generator vs its numpy restatement, determinism, overflow reporting and the captum.attr front end."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attribution_baselines_ref as R
from addvisor_hip import attribution as AT, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": (1e-4, 0.999999), "f16": (3e-2, 0.999)}
# delta vs the restatement's delta: within rel * |F(x) - F(b)| + abs (the fp16 chain's attributions carry its 3e-2 bar)
DELTA_TOL = {"f32": (1e-3, 1e-4), "f16": (3e-2, 1e-2)}
# |delta| of the CPU restatement (fp32 autograd) for the noise baseline below at 50 Gauss-Legendre steps, measured before
# any GPU run: 1.94e-6 (clip 0) and 5.8e-7 (clip 1) against F(x) - F(b) = 1.33 / -1.22.  Twice that (3.9e-6) is the
# rounding floor of a 16 000-term fp32 sum: the fp32-class engine measured 4.05e-6 on clip 1.  The bound is 5x the
# restatement's delta -- still five orders of magnitude below the 4-step quadrature delta (~1.8) of the same baseline.
COMPLETENESS_BOUND = 1e-5


def relerr(a, b):
    return ((a.cpu() - b).abs().max() / (b.abs().max() + 1e-30)).item()


def close(ours, ref, precision, what):
    tol, cmin = TOL[precision]
    err = relerr(ours, ref)
    cos = F.cosine_similarity(ours.cpu().double().flatten(), ref.double().flatten(), dim=0).item()
    print(f"{what} [{precision}]: max rel err {err:.3e}, cosine {cos:.8f}")
    assert err < tol and cos > cmin, (what, err, cos)


_CACHE = {}


def setup(dev, precision, cfg_name="tiny"):
    key = (cfg_name, precision)
    if key not in _CACHE:
        cfg = syn.tiny_config(False) if cfg_name == "tiny" else syn.base_config()
        sd = syn.embedder_weights(cfg)
        coef, icpt = syn.logreg_weights(cfg.hidden_size)
        _CACHE[key] = (HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision)), (sd, cfg, coef, icpt))
    return _CACHE[key]


def noise_baseline(B, L, seed=3):
    return 0.05 * torch.randn(B, L, generator=torch.Generator().manual_seed(seed))


def check_delta(att, x, base, attr, delta, ref_delta, ref_df, precision):
    """delta = sum attr - (F(x) - F(b)) from the returned attribution and the engine's own logits (float64), and the
    restatement's delta within DELTA_TOL (fp32-class: 1e-3 |F(x) - F(b)| + 1e-4)."""
    rel, ab = DELTA_TOL[precision]
    B = x.shape[0]
    f = att.logits(torch.cat([x, base.to(x.device)])).double().cpu()
    fb = f[B:].expand(B) if base.shape[0] == 1 else f[B:]
    mine = attr.double().cpu().sum(1) - (f[:B] - fb)
    assert delta.shape == (B,)
    assert (delta.double().cpu() - mine).abs().max().item() < 1e-5
    assert ((delta.double().cpu() - ref_delta).abs() <= rel * ref_df.abs() + ab).all(), (delta, ref_delta)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_ig_baselines_and_methods(gpu_device, precision):
    att, model = setup(gpu_device, precision)
    w = syn.make_clips(2, 16000, seed=12)
    wd = w.to(gpu_device)
    nb = noise_baseline(2, 16000)
    for bname, base_arg, base_t in (("[B,L]", nb.to(gpu_device), nb), ("[1,L]", nb[:1].to(gpu_device), nb[:1]),
                                    ("scalar", 0.05, torch.full((1, 16000), 0.05))):
        for method in AT.METHODS:
            if bname == "scalar" and method in ("riemann_left", "riemann_trapezoid"):
                continue                    # alpha = 0 is a constant clip: the chain reports an overflow (see the docstring)
            attr, delta = att.integrated_gradients(wd, n_steps=4, baselines=base_arg, method=method, return_convergence_delta=True)
            ref, ref_delta = R.integrated_gradients(w, base_t, model, 4, method)
            close(attr, ref, precision, f"IG {bname} {method}")
            ref_df = ref.double().sum(1) - ref_delta
            check_delta(att, wd, base_t, attr, delta, ref_delta, ref_df, precision)
    g = att.integrated_gradients(wd, n_steps=4, baselines=nb.to(gpu_device), method="riemann_middle", multiply_by_inputs=False)
    ref, _ = R.integrated_gradients(w, nb, model, 4, "riemann_middle", multiply_by_inputs=False)
    close(g, ref, precision, "IG multiply_by_inputs=False")


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_ig_default_baseline_equals_a_zero_tensor_baseline(gpu_device, precision):
    """``baselines=None`` and a ``[B, L]`` tensor of zeros run the same path loop: the same bits."""
    att, _ = setup(gpu_device, precision)
    wd = syn.make_clips(2, 16000, seed=12).to(gpu_device)
    for n_steps, ib in ((8, None), (50, 32)):
        a = att.integrated_gradients(wd, n_steps=n_steps, internal_batch_size=ib).cpu().numpy()
        b = att.integrated_gradients(wd, n_steps=n_steps, internal_batch_size=ib, baselines=torch.zeros_like(wd)).cpu().numpy()
        print(f"default vs zero tensor baseline [{precision}] n={n_steps}: max |a - b| {np.abs(a - b).max():.3e}")
        assert np.array_equal(a, b), np.abs(a - b).max()


def test_ig_completeness_with_a_noise_baseline(gpu_device):
    att, model = setup(gpu_device, "f32")
    wd = syn.make_clips(2, 16000, seed=12).to(gpu_device)
    _, delta = att.integrated_gradients(wd, n_steps=50, baselines=noise_baseline(2, 16000).to(gpu_device),
                                        return_convergence_delta=True)
    print("IG 50 GL steps, noise baseline: delta", delta.tolist())
    assert delta.abs().max().item() < COMPLETENESS_BOUND


def test_noise_generator(gpu_device):
    seed = 0x1234_5678_9ABC_DEF1
    for row0, rows, n in ((0, 3, 1024), (5, 3, 1001), (2 ** 33 + 7, 2, 64)):
        words = AT.philox_normal(seed, row0, rows, n, gpu_device, raw=True).cpu().numpy().view(np.uint32)
        ref = R.philox_words(seed, row0, rows, n).reshape(rows, -1)[:, :n]
        assert np.array_equal(words, ref), (row0, rows, n)
        z = AT.philox_normal(seed, row0, rows, n, gpu_device).cpu().numpy().astype(np.float64)
        rz = R.philox_normal(seed, row0, rows, n)
        assert np.all(np.abs(z - rz) <= 2e-6 * (1 + np.abs(rz))), np.abs(z - rz).max()
    full = AT.philox_normal(seed, 0, 40, 1000, gpu_device)
    part = AT.philox_normal(seed, 13, 9, 1000, gpu_device)
    assert torch.equal(full[13:22], part)                                # rows do not depend on the launch
    big = AT.philox_normal(99, 0, 256, 4096, gpu_device).double()       # 2^20 samples
    m, v = big.mean().item(), big.var().item()
    print(f"noise: mean {m:.3e}, variance {v:.5f}")
    assert abs(m) < 5e-3 and abs(v - 1) < 1e-2


def shap_case(att, model, dev, w, base, S, sigma, seed, precision):
    B, L = w.shape
    attr, delta = att.gradient_shap(w.to(dev), base.to(dev), n_samples=S, stdevs=sigma, seed=seed, return_convergence_delta=True)
    idx, alpha = AT.shap_draws(seed, B, S, base.shape[0])
    noise = AT.philox_normal(seed, 0, B * S, L, dev).cpu()
    ref, ref_delta = R.gradient_shap(w, base, idx, alpha, noise, sigma, S, model)
    close(attr, ref, precision, f"GradientShap S={S} stdevs={sigma}")
    assert delta.shape == (B * S,)
    xt = w.repeat_interleave(S, 0) + sigma * noise
    bt = base[torch.as_tensor(idx).long()]
    with torch.no_grad():
        from oracle import attribution_ref as A
        ref_df = (A.model_logit(xt, *model).double() - A.model_logit(bt, *model).double()).view(-1)
    rel, ab = DELTA_TOL[precision]
    assert ((delta.double().cpu() - ref_delta).abs() <= rel * ref_df.abs() + ab).all(), (delta, ref_delta)
    return attr


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_gradient_shap(gpu_device, precision):
    att, model = setup(gpu_device, precision)
    w = syn.make_clips(2, 16000, seed=12)
    base = torch.cat([noise_baseline(2, 16000, 4), torch.zeros(1, 16000)])          # N_b = 3
    for S in (1, 5):
        for sigma in (0.0, 0.05):
            shap_case(att, model, gpu_device, w, base, S, sigma, 1000 + S, precision)
    g = att.gradient_shap(w.to(gpu_device), base.to(gpu_device), n_samples=5, stdevs=0.05, seed=7, multiply_by_inputs=False)
    idx, alpha = AT.shap_draws(7, 2, 5, 3)
    ref, _ = R.gradient_shap(w, base, idx, alpha, AT.philox_normal(7, 0, 10, 16000, gpu_device).cpu(), 0.05, 5, model,
                             multiply_by_inputs=False)
    close(g, ref, precision, "GradientShap multiply_by_inputs=False")


def test_gradient_shap_determinism(gpu_device):
    att, _ = setup(gpu_device, "f32")
    wd = syn.make_clips(2, 16000, seed=12).to(gpu_device)
    base = noise_baseline(3, 16000, 5).to(gpu_device)
    kw = dict(n_samples=20, stdevs=0.05)
    a = att.gradient_shap(wd, base, seed=11, internal_batch_size=40, **kw)
    assert torch.equal(a, att.gradient_shap(wd, base, seed=11, internal_batch_size=40, **kw))
    assert not torch.equal(a, att.gradient_shap(wd, base, seed=12, internal_batch_size=40, **kw))
    b = att.gradient_shap(wd, base, seed=11, internal_batch_size=8, **kw)
    assert (a - b).abs().max().item() <= 1e-6 * a.abs().max().item()
    print(f"GradientShap internal batch 8 vs 40: bit-identical {torch.equal(a, b)}")
    torch.manual_seed(3)
    c = att.gradient_shap(wd, base, **kw)
    torch.manual_seed(3)
    assert torch.equal(c, att.gradient_shap(wd, base, **kw))


def test_new_methods_report_overflow(gpu_device):
    cfg = syn.tiny_config(False)
    sd = syn.embedder_weights(cfg)
    coef, icpt = syn.logreg_weights(cfg.hidden_size)
    w = syn.make_clips(1, 16000, seed=5).to(gpu_device)
    for precision in ("f32", "f16"):
        att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, gpu_device, precision=precision), loss_scale=2.0 ** 40)
        with pytest.raises(FloatingPointError):
            att.integrated_gradients(w, n_steps=4, baselines=noise_baseline(1, 16000).to(gpu_device))
        with pytest.raises(FloatingPointError):
            att.gradient_shap(w, noise_baseline(2, 16000).to(gpu_device), n_samples=2, seed=1)


_BASE_REF = {}


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_base_4s(gpu_device, precision):
    """wav2vec2-base, 1 clip x 4 s: GradientShap (4 samples) and IG with a noise baseline (8 steps) vs the restatement."""
    att, model = setup(gpu_device, precision, "base")
    tol, cmin = (1e-4, 0.999999) if precision == "f32" else (5e-2, 0.999)
    w = syn.make_clips(1, 64000)
    base = noise_baseline(2, 64000, 6)
    if not _BASE_REF:
        idx, alpha = AT.shap_draws(21, 1, 4, 2)
        noise = AT.philox_normal(21, 0, 4, 64000, gpu_device).cpu()
        _BASE_REF["shap"] = R.gradient_shap(w, base, idx, alpha, noise, 0.05, 4, model, internal_batch=4)[0]
        _BASE_REF["ig"] = R.integrated_gradients(w, base[:1], model, 8, internal_batch=4)[0]
    shap = att.gradient_shap(w.to(gpu_device), base.to(gpu_device), n_samples=4, stdevs=0.05, seed=21)
    ig = att.integrated_gradients(w.to(gpu_device), n_steps=8, baselines=base[:1].to(gpu_device))
    for name, ours, ref in (("shap", shap, _BASE_REF["shap"]), ("ig", ig, _BASE_REF["ig"])):
        err = relerr(ours, ref)
        cos = F.cosine_similarity(ours.cpu().double().flatten(), ref.double().flatten(), dim=0).item()
        print(f"base 4 s {name} [{precision}]: max rel err {err:.3e}, cosine {cos:.8f}")
        assert err < tol and cos > cmin, (name, err, cos)


@pytest.fixture
def tiny_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_captum_front_end(gpu_device, tiny_runtime):
    import captum_saliency as cs
    from captum.attr import GradientShap, IntegratedGradients
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(gpu_device)
    x = syn.make_clips(2, 16000, seed=12).to(gpu_device)
    dist = noise_baseline(3, 16000, 8).to(gpu_device)
    torch.manual_seed(17)
    attr, delta = GradientShap(model).attribute(x, baselines=dist, n_samples=4, stdevs=0.05, return_convergence_delta=True)
    assert attr.shape == x.shape and delta.shape == (8,)
    torch.manual_seed(17)
    a2, d2 = model.hip_attribution().gradient_shap(x, dist, n_samples=4, stdevs=0.05, return_convergence_delta=True)
    assert torch.equal(attr, a2) and torch.equal(delta, d2)
    b = noise_baseline(2, 16000, 9).to(gpu_device)
    ig, igd = IntegratedGradients(model).attribute(x, baselines=b, method="riemann_trapezoid", return_convergence_delta=True)
    assert ig.shape == x.shape and igd.shape == (2,)
    i2, id2 = model.hip_attribution().integrated_gradients(x, baselines=b, method="riemann_trapezoid", return_convergence_delta=True)
    assert torch.equal(ig, i2) and torch.equal(igd, id2)
    with pytest.raises(NotImplementedError):
        GradientShap(model).attribute(x, baselines=dist, target=0)
