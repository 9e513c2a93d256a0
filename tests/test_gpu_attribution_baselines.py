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


def misaligned(t):
    """A contiguous copy of ``t`` whose data pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


U24 = 2.0 ** -24                                                          # unit roundoff of fp32


@pytest.mark.parametrize("n,shift", [(1000, False), (1001, False), (1000, True)], ids=["float4", "scalar", "misaligned"])
def test_path_accumulate_kernel_modes(gpu_device, n, shift):
    """advh_attr_path_accumulate called directly, its five modes with ``row_sum`` where it is allowed, against an fp64 numpy
    restatement: B = 3 clips, S = 4 rows per clip, two chunks [0, 5) and [5, 12) that cut a clip's (a step's) rows.

    Bars, from the arithmetic: an element of ``total`` is a sum of at most R products of fp32 values (the fp32 difference
    x~ - b counts as one such value) added in order, so it is within (R + 2) * 2^-24 * sum |terms| of the fp64 sum of the same
    terms (one rounding of the factor, one of the product, at most R of the running sum); a row sum over n terms within
    (n + 2) * 2^-24 * sum |terms|.  The running sums start from a non-zero ``total``, which counts as one of the R terms
    (R = S + 1).  With sigma != 0 the restatement forms x~ = x + sigma * z unfused where the kernel may fuse
    it: both lie within 2^-24 (|x~| + |sigma z|) of the exact value, which adds 2^-22 * sum (|x| + |sigma z|) |grad| (zero at
    sigma = 0)."""
    dev = gpu_device
    B, S, rows = 3, 4, 12
    place = (lambda t: misaligned(t.to(dev))) if shift else (lambda t: t.to(dev).contiguous())
    gen = torch.Generator().manual_seed(n + 7 * shift)
    x, base = torch.randn(B, n, generator=gen), torch.randn(5, n, generator=gen)
    grad, w = torch.randn(rows, n, generator=gen), torch.rand(rows, generator=gen)
    tot0 = torch.randn(B, n, generator=gen)
    bidx = torch.tensor([4, 0, 2, 2, 1, 3, 0, 4, 1, 1, 3, 0], dtype=torch.int32)
    xd, gd, wd, bid = place(x), place(grad), w.to(dev), bidx.to(dev)
    x64, g64, w64 = x.double().numpy(), grad.double().numpy(), w.double().numpy()
    chunks = ((0, 5), (5, 7))

    def run(desc, mode, w_):
        total = place(tot0)
        sums = torch.full((rows,), 7.0, device=dev)
        for r0, nr in chunks:
            AT._accumulate(desc, gd[r0:r0 + nr], w_, mode, r0, nr, total, None if mode == AT.ACC_IG else sums)
        return total.cpu().double().numpy(), sums.cpu().double().numpy()

    def check(what, got, ref, mag, terms):
        err, bar = np.abs(got - ref), (terms + 2) * U24 * mag
        print(f"{what} n={n} shift={shift}: max err / bar {np.max(err / np.maximum(bar, 1e-300)):.3f}, max |ref| {np.abs(ref).max():.3e}")
        assert np.all(err <= bar), (what, float(err.max()))

    # ACC_IG: step-major rows g = s * B + b, total[b] += w[g] * grad[g]
    bd = place(base[:B])
    got, _ = run(AT._desc(xd, bd, None, S, 0), AT.ACC_IG, wd)
    terms = (w64[:, None] * g64).reshape(S, B, n)
    check("ACC_IG", got, tot0.double().numpy() + terms.sum(0), np.abs(tot0.double().numpy()) + np.abs(terms).sum(0), S + 1)

    # ACC_SHAP / ACC_SHAP_GRAD: clip-major rows g = b * S + s, gathered baselines, x~ = x + sigma * N(seed, g, :)
    b5 = place(base)
    for sigma in (0.0, 0.25):
        seed = 11
        z = AT.philox_normal(seed, 0, rows, n, dev).cpu().numpy() if sigma else np.zeros((rows, n), np.float32)
        xt = np.repeat(x.numpy(), S, axis=0) + (np.float32(sigma) * z).astype(np.float32)
        d64 = (xt - base.numpy()[bidx.numpy()]).astype(np.float64)         # the fp32 difference, as the kernel forms it
        extra = 4 * U24 * (np.abs(np.repeat(x64, S, axis=0)) + np.abs(sigma * z)) * np.abs(g64) * (sigma != 0)
        desc = AT._desc(xd, b5, bid, S, 1, sigma, seed)
        for mode, terms in ((AT.ACC_SHAP, d64 * g64), (AT.ACC_SHAP_GRAD, g64)):
            got, sums = run(desc, mode, None)
            ex = extra if mode == AT.ACC_SHAP else 0 * extra
            t3, e3 = terms.reshape(B, S, n), ex.reshape(B, S, n)
            ref, mag = tot0.double().numpy() + t3.sum(1), np.abs(tot0.double().numpy()) + np.abs(t3).sum(1)
            err, bar = np.abs(got - ref), (S + 3) * U24 * mag + e3.sum(1)
            print(f"mode {mode} sigma={sigma} n={n} shift={shift}: max err / bar {np.max(err / bar):.3f}")
            assert np.all(err <= bar), (mode, sigma, float(err.max()))
            rt = d64 * g64                                                # both modes report the row's (x~ - b) . grad
            serr, sbar = np.abs(sums - rt.sum(1)), (n + 2) * U24 * np.abs(rt).sum(1) + extra.sum(1)
            print(f"mode {mode} sigma={sigma} row sums: max err / bar {np.max(serr / sbar):.3f}")
            assert np.all(serr <= sbar), (mode, sigma, float(serr.max()))

    # FIN_IG: out = (x - b) * total, row sums of out;  FIN_MEAN: out = total / S
    td = place(tot0)
    for brows in (B, 1):
        bd = place(base[:brows])
        out, sums = place(torch.zeros(B, n)), torch.full((B,), 7.0, device=dev)
        AT._accumulate(AT._desc(xd, bd, None, S, 0), td, None, AT.FIN_IG, 0, B, out, sums)
        terms = (x.numpy() - base.numpy()[:brows]).astype(np.float64) * tot0.double().numpy()
        check(f"FIN_IG base_rows={brows}", out.cpu().double().numpy(), terms, np.abs(terms), 1)
        check(f"FIN_IG base_rows={brows} row sums", sums.cpu().double().numpy(), terms.sum(1), np.abs(terms).sum(1), n)
    out = place(torch.zeros(B, n))
    AT._accumulate(AT._desc(xd, bd, None, S, 0), td, None, AT.FIN_MEAN, 0, B, out)
    terms = tot0.double().numpy() / S
    check("FIN_MEAN", out.cpu().double().numpy(), terms, np.abs(terms), 1)
