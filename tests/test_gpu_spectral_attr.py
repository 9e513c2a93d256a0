"""GPU: the time-frequency attributions over the STFT mask (addvisor_hip/spectral_attribution.py; csrc/stft.hip's row-mapped
ISTFT pair, csrc/attribution_spectral.hip) against the CPU restatement of tests/spectral_attr_ref.py: the row-mapped forward
bit for bit against ``ops.istft_masked_c64``, its adjoint against autograd and the inner-product identity, the 2-D occlusion
and pooling kernels, every method, chunking and determinism, and the captum.attr front end.

``tiny_config``, B = 2, L = 16000 (T = 50: a partial last tile at both ``stft_frames_per_workgroup`` values), the crop (512, 48)
and the full (513, 50); random masks in [0.25, 1] and a ``torch.rand`` baseline mask, never the zero mask."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spectral_attr_ref as R
from addvisor_hip import _lib, attribution as AT, ops, spectral_attribution as SA, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.spectral_attribution import HipSpectralAttribution

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": (1e-4, 0.999999), "f16": (3e-2, 0.999)}                  # tests/test_gpu_layer_attr.py
DELTA_TOL = {"f32": (1e-3, 1e-4), "f16": (3e-2, 1e-2)}                 # tests/test_gpu_neuron_attr.py
ADJ_TOL = 1e-4                                                         # tests/test_gpu_training.py: the existing adjoint's bar
B, L, T = 2, 16000, 50
CROPS = [(512, 48), (513, 50)]
CROP_IDS = ["crop", "full"]
DOMAINS = ["linear", "log1p"]
OCC = ((64, 8), (64, 4))


def relerr(a, b):
    return ((a.cpu() - b).abs().max() / (b.abs().max() + 1e-30)).item()


def close(ours, ref, precision, what):
    tol, cmin = TOL[precision]
    err = relerr(ours, ref)
    cos = F.cosine_similarity(ours.cpu().double().flatten(), ref.double().flatten(), dim=0).item()
    print(f"{what} [{precision}]: max rel err {err:.3e}, cosine {cos:.8f}")
    assert tuple(ours.shape) == tuple(ref.shape), (what, ours.shape, ref.shape)
    assert err < tol and cos > cmin, (what, err, cos)


_ATT, _ENG, _MM, _REF = {}, {}, {}, {}


def clips():
    return syn.make_clips(B, L, seed=12)


def model():
    if "model" not in _ATT:
        cfg = syn.tiny_config(False)
        _ATT["model"] = (syn.embedder_weights(cfg), cfg) + tuple(syn.logreg_weights(cfg.hidden_size))
    return _ATT["model"]


def attribution(dev, precision):
    if precision not in _ATT:
        sd, cfg, coef, icpt = model()
        _ATT[precision] = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision))
    return _ATT[precision]


def engine(dev, precision="f32", domain="linear"):
    if (precision, domain) not in _ENG:
        _ENG[precision, domain] = HipSpectralAttribution(attribution(dev, precision), clips().to(dev), domain)
    return _ENG[precision, domain]


def restatement(domain="linear"):
    if domain not in _MM:
        _MM[domain] = R.MaskModel(clips(), model(), domain)
    return _MM[domain]


def ref_of(key, fn):
    """The restatement's result, computed once and shared by the precisions."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def masks(Fm, Tm, rows=B, seed=5):
    return 0.25 + 0.75 * torch.rand(rows, Fm, Tm, generator=torch.Generator().manual_seed(seed))


def base_mask(Fm, Tm, rows=B, seed=7):
    return torch.rand(rows, Fm, Tm, generator=torch.Generator().manual_seed(seed))


@pytest.fixture
def frames_per_workgroup():
    def set_fb(fb):
        assert _lib.lib().advh_set_option(b"stft_frames_per_workgroup", fb) == 0
    yield set_fb
    set_fb(8)


def spectrogram(dev):
    return ops.stft_forward(clips().to(dev), L, want_mag=False, want_phase=False)[0]


# (clip_major, row0, S): clips 1, 0, 1, 0, 1; 0, 0, 1, 1, 1; and 1, 1, then 2 clamped to 1 (rows past the last clip's)
ROW_RULES = [(0, 3, 1), (1, 1, 3), (1, 4, 3)]
RULE_IDS = ["step_major", "clip_major", "clamped"]


def clips_of(rule, rows=5):
    cm, row0, S = rule
    return [min((row0 + r) // S, B - 1) if cm else (row0 + r) % B for r in range(rows)]


# ------------------------------------------------------------------------------------------------------------- forward rows
@pytest.mark.parametrize("fb", [8, 16])
@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("rule", ROW_RULES, ids=RULE_IDS)
def test_forward_rows_equal_the_per_clip_resynthesis(gpu_device, frames_per_workgroup, rule, domain, fb):
    """Row r equals, bit for bit, ``ops.istft_masked_c64`` of clip c(r) with mask row r."""
    frames_per_workgroup(fb)
    spec = spectrogram(gpu_device)
    assert [clips_of(r) for r in ROW_RULES] == [[1, 0, 1, 0, 1], [0, 0, 1, 1, 1], [1, 1, 1, 1, 1]]
    for Fm, Tm in CROPS:
        m = masks(Fm, Tm, 5).to(gpu_device)
        cm, row0, S = rule
        w = ops.istft_masked_rows(spec, m, L, domain, row0=row0, clip_major=cm, S=S)
        assert w.shape == (5, L) and bool(torch.isfinite(w).all())
        for r, c in enumerate(clips_of(rule)):
            mb = m[r][None].expand(B, Fm, Tm).contiguous()
            want = ops.istft_masked_c64(spec, mb, L, domain, want_out=False)[0][c]
            assert torch.equal(w[r], want), (rule, domain, fb, (Fm, Tm), r, (w[r] - want).abs().max().item())


# ------------------------------------------------------------------------------------------------------------- adjoint rows
@pytest.mark.parametrize("fb", [8, 16])
@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("crop", CROPS, ids=CROP_IDS)
def test_adjoint_rows_match_autograd(gpu_device, frames_per_workgroup, crop, domain, fb):
    frames_per_workgroup(fb)
    Fm, Tm = crop
    spec = spectrogram(gpu_device)
    mm = restatement(domain)
    g_wave = torch.randn(5, L, generator=torch.Generator().manual_seed(11))
    m = masks(Fm, Tm, 5)
    for rule in ROW_RULES:
        cm, row0, S = rule
        ref = ref_of(("adjoint", crop, domain, rule), lambda: R.istft_adjoint(mm, m, clips_of(rule), g_wave))
        ours = ops.istft_masked_rows_bwd(g_wave.to(gpu_device), spec, m.to(gpu_device), domain, row0=row0, clip_major=cm, S=S)
        err = relerr(ours, ref)
        print(f"adjoint rows {crop} {domain} FB={fb} rule={rule}: max err / max |ref| {err:.3e}")
        assert ours.shape == m.shape and err < ADJ_TOL, (crop, domain, fb, rule, err)


@pytest.mark.parametrize("fb", [8, 16])
@pytest.mark.parametrize("crop", CROPS, ids=CROP_IDS)
def test_linear_adjoint_inner_product(gpu_device, frames_per_workgroup, crop, fb):
    """``<istft_rows(m), r> = <m, adj(r)>`` in the linear domain (the forward is linear in m), summed in fp64 on the host."""
    frames_per_workgroup(fb)
    Fm, Tm = crop
    spec = spectrogram(gpu_device)
    m = masks(Fm, Tm, 5).to(gpu_device)
    r = torch.randn(5, L, generator=torch.Generator().manual_seed(13)).to(gpu_device)
    for cm, row0, S in ROW_RULES:
        w = ops.istft_masked_rows(spec, m, L, "linear", row0=row0, clip_major=cm, S=S)
        a = ops.istft_masked_rows_bwd(r, spec, m, "linear", row0=row0, clip_major=cm, S=S)
        lhs = (w.double().cpu() * r.double().cpu()).sum(1)
        rhs = (m.double().cpu() * a.double().cpu()).flatten(1).sum(1)
        err = ((lhs - rhs).abs().max() / lhs.abs().max()).item()
        print(f"<istft m, r> vs <m, adj r> {crop} FB={fb} clip_major={cm}: {lhs.tolist()} vs {rhs.tolist()}, rel {err:.3e}")
        assert err < ADJ_TOL, (crop, fb, cm, err)


# ------------------------------------------------------------------------------------------------- occlusion and pooling kernels
@pytest.mark.parametrize("Fm,Tm,window,stride", [(7, 5, (3, 2), (2, 1)), (7, 5, (3, 2), (3, 2)), (7, 5, (7, 5), (1, 1)),
                                                 (513, 50, (64, 8), (64, 4)), (512, 48, (64, 8), (64, 4))])
def test_occlusion2d_kernels_bit_for_bit(gpu_device, Fm, Tm, window, stride):
    """Points and accumulate against the numpy restatement given the same logits; (7, 5) / (3, 2) / (3, 2), (513, 50) and the
    time axis of (512, 48) end in a cropped window."""
    g = torch.Generator().manual_seed(17)
    x, base = torch.rand(B, Fm, Tm, generator=g), torch.rand(B, Fm, Tm, generator=g)
    rmasks = R.occlusion2d_masks(Fm, Tm, window, stride)
    K = rmasks.shape[0]
    w, s, Ks = SA.check_occlusion2d_args(Fm, Tm, window, stride)
    assert Ks[0] * Ks[1] == K
    for bt in (base, base[:1]):
        xd, bd = x.to(gpu_device).view(B, -1).contiguous(), bt.to(gpu_device).view(bt.shape[0], -1).contiguous()
        d = SA.occlusion2d_desc(xd, bd, Fm, Tm, w, s, Ks)
        want = torch.from_numpy(R.occlusion2d_rows(x.numpy(), bt.numpy(), rmasks)).view(K * B, -1)
        rows = K * B + 3                                                 # three padding rows: copies of x
        out = torch.empty((rows, Fm * Tm), dtype=torch.float32, device=gpu_device)
        SA.occlusion2d_points(d, 0, rows, out)
        padded = torch.cat([want, x.view(B, -1)[[(K * B + i) % B for i in range(8)]]])     # row g >= K * B copies x[g % B]
        assert torch.equal(out.cpu(), padded[:rows])
        part = torch.empty((5, Fm * Tm), dtype=torch.float32, device=gpu_device)   # a chunk that starts inside a window
        SA.occlusion2d_points(d, B + 1, 5, part)
        assert torch.equal(part.cpu(), padded[B + 1:B + 6])
        f0, fk = torch.randn(B, generator=g), torch.randn(K * B, generator=g)
        attr = torch.empty((B, Fm * Tm), dtype=torch.float32, device=gpu_device)
        SA.occlusion2d_accumulate(d, f0.to(gpu_device), fk.to(gpu_device), attr)
        ref = torch.from_numpy(R.occlusion2d_accumulate(f0.numpy(), fk.numpy(), rmasks, B))
        assert torch.equal(attr.cpu().view(B, Fm, Tm), ref)


@pytest.mark.parametrize("Fm,Tm,bw,sw", [(513, 50, 64, 16), (512, 48, 64, 16), (7, 5, 3, 2), (513, 50, 64, None), (300, 50, 513, 50)])
def test_tf_pool_against_float64(gpu_device, Fm, Tm, bw, sw):
    """Box sums against a float64 sum: max error / max |ref| over the boxes < 1e-6; (513, 50) and (7, 5) end in cropped boxes on
    both axes."""
    a = torch.randn(B, Fm, Tm, generator=torch.Generator().manual_seed(19))
    out = SA.tf_pool(a.to(gpu_device), bw, sw)
    ref = R.tf_pool(a.numpy(), bw, sw or Tm)
    assert tuple(out.shape) == ref.shape
    err = np.abs(out.double().cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"tf_pool {(Fm, Tm)} / {(bw, sw)}: max err / max |ref| {err:.3e}")
    assert err < 1e-6
    assert torch.equal(out, SA.tf_pool(a.to(gpu_device), bw, sw))


# -------------------------------------------------------------------------------------------------------------------- methods
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("crop", CROPS, ids=CROP_IDS)
def test_saliency_and_input_x_gradient(gpu_device, crop, domain, precision):
    eng, mm = engine(gpu_device, precision, domain), restatement(domain)
    m = masks(*crop)
    g = ref_of(("grad", crop, domain), lambda: mm.gradient(m))
    md = m.to(gpu_device)
    close(eng.saliency(md), g.abs(), precision, f"Saliency {crop} {domain}")
    close(eng.input_x_gradient(md), m * g, precision, f"InputXGradient {crop} {domain}")
    f = eng.logits(md).cpu()
    fr = ref_of(("logit", crop, domain), lambda: mm.logit(m))
    print(f"logits {crop} {domain} [{precision}]: {f.tolist()} vs {fr.tolist()}")
    assert (f - fr).abs().max().item() < (1e-4 if precision == "f32" else 1e-2)
    if domain == "linear":                                               # printed, not gated: F(alpha m) = F(m), so sum m dF/dm = 0
        euler = (md * eng.input_gradient(md)).double().flatten(1).sum(1)
        print(f"Euler sum {crop} [{precision}]: {euler.tolist()} (sum |m dF/dm| {(md * eng.input_gradient(md)).abs().sum().item():.3e})")


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("rule", [("gausslegendre", 5), ("gausslegendre", 50), ("riemann_trapezoid", 4)], ids=["gl5", "gl50", "trap4"])
@pytest.mark.parametrize("crop", CROPS, ids=CROP_IDS)
def test_integrated_gradients(gpu_device, crop, rule, precision):
    method, n = rule
    eng, mm = engine(gpu_device, precision), restatement()
    m, bm = masks(*crop), base_mask(*crop)
    ref, ref_delta = ref_of(("ig", crop, rule), lambda: R.integrated_gradients(mm, m, bm, n, method))
    attr, delta = eng.integrated_gradients(m.to(gpu_device), n_steps=n, baselines=bm.to(gpu_device), method=method,
                                           return_convergence_delta=True)
    close(attr, ref, precision, f"IG {method} {n} {crop}")
    rel, ab = DELTA_TOL[precision]
    ref_df = ref.double().flatten(1).sum(1) - ref_delta
    print(f"IG {method} {n} {crop} [{precision}]: delta {delta.tolist()}, restatement {ref_delta.tolist()}, F(m) - F(b) {ref_df.tolist()}")
    assert delta.shape == (B,)
    assert ((delta.double().cpu() - ref_delta).abs() <= rel * ref_df.abs() + ab).all(), (delta, ref_delta)
    plain = eng.integrated_gradients(m.to(gpu_device), n_steps=n, baselines=bm.to(gpu_device), method=method)
    assert torch.equal(plain, attr)
    if rule == ("gausslegendre", 5):                                     # the other baseline forms and multiply_by_inputs=False
        one = eng.integrated_gradients(m.to(gpu_device), n_steps=n, baselines=bm[:1].to(gpu_device), multiply_by_inputs=False)
        ref1 = ref_of(("ig1", crop), lambda: R.integrated_gradients(mm, m, bm[:1], n, multiply_by_inputs=False)[0])
        close(one, ref1, precision, f"IG [1, Fm, Tm] baseline, gradients only {crop}")
        num = eng.integrated_gradients(m.to(gpu_device), n_steps=n, baselines=0.125)
        refn = ref_of(("ign", crop), lambda: R.integrated_gradients(mm, m, torch.full((1,) + crop, 0.125), n)[0])
        close(num, refn, precision, f"IG number baseline {crop}")


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("crop", CROPS, ids=CROP_IDS)
def test_gradient_shap(gpu_device, crop, precision):
    eng, mm = engine(gpu_device, precision), restatement()
    Fm, Tm = crop
    m, dist = masks(*crop), base_mask(Fm, Tm, rows=3, seed=23)
    S, seed, sigma = 3, 1234, 0.01
    idx, alpha = AT.shap_draws(seed, B, S, 3)
    noise = AT.philox_normal(seed, 0, B * S, Fm * Tm, gpu_device).cpu()
    ref = ref_of(("shap", crop), lambda: R.gradient_shap(mm, m, dist, idx, alpha, noise, sigma, S))
    ours = eng.gradient_shap(m.to(gpu_device), dist.to(gpu_device), n_samples=S, stdevs=sigma, seed=seed)
    close(ours, ref, precision, f"GradientShap {crop}")
    assert torch.equal(ours, eng.gradient_shap(m.to(gpu_device), dist.to(gpu_device), n_samples=S, stdevs=sigma, seed=seed,
                                               internal_batch_size=4))


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("crop", CROPS, ids=CROP_IDS)
def test_occlusion(gpu_device, crop, precision):
    eng, mm = engine(gpu_device, precision), restatement()
    m, bm = masks(*crop), base_mask(*crop)
    ref = ref_of(("occ", crop), lambda: R.occlusion(mm, m, bm, *OCC))
    close(eng.occlusion(m.to(gpu_device), *OCC, baselines=bm.to(gpu_device)), ref, precision, f"Occlusion {OCC} {crop}")


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("crop", CROPS, ids=CROP_IDS)
def test_feature_ablation_and_shapley(gpu_device, crop, precision):
    eng, mm = engine(gpu_device, precision), restatement()
    Fm, Tm = crop
    m, bm = masks(*crop), base_mask(*crop)
    ids = SA.tf_feature_mask(Fm, Tm, 64, 16)
    ref = ref_of(("abl", crop), lambda: R.feature_ablation(mm, m, bm, ids))
    close(eng.feature_ablation(m.to(gpu_device), baselines=bm.to(gpu_device), feature_mask=ids), ref, precision, f"FeatureAblation {crop}")
    index, K = AT.shapley_feature_indices(ids.view(1, -1), B, Fm * Tm)
    assert K == (24 if crop == (512, 48) else 36)
    perm = np.argsort(AT.shapley_permutations(99, 2, K), axis=1)
    ref = ref_of(("shapley", crop), lambda: R.shapley_value_sampling(mm, m, bm, index.long(), perm))
    ours = eng.shapley_value_sampling(m.to(gpu_device), baselines=bm.to(gpu_device), feature_mask=ids, n_samples=2, seed=99)
    close(ours, ref, precision, f"ShapleyValueSampling {crop}")
    pooled = eng.pool(ours, 64, 16)                                      # one feature per box: the box sum is its bins x the value
    assert pooled.shape == (B, -(-Fm // 64), -(-Tm // 16))


# ---------------------------------------------------------------------------------------------------------------- determinism
def test_chunking_and_repeat_are_bit_identical(gpu_device):
    eng = engine(gpu_device)
    crop = CROPS[0]
    m, bm = masks(*crop).to(gpu_device), base_mask(*crop).to(gpu_device)
    ids = SA.tf_feature_mask(*crop, 64, 16)
    dist = base_mask(*crop, rows=3, seed=23).to(gpu_device)
    calls = {
        "IG": lambda ibs: eng.integrated_gradients(m, n_steps=7, baselines=bm, internal_batch_size=ibs),
        "GradientShap": lambda ibs: eng.gradient_shap(m, dist, n_samples=3, stdevs=0.01, seed=5, internal_batch_size=ibs),
        "Occlusion": lambda ibs: eng.occlusion(m, (128, 16), (128, 16), baselines=bm, internal_batch_size=ibs),
        "FeatureAblation": lambda ibs: eng.feature_ablation(m, baselines=bm, feature_mask=ids, internal_batch_size=ibs),
        "ShapleyValueSampling": lambda ibs: eng.shapley_value_sampling(m, baselines=bm, feature_mask=ids, n_samples=1, seed=3,
                                                                       internal_batch_size=ibs),
    }
    for name, call in calls.items():
        first = call(B)
        for ibs in (5 * B, 64):
            assert torch.equal(first, call(ibs)), (name, ibs)
        assert torch.equal(first, call(B)), name
    assert torch.equal(eng.saliency(m), eng.saliency(m))


# ------------------------------------------------------------------------------------------------------------------ front end
class _Wave:
    """The waveform model of the front end, on the tiny embedder."""
    def __init__(self, att):
        self._att = att

    def hip_attribution(self):
        return self._att


def test_captum_front_end_equals_the_engine(gpu_device):
    import captum.attr as CA
    import captum_saliency as CS
    att = attribution(gpu_device, "f32")
    x = clips().to(gpu_device)
    model_ = CS.MaskedSpectrogramLogReg(_Wave(att), x, "linear")
    eng = model_.hip_mask_attribution()
    assert eng is model_.hip_mask_attribution() and eng.T == model_.mask_frames() == T
    crop = CROPS[0]
    m, bm = masks(*crop).to(gpu_device), base_mask(*crop).to(gpu_device)
    ids = CS.tf_feature_mask(*crop, 64, 16)
    dist = base_mask(*crop, rows=3, seed=23).to(gpu_device)
    assert torch.equal(model_(m), eng.logits(m).view(-1, 1))
    assert torch.equal(CA.Saliency(model_).attribute(m), eng.saliency(m))
    assert torch.equal(CA.Saliency(model_).attribute(m, abs=False), eng.input_gradient(m))
    assert torch.equal(CA.InputXGradient(model_).attribute(m), eng.input_x_gradient(m))
    a, d = CA.IntegratedGradients(model_).attribute(m, baselines=bm, n_steps=5, return_convergence_delta=True)
    ea, ed = eng.integrated_gradients(m, n_steps=5, baselines=bm, return_convergence_delta=True)
    assert torch.equal(a, ea) and torch.equal(d, ed)
    torch.manual_seed(3)
    gs = CA.GradientShap(model_).attribute(m, dist, n_samples=2)
    torch.manual_seed(3)
    assert torch.equal(gs, eng.gradient_shap(m, dist, n_samples=2))
    assert torch.equal(CA.Occlusion(model_).attribute(m, (128, 16), strides=(128, 16), baselines=bm, perturbations_per_eval=3),
                       eng.occlusion(m, (128, 16), (128, 16), baselines=bm))
    assert torch.equal(CA.FeatureAblation(model_).attribute(m, baselines=bm, feature_mask=ids),
                       eng.feature_ablation(m, baselines=bm, feature_mask=ids))
    torch.manual_seed(4)
    sv = CA.ShapleyValueSampling(model_).attribute(m, baselines=bm, feature_mask=ids, n_samples=1)
    torch.manual_seed(4)
    assert torch.equal(sv, eng.shapley_value_sampling(m, baselines=bm, feature_mask=ids, n_samples=1))
    with pytest.raises(ValueError):
        CA.Saliency(model_).attribute(x)                                 # a waveform is not a mask


def test_explain_spectrogram(gpu_device):
    import captum_saliency as CS
    att = attribution(gpu_device, "f32")
    x = clips().to(gpu_device)
    m = masks(*CROPS[0]).to(gpu_device)
    out = CS.explain_spectrogram(_Wave(att), x, "input_x_gradient", mask=m)
    assert all(tuple(o.shape) == (B, 1) for o in out)
    eng = HipSpectralAttribution(att, x, "linear")
    attr = eng.input_x_gradient(m)
    rel = att.time_mask(attr.view(B, -1)).view_as(m)                     # |attr| / (max |attr| + 1e-8) per clip
    assert (rel - attr.abs() / (attr.abs().amax(dim=(1, 2), keepdim=True) + 1e-8)).abs().max().item() < 1e-6
    w_in, w_out = ops.istft_masked_c64(eng.spec, rel, L, "log1p")
    p = att.emb.forward(torch.cat([x, w_in, w_out]), want_hidden=False)[2]
    for o, want in zip(out, (p[:B], p[B:2 * B], p[2 * B:])):
        assert torch.equal(o, want)
    full = CS.explain_spectrogram(_Wave(att), x, "saliency")             # the default input: ones(B, 513, T)
    assert all(tuple(o.shape) == (B, 1) and bool(torch.isfinite(o).all()) for o in full)
