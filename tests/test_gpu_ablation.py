"""GPU: the perturbation attributions (Occlusion, FeatureAblation) on csrc/attribution_ablation.hip and the HIP forward, against
the Captum-style restatement of tests/ablation_ref.py: the ablated batches and the accumulation bit for bit, the end-to-end
attributions with the oracle's CPU forward within the logit parity, chunking, and the captum.attr front end."""
import os

import pytest
import torch

import ablation_ref as R
from addvisor_hip import attribution as AT, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_LOGIT = {"f32": 1e-4, "f16": 1e-2}          # the stated logit parities; a diff carries two logits

_CACHE = {}


def setup(dev, precision, cfg_name="tiny"):
    key = (cfg_name, precision)
    if key not in _CACHE:
        cfg = syn.tiny_config(False) if cfg_name == "tiny" else syn.base_config()
        sd = syn.embedder_weights(cfg)
        coef, icpt = syn.logreg_weights(cfg.hidden_size)
        _CACHE[key] = (HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision)), (sd, cfg, coef, icpt))
    return _CACHE[key]


def noise(B, L, seed):
    return 0.05 * torch.randn(B, L, generator=torch.Generator().manual_seed(seed))


def check(ours, ref, f0, precision, what):
    """Elementwise |ours - ref| <= 2 tol_logit max(1, max |F(x)|)."""
    bound = 2 * TOL_LOGIT[precision] * max(1.0, f0.abs().max().item())
    err = (ours.cpu() - ref).abs().max().item()
    print(f"{what} [{precision}]: max |err| {err:.3e} (bound {bound:.3e}), max |attr| {ref.abs().max().item():.3e}")
    assert err <= bound, (what, err, bound)


def misaligned(t):
    """A contiguous copy of ``t`` whose data pointer is 4 bytes past a 16-byte boundary (an ``x[:, 1:]``-style view)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def present_masks(mask, L):
    """The restatement's [min, max] masks of the ids present in ``mask`` (the engine's K ablations, in id order)."""
    ids = torch.unique(mask)
    return R.feature_masks(mask, L)[ids - ids.min()]


def test_points_equal_the_restatement(gpu_device):
    dev = gpu_device
    B = 3
    for L in (1000, 1001):                                               # float4 and scalar forms
        x = syn.make_clips(B, L, seed=L)
        g = torch.Generator().manual_seed(L)
        for bname, base in (("scalar", torch.full((1, L), 0.25)), ("[1,L]", noise(1, L, 1)), ("[B,L]", noise(B, L, 2))):
            cases = [("occlusion", AT.ABL_OCCLUSION, R.occlusion_masks(L, 64, 48), None)]
            seg = torch.tensor([-7, -2, 3, 11])[torch.randint(0, 4, (B, L), generator=g)]
            for mask in (seg, seg[:1]):
                index, _ = AT.feature_indices(mask, B, L)
                cases.append((f"feature {list(mask.shape)}", AT.ABL_FEATURE, present_masks(mask, L), index))
            for name, mode, masks, index in cases:
                K = masks.shape[0]
                ref = R.ablated_batch(x, base, masks)
                for view in ("aligned", "misaligned"):
                    xd = x.to(dev) if view == "aligned" else misaligned(x.to(dev))
                    bd = base.to(dev) if view == "aligned" else misaligned(base.to(dev))
                    md = None if index is None else index.to(dev)
                    d = AT.ablation_desc(xd, bd, mode, K, 64, 48, md)
                    out = torch.full((K * B, L), float("nan"), device=dev)
                    AT.ablation_points(d, 0, K * B, out)
                    assert torch.equal(out.cpu(), ref), (L, bname, name, view)
                    # a chunk running past K * B: the padding rows copy x[g % B]
                    tail = torch.full((B + 4, L), float("nan"), device=dev)
                    AT.ablation_points(d, K * B - 2, B + 4, tail)
                    want = torch.cat([ref[K * B - 2:], x[[(K * B + i) % B for i in range(B + 2)]]])
                    assert torch.equal(tail.cpu(), want), (L, bname, name, view, "tail")


@pytest.mark.parametrize("L,B", [(1000, 9), (1001, 3)])               # float4 and scalar forms
def test_points_second_trip_of_the_grid_stride_loop(gpu_device, L, B):
    """One call with more items than the capped grid covers in one trip (8192 blocks x 256 threads), so the row skeleton's loop
    wraps: Occlusion with win = stride = 1 (K = L), the smallest shapes whose wrapped part holds real rows, plus a padding tail."""
    dev = gpu_device
    K, pad = AT.occlusion_windows(L, 1, 1), 4
    assert K == L and (K * B + pad) * (L // 4 if L % 4 == 0 else L) > 8192 * 256
    x, base = syn.make_clips(B, L, seed=L), noise(B, L, 3)
    xd, bd = x.to(dev), base.to(dev)                                     # the descriptor holds their addresses
    d = AT.ablation_desc(xd, bd, AT.ABL_OCCLUSION, K, 1, 1, None)
    out = torch.full((K * B + pad, L), float("nan"), device=dev)
    AT.ablation_points(d, 0, K * B + pad, out)
    want = torch.cat([R.ablated_batch(x, base, R.occlusion_masks(L, 1, 1)), x[[(K * B + i) % B for i in range(pad)]]])
    assert torch.equal(out.cpu(), want)


def test_accumulate_bit_identical_to_the_restatement(gpu_device):
    dev = gpu_device
    B = 3
    g = torch.Generator().manual_seed(5)
    for L, win, stride in ((1000, 64, 48), (1001, 50, 1), (500, 500, 1), (999, 100, 100)):
        K = AT.occlusion_windows(L, win, stride)
        f0 = torch.randn(B, generator=g)
        fk = f0.repeat(K) + 0.1 * torch.randn(K * B, generator=g)
        x = torch.zeros(B, L, device=dev)
        base = torch.zeros(1, L, device=dev)
        attr = torch.empty(B, L, device=dev)
        AT.ablation_accumulate(AT.ablation_desc(x, base, AT.ABL_OCCLUSION, K, win, stride), f0.to(dev), fk.to(dev), attr)
        ref, _ = R.occlusion(x.cpu(), 0.0, win, stride, f0=f0, fk=fk)
        assert torch.equal(attr.cpu(), ref), (L, win, stride, (attr.cpu() - ref).abs().max())
    L = 1001
    mask = torch.tensor([-7, -2, 3, 11])[torch.randint(0, 4, (B, L), generator=g)]
    f0 = torch.randn(B, generator=g)
    for m in (mask, mask[:1]):
        ids = torch.unique(m)
        Kr = int(ids.max() - ids.min()) + 1
        fk = torch.randn(Kr * B, generator=g)
        ref, _ = R.feature_ablation(torch.zeros(B, L), 0.0, m, f0=f0, fk=fk)
        index, K = AT.feature_indices(m, B, L)
        fk_present = fk.view(Kr, B)[ids - ids.min()].reshape(-1)        # the engine evaluates the present ids only
        x = torch.zeros(B, L, device=dev)
        attr = torch.empty(B, L, device=dev)
        AT.ablation_accumulate(AT.ablation_desc(x, torch.zeros(1, L, device=dev), AT.ABL_FEATURE, K, mask=index.to(dev)),
                               f0.to(dev), fk_present.to(dev), attr)
        assert torch.equal(attr.cpu(), ref), list(m.shape)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_occlusion_end_to_end(gpu_device, precision):
    for cfg_name, B, L in (("tiny", 2, 16000), ("base", 2, 16000)):
        att, model = setup(gpu_device, precision, cfg_name)
        x = syn.make_clips(B, L, seed=41)
        fwd = R.model_forward(model)
        ref, K = R.occlusion(x, 0.0, 1600, 800, forward=fwd)
        assert K == 19
        ours = att.occlusion(x.to(gpu_device), 1600, 800)
        f0 = fwd(x)
        print(f"{cfg_name}: F(x) {f0.tolist()}, max |diff| {(ref.abs().max()).item():.3e}")
        check(ours, ref, f0, precision, f"Occlusion {cfg_name} 1 s")
    base = noise(1, L, 3)                                              # a [1, L] baseline on tiny
    att, model = setup(gpu_device, precision)
    ref, _ = R.occlusion(x, base, 1600, 800, forward=R.model_forward(model))
    check(att.occlusion(x.to(gpu_device), 1600, 800, baselines=base.to(gpu_device)), ref, R.model_forward(model)(x), precision,
          "Occlusion tiny, [1,L] baseline")


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_feature_ablation_end_to_end(gpu_device, precision):
    att, model = setup(gpu_device, precision)
    fwd = R.model_forward(model)
    B, L = 2, 16000
    x = syn.make_clips(B, L, seed=42)
    # [B, L] segment masks: 1000-sample segments with non-contiguous, negative ids, different per clip
    seg = torch.arange(L) // 1000
    mask = torch.stack([seg * 3 - 20, (15 - seg) * 5 - 7])
    base = noise(B, L, 4)
    ref, _ = R.feature_ablation(x, base, mask, forward=fwd)
    ours = att.feature_ablation(x.to(gpu_device), baselines=base.to(gpu_device), feature_mask=mask.to(gpu_device))
    check(ours, ref, fwd(x), precision, "FeatureAblation [B,L] segments")
    # feature_mask=None: every sample its own feature (L ablations), on the shortest clip the GPU tests run the tiny embedder on
    xs = syn.make_clips(1, 4000, seed=43)
    ref, K = R.feature_ablation(xs, 0.0, None, forward=R.model_forward(model, 250))
    assert K == 4000
    ours = att.feature_ablation(xs.to(gpu_device), internal_batch_size=500)
    check(ours, ref, fwd(xs), precision, "FeatureAblation per sample")


def test_chunking(gpu_device):
    att, model = setup(gpu_device, "f32")
    B, L = 2, 16000
    x = syn.make_clips(B, L, seed=44).to(gpu_device)
    K = AT.occlusion_windows(L, 1600, 800)
    f0 = att.logits(x).cpu()
    outs = [att.occlusion(x, 1600, 800, internal_batch_size=ibs) for ibs in (B, 3 * B, K * B, None)]
    for ibs, o in zip((3 * B, K * B, 128), outs[1:]):
        check(o, outs[0].cpu(), f0, "f32", f"Occlusion internal batch {ibs} vs {B}")
        print(f"internal batch {ibs} vs {B}: bit-identical {torch.equal(o, outs[0])}")
    mask = (torch.arange(L) // 2000)[None].to(gpu_device)
    a = att.feature_ablation(x, feature_mask=mask, internal_batch_size=B)
    b = att.feature_ablation(x, feature_mask=mask, internal_batch_size=5)
    check(b, a.cpu(), f0, "f32", "FeatureAblation internal batch 5 vs 2")
    print(f"FeatureAblation internal batch 5 vs 2: bit-identical {torch.equal(a, b)}")


@pytest.fixture
def tiny_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_captum_front_end(gpu_device, tiny_runtime):
    import captum_saliency as cs
    from captum.attr import FeatureAblation, Occlusion
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(gpu_device)
    eng = model.hip_attribution()
    x = syn.make_clips(2, 16000, seed=45).to(gpu_device)
    base = noise(2, 16000, 6).to(gpu_device)
    a = Occlusion(model).attribute(x, sliding_window_shapes=(1600,), strides=(800,), baselines=base)
    assert a.shape == x.shape and torch.equal(a, eng.occlusion(x, 1600, 800, baselines=base))
    a = Occlusion(model).attribute(x, (1600,), strides=800, perturbations_per_eval=3)
    assert torch.equal(a, eng.occlusion(x, 1600, 800, internal_batch_size=6))
    mask = (torch.arange(16000) // 4000)[None].to(gpu_device)
    f = FeatureAblation(model).attribute(x, baselines=0.1, feature_mask=mask)
    assert torch.equal(f, eng.feature_ablation(x, baselines=0.1, feature_mask=mask))
    with pytest.raises(ValueError):
        Occlusion(model).attribute(x, (1600,), target=0)
    # explain_waves(method="occlusion") = occlusion (100 ms windows, 50 ms stride) -> time mask -> three classifier passes
    p, t, m = cs.explain_waves(model, x, method="occlusion")
    attr = eng.occlusion(x, 1600, 800)
    _, w_rel, w_irr = eng.time_mask(attr, x)
    _, _, probs = runtime.hip_embedder().forward(torch.cat([x, w_rel, w_irr], 0), want_hidden=False)
    assert torch.equal(p, probs[:2]) and torch.equal(t, probs[2:4]) and torch.equal(m, probs[4:])
