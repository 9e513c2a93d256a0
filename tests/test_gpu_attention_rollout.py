"""GPU: attention maps, attention rollout and gradient-weighted rollout (csrc/attention_maps.hip, EmbedderGrad.attention_probs /
backward(attention_maps=...), HipAttribution.attention_maps / attention_rollout / attention_grad_rollout).

* the three entry points against fp64 on exact inputs (split planes joined for the reference, or plain fp16), every tile count,
  head-dim class and fusion, with the attention backward's own bar;
* the engine end to end against the float64 restatement of tests/attention_rollout_ref.py with the project's attribution bars;
* determinism, a clean chain state, and the captum_saliency front end.

Every test prints the figures it asserts on (max relative error of max|ref|, cosine): run with ``-s`` to read them.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import attention_rollout_ref as AR
from addvisor_hip import _lib, gemm as G, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

KERNEL_BAR = 5e-6            # tests/test_gpu_backward.py::test_attention_bwd_split: P and dP are intermediates of that computation
ROLLOUT_BAR = 2e-5           # tests/test_gpu_backward.py::test_layernorm_bwd_split's fp32 bar
TOL = {"f32": (1e-4, 0.999999), "f16": (3e-2, 0.999)}      # tests/test_gpu_layer_attr.py: every attribution map


def relerr(a, b):
    return ((a.cpu().double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300)).item()


def _st():
    return torch.cuda.current_stream().cuda_stream


# --------------------------------------------------------------------------------------------------------------- kernels
def launch_maps(qkv, dctx, dscale, fuse, B, T, H, heads, split):
    dev = qkv.device
    out = torch.full((B, T, T) if fuse else (B, heads, T, T), float("nan"), dtype=torch.float32, device=dev)
    lo = lambda t: t.stride(0) if (split and t is not None) else 0
    rc = _lib.lib().advh_attention_maps(qkv.data_ptr(), lo(qkv), None if dctx is None else dctx.data_ptr(), lo(dctx), dscale, fuse,
                                        out.data_ptr(), B, T, H, heads, _st())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out


def fuse_ref(m, fuse):
    return m if fuse == 0 else AR.fuse_heads(m, {1: "mean", 2: "max", 3: "min"}[fuse])


@pytest.mark.parametrize("T,heads,D", [(1, 1, 8), (15, 2, 16), (16, 1, 32), (17, 3, 32), (49, 2, 32), (99, 2, 64), (199, 3, 64), (249, 2, 64),
                                       (199, 2, 120), (256, 1, 128), (60, 1, 40)])
def test_attention_maps_kernel(gpu_device, T, heads, D):
    """advh_attention_maps vs fp64 on exact inputs: both operand formats, probabilities and gradient-weighted maps, every fusion,
    dscale 1 and 1/4096; every element written, bit-identical across launches and across the batch size."""
    _lib.init()
    g = torch.Generator().manual_seed(T + D)
    B, H = 2, heads * D
    q32, d32 = torch.randn(B * T, 3 * H, generator=g) * 0.7, torch.randn(B * T, H, generator=g)
    worst = {"P": 0.0, "GA": 0.0, "rowsum": 0.0}
    for split in (True, False):
        if split:
            qh, dh = G.split_planes(q32), G.split_planes(d32)
            x, do = G.join_planes(qh).double(), G.join_planes(dh).double()
            first = lambda t: t[:, :T].contiguous()
        else:
            qh, dh = q32.half(), d32.half()
            x, do = qh.double(), dh.double()
            first = lambda t: t[:T].contiguous()
        q, k, v = [t.view(B, T, heads, D).transpose(1, 2) for t in x.split(H, dim=1)]
        P = torch.softmax(q @ k.transpose(2, 3) * D ** -0.5, -1)
        GA = (P * (do.view(B, T, heads, D).transpose(1, 2) @ v.transpose(2, 3))).clamp_min(0)
        qd, dd = qh.to(gpu_device), dh.to(gpu_device)
        q1, d1 = first(qh).to(gpu_device), first(dh).to(gpu_device)
        for dctx, dctx1, ref, dscales, what in ((None, None, P, (1.0,), "P"), (dd, d1, GA, (1.0, 1.0 / 4096), "GA")):
            for fuse in (0, 1, 2, 3):
                for ds in dscales:
                    out = launch_maps(qd, dctx, ds, fuse, B, T, H, heads, split)
                    assert torch.isfinite(out).all()                                   # pre-filled with NaN: every element is written
                    err = relerr(out, fuse_ref(ref, fuse) * ds)
                    worst[what] = max(worst[what], err)
                    assert err < KERNEL_BAR, (what, split, fuse, ds, err)
                    if what == "P" and fuse in (0, 1):
                        rs = (out.double().sum(-1) - 1).abs().max().item()
                        worst["rowsum"] = max(worst["rowsum"], rs)
                        assert rs < 1e-6, (split, fuse, rs)
                    assert torch.equal(out, launch_maps(qd, dctx, ds, fuse, B, T, H, heads, split))
                    assert torch.equal(out[0], launch_maps(q1, dctx1, ds, fuse, 1, T, H, heads, split)[0])
    print(f"attention maps T={T} heads={heads} d={D}: P rel err {worst['P']:.2e}, (G A)+ rel err {worst['GA']:.2e}, "
          f"|rowsum - 1| {worst['rowsum']:.2e}")


@pytest.mark.parametrize("T", [1, 17, 49, 199, 256])
def test_rollout_step_and_relevance_kernels(gpu_device, T):
    _lib.init()
    g = torch.Generator().manual_seed(T)
    B = 2
    M = torch.rand(B, T, T, generator=g)
    M = M / M.sum(-1, keepdim=True) * torch.rand(B, T, 1, generator=g)                # non-negative, row sums <= 1
    X = torch.rand(B, T, T, generator=g) / T
    Md, Xd = M.to(gpu_device), X.to(gpu_device)
    lib = _lib.lib()
    for name, (al, be, ga, nrm) in (("plain", (1.0, 1.0, 0.0, 1)), ("grad", (1.0, 1.0, 1.0, 0))):
        Y = torch.full((B, T, T), float("nan"), dtype=torch.float32, device=gpu_device)
        assert lib.advh_rollout_step(Md.data_ptr(), Xd.data_ptr(), Y.data_ptr(), al, be, ga, nrm, B, T, _st()) == 0
        Y2 = torch.full_like(Y, float("nan"))
        assert lib.advh_rollout_step(Md.data_ptr(), Xd.data_ptr(), Y2.data_ptr(), al, be, ga, nrm, B, T, _st()) == 0
        Md64, Xd64 = M.double(), X.double()
        ref = al * Xd64 + be * (Md64 @ Xd64) + ga * Md64
        if nrm:
            ref = ref / (al + be * Md64.sum(-1, keepdim=True))
        rel = torch.full((B, T), float("nan"), dtype=torch.float32, device=gpu_device)
        assert lib.advh_rollout_relevance(Y.data_ptr(), rel.data_ptr(), B, T, _st()) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(Y).all() and torch.isfinite(rel).all() and torch.equal(Y, Y2)
        e1, e2 = relerr(Y, ref), relerr(rel, Y.cpu().double().mean(1))
        print(f"rollout step ({name}) T={T}: rel err {e1:.2e}; relevance rel err {e2:.2e}")
        assert e1 < ROLLOUT_BAR and e2 < ROLLOUT_BAR


# --------------------------------------------------------------------------------------------------------------- end to end
def d120_config():
    return syn.tiny_config(True, hidden_size=240, num_attention_heads=2, intermediate_size=480, num_conv_pos_embedding_groups=2,
                           num_hidden_layers=10)


CONFIGS = {"post_ln_1s": (lambda: syn.tiny_config(False), 2, 16000), "pre_ln_1s": (lambda: syn.tiny_config(True), 2, 16000),
           "pre_ln_5s": (lambda: syn.tiny_config(True), 1, 80000), "post_ln_2s": (lambda: syn.tiny_config(False), 2, 32000),
           "d120_1s": (d120_config, 2, 16000), "base_1s": (syn.base_config, 1, 16000)}
_ENG, _REF = {}, {}


def engine(dev, name, precision):
    cfg_key = name.rsplit("_", 1)[0]
    if (cfg_key, precision) not in _ENG:
        cfg = CONFIGS[name][0]()
        sd = syn.embedder_weights(cfg)
        coef, icpt = syn.logreg_weights(cfg.hidden_size)
        _ENG[(cfg_key, precision)] = (HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision)), (sd, cfg, coef, icpt))
    return _ENG[(cfg_key, precision)]


def reference(name, model, x):
    """The float64 restatement for target 1 and target 0, computed once and shared by the precisions."""
    if name not in _REF:
        _REF[name] = (AR.explain(x, model, target=1), AR.explain(x, model, target=0))
    return _REF[name]


def close(ours, ref, precision, what, worst):
    tol, cmin = TOL[precision]
    assert tuple(ours.shape) == tuple(ref.shape), (what, ours.shape, ref.shape)
    if not bool(ref.any()):                                # e.g. the min over 12 heads of a positive part: no cosine to take
        assert not bool(ours.any()), what
        return
    err = relerr(ours, ref)
    cos = F.cosine_similarity(ours.cpu().double().flatten(), ref.double().flatten(), dim=0).item()
    key = what.split(" ")[0]
    w = worst.setdefault(key, [0.0, 1.0])
    w[0], w[1] = max(w[0], err), min(w[1], cos)
    assert tuple(ours.shape) == tuple(ref.shape), (what, ours.shape, ref.shape)
    assert ours.dtype == torch.float32
    assert err < tol and cos > cmin, (what, err, cos)


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_engine_against_the_float64_restatement(gpu_device, name, precision):
    att, model = engine(gpu_device, name, precision)
    _, B, L = CONFIGS[name]
    x = syn.make_clips(B, L, seed=12)
    r1, r0 = reference(name, model, x)
    xd = x.to(gpu_device)
    nl = att.eg.emb.nl
    assert nl == len(r1["A"])
    worst = {}
    sal = att.saliency(xd)
    for l in (0, 4, nl - 1):                                                        # per-head maps
        close(att.attention_maps(xd, l), r1["A"][l], precision, f"A l={l}", worst)
        close(att.attention_maps(xd, l, grad=True), r1["GA"][l], precision, f"GA l={l}", worst)
    for f in AR.FUSIONS:
        close(att.attention_maps(xd, 4, f), AR.fuse_heads(r1["A"][4], f), precision, f"A_fused {f}", worst)
        close(att.attention_maps(xd, 4, f, grad=True), AR.fuse_heads(r1["GA"][4], f), precision, f"GA_fused {f}", worst)
    for l in range(nl):                                                             # each layer against its own max|ref|
        close(att.attention_maps(xd, l, "mean", grad=True), r1["Abar"][l], precision, f"Abar l={l}", worst)
    for f in AR.FUSIONS:
        rel, R = att.attention_rollout(xd, f, return_joint=True)
        close(R, r1["R"][f], precision, f"R {f}", worst)
        close(rel, r1["rel"][f], precision, f"rel {f}", worst)
        rs = (R.double().sum(-1) - 1).abs().max().item()
        assert rs < 1e-5 and (rel.double().sum(-1) - 1).abs().max().item() < 1e-5, (f, rs)
    rel, D = att.attention_grad_rollout(xd, return_joint=True)
    close(D, r1["D"], precision, "D", worst)
    close(rel, r1["rel_grad"], precision, "rel_grad", worst)
    assert bool((D >= 0).all())
    # targets: 1 is the default, 0 explains -F, "predicted" and a tensor pick per clip
    assert torch.equal(att.attention_grad_rollout(xd, target=1), rel)
    close(att.attention_grad_rollout(xd, target=0), r0["rel_grad"], precision, "rel_grad target=0", worst)
    close(att.attention_maps(xd, 0, "mean", grad=True, target=0), r0["Abar"][0], precision, "Abar target=0", worst)
    pick = lambda t, key: torch.stack([(r0, r1)[int(t[b])][key][b] for b in range(B)])
    pred = (r1["logits"] > 0).long()
    close(att.attention_grad_rollout(xd, target="predicted"), pick(pred, "rel_grad"), precision, "rel_grad predicted", worst)
    tens = torch.arange(B) % 2
    close(att.attention_grad_rollout(xd, target=tens), pick(tens, "rel_grad"), precision, "rel_grad tensor", worst)
    close(att.attention_grad_rollout(xd, target=tens.to(gpu_device)), pick(tens, "rel_grad"), precision, "rel_grad tensor", worst)
    # start_layer = 4: the product over the layers >= 4
    rel4, D4 = att.attention_grad_rollout(xd, start_layer=4, return_joint=True)
    D4_ref = AR.grad_rollout(r1["Abar"], 4)
    close(D4, D4_ref, precision, "D start_layer=4", worst)
    close(rel4, D4_ref.mean(1), precision, "rel_grad start_layer=4", worst)
    for f in AR.FUSIONS:
        R4_ref = AR.rollout(r1["A"], f, 4)
        rel4, R4 = att.attention_rollout(xd, f, start_layer=4, return_joint=True)
        close(R4, R4_ref, precision, f"R start_layer=4 {f}", worst)
        close(rel4, R4_ref.mean(1), precision, f"rel start_layer=4 {f}", worst)
    # bit-identical across calls; the chain's state is clean afterwards
    rel_b, D_b = att.attention_grad_rollout(xd, return_joint=True)
    assert torch.equal(rel_b, rel) and torch.equal(D_b, D)
    assert torch.equal(att.attention_rollout(xd, "max"), att.attention_rollout(xd, "max"))
    assert torch.equal(att.attention_maps(xd, 4, grad=True), att.attention_maps(xd, 4, grad=True))
    assert torch.equal(att.saliency(xd), sal)
    L_ = xd.shape[1]
    assert tuple(att.frames_to_wave(rel, L_).shape) == (B, L_)
    print(f"{name} [{precision}] vs float64 restatement, max rel err of max|ref| / min cosine: "
          + ", ".join(f"{k} {v[0]:.2e} / {v[1]:.8f}" for k, v in worst.items()))


def test_backward_writes_every_layers_map_and_leaves_the_gradient_alone(gpu_device):
    """EmbedderGrad.backward(attention_maps=...): the input gradient is bit-identical with and without the maps, the maps of a
    full backward equal the per-layer ones, and the forward-only accessor refuses layers the pass did not run."""
    att, _ = engine(gpu_device, "pre_ln_1s", "f32")
    eg = att.eg
    x = syn.make_clips(2, 16000, seed=12).to(gpu_device)
    eg.forward(x)
    g0 = eg.backward(att.loss_scale)
    nl, T = eg.emb.nl, 49
    maps = torch.full((nl, 2, T, T), float("nan"), device=gpu_device)
    g1 = eg.backward(att.loss_scale, attention_maps=(maps, 1))
    assert torch.equal(g0, g1) and bool(torch.isfinite(maps).all())
    for l in (0, 5, nl - 1):
        assert torch.equal(maps[l], att.attention_maps(x, l, "mean", grad=True))
    eg.forward(x)
    for bad in ((maps[:, :1], 1), (maps, 0), (maps, 4), (maps.cpu(), 1), (maps.double(), 1), (torch.zeros(nl + 1, 2, T, T, device=gpu_device), 1)):
        with pytest.raises(ValueError):
            eg.backward(att.loss_scale, attention_maps=bad)
    eg.forward(x, to_layer=3)
    assert tuple(eg.attention_probs(2).shape) == (2, 2, T, T)
    with pytest.raises(ValueError):
        eg.attention_probs(3)
    with pytest.raises(ValueError):
        eg.attention_probs(nl)


# --------------------------------------------------------------------------------------------------------------- front end
@pytest.fixture
def tiny_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_captum_saliency_front_end(gpu_device, tiny_runtime):
    import captum_saliency as cs
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(gpu_device)
    att = model.hip_attribution()
    B, L = 2, 16000
    x = syn.make_clips(B, L, seed=45).to(gpu_device)
    for method, rel in (("attention_rollout", att.attention_rollout(x)), ("attention_grad_rollout", att.attention_grad_rollout(x))):
        assert torch.equal(cs._explainer(att, method)(x), att.frames_to_wave(rel, L))
        out = cs.explain_waves(model, x, method=method)
        assert len(out) == 3
        for p in out:
            assert p.shape == (B, 1) and bool(((p >= 0) & (p <= 1)).all())
        sc = cs.score_explanations(model, x, method=method, n_perturb_samples=2)
        assert sc["infidelity"].shape == (B,) and sc["sensitivity_max"].shape == (B,)
        assert bool(torch.isfinite(sc["infidelity"]).all()) and bool(torch.isfinite(sc["sensitivity_max"]).all())
    out = cs.explain_waves(model, x, method="attention_rollout", layer=4, nt_type="smoothgrad", nt_samples=2)
    assert all(p.shape == (B, 1) for p in out)
    out = cs.attack_waves(model, x, torch.tensor([0, 1]), attack="fgsm", explain="attention_grad_rollout", epsilon=5e-4)
    assert out["explanation_shift"].shape == (B,) and bool(torch.isfinite(out["explanation_shift"]).all())
    print(f"attack_waves(fgsm, explain=attention_grad_rollout): explanation_shift {out['explanation_shift'].tolist()}")
    with pytest.raises(ValueError):
        cs.explain_waves(model, x, method="attention_rollout", layer=9)
