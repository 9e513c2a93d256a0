"""GPU: the layer attributions (LayerActivation, LayerGradientXActivation, LayerIntegratedGradients, LayerConductance,
InternalInfluence) on the HIP encoder chain started and stopped at a layer (csrc/attribution_layer.hip,
EmbedderGrad.forward_from / backward(to_layer=...)) vs the CPU restatement of tests/layer_attr_ref.py: parity, completeness,
chunking and determinism, truncation, the split format's range contract and the captum.attr front end."""
import os

import pytest
import torch
import torch.nn.functional as F

import layer_attr_ref as LR
from addvisor_hip import _lib, attribution as AT, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": (1e-4, 0.999999), "f16": (3e-2, 0.999)}
# delta vs the restatement's delta: within rel * |F(x) - F(b)| + abs (tests/test_gpu_attribution_baselines.py)
DELTA_TOL = {"f32": (1e-3, 1e-4), "f16": (3e-2, 1e-2)}
LOGIT_TOL = {"f32": 1e-4, "f16": 1e-2}
# |delta| of the restatement (fp32 autograd) at 50 Gauss-Legendre steps with the noise baseline below: <= 1.3e-6 over layers
# 0 / 4 / 9 of both LayerNorm flavours (tests/test_layer_attr_cpu.py prints them), up to 4.4e-2 at 4 steps.  The bound is the one
# of the input-space IG (tests/test_gpu_attribution_baselines.py): ~7.7x the restatement's largest delta, more than three orders
# of magnitude below the 4-step quadrature error.
COMPLETENESS_BOUND = 1e-5
B, L, T, H = 2, 16000, 49, 64
# The number baseline is a constant clip: zero variance, so the classifier's per-clip normalisation (x - mean) / (std + 1e-7)
# is 0 / 1e-7 where the mean is exact.  A power of two sums exactly in fp32 in any order, so the restatement and the engine both
# normalise it to 0.  A constant such as 0.05 does not: torch's fp32 mean is off by 3.7e-9, which the 1e-7 amplifies to -0.036
# (measured) -- the restatement's own rounding noise, which moves hidden_states[0] of the pre-LN model by 4.9 (|h| <= 2.9) --
# while the engine's fp64 mean gives 0.
NUMBER = 0.0625
FLAVOURS = [False, True]                                                   # do_stable_layer_norm: post-LN, pre-LN
IDS = ["post_ln", "pre_ln"]


def relerr(a, b):
    return ((a.cpu() - b).abs().max() / (b.abs().max() + 1e-30)).item()


def close(ours, ref, precision, what):
    tol, cmin = TOL[precision]
    err = relerr(ours, ref)
    cos = F.cosine_similarity(ours.cpu().double().flatten(), ref.double().flatten(), dim=0).item()
    print(f"{what} [{precision}]: max rel err {err:.3e}, cosine {cos:.8f}")
    assert tuple(ours.shape) == tuple(ref.shape), (what, ours.shape, ref.shape)
    assert err < tol and cos > cmin, (what, err, cos)


_CACHE, _REF = {}, {}


def setup(dev, precision, stable=False, cfg_name="tiny"):
    key = (cfg_name, stable, precision)
    if key not in _CACHE:
        cfg = syn.tiny_config(stable) if cfg_name == "tiny" else syn.base_config()
        sd = syn.embedder_weights(cfg)
        coef, icpt = syn.logreg_weights(cfg.hidden_size)
        _CACHE[key] = (HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision)), (sd, cfg, coef, icpt))
    return _CACHE[key]


def ref_of(key, fn):
    """The restatement's result, computed once and shared by the precisions."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def clips():
    return syn.make_clips(B, L, seed=12)


def noise_baseline(rows=B, seed=3):
    return 0.05 * torch.randn(rows, L, generator=torch.Generator().manual_seed(seed))


def check_delta(delta, attr, ref_delta, ref_attr, precision):
    """The returned delta is ``sum attr - (F(x) - F(b))`` of the returned attribution up to the fp32 sum's rounding, and the
    restatement's delta within DELTA_TOL (fp32-class: 1e-3 |F(x) - F(b)| + 1e-4)."""
    rel, ab = DELTA_TOL[precision]
    ref_df = ref_attr.double().sum((1, 2)) - ref_delta
    assert delta.shape == (B,)
    assert ((delta.double().cpu() - ref_delta).abs() <= rel * ref_df.abs() + ab).all(), (delta, ref_delta)
    implied_df = attr.double().cpu().sum((1, 2)) - delta.double().cpu()
    assert ((implied_df - ref_df).abs() <= rel * ref_df.abs() + ab).all(), (implied_df, ref_df)


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_layer_activation(gpu_device, stable, precision):
    att, model = setup(gpu_device, precision, stable)
    x = clips()
    hs = ref_of(("hidden", stable), lambda: LR.hidden(x, model))
    for l in (0, 4, att.eg.emb.nl):
        close(att.layer_activation(x.to(gpu_device), l), hs[l], precision, f"LayerActivation l={l}")


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_layer_gradient_and_gradient_x_activation(gpu_device, stable, precision):
    att, model = setup(gpu_device, precision, stable)
    x = clips()
    nl = att.eg.emb.nl
    assert nl == 9
    for l in (0, 4, nl):
        g = att.layer_gradient_x_activation(x.to(gpu_device), l, multiply_by_inputs=False)
        gxa = att.layer_gradient_x_activation(x.to(gpu_device), l)
        close(g, ref_of(("grad", stable, l), lambda: LR.layer_gradient_x_activation(x, l, model, False)), precision, f"layer gradient l={l}")
        close(gxa, ref_of(("gxa", stable, l), lambda: LR.layer_gradient_x_activation(x, l, model)), precision, f"gradient x activation l={l}")
    # no final LayerNorm (9 of 10 layers): the gradient at hidden_states[nl] is coef / T in every frame
    coef = torch.as_tensor(model[2], dtype=torch.float32).view(1, 1, H)
    close(g, (coef / T).expand(B, T, H), precision, "layer gradient at nl = coef / T")


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_forward_from_reproduces_the_forward(gpu_device, stable, precision):
    att, _ = setup(gpu_device, precision, stable)
    eg = att.eg
    x = clips().to(gpu_device)
    logits, probs = eg.forward(x)
    hs = [eg.hidden(l) for l in range(eg.emb.nl + 1)]
    for l in (0, 4, eg.emb.nl):
        lg, pr = eg.forward_from(l, hs[l])
        err = (lg - logits).abs().max().item()
        print(f"forward_from({l}) vs forward [{precision}]: max |dlogit| {err:.3e}, bit-identical {torch.equal(lg, logits)}")
        assert err < LOGIT_TOL[precision] and (pr - probs).abs().max().item() < LOGIT_TOL[precision]
        if l < eg.emb.nl:
            assert torch.equal(eg.hidden(eg.emb.nl), hs[-1]) or (eg.hidden(eg.emb.nl) - hs[-1]).abs().max().item() < LOGIT_TOL[precision]
    with pytest.raises(RuntimeError):
        eg.backward(att.loss_scale)                                      # the lower chain's saves are not those of this pass
    with pytest.raises(ValueError):
        eg.backward(att.loss_scale, to_layer=eg.emb.nl - 1)              # ... nor is anything below the starting layer
    with pytest.raises(ValueError):
        eg.forward_from(4, hs[4][:, :-1])


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("layer", [0, 4])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_layer_ig_rules_and_baselines(gpu_device, stable, layer, precision):
    att, model = setup(gpu_device, precision, stable)
    x = clips()
    xd = x.to(gpu_device)
    nb = noise_baseline()
    for bname, base_arg, base_t in (("None", None, torch.zeros(1, L)), ("[1,L]", nb[:1].to(gpu_device), nb[:1]),
                                    ("[B,L]", nb.to(gpu_device), nb), ("number", NUMBER, torch.full((1, L), NUMBER))):
        for method in AT.METHODS:
            attr, delta = att.layer_integrated_gradients(xd, layer, baselines=base_arg, n_steps=4, method=method,
                                                         return_convergence_delta=True)
            ref, ref_delta = ref_of(("lig", stable, layer, bname, method),
                                    lambda: LR.layer_integrated_gradients(x, base_t, layer, model, 4, method))
            close(attr, ref, precision, f"LayerIG l={layer} {bname} {method}")
            check_delta(delta, attr, ref_delta, ref, precision)
    g = att.layer_integrated_gradients(xd, layer, baselines=nb.to(gpu_device), n_steps=4, method="riemann_middle", multiply_by_inputs=False)
    ref, _ = ref_of(("lig-nomul", stable, layer), lambda: LR.layer_integrated_gradients(x, nb, layer, model, 4, "riemann_middle", False))
    close(g, ref, precision, f"LayerIG l={layer} multiply_by_inputs=False")


@pytest.mark.parametrize("layer", [0, 4])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_layer_ig_completeness(gpu_device, stable, layer):
    att, _ = setup(gpu_device, "f32", stable)
    _, delta = att.layer_integrated_gradients(clips().to(gpu_device), layer, baselines=noise_baseline().to(gpu_device), n_steps=50,
                                              return_convergence_delta=True)
    print(f"LayerIG 50 GL steps, noise baseline, l={layer}, stable={stable}: delta", delta.tolist())
    assert delta.abs().max().item() < COMPLETENESS_BOUND


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_conductance_and_internal_influence(gpu_device, stable, precision):
    att, model = setup(gpu_device, precision, stable)
    x = clips()
    nb = noise_baseline()
    for method in ("gausslegendre", "riemann_trapezoid"):
        c = att.layer_conductance(x.to(gpu_device), 4, baselines=nb.to(gpu_device), n_steps=4, method=method)
        close(c, ref_of(("cond", stable, method), lambda: LR.layer_conductance(x, nb, 4, model, 4, method)), precision,
              f"LayerConductance {method}")
        i = att.internal_influence(x.to(gpu_device), 4, baselines=nb.to(gpu_device), n_steps=4, method=method)
        close(i, ref_of(("infl", stable, method), lambda: LR.internal_influence(x, nb, 4, model, 4, method)), precision,
              f"InternalInfluence {method}")


@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_chunking_and_determinism(gpu_device, stable):
    """``internal_batch_size = B``: one step per chunk, so every conductance pair straddles a chunk boundary; ``5 * B``: a short
    last chunk for the conductance's six points.  One chunk, one step per chunk and a second call give the same bits."""
    att, _ = setup(gpu_device, "f32", stable)
    xd, nb = clips().to(gpu_device), noise_baseline().to(gpu_device)
    for name, fn in (("LayerIG", att.layer_integrated_gradients), ("LayerConductance", att.layer_conductance),
                     ("InternalInfluence", att.internal_influence)):
        one = fn(xd, 4, baselines=nb, n_steps=5, internal_batch_size=64)
        assert torch.equal(one, fn(xd, 4, baselines=nb, n_steps=5, internal_batch_size=64)), name
        for ibs in (B, 2 * B, 5 * B):
            assert torch.equal(one, fn(xd, 4, baselines=nb, n_steps=5, internal_batch_size=ibs)), (name, ibs)


def test_tap_row_sums_and_layer_relevance(gpu_device):
    att, _ = setup(gpu_device, "f32")
    g = torch.randn(6, 49, 63, generator=torch.Generator().manual_seed(1)).to(gpu_device)     # n % 4 != 0: the scalar path
    a = torch.randn(6, 49, 63, generator=torch.Generator().manual_seed(2)).to(gpu_device)
    for gg, aa in ((g, a), (g[:, :, :60].contiguous(), a[:, :, :60].contiguous())):
        sums = torch.empty(6, device=gpu_device)
        out = att.eg.layer_tap(gg, 0.25, aa, row_sum=sums)
        assert torch.equal(out, gg * 0.25 * aa)
        assert torch.allclose(sums.double().cpu(), out.double().sum((1, 2)).cpu(), rtol=1e-5, atol=1e-4)
        only = torch.empty(6, device=gpu_device)
        assert att.eg.layer_tap(gg, 0.25, aa, want_out=False, row_sum=only) is None and torch.equal(only, sums)
    attr = torch.randn(B, T, H, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    rel = att.layer_relevance(attr, L)
    ref = attr.double().sum(2).cpu()[:, torch.from_numpy(LR.frame_index(L, T))]
    assert rel.shape == (B, L) and torch.allclose(rel.double().cpu(), ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_truncation(gpu_device, stable):
    """Nothing below the layer runs: sentinels in the buffers only the lower chain writes survive ``forward_from(4, .)`` and
    ``backward(to_layer=4)``."""
    att, _ = setup(gpu_device, "f32", stable)
    eg = att.eg
    xd = clips().to(gpu_device)
    eg.forward(xd)
    h4 = eg.hidden(4)
    w = eg._workspace(B, L)
    lower_saves = [w["y"][0], w["feat"], w["pc"], w["x"][0], w["x"][3], w["qkv"][3], w["g1"][0]] + ([] if stable else [w["h1"]])
    lower_grads = [w["dz"][0], w["dz"][-1], w["dfeatn"], w["g"], w["dxh"]]
    for t in lower_saves + lower_grads:
        t.fill_(7.0)
    eg.forward_from(4, h4)
    for t in lower_saves:
        assert bool((t == 7.0).all())
    g = eg.backward(att.loss_scale, to_layer=4)
    for t in lower_saves + lower_grads:
        assert bool((t == 7.0).all())
    assert bool(torch.isfinite(g).all()) and g.shape == (B, T, H)
    for t in lower_saves + lower_grads:
        t.zero_()
    eg.forward(xd)                                                        # a full pass restores the lower chain's saves
    full = eg.backward(att.loss_scale, to_layer=4)
    assert torch.equal(full, g) or relerr(g, full.cpu()) < 1e-5
    assert bool(torch.isfinite(eg.backward(att.loss_scale)).all())


def test_range_contract(gpu_device):
    """fp32-class, post-LN: an injected value outside the split format's range saturates and raises the sticky flag -- the call
    reports SplitRangeError -- and the next valid call succeeds."""
    att, model = setup(gpu_device, "f32", False)
    eg = att.eg
    xd = clips().to(gpu_device)
    logits, _ = eg.forward(xd)
    h = eg.hidden(0)
    bad = h.clone()
    bad[1, 7, 5] = 1e5
    with pytest.raises(_lib.SplitRangeError):
        att._checked(eg.forward_from(0, bad)[0], "logits")
    lg = att._checked(eg.forward_from(0, h)[0], "logits")
    assert (lg - logits).abs().max().item() < LOGIT_TOL["f32"]
    close(att.layer_gradient_x_activation(xd, 0), ref_of(("gxa", False, 0), lambda: LR.layer_gradient_x_activation(clips(), 0, model)),
          "f32", "gradient x activation after a range error")


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_full_depth_pre_ln_model(gpu_device, precision):
    """A full-depth pre-LN encoder has a final LayerNorm: ``hidden_states[nl]`` is its output, a chain started or stopped
    below ``nl`` passes through it, one started or stopped at ``nl`` does not."""
    cfg = syn.tiny_config(True, layer_index=10)
    sd = syn.embedder_weights(cfg)
    coef, icpt = syn.logreg_weights(cfg.hidden_size)
    model = (sd, cfg, coef, icpt)
    att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, gpu_device, precision=precision))
    x = clips()
    xd = x.to(gpu_device)
    assert att.eg.emb.nl == 10
    hs = LR.hidden(x, model)
    for l in (4, 10):
        close(att.layer_activation(xd, l), hs[l], precision, f"full depth: LayerActivation l={l}")
        close(att.layer_gradient_x_activation(xd, l), LR.layer_gradient_x_activation(x, l, model), precision,
              f"full depth: gradient x activation l={l}")
        logits, _ = att.eg.forward(xd)
        assert (att.eg.forward_from(l, att.eg.hidden(l))[0] - logits).abs().max().item() < LOGIT_TOL[precision]
    attr, delta = att.layer_integrated_gradients(xd, 10, baselines=noise_baseline().to(gpu_device), n_steps=4, return_convergence_delta=True)
    ref, ref_delta = LR.layer_integrated_gradients(x, noise_baseline(), 10, model, 4)
    close(attr, ref, precision, "full depth: LayerIG l=nl")
    check_delta(delta, attr, ref_delta, ref, precision)


def test_base_1s(gpu_device):
    """wav2vec2-base (H = 768: the production tile shapes), 2 clips x 1 s, layer 6: gradient x activation vs autograd."""
    att, model = setup(gpu_device, "f32", cfg_name="base")
    x = syn.make_clips(2, 16000)
    close(att.layer_gradient_x_activation(x.to(gpu_device), 6), LR.layer_gradient_x_activation(x, 6, model), "f32", "base 1 s, l=6")


@pytest.fixture
def tiny_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_captum_front_end(gpu_device, tiny_runtime):
    import captum_saliency as cs
    from captum.attr import InternalInfluence, LayerActivation, LayerConductance, LayerGradientXActivation, LayerIntegratedGradients
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(gpu_device)
    eng = model.hip_attribution()
    assert model.num_layers() == eng.eg.emb.nl == 9
    x = clips().to(gpu_device)
    nb = noise_baseline().to(gpu_device)
    attr, delta = LayerIntegratedGradients(model, 4).attribute(x, n_steps=4, return_convergence_delta=True)
    a2, d2 = eng.layer_integrated_gradients(x, 4, n_steps=4, return_convergence_delta=True)
    assert attr.shape == (B, T, H) and delta.shape == (B,) and torch.equal(attr, a2) and torch.equal(delta, d2)
    assert torch.equal(LayerIntegratedGradients(model, 4, multiply_by_inputs=False).attribute(x, baselines=nb, n_steps=4, method="riemann_right"),
                       eng.layer_integrated_gradients(x, 4, baselines=nb, n_steps=4, method="riemann_right", multiply_by_inputs=False))
    assert torch.equal(LayerActivation(model, 4).attribute(x), eng.layer_activation(x, 4))
    assert torch.equal(LayerGradientXActivation(model, 9).attribute(x), eng.layer_gradient_x_activation(x, 9))
    assert torch.equal(LayerGradientXActivation(model, 0, multiply_by_inputs=False).attribute(x),
                       eng.layer_gradient_x_activation(x, 0, multiply_by_inputs=False))
    assert torch.equal(LayerConductance(model, 4).attribute(x, baselines=nb, n_steps=4, internal_batch_size=4),
                       eng.layer_conductance(x, 4, baselines=nb, n_steps=4))
    assert torch.equal(InternalInfluence(model, 4).attribute(x, baselines=nb, n_steps=4, method="riemann_middle"),
                       eng.internal_influence(x, 4, baselines=nb, n_steps=4, method="riemann_middle"))
    with pytest.raises(ValueError):
        LayerActivation(model, 10).attribute(x)
    for method, kw in (("layer_integrated_gradients", dict(layer=4, n_steps=4)), ("layer_gradient_x_activation", dict())):
        out = cs.explain_waves(model, x, method=method, **kw)
        assert len(out) == 3
        for p in out:
            assert p.shape == (B, 1) and bool(((p >= 0) & (p <= 1)).all())


def misaligned(t):
    """A contiguous copy of ``t`` whose data pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


KERNEL_SHAPES = [(7 * 8, False), (7 * 6, False), (7 * 8, True)]           # float4 form, scalar form (n % 4 != 0), misaligned base
KERNEL_IDS = ["float4", "scalar", "misaligned"]


@pytest.mark.parametrize("n,shift", KERNEL_SHAPES, ids=KERNEL_IDS)
def test_layer_inject_kernel(gpu_device, n, shift):
    """advh_layer_inject called directly: the residual copy and the fp16 / split operand are conversions of the input, so they
    compare bit for bit with the input, ``.half()`` and the host packer ``split_planes``."""
    from addvisor_hip.gemm import split_planes
    _lib.init()
    dev, rows = gpu_device, 3
    src = torch.randn(rows, n, generator=torch.Generator().manual_seed(n))
    src[0, :6] = torch.tensor([0.0, -0.0, 3e-5, -6.2e-5, 65504.0, -1234.567])      # below the hi plane's flush threshold, the edge
    sd = misaligned(src.to(dev)) if shift else src.to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for split in (None, 0, 1):
        resid = torch.full((rows, n), 7.0, device=dev)
        op = None if split is None else torch.full((2, rows, n), 7.0, dtype=torch.float16, device=dev)
        _lib.check(_lib.lib().advh_layer_inject(sd.data_ptr(), rows, n, resid.data_ptr(), None if op is None else op.data_ptr(),
                                                int(bool(split)), rows * n if split else 0, st), "advh_layer_inject")
        assert torch.equal(resid.cpu().view(torch.int32), src.view(torch.int32)), split
        if split == 0:
            assert torch.equal(op[0].cpu().view(torch.int16), src.half().view(torch.int16))
            assert bool((op[1] == 7.0).all())                             # the fp16 form writes no second plane
        elif split == 1:
            assert torch.equal(op.cpu().view(torch.int16), split_planes(src).view(torch.int16))


def fma32(a, b, c):
    """The correctly rounded float32 of ``a * b + c`` for float32 arrays: the product is exact in float64, TwoSum gives the
    float64 sum and its exact error, the sum is moved to the odd neighbour when it is inexact (round to odd), and the final
    rounding to float32 then equals a single rounding of the exact value (53 >= 24 + 2 bits)."""
    import numpy as np
    p, c64 = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c64
    t = s - p
    e = (p - (s - t)) + (c64 - t)                                         # s + e == p + c exactly
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    bits = np.where(fix, np.where((e > 0) == (s > 0), bits + 1, bits - 1), bits)
    return bits.view(np.float64).astype(np.float32)


@pytest.mark.parametrize("n,shift", KERNEL_SHAPES, ids=KERNEL_IDS)
def test_layer_conductance_kernel(gpu_device, n, shift):
    """advh_layer_conductance_accumulate called directly: three steps in two chunks (2 + 1), the last chunk with
    ngrad = steps - 1.  The kernel runs a fixed sequence of fp32 operations per element -- the rounded difference
    ``act[k] - pa``, then one fused multiply-add into the total -- so it compares bit for bit with a float32 numpy replay of
    that sequence.  (A replay that rounds the product before the add does not match, before or after the lane-pack rewrite:
    the step has always compiled to a fused multiply-add, in both forms; the kernel now says so with ``fmaf``.)"""
    import numpy as np
    _lib.init()
    dev, nb = gpu_device, 3
    gen = torch.Generator().manual_seed(100 + n)
    act, grad = torch.randn(3, nb, n, generator=gen), torch.randn(3, nb, n, generator=gen)
    tot0 = torch.randn(nb, n, generator=gen)
    place = (lambda t: misaligned(t.to(dev))) if shift else (lambda t: t.to(dev).contiguous())
    total, pg, pa = place(tot0), place(torch.full((nb, n), 7.0)), place(torch.full((nb, n), 7.0))
    st = torch.cuda.current_stream().cuda_stream
    for k0, steps, ngrad, first in ((0, 2, 2, 1), (2, 1, 0, 0)):
        a, g = place(act[k0:k0 + steps]), place(grad[k0:k0 + steps])
        _lib.check(_lib.lib().advh_layer_conductance_accumulate(g.data_ptr() if ngrad else None, a.data_ptr(), nb, n, steps, ngrad, first,
                                                                pg.data_ptr(), pa.data_ptr(), total.data_ptr(), st),
                   "advh_layer_conductance_accumulate")
    A, G = act.numpy(), grad.numpy()
    acc = tot0.numpy().copy()
    rpg, rpa = np.zeros_like(acc), np.zeros_like(acc)
    for k in range(3):
        if k > 0:
            acc = fma32(rpg, A[k] - rpa, acc)                             # the float32 difference rounds on its own
        rpa = A[k]
        if k < 2:
            rpg = G[k]
    assert acc.dtype == np.float32
    for what, got, ref in (("total", total, acc), ("prev_grad", pg, rpg), ("prev_act", pa, rpa)):
        diff = int((got.cpu().numpy().view(np.uint32) != ref.view(np.uint32)).sum())
        print(f"conductance {what} n={n} shift={shift}: {diff} of {ref.size} words differ")
        assert diff == 0, what
