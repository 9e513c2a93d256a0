"""GPU: conservative propagation through the encoder (csrc/lrp.hip, EmbedderGrad.backward(rules=...),
HipAttribution.transformer_lrp).

* the entry points against fp64 on exact inputs (split planes joined for the reference, or plain fp16): the value-only attention
  backward over every tile-count and head-dim class with the attention backward's own bar, the frozen-sigma LayerNorm backward with
  the LayerNorm backward's, the GELU identity multiply;
* the engine end to end against the float64 restatement of tests/lrp_ref.py with the project's attribution bars;
* rules=None and all rules off against the plain chain to the bit, conservation on a bias-free model, the captum_saliency front end.

Every test prints the figures it asserts on (max relative error of max|ref|, cosine): run with ``-s`` to read them.
"""
import itertools
import os

import pytest
import torch
import torch.nn.functional as F

import lrp_ref as LR
from addvisor_hip import _lib, gemm as G, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
from addvisor_hip.embedder_grad import LrpRules

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

VALUE_BAR = 5e-6             # tests/test_gpu_backward_kernels.py::test_attention_bwd_split: dV of that computation
LN_BAR = 2e-5                # tests/test_gpu_backward_kernels.py::test_layernorm_bwd's fp32 bar
GELU_BAR = 1e-6              # fp32 product of two 22-bit values re-split to 22 bits
TOL = {"f32": (1e-4, 0.999999), "f16": (3e-2, 0.999)}      # tests/test_gpu_layer_attr.py: every attribution map
SPLIT_MAX, SAT_MAX = 65504.0, 65504.0 + 65504.0 / 2048.0   # csrc/device_math.h: hi saturates, lo carries the clamped remainder


def relerr(a, b):
    return ((a.cpu().double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300)).item()


def _st():
    return torch.cuda.current_stream().cuda_stream


def flag_after(launch) -> bool:
    """Run ``launch`` with the sticky range flag cleared first; True iff it is set afterwards."""
    lib = _lib.lib()
    torch.cuda.synchronize()
    lib.advh_split_overflow(1)
    launch()
    torch.cuda.synchronize()
    return bool(lib.advh_split_overflow(1))


# --------------------------------------------------------------------------------------------------------------- value-only attention backward
def launch_value(qkv, dctx, B, T, H, heads, split):
    out = torch.full((2, B * T, 3 * H) if split else (B * T, 3 * H), float("nan"), dtype=torch.float16, device=qkv.device)
    lo = lambda t: t.stride(0) if split else 0
    rc = _lib.lib().advh_attention_bwd_value(qkv.data_ptr(), lo(qkv), dctx.data_ptr(), lo(dctx), out.data_ptr(), lo(out), B, T, H, heads, _st())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out


def value_ref(x, do, B, T, heads, D):
    """dV [B*T, H] in fp64 from the joined operands: P^T dO per (clip, head)."""
    H = heads * D
    q, k, _ = [t.view(B, T, heads, D).transpose(1, 2) for t in x.split(H, dim=1)]
    P = torch.softmax(q @ k.transpose(2, 3) * D ** -0.5, -1)
    return (P.transpose(2, 3) @ do.view(B, T, heads, D).transpose(1, 2)).transpose(1, 2).reshape(B * T, H)


def operands(q32, d32, split):
    """The operands in the kernel's format and their exact fp64 values."""
    if split:
        qh, dh = G.split_planes(q32), G.split_planes(d32)
        return qh, dh, G.join_planes(qh).double(), G.join_planes(dh).double()
    qh, dh = q32.half(), d32.half()
    return qh, dh, qh.double(), dh.double()


@pytest.mark.parametrize("T,heads,D", [(1, 1, 8), (15, 2, 16), (16, 1, 32), (17, 3, 32), (49, 2, 32), (99, 2, 64), (199, 3, 64), (249, 2, 64),
                                       (256, 1, 64), (49, 2, 120), (249, 1, 128), (256, 1, 128)])
def test_attention_bwd_value_kernel(gpu_device, T, heads, D):
    """advh_attention_bwd_value vs fp64 on exact inputs, B = 1 and 2, both operand formats: dV within the attention backward's bar
    (in the plain-fp16 format dV leaves as one fp16, whose own rounding, 2^-11 relative, is added to the bar: the arithmetic is the
    same fp32 MFMA path), the Q and K thirds exactly zero, every element written, bit-identical across launches and across the
    batch size."""
    _lib.init()
    g = torch.Generator().manual_seed(T + D)
    H = heads * D
    q32, d32 = torch.randn(2 * T, 3 * H, generator=g) * 0.7, torch.randn(2 * T, H, generator=g)
    worst = {}
    for split in (True, False):
        qh, dh, x, do = operands(q32, d32, split)
        ref = value_ref(x, do, 2, T, heads, D)
        first = (lambda t: t[:, :T].contiguous()) if split else (lambda t: t[:T].contiguous())
        join = (lambda t: G.join_planes(t.cpu())) if split else (lambda t: t.cpu().float())
        out2 = launch_value(qh.to(gpu_device), dh.to(gpu_device), 2, T, H, heads, split)
        out1 = launch_value(first(qh).to(gpu_device), first(dh).to(gpu_device), 1, T, H, heads, split)
        assert torch.equal(out2, launch_value(qh.to(gpu_device), dh.to(gpu_device), 2, T, H, heads, split))
        assert torch.equal(first(out2), out1)                                          # clip 0 does not depend on B
        for B, out in ((2, out2), (1, out1)):
            got = join(out)
            assert torch.isfinite(got).all()                                           # pre-filled with NaN: every element is written
            assert not bool(out.cpu()[..., :2 * H].any())                              # dQ = dK = 0, both planes
            err = relerr(got[:, 2 * H:], ref[:B * T])
            bar = VALUE_BAR if split else VALUE_BAR + 2.0 ** -11                       # plain fp16 output: one more rounding, of dV to fp16
            worst[(split, B)] = err
            assert err < bar, (split, B, err)
    print(f"attention bwd value T={T} heads={heads} d={D}: dV rel err of max|ref| "
          + ", ".join(f"{'split' if s else 'fp16'} B={b} {e:.2e}" for (s, b), e in worst.items()))


def test_attention_bwd_value_range_contract(gpu_device):
    """The V third goes through the checked split conversion: a dV past 65 504 saturates and raises the sticky flag, a NaN in dO
    gives NaN planes in its column with the flag clear, and in-range launches leave it clear."""
    _lib.init()
    T, heads, D, B = 17, 2, 16, 1
    H = heads * D
    g = torch.Generator().manual_seed(5)
    q32, d32 = torch.randn(B * T, 3 * H, generator=g) * 0.7, torch.randn(B * T, H, generator=g)
    run = lambda qh, dh: launch_value(qh.to(gpu_device), dh.to(gpu_device), B, T, H, heads, True)
    qh, dh, x, do = operands(q32, d32, True)
    assert not flag_after(lambda: run(qh, dh))
    big = d32.clone()
    big[:, 3] = 60000.0                                     # dV[k, 3] = 60000 sum_q P[q, k]: past the range where a key's column sum > 1.092
    qh, dh, x, do = operands(q32, big, True)
    ref = value_ref(x, do, B, T, heads, D)
    over = ref.abs() > SPLIT_MAX * (1 + 1e-4)
    assert bool(over.any()) and bool((ref.abs() > SAT_MAX * (1 + 1e-4)).any())         # the case is what it says: past hi, and past hi + lo
    ref = ref.clamp(-SAT_MAX, SAT_MAX)                                                 # the planes saturate at 65504 + 65504 / 2048
    out = []
    assert flag_after(lambda: out.append(run(qh, dh)))
    hi, got = out[0][0].cpu()[:, 2 * H:], G.join_planes(out[0].cpu())[:, 2 * H:]
    assert bool((hi[over].float().abs() == SPLIT_MAX).all())                           # hi saturates, lo carries the remainder
    err = relerr(got, ref)
    print(f"saturating dV: {int(over.sum())} values past 65504 (max |ref| {ref.abs().max():.1f}), joined planes rel err {err:.2e}")
    assert err < VALUE_BAR
    nan = G.split_planes(d32)
    nan[:, 5, 3] = float("nan")
    out = []
    assert not flag_after(lambda: out.append(run(G.split_planes(q32), nan)))
    dv = out[0].cpu()[:, :, 2 * H:]
    assert bool(torch.isnan(dv[:, :, 3]).all())                                        # P > 0: the NaN reaches every key of head 0's column 3
    keep = torch.ones(H, dtype=torch.bool)
    keep[3] = False
    assert bool(torch.isfinite(dv[:, :, keep]).all()) and not bool(out[0].cpu()[..., :2 * H].any())


# --------------------------------------------------------------------------------------------------------------- frozen-sigma LayerNorm backward
@pytest.mark.parametrize("C", [32, 64, 120, 768, 1920])
def test_layernorm_bwd_frozen_kernels(gpu_device, C):
    """advh_layernorm_bwd_frozen(_split) vs fp64 autograd through a LayerNorm with detached 1/sigma: x and dy as fp32 and as
    planes (and as plain fp16), every present / absent combination of add, out_f and out_h, rows that fill and do not fill a
    workgroup."""
    _lib.init()
    lib, d = _lib.lib(), gpu_device
    g = torch.Generator().manual_seed(C)
    worst = {"f32": 0.0, "planes": 0.0, "fp16": 0.0}
    for M in (1, 7, 98, 499):
        gamma = torch.rand(C, generator=g) + 0.5
        x32, dy32, add = torch.randn(M, C, generator=g) + 0.3, torch.randn(M, C, generator=g) * 3.0, torch.randn(M, C, generator=g)
        xs, dys = G.split_planes(x32), G.split_planes(dy32)
        forms = {"f32": (x32, dy32), "planes": (xs, dys), "fp16": (x32.half(), dy32.half())}
        exact = {"f32": (x32.double(), dy32.double()), "planes": (G.join_planes(xs).double(), G.join_planes(dys).double()),
                 "fp16": (x32.half().double(), dy32.half().double())}
        refs = {}
        for (kx, kd) in itertools.product(exact, exact):
            with torch.enable_grad():
                xr = exact[kx][0].clone().requires_grad_(True)
                y = LR.layer_norm(xr, gamma.double(), torch.zeros(C, dtype=torch.float64), 1e-5, True)
                (refs[(kx, kd)],) = torch.autograd.grad(y, xr, exact[kd][1])
        gd, ad = gamma.to(d), add.to(d)
        dev = {k: (a.to(d), b.to(d)) for k, (a, b) in forms.items()}
        p = lambda t: None if t is None else t.data_ptr()
        for kx, kd, use_add, (use_f, use_h) in itertools.product(("f32", "planes"), ("f32", "planes"), (False, True),
                                                                 ((True, False), (False, True), (True, True))):
            xd, dyd = dev[kx][0], dev[kd][1]
            ref = refs[(kx, kd)] + (add.double() if use_add else 0)
            out_f = torch.full((M, C), float("nan"), device=d) if use_f else None
            out_h = torch.full((2, M, C), float("nan"), dtype=torch.float16, device=d) if use_h else None
            lo = lambda t, k: t.stride(0) if k == "planes" else 0
            rc = lib.advh_layernorm_bwd_frozen_split(xd.data_ptr(), int(kx == "f32"), lo(xd, kx), dyd.data_ptr(), int(kd == "f32"), lo(dyd, kd),
                                                     gd.data_ptr(), ad.data_ptr() if use_add else None, p(out_f), p(out_h),
                                                     out_h.stride(0) if use_h else 0, M, C, 1e-5, _st())
            torch.cuda.synchronize()
            assert rc == 0, rc
            for got in ([out_f.cpu()] if use_f else []) + ([G.join_planes(out_h.cpu())] if use_h else []):
                err = relerr(got, ref)
                key = "planes" if "planes" in (kx, kd) else "f32"
                worst[key] = max(worst[key], err)
                assert err < LN_BAR, (M, kx, kd, use_add, use_f, use_h, err)
        # the plain-fp16 entry point: fp16 x / dy (fp32 ones take the same path as above), fp32 and fp16 outputs
        for use_add, (use_f, use_h) in itertools.product((False, True), ((True, False), (False, True), (True, True))):
            xd, dyd = dev["fp16"]
            ref = refs[("fp16", "fp16")] + (add.double() if use_add else 0)
            out_f = torch.full((M, C), float("nan"), device=d) if use_f else None
            out_h = torch.full((M, C), float("nan"), dtype=torch.float16, device=d) if use_h else None
            rc = lib.advh_layernorm_bwd_frozen(xd.data_ptr(), 0, dyd.data_ptr(), 0, gd.data_ptr(), ad.data_ptr() if use_add else None,
                                               p(out_f), p(out_h), M, C, 1e-5, _st())
            torch.cuda.synchronize()
            assert rc == 0, rc
            if use_f:
                err = relerr(out_f, ref)
                worst["fp16"] = max(worst["fp16"], err)
                assert err < LN_BAR, (M, use_add, err)
            if use_h:
                assert relerr(out_h.float(), ref) < 2.0 ** -11 + LN_BAR                 # one fp16 rounding of the fp32 result
                if use_f:
                    assert torch.equal(out_h, out_f.half())
    print(f"frozen LayerNorm bwd C={C}: rel err of max|ref| " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# --------------------------------------------------------------------------------------------------------------- GELU identity rule
@pytest.mark.parametrize("n", [1, 7, 8, 3072 * 3 + 5])
def test_gelu_identity_bwd_kernel(gpu_device, n):
    """advh_gelu_identity_bwd vs fp64 d * Phi(g1) on exact inputs: plane pairs (tight planes -- the one-by-one path unless n % 8 ==
    0 -- and planes padded to a multiple of 8 -- vectors plus the n % 8 tail) and plain fp16, in place and out of place."""
    _lib.init()
    lib, dev = _lib.lib(), gpu_device
    g = torch.Generator().manual_seed(n)
    d32, g32 = torch.randn(n, generator=g) * 5.0, torch.randn(n, generator=g) * 2.0
    phi = lambda t: 0.5 * (1.0 + torch.erf(t / 2.0 ** 0.5))
    worst = {}
    pad = (n + 7) // 8 * 8
    for name, width in (("planes", n), ("planes padded", pad)):
        def planes(t):
            out = torch.zeros(2, width, dtype=torch.float16)
            out[:, :n] = G.split_planes(t)
            return out
        dp, gp = planes(d32), planes(g32)
        ref = G.join_planes(dp[:, :n]).double() * phi(G.join_planes(gp[:, :n]).double())
        for inplace in (False, True):
            dd, gd = dp.to(dev), gp.to(dev)
            out = dd if inplace else torch.full((2, width), float("nan"), dtype=torch.float16, device=dev)
            rc = lib.advh_gelu_identity_bwd(dd.data_ptr(), width, gd.data_ptr(), width, out.data_ptr(), width, n, _st())
            torch.cuda.synchronize()
            assert rc == 0, rc
            err = relerr(G.join_planes(out.cpu()[:, :n]), ref)
            worst[f"{name}{' in place' if inplace else ''}"] = err
            assert err < GELU_BAR, (name, inplace, err)
            if not inplace:
                assert torch.equal(dd.cpu(), dp) and bool(torch.isnan(out.cpu()[:, n:]).all())       # nothing past n is touched
    dh, gh = d32.half(), g32.half()
    ref = dh.double() * phi(gh.double())
    # fp16 output: one rounding of the fp32 product (2^-11 relative, or half the subnormal spacing 2^-25 below 2^-14), on top of
    # fast_erf's documented 1.5e-7 absolute error in Phi's erf (csrc/device_math.h): |d| * 7.5e-8
    # and four fp32 roundings (the argument of erf, 1 + erf, the halving's product with d): 4 * 2^-24 relative
    bound = (2.0 ** -11 + 2.0 ** -22) * ref.abs() + 2.0 ** -25 + 1e-7 * dh.double().abs()
    for inplace in (False, True):
        dd, gd = dh.to(dev), gh.to(dev)
        out = dd if inplace else torch.full((n,), float("nan"), dtype=torch.float16, device=dev)
        rc = lib.advh_gelu_identity_bwd(dd.data_ptr(), 0, gd.data_ptr(), 0, out.data_ptr(), 0, n, _st())
        torch.cuda.synchronize()
        assert rc == 0, rc
        gap = (out.cpu().double() - ref).abs()
        worst[f"fp16{' in place' if inplace else ''} (of its bound)"] = (gap / bound).max().item()
        assert bool((gap <= bound).all()), (inplace, (gap / bound).max().item())
    print(f"GELU identity bwd n={n}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# --------------------------------------------------------------------------------------------------------------- end to end
def d120_config():
    return syn.tiny_config(True, hidden_size=240, num_attention_heads=2, intermediate_size=480, num_conv_pos_embedding_groups=2,
                           num_hidden_layers=10)


CONFIGS = {"post_ln_1s": (lambda: syn.tiny_config(False), 2, 16000), "post_ln_5s": (lambda: syn.tiny_config(False), 1, 80000),
           "pre_ln_1s": (lambda: syn.tiny_config(True), 2, 16000), "pre_ln_5s": (lambda: syn.tiny_config(True), 1, 80000),
           "d120_1s": (d120_config, 2, 16000), "d120_5s": (d120_config, 1, 80000), "base_1s": (syn.base_config, 1, 16000)}
RULES = {"default": dict(), "all identity": dict(gelu_rule="identity"), "ln alone": dict(attention_rule=False),
         "attention alone": dict(ln_rule=False), "gelu alone": dict(ln_rule=False, attention_rule=False, gelu_rule="identity")}
_ENG, _REF = {}, {}


def engine(dev, name, precision, zero_bias=False):
    key = (name.rsplit("_", 1)[0], precision, zero_bias)
    if key not in _ENG:
        cfg = CONFIGS[name][0]()
        model = (syn.embedder_weights(cfg), cfg) + tuple(syn.logreg_weights(cfg.hidden_size))
        if zero_bias:
            model = LR.zero_bias_model(model)
        sd, _, coef, icpt = model
        _ENG[key] = (HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision)), model)
    return _ENG[key]


def reference(name, model, x):
    """The float64 restatement (target 1) for every rule set at start_layer 0 and the default rules at start_layer 4, computed once
    and shared by the precisions; the other targets are per-clip sign flips of it (the chain is linear in the seed)."""
    if name not in _REF:
        r = {k: LR.explain(x, model, **kw) for k, kw in RULES.items()}
        r["start_layer=4"] = LR.explain(x, model, start_layer=4)
        _REF[name] = r
    return _REF[name]


def close(ours, ref, precision, what, worst):
    tol, cmin = TOL[precision]
    assert tuple(ours.shape) == tuple(ref.shape), (what, ours.shape, ref.shape)
    assert ours.dtype == torch.float32
    err = relerr(ours, ref)
    cos = F.cosine_similarity(ours.cpu().double().flatten(), ref.double().flatten(), dim=0).item()
    w = worst.setdefault(what, [0.0, 1.0])
    w[0], w[1] = max(w[0], err), min(w[1], cos)
    assert err < tol and cos > cmin, (what, err, cos)


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_engine_against_the_float64_restatement(gpu_device, name, precision):
    att, model = engine(gpu_device, name, precision)
    _, B, L = CONFIGS[name]
    x = syn.make_clips(B, L, seed=12)
    ref = reference(name, model, x)
    xd = x.to(gpu_device)
    worst = {}
    # The fp16 chain's own attention backward (advh_attention_bwd_f16) has no instance for head dims > 64 at T > 208: at d120 / 5 s
    # the plain fp16 chain, and every rule set that keeps the plain attention backward, returns ADVH_EUNSUPPORTED as it always
    # has.  The value-only kernel has the instance, so the rule sets with the attention rule are checked there like anywhere.
    plain = not (precision == "f16" and name == "d120_5s")
    sal = att.saliency(xd) if plain else None
    for k, kw in RULES.items():
        if not plain and kw.get("attention_rule") is False:
            with pytest.raises(_lib.AdvhError, match="ADVH_EUNSUPPORTED"):
                att.transformer_lrp(xd, **kw)
            continue
        rel, R = att.transformer_lrp(xd, return_hidden=True, **kw)
        close(rel, ref[k]["rel"], precision, f"rel {k}", worst)
        close(R, ref[k]["R"], precision, f"R {k}", worst)
    rel4, R4 = att.transformer_lrp(xd, start_layer=4, return_hidden=True)
    close(rel4, ref["start_layer=4"]["rel"], precision, "rel start_layer=4", worst)
    close(R4, ref["start_layer=4"]["R"], precision, "R start_layer=4", worst)
    # targets: 1 is the default, 0 explains -F, "predicted" and a tensor pick per clip
    r = ref["default"]
    rel, R = att.transformer_lrp(xd, return_hidden=True)
    assert torch.equal(att.transformer_lrp(xd, target=1), rel) and torch.equal(att.transformer_lrp(xd), rel)
    signed = lambda s, key: r[key] * s.to(torch.float64).view(-1, *([1] * (r[key].dim() - 1)))
    pred, tens = torch.sign(r["logits"]), (torch.arange(B) % 2) * 2.0 - 1.0
    for what, target, s in (("target=0", 0, -torch.ones(B)), ("predicted", "predicted", pred), ("tensor", torch.arange(B) % 2, tens),
                            ("device tensor", (torch.arange(B) % 2).to(gpu_device), tens)):
        rel_t, R_t = att.transformer_lrp(xd, target=target, return_hidden=True)
        close(rel_t, signed(s, "rel"), precision, f"rel {what}", worst)
        close(R_t, signed(s, "R"), precision, f"R {what}", worst)
    # bit-identical across calls; the chain's state is clean afterwards
    rel_b, R_b = att.transformer_lrp(xd, return_hidden=True)
    assert torch.equal(rel_b, rel) and torch.equal(R_b, R)
    assert not plain or torch.equal(att.saliency(xd), sal)
    assert tuple(att.frames_to_wave(rel, L).shape) == (B, L)
    print(f"{name} [{precision}] vs float64 restatement, max rel err of max|ref| / min cosine: "
          + ", ".join(f"{k} {v[0]:.2e} / {v[1]:.8f}" for k, v in worst.items()))


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("name", ["post_ln_1s", "pre_ln_1s"])
def test_rules_none_and_rules_off_are_the_plain_chain(gpu_device, name, precision):
    """backward(rules=None) is the call without the argument, bit for bit, for the input gradient and for to_layer gradients; all
    rules off is layer_gradient_x_activation and its row sums; the rules combine with attention_maps, which only reads."""
    att, _ = engine(gpu_device, name, precision)
    eg = att.eg
    _, B, L = CONFIGS[name]
    x = syn.make_clips(B, L, seed=12).to(gpu_device)
    eg.forward(x)
    g0, g4 = eg.backward(att.loss_scale), eg.backward(att.loss_scale, to_layer=4)
    assert torch.equal(eg.backward(att.loss_scale, rules=None), g0)
    assert torch.equal(eg.backward(att.loss_scale, to_layer=4, rules=None), g4)
    off = LrpRules(False, False, "gradient")
    assert torch.equal(eg.backward(att.loss_scale, to_layer=4, rules=off), g4)
    on = eg.backward(att.loss_scale, to_layer=4, rules=LrpRules())
    assert not torch.equal(on, g4)
    T, heads = g4.shape[1], eg.cfg.num_attention_heads
    maps = torch.full((2, B, heads, T, T), float("nan"), device=gpu_device)
    assert torch.equal(eg.backward(att.loss_scale, to_layer=4, rules=LrpRules(), attention_maps=(maps, 0)), on)
    assert bool(torch.isfinite(maps).all())
    assert torch.equal(eg.backward(att.loss_scale), g0)                                # the plain chain is untouched afterwards
    for bad in (dict(rules=LrpRules()), dict(rules=LrpRules(), from_layer=3, neuron=(0, 1, 1, 0, 1, 1)), dict(rules="all", to_layer=0)):
        with pytest.raises(ValueError):
            eg.backward(att.loss_scale, **bad)
    for s0 in (0, 4):
        rel, R = att.transformer_lrp(x, start_layer=s0, ln_rule=False, attention_rule=False, return_hidden=True)
        gxa = att.layer_gradient_x_activation(x, s0)
        assert torch.equal(R, gxa)
        sums = torch.empty(B * T, dtype=torch.float32, device=gpu_device)
        eg.layer_tap(gxa.view(B * T, -1), 1.0, want_out=False, row_sum=sums)
        assert torch.equal(rel, sums.view(B, T))
        assert torch.equal(att.frames_to_wave(rel, L), att.layer_relevance(gxa, L))
    print(f"{name} [{precision}]: rules=None and rules off are the plain chain to the bit; max |rules on - plain| / max |plain| at layer 4 "
          f"{relerr(on, g4.cpu()):.2e}")


@pytest.mark.parametrize("name", ["post_ln_1s", "pre_ln_1s"])
def test_conservation_on_a_bias_free_model(gpu_device, name):
    """All three rules on (GELU by identity), every bias, LayerNorm beta and the intercept zero: sum_t rel = +-F."""
    att, model = engine(gpu_device, name, "f32", zero_bias=True)
    _, B, L = CONFIGS[name]
    x = syn.make_clips(B, L, seed=12)
    xd = x.to(gpu_device)
    logit = att.logits(xd).cpu().double()
    for target, s0, sign in ((None, 0, 1.0), (0, 0, -1.0), (None, 4, 1.0)):
        rel = att.transformer_lrp(xd, target=target, start_layer=s0, gelu_rule="identity").cpu().double()
        gap, mass = (rel.sum(-1) - sign * logit).abs(), rel.abs().sum(-1)
        print(f"{name} target={target} start_layer={s0}: |sum_t rel - (+-F)| {gap.tolist()} of sum_t |rel| {mass.tolist()} "
              f"(ratio {(gap / mass).max().item():.2e})")
        assert bool((gap <= 1e-4 * mass).all())


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
    rel = att.transformer_lrp(x)
    assert torch.equal(cs._explainer(att, "transformer_lrp")(x), att.frames_to_wave(rel, L))
    assert torch.equal(cs._explainer(att, "transformer_lrp", layer=4)(x), att.frames_to_wave(att.transformer_lrp(x, start_layer=4), L))
    out = cs.explain_waves(model, x, method="transformer_lrp")
    assert len(out) == 3
    for p in out:
        assert p.shape == (B, 1) and bool(torch.isfinite(p).all()) and bool(((p >= 0) & (p <= 1)).all())
    out = cs.explain_waves(model, x, method="transformer_lrp", layer=4, nt_type="smoothgrad", nt_samples=2)
    assert all(p.shape == (B, 1) and bool(torch.isfinite(p).all()) for p in out)
    nt = cs._explainer(att, "transformer_lrp", nt_type="smoothgrad", nt_samples=2)(x)
    assert nt.shape == (B, L) and bool(torch.isfinite(nt).all())
    sc = cs.score_explanations(model, x, method="transformer_lrp", n_perturb_samples=2)
    assert bool(torch.isfinite(sc["infidelity"]).all()) and bool(torch.isfinite(sc["sensitivity_max"]).all())
    out = cs.attack_waves(model, x, torch.tensor([0, 1]), attack="fgsm", explain="transformer_lrp", epsilon=5e-4)
    assert out["explanation_shift"].shape == (B,) and bool(torch.isfinite(out["explanation_shift"]).all())
    print(f"transformer_lrp front end: NoiseTunnel max |attr| {nt.abs().max().item():.3e}, infidelity {sc['infidelity'].tolist()}, "
          f"sensitivity_max {sc['sensitivity_max'].tolist()}, explanation_shift {out['explanation_shift'].tolist()}")
    with pytest.raises(ValueError):
        cs.explain_waves(model, x, method="transformer_lrp", layer=9)
