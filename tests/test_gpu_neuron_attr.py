"""GPU: the neuron attributions (NeuronGradient, NeuronIntegratedGradients, NeuronGradientShap, NeuronConductance,
NeuronFeatureAblation) on the HIP encoder chain stopped at a layer in the forward and started there in the backward
(csrc/attribution_neuron.hip, EmbedderGrad.forward(to_layer=...) / backward(from_layer=...)) vs the CPU restatement of
tests/neuron_attr_ref.py: the two kernels alone, chain consistency, parity, completeness, chunking and determinism, truncation
and the captum.attr front end.  The bars are those of tests/test_gpu_layer_attr.py."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import neuron_attr_ref as NR
from addvisor_hip import _lib, attribution as AT, runtime, synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = {"f32": (1e-4, 0.999999), "f16": (3e-2, 0.999)}
# delta vs the restatement's delta: within rel * |s_n(x) - s_n(b)| + abs
DELTA_TOL = {"f32": (1e-3, 1e-4), "f16": (3e-2, 1e-2)}
B, L, T, H = 2, 16000, 49, 64
NUMBER = 0.0625                                                             # tests/test_gpu_layer_attr.py: a constant clip that normalises exactly
FLAVOURS = [False, True]                                                   # do_stable_layer_norm: post-LN, pre-LN
IDS = ["post_ln", "pre_ln"]
BAND = (slice(0, 49, 2), slice(60, 64))
SELECTORS = [(7, 5), (-1, -1), BAND]


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
        cfg = {"tiny": lambda: syn.tiny_config(stable), "full": lambda: syn.tiny_config(True, layer_index=10), "base": syn.base_config}[cfg_name]()
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


# ---------------------------------------------------------------------------------------------------- the kernels alone
def _box(*v):
    return (C.c_int * 6)(*v)


def _st():
    return torch.cuda.current_stream().cuda_stream


def boxes(Tk, Hk):
    """Boxes on every edge of a [Tk, Hk] frame, the full frame, and steps 2 and 3."""
    return [(0, 1, 1, 0, Hk, 1), (Tk - 1, Tk, 1, 0, Hk, 1), (0, Tk, 1, 0, 1, 1), (0, Tk, 1, Hk - 1, Hk, 1), (0, Tk, 1, 0, Hk, 1),
            (0, Tk, 2, 1, Hk, 3), (1, Tk, 3, 0, Hk - 1, 2), (2, 3, 1, 3, 4, 1)]


def indicator(Tk, Hk, box):
    m = torch.zeros(Tk, Hk)
    m[box[0]:box[1]:box[2], box[3]:box[4]:box[5]] = 1
    return m


def run_seed(dev, R, Tk, Hk, scale, box=None, row_scale=None, src=None, split=1, offset=0):
    """advh_layer_seed into poisoned buffers whose base is ``offset`` floats (``2 * offset`` halves) past an aligned
    allocation; returns ``(resid, hi, lo | None)`` on the host."""
    n = R * Tk * Hk
    resid = torch.full((n + 4,), float("nan"), device=dev)[offset:offset + n]
    op = torch.full((2 * n + 8,), float("nan"), dtype=torch.float16, device=dev)[2 * offset:2 * offset + 2 * n]
    if src is not None:
        src = torch.cat([torch.zeros(offset), src.flatten()]).to(dev)[offset:]
    rs = None if row_scale is None else row_scale.to(dev)
    p = lambda t: None if t is None else t.data_ptr()
    rc = _lib.lib().advh_layer_seed(p(src), p(rs), scale, R, Tk, Hk, None if box is None else _box(*box), resid.data_ptr(), op.data_ptr(),
                                    split, n if split else 0, _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    resid, op = resid.cpu().view(R, Tk, Hk), op.cpu()
    return resid, op[:n].view(R, Tk, Hk), (op[n:].view(R, Tk, Hk) if split else None)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset_by_one_float"])
@pytest.mark.parametrize("Hk", [6, 8], ids=["scalar_path", "vector_path"])
def test_layer_seed_kernel(gpu_device, Hk, offset):
    _lib.init()
    R, Tk = 3, 5
    rs = torch.tensor([1.0, 2.0, 0.25])
    for split in (0, 1):
        for box in boxes(Tk, Hk):
            for row_scale in (None, rs):
                resid, hi, lo = run_seed(gpu_device, R, Tk, Hk, 0.5, box, row_scale, split=split, offset=offset)
                want = 0.5 * indicator(Tk, Hk, box)[None] * (torch.ones(R) if row_scale is None else rs)[:, None, None]
                assert torch.equal(resid, want), (box, split)
                # powers of two (and zeros): the fp16 plane holds the value, the split pair sums to it exactly
                assert torch.equal(hi.float() + (lo.float() / 2048 if split else 0), want), (box, split)
        src = torch.randint(-8, 9, (R, Tk, Hk), generator=torch.Generator().manual_seed(5)).float() * 0.25
        resid, hi, lo = run_seed(gpu_device, R, Tk, Hk, 2.0, src=src, split=split, offset=offset)
        assert torch.equal(resid, 2.0 * src) and torch.equal(hi.float() + (lo.float() / 2048 if split else 0), 2.0 * src)
    # a value the fp16 plane cannot hold exactly: the pair carries it to the format's ~22 bits
    src = torch.randn(R, Tk, Hk, generator=torch.Generator().manual_seed(6))
    resid, hi, lo = run_seed(gpu_device, R, Tk, Hk, 3.0, src=src, offset=offset)
    assert torch.equal(resid, 3.0 * src) and torch.equal(hi, (3.0 * src).half())
    assert ((hi.double() + lo.double() / 2048 - resid.double()).abs() <= 2.0 ** -21 * resid.double().abs()).all()
    _lib.check_overflow("in-range seeds")


def test_layer_seed_range_contract(gpu_device):
    """Out of range saturates and raises the sticky flag -- SplitRangeError -- and the next call succeeds; NaN stays NaN and
    leaves the flag clear."""
    _lib.init()
    src = torch.ones(3, 5, 8)
    src[1, 2, 3] = 1e5
    resid, hi, lo = run_seed(gpu_device, 3, 5, 8, 1.0, src=src)
    assert resid[1, 2, 3].item() == 1e5 and hi[1, 2, 3].item() == 65504.0
    with pytest.raises(_lib.SplitRangeError):
        _lib.check_overflow("advh_layer_seed")
    src[1, 2, 3] = float("nan")
    resid, hi, lo = run_seed(gpu_device, 3, 5, 8, 1.0, src=src)
    _lib.check_overflow("advh_layer_seed after a range error")
    assert torch.isnan(hi[1, 2, 3]) and torch.isnan(lo[1, 2, 3]) and hi.flatten()[0].item() == 1.0
    run_seed(gpu_device, 3, 5, 8, 1e5, box=(0, 1, 1, 0, 1, 1))             # box mode: the scale itself is out of range
    with pytest.raises(_lib.SplitRangeError):
        _lib.check_overflow("advh_layer_seed")
    run_seed(gpu_device, 3, 5, 8, 1.0, box=(0, 1, 1, 0, 1, 1))
    _lib.check_overflow("advh_layer_seed after a range error")


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset_by_one_float"])
@pytest.mark.parametrize("Hk", [6, 8], ids=["scalar_path", "vector_path"])
def test_neuron_values_kernel(gpu_device, Hk, offset):
    R, Tk = 3, 5
    v = torch.randn(R, Tk, Hk, generator=torch.Generator().manual_seed(7))
    vd = torch.cat([torch.zeros(offset), v.flatten()]).to(gpu_device)[offset:]
    shapes = [(R, Tk, Hk, v, vd)]
    if not offset:                                                          # more than one trip of the workgroup's loop: 49 x 64 > 256
        big = torch.randn(R, T, H, generator=torch.Generator().manual_seed(8))
        shapes.append((R, T, H, big, big.to(gpu_device)))
    for Rk, Tq, Hq, host, dev_t in shapes:
        for box in boxes(Tq, Hq):
            out = torch.full((Rk,), float("nan"), device=gpu_device)
            call = lambda o: _lib.check(_lib.lib().advh_neuron_values(dev_t.data_ptr(), Rk, Tq, Hq, _box(*box), o.data_ptr(), _st()), "advh_neuron_values")
            call(out)
            ref = (host.double() * indicator(Tq, Hq, box).double()[None]).sum((1, 2))
            assert torch.allclose(out.double().cpu(), ref, rtol=1e-5, atol=1e-5 * host.abs().max().item()), (box, out, ref)
            again = torch.empty_like(out)
            call(again)
            assert torch.equal(out, again), box


# ---------------------------------------------------------------------------------------------------- chain consistency
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("cfg_name,stable", [("tiny", False), ("tiny", True), ("full", True)], ids=IDS + ["pre_ln_full_depth"])
def test_seeded_backward_continues_the_stopped_backward(gpu_device, cfg_name, stable, precision):
    """``backward(to_layer=l)`` then ``backward(from_layer=l, layer_seed=that gradient)`` is ``backward()``: the two halves of
    the chain meet at every layer, the final LayerNorm of a full-depth pre-LN model included.  No reference needed."""
    att, _ = setup(gpu_device, precision, stable, cfg_name)
    eg = att.eg
    nl = eg.emb.nl
    assert nl == (10 if cfg_name == "full" else 9)
    eg.forward(clips().to(gpu_device))
    full = att._checked(eg.backward(att.loss_scale))
    for l in (0, 4, nl):
        g = eg.backward(att.loss_scale, to_layer=l)
        dx = att._checked(eg.backward(att.loss_scale, from_layer=l, layer_seed=g))
        close(dx, full.cpu(), precision, f"{cfg_name} stable={stable}: stopped + seeded backward at l={l}")
    with pytest.raises(ValueError):
        eg.backward(att.loss_scale, from_layer=4)                          # neither a neuron nor a seed
    with pytest.raises(ValueError):
        eg.backward(att.loss_scale, from_layer=4, neuron=(0, 1, 1, 0, 1, 1), layer_seed=g)
    with pytest.raises(ValueError):
        eg.backward(att.loss_scale, from_layer=4, layer_seed=g[:, :-1])
    with pytest.raises(ValueError):
        eg.backward(att.loss_scale, neuron=(0, 1, 1, 0, 1, 1))             # a neuron without from_layer


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_neuron_gradient_is_linear_in_the_selection(gpu_device, stable, precision):
    att, _ = setup(gpu_device, precision, stable)
    xd = clips().to(gpu_device)
    box = att.neuron_gradient(xd, 4, (slice(7, 9), slice(5, 7)))
    units = sum(att.neuron_gradient(xd, 4, (t, h)).double() for t in (7, 8) for h in (5, 6))
    close(box, units.float().cpu(), precision, "2 x 2 box vs the sum of its units")


# ---------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_neuron_gradient(gpu_device, stable, precision):
    att, model = setup(gpu_device, precision, stable)
    x = clips()
    nl = att.eg.emb.nl
    for l in (0, 4, nl):
        for sel in SELECTORS:
            g = att.neuron_gradient(x.to(gpu_device), l, sel)
            close(g, ref_of(("grad", stable, l, str(sel)), lambda: NR.neuron_gradient(x, l, sel, model)), precision,
                  f"NeuronGradient l={l} {sel}")


def test_neuron_gradient_full_depth_pre_ln(gpu_device):
    """``hidden_states[nl]`` of a full-depth pre-LN model is the final LayerNorm's output: the seed passes through its backward."""
    att, model = setup(gpu_device, "f32", True, "full")
    x = clips()
    for sel in ((7, 5), BAND):
        close(att.neuron_gradient(x.to(gpu_device), 10, sel), NR.neuron_gradient(x, 10, sel, model), "f32", f"full depth, l=nl {sel}")


BASELINES = {"None": lambda dev: (None, torch.zeros(1, L)), "[1,L]": lambda dev: (noise_baseline()[:1].to(dev), noise_baseline()[:1]),
             "[B,L]": lambda dev: (noise_baseline().to(dev), noise_baseline()), "number": lambda dev: (NUMBER, torch.full((1, L), NUMBER))}


CONSTANT = ("None", "number")                                              # baselines that are constant clips


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("bname", list(BASELINES))
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_neuron_ig_rules_and_baselines(gpu_device, stable, bname, precision):
    att, model = setup(gpu_device, precision, stable)
    x = clips()
    xd = x.to(gpu_device)
    base_arg, base_t = BASELINES[bname](gpu_device)
    for method in AT.METHODS:
        if bname in CONSTANT and method in ("riemann_left", "riemann_trapezoid"):
            # alpha = 0 is the baseline itself, a constant clip: the classifier's per-clip normalisation has no scale there
            # (std = 0: the restatement's gradient at that point is 1e9 - 1e10, its own 1 / 1e-7 amplified rounding noise, against
            # 0.3 - 30 elsewhere), and the engine reports it, as ``integrated_gradients`` documents and
            # tests/test_gpu_attribution_baselines.py expects of the input-space path.  The next call must run clean.
            with pytest.raises(FloatingPointError):
                att.neuron_integrated_gradients(xd, 4, BAND, baselines=base_arg, n_steps=4, method=method)
            continue
        attr = att.neuron_integrated_gradients(xd, 4, BAND, baselines=base_arg, n_steps=4, method=method)
        ref, _ = ref_of(("nig", stable, bname, method), lambda: NR.neuron_integrated_gradients(x, base_t, 4, BAND, model, 4, method))
        close(attr, ref, precision, f"NeuronIG l=4 {bname} {method}")
    if bname == "[B,L]":
        g = att.neuron_integrated_gradients(xd, 4, (7, 5), baselines=base_arg, n_steps=4, method="riemann_middle", multiply_by_inputs=False)
        ref, _ = ref_of(("nig-nomul", stable), lambda: NR.neuron_integrated_gradients(x, base_t, 4, (7, 5), model, 4, "riemann_middle", False))
        close(g, ref, precision, "NeuronIG multiply_by_inputs=False")


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_neuron_gradient_shap(gpu_device, stable, precision):
    att, model = setup(gpu_device, precision, stable)
    x = clips()
    base = torch.cat([noise_baseline(2, 4), torch.zeros(1, L)])             # N_b = 3
    S, sigma, seed = 3, 0.05, 1003
    idx, alpha = AT.shap_draws(seed, B, S, 3)
    noise = AT.philox_normal(seed, 0, B * S, L, gpu_device).cpu()
    for mul in (True, False):
        attr = att.neuron_gradient_shap(x.to(gpu_device), 4, BAND, base.to(gpu_device), n_samples=S, stdevs=sigma, seed=seed,
                                        multiply_by_inputs=mul)
        ref = ref_of(("shap", stable, mul), lambda: NR.neuron_gradient_shap(x, base, idx, alpha, noise, sigma, S, 4, BAND, model, mul))
        close(attr, ref, precision, f"NeuronGradientShap multiply_by_inputs={mul}")


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_neuron_conductance(gpu_device, stable, precision):
    att, model = setup(gpu_device, precision, stable)
    x = clips()
    nb = noise_baseline()
    for method in ("gausslegendre", "riemann_trapezoid"):
        c = att.neuron_conductance(x.to(gpu_device), 4, (7, 5), baselines=nb.to(gpu_device), n_steps=4, method=method)
        close(c, ref_of(("cond", stable, method), lambda: NR.neuron_conductance(x, nb, 4, (7, 5), model, 4, method)), precision,
              f"NeuronConductance {method}")
    with pytest.raises(ValueError):
        att.neuron_conductance(x.to(gpu_device), 4, BAND)


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_neuron_feature_ablation(gpu_device, stable, precision):
    att, model = setup(gpu_device, precision, stable)
    x = clips()
    nb = noise_baseline()
    mask = (torch.arange(L) // 400)[None]                                   # 40 segments
    attr = att.neuron_feature_ablation(x.to(gpu_device), 4, BAND, baselines=nb.to(gpu_device), feature_mask=mask.to(gpu_device))
    ref = ref_of(("abl", stable), lambda: NR.neuron_feature_ablation(x, nb, mask, 4, BAND, model))
    close(attr, ref, precision, "NeuronFeatureAblation, 40 segments")


# ---------------------------------------------------------------------------------------------------- completeness
@pytest.mark.parametrize("sel", [(7, 5), BAND], ids=["unit", "band"])
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_neuron_ig_completeness(gpu_device, stable, sel):
    """50 Gauss-Legendre steps, noise baseline: ``sum attr - (s_n(x) - s_n(b))`` with ``s_n`` from the engine's own
    ``layer_activation`` and advh_neuron_values, against the restatement's delta -- its quadrature error, up to 1.5e-2 for the
    pre-LN band (tests/test_neuron_attr_cpu.py) -- within DELTA_TOL."""
    att, model = setup(gpu_device, "f32", stable)
    x, nb = clips(), noise_baseline()
    attr = att.neuron_integrated_gradients(x.to(gpu_device), 4, sel, baselines=nb.to(gpu_device), n_steps=50)
    box = AT.check_neuron_selector(sel, T, H)
    sx = att.eg.neuron_values(att.layer_activation(x.to(gpu_device), 4), box).double().cpu()
    sb = att.eg.neuron_values(att.layer_activation(nb.to(gpu_device), 4), box).double().cpu()
    delta = attr.double().sum(1).cpu() - (sx - sb)
    ref, ref_delta = NR.neuron_integrated_gradients(x, nb, 4, sel, model, 50)
    ref_ds = ref.double().sum(1) - ref_delta
    rel, ab = DELTA_TOL["f32"]
    print(f"NeuronIG 50 GL steps l=4 {sel} stable={stable}: delta {delta.tolist()}, restatement {ref_delta.tolist()}, "
          f"s_n(x) - s_n(b) {(sx - sb).tolist()} vs {ref_ds.tolist()}")
    assert ((delta - ref_delta).abs() <= rel * ref_ds.abs() + ab).all(), (delta, ref_delta)
    assert ((sx - sb - ref_ds).abs() <= rel * ref_ds.abs() + ab).all(), (sx - sb, ref_ds)


# ---------------------------------------------------------------------------------------------------- chunking and determinism
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_chunking_and_determinism(gpu_device, stable):
    """One chunk, one step (or B rows) per chunk, a short last chunk and a second call give the same bits."""
    att, _ = setup(gpu_device, "f32", stable)
    xd, nb = clips().to(gpu_device), noise_baseline().to(gpu_device)
    dist = noise_baseline(3, 5).to(gpu_device)
    mask = (torch.arange(L, device=gpu_device) // 400)[None]
    cases = (("NeuronIG", lambda ibs: att.neuron_integrated_gradients(xd, 4, BAND, baselines=nb, n_steps=5, internal_batch_size=ibs)),
             ("NeuronGradientShap", lambda ibs: att.neuron_gradient_shap(xd, 4, BAND, dist, n_samples=5, stdevs=0.05, seed=11,
                                                                         internal_batch_size=ibs)),
             ("NeuronConductance", lambda ibs: att.neuron_conductance(xd, 4, (7, 5), baselines=nb, n_steps=5, internal_batch_size=ibs)),
             ("NeuronFeatureAblation", lambda ibs: att.neuron_feature_ablation(xd, 4, BAND, baselines=nb, feature_mask=mask,
                                                                               internal_batch_size=ibs)))
    for name, fn in cases:
        one = fn(64)
        assert torch.equal(one, fn(64)), name
        for ibs in (B, 2 * B, 5 * B):
            assert torch.equal(one, fn(ibs)), (name, ibs)


# ---------------------------------------------------------------------------------------------------- truncation
@pytest.mark.parametrize("stable", FLAVOURS, ids=IDS)
def test_truncation(gpu_device, stable):
    """Nothing at or above the layer runs: sentinels in the buffers only layers >= 4, the pooling and the logreg write
    survive ``forward(to_layer=4)`` and the seeded backward."""
    att, _ = setup(gpu_device, "f32", stable)
    eg = att.eg
    xd = clips().to(gpu_device)
    eg.forward(xd)
    full = att.neuron_gradient(xd, 4, BAND) * 1.0                           # its own truncated forward
    eg.forward(xd)
    after_full = att._checked(eg.backward(att.neuron_loss_scale, from_layer=4, neuron=AT.check_neuron_selector(BAND, T, H)))
    w = eg._workspace(B, L)
    upper = [w["qkv"][4], w["x"][5], w["g1"][4], w["qkv"][8], w["x"][9], w["f"]["logit"], w["f"]["prob"]]
    for t in upper:
        t.fill_(7.0)
    h4 = eg.forward(xd, to_layer=4)
    assert h4.shape == (B, T, H) and torch.equal(h4, eg.hidden(4)) and eg.hidden(0).shape == (B, T, H)
    g = att._checked(eg.backward(att.neuron_loss_scale, from_layer=4, neuron=AT.check_neuron_selector(BAND, T, H)))
    for t in upper:
        assert bool((t == 7.0).all())
    with pytest.raises(RuntimeError):
        eg.backward(att.loss_scale)
    with pytest.raises(RuntimeError):
        eg.backward(att.loss_scale, to_layer=6)
    with pytest.raises(ValueError):
        eg.hidden(5)
    with pytest.raises(ValueError):
        eg.backward(att.neuron_loss_scale, from_layer=5, neuron=(0, 1, 1, 0, 1, 1))
    assert torch.equal(g, full) and torch.equal(g, after_full)
    for t in upper:
        t.zero_()
    eg.forward(xd)                                                        # a full pass restores the upper chain
    assert eg.hidden(9).shape == (B, T, H) and bool(torch.isfinite(eg.backward(att.loss_scale)).all())


# ---------------------------------------------------------------------------------------------------- other cases
def test_base_1s(gpu_device):
    """wav2vec2-base (H = 768: the production tile shapes), one clip x 1 s, layer 6: the neuron gradient vs autograd."""
    att, model = setup(gpu_device, "f32", cfg_name="base")
    x = syn.make_clips(1, 16000)
    close(att.neuron_gradient(x.to(gpu_device), 6, BAND), NR.neuron_gradient(x, 6, BAND, model), "f32", "base 1 s, l=6")


def test_overflow_is_reported(gpu_device):
    """A seed scale far outside the planes' range: SplitRangeError, and the next call is clean."""
    att, model = setup(gpu_device, "f32", False)
    hot = HipAttribution(att.emb, neuron_loss_scale=2.0 ** 40)
    xd = clips().to(gpu_device)
    with pytest.raises(FloatingPointError):
        hot.neuron_gradient(xd, 4, BAND)
    torch.cuda.synchronize()                                              # the flag is sticky: kernels still in flight may raise it again
    _lib.lib().advh_split_overflow(1)
    close(att.neuron_gradient(xd, 4, BAND), ref_of(("grad", False, 4, str(BAND)), lambda: NR.neuron_gradient(clips(), 4, BAND, model)),
          "f32", "NeuronGradient after a range error")


@pytest.fixture
def tiny_runtime():
    os.environ["ADDVISOR_EMBEDDER"] = "tiny"
    runtime.reset()
    yield
    os.environ.pop("ADDVISOR_EMBEDDER", None)
    runtime.reset()


def test_captum_front_end(gpu_device, tiny_runtime):
    import captum_saliency as cs
    from captum.attr import NeuronConductance, NeuronFeatureAblation, NeuronGradient, NeuronGradientShap, NeuronIntegratedGradients
    model = cs.Wav2vec2LogReg(cs.audioprocessor, cs.TorchLogReg()).to(gpu_device)
    eng = model.hip_attribution()
    assert model.num_layers() == eng.eg.emb.nl == 9 and model.frame_shape(L) == (T, H)
    x = clips().to(gpu_device)
    nb = noise_baseline().to(gpu_device)
    mask = (torch.arange(L, device=gpu_device) // 400)[None]
    g = NeuronGradient(model, 4).attribute(x, (7, 5))
    assert g.shape == (B, L) and torch.equal(g, eng.neuron_gradient(x, 4, (7, 5)))
    assert torch.equal(NeuronGradient(model, 9).attribute(x, (-1, slice(None))), eng.neuron_gradient(x, 9, (48, slice(0, 64))))
    assert torch.equal(NeuronIntegratedGradients(model, 4).attribute(x, BAND, n_steps=4), eng.neuron_integrated_gradients(x, 4, BAND, n_steps=4))
    assert torch.equal(NeuronIntegratedGradients(model, 4, multiply_by_inputs=False).attribute(x, BAND, baselines=nb, n_steps=4,
                                                                                               method="riemann_right", internal_batch_size=4),
                       eng.neuron_integrated_gradients(x, 4, BAND, baselines=nb, n_steps=4, method="riemann_right", multiply_by_inputs=False))
    torch.manual_seed(17)
    s1 = NeuronGradientShap(model, 4).attribute(x, BAND, nb, n_samples=3, stdevs=0.05)
    torch.manual_seed(17)
    assert torch.equal(s1, eng.neuron_gradient_shap(x, 4, BAND, nb, n_samples=3, stdevs=0.05))
    assert torch.equal(NeuronConductance(model, 4).attribute(x, (7, 5), baselines=nb, n_steps=4),
                       eng.neuron_conductance(x, 4, (7, 5), baselines=nb, n_steps=4, method="riemann_trapezoid"))
    assert torch.equal(NeuronFeatureAblation(model, 4).attribute(x, BAND, baselines=nb, feature_mask=mask, perturbations_per_eval=8),
                       eng.neuron_feature_ablation(x, 4, BAND, baselines=nb, feature_mask=mask))
    with pytest.raises(ValueError):
        NeuronGradient(model, 4).attribute(x, (49, 0))
    with pytest.raises(ValueError):
        NeuronGradient(model, 10).attribute(x, (7, 5))
    out = cs.explain_waves(model, x, method="neuron_integrated_gradients", n_steps=4, layer=4, neuron=BAND)
    assert len(out) == 3
    for p in out:
        assert p.shape == (B, 1) and bool(((p >= 0) & (p <= 1)).all())
