"""Pins tests/unet_layer_ref.py on the CPU: the fp64 layer references chained through the whole network are the oracle's U-Net; a CPU
model of every kernel's arithmetic stays under ``bound`` at every element (the bound is sound); and the same model with one small
mistake in it violates the bound (the bound has teeth).

Share of the elements at which each mutation violates the fp16 bound (conv_layer: the e2.block.0 shape at (B, Ho, W) = (3, 5, 15) /
(2, 33, 16); upconv_layer: the up1 + d1.block.0 shape at (B, Hc, W) = (3, 8, 15) / (1, 16, 33)):

    mutation                                   conv_layer      upconv_layer
    output channels 3 and 4 swapped (of them)  97.8 / 98.9 %   94.2 / 92.2 %
    taps kw = 0 and kw = 1 swapped             98.5 / 98.4 %   92.6 / 91.4 %
    one weight zeroed (of its channel)         45.3 / 52.1 %   19.3 / 17.0 %
    input shifted by one column                98.9 / 98.8 %   93.9 / 93.0 %
    ConvTranspose2d bias dropped               --              86.8 / 87.5 %

The zeroed weight is the one of median magnitude among its output channel's (480 of e2.block.0, 297 of d1.block.0).
The unmutated models' worst |err| / bound is 0.05 - 0.46 in fp16 for the matrix-core layers and at most 0.13 in split mode, where the
worst-case accumulation term K 2^-24 A leads the bound.  The direct kernels (stem, spectrogram pack, head: fp32 weights, no operand
rounding, ``bound(..., operands="exact")``) reach 0.99 / 0.98 / 0.09: an fp16 store with nothing but its half ulp allowed (printed per case)."""
import pytest
import torch
import torch.nn.functional as F

import unet_layer_ref as R
from addvisor_hip import synthetic as syn
from addvisor_hip.unet import _fold_bn
from oracle import unet_ref

torch.set_grad_enabled(False)


def ratio(got, ref, bnd):
    return float(((got - ref).abs() / bnd).max())


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("shape", [(2, 32, 8), (1, 48, 20)])
def test_chained_references_are_the_oracle_unet(shape):
    B, H, W = shape
    sd = {k: v.double() if v.is_floating_point() else v for k, v in syn.unet_weights().items()}
    x = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(H + W), dtype=torch.float64) * 3
    conv = lambda dst, srcs, w, b, ab, st, pd, dl: R.conv_layer(srcs, w, b, st, pd, dl)
    convT = lambda dst, src, wt, bt, stride: R.convT_layer(src, wt, bt, stride)
    stage = lambda dst, coarse, skip, wt, bt, wc, bc, abc, stride: R.upconv_layer(coarse, skip, wt, bt, wc, bc, stride)
    want_l, want_m = unet_ref.unet_forward(x, sd, return_logits=True), unet_ref.unet_forward(x, sd)
    for st in (None, stage):
        logits, mask = R.unet_chain(x, sd, conv, convT, st)
        assert want_l.abs().max() > 0.1
        assert (logits - want_l).abs().max() <= 1e-12 * want_l.abs().max()
        assert (mask - want_m).abs().max() <= 1e-12 * want_m.abs().max()


@pytest.mark.parametrize("stride,indicator,Cs", [((2, 1), "skip", 1), ((2, 1), "coarse", 8), ((2, 2), "coarse", 16)])
def test_the_fused_stage_model_without_rounding_is_upconv_layer(stride, indicator, Cs):
    """The model evaluates composed weights per parity class; in fp64 without any rounding it must be the layer-by-layer definition."""
    g = torch.Generator().manual_seed(3)
    Cb, Cu, N, Hc, Wc = 16, 8, 8, 5, 7
    coarse, skip = R._randn(g, 2, Cb, Hc, Wc), R._randn(g, 2, Cs, stride[0] * Hc, stride[1] * Wc)
    wt, bt, wc, bc = R._randn(g, Cb, Cu, *stride), R._randn(g, Cu), R._randn(g, N, Cu + Cs, 3, 3), R._randn(g, N)
    got = R.model_upconv(coarse, skip, wt, bt, wc, bc, stride, indicator=indicator, exact=True)
    want = R.upconv_layer(coarse, skip, wt, bt, wc, bc, stride)
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()


# ------------------------------------------------------------------------------------------------ the bound is sound
@pytest.mark.parametrize("shape", [(2, 32, 8), (3, 48, 20), (1, 64, 36)])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("mode", ["f16", "split"])
def test_model_of_every_network_layer_stays_under_the_bound(mode, fused, shape):
    """The network of tests/test_gpu_unet_layers.py with every kernel replaced by its CPU model, each layer checked on the operands
    the model handed it."""
    B, H, W = shape
    sd = {k: v.clone() for k, v in syn.unet_weights().items()}
    for n in ("up1", "up2", "up3", "up4"):
        sd[n + ".bias"] = sd[n + ".bias"] * 8.0
    x = R.as_stored(torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(H + W), dtype=torch.float64) * 3, mode)
    worst, maps = {}, {}

    def conv(dst, srcs, w, b, ab, st, pd, dl):
        ref, A = R.conv_layer(srcs, w, b, st, pd, dl), R.conv_layer([s.abs() for s in srcs], w.abs(), ab, st, pd, dl)
        if dst == "x1a":                                                   # the stem is a direct kernel: fp32 weights (folded in fp32 in fp16 mode), fp32 sums
            w32, b32 = (w.float(), b.float()) if mode == "split" else _fold_bn(sd, *R.CONVS[dst][:2], torch.float32)
            got = R.store(F.leaky_relu(F.conv2d(srcs[0].float(), w32, b32, st, pd, dl), R.SLOPE), mode)
            worst[dst] = ratio(got, ref, R.bound(ref, A, R.K_STEM, mode, operands="exact"))
            return got
        got = R.model_conv(srcs, w, b, st, pd, dl, mode=mode)
        worst[dst] = ratio(got, ref, R.bound(ref, A, w[0].numel(), mode))
        if dst == "y1":
            maps[dst] = got
        return got

    def convT(dst, src, wt, bt, stride):
        got = R.model_convT(src, wt, bt, stride, mode=mode)
        ref, A = R.convT_layer(src, wt, bt, stride), R.convT_layer(src.abs(), wt.abs(), bt.abs(), stride)
        worst[dst] = ratio(got, ref, R.bound(ref, A, wt.shape[0], mode))
        return got

    def stage(dst, coarse, skip, wt, bt, wc, bc, abc, stride):
        ind = "skip" if skip.shape[1] == 1 else "coarse"
        got = R.model_upconv(coarse, skip, wt, bt, wc, bc, stride, mode=mode, indicator=ind)
        ref = R.upconv_layer(coarse, skip, wt, bt, wc, bc, stride)
        A = R.upconv_layer(coarse.abs(), skip.abs(), wt.abs(), bt.abs(), wc.abs(), abc, stride)
        K = 2 * (2 if stride[1] == 2 else 3) * (wt.shape[0] + 8) + 9 * (skip.shape[1] + 8)
        worst[dst] = ratio(got, ref, R.bound(ref, A, K, mode))
        return got

    ref, ref_mask = R.unet_chain(x, sd, conv, convT, stage if fused else None)       # the fp64 head on the model's y1
    # the head (direct kernel: fp32 weights, fp32 sums, fp32 logits) and the spectrogram pack (a store)
    hw, hb, y1 = sd["mask_head.0.weight"].double().reshape(32), sd["mask_head.0.bias"].double(), maps["y1"]
    logits = F.conv2d(y1.float(), hw.float().reshape(1, 32, 1, 1), hb.float())
    bnd = R.bound(ref, R.head(y1.abs(), hw.abs(), hb.abs()), R.K_HEAD, mode, out="f32", operands="exact")
    worst["logits"] = ratio(logits.double(), ref, bnd)
    worst["mask"] = ratio(torch.sigmoid(logits).double(), ref_mask, R.sigmoid_bound(bnd))
    x32 = (x + torch.rand(x.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 1e-3).float().double()
    worst["pack_x"] = ratio(R.as_stored(x32, mode), x32, R.bound(x32, x32.abs(), 0, mode, operands="exact"))
    print(f"UNETMODEL {mode} fused={fused} {shape}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert len(worst) == (18 if fused else 22) + 3 and max(worst.values()) <= 1.0, worst


def _tile_cases():
    out = [("s21",) + c[:3] for c in R.S21_CASES] + [("upconv",) + c[:3] for c in R.UPCONV_CASES]
    return out + [("taps2d",) + c[:4] for c in R.TAPS2D_CASES]


@pytest.mark.parametrize("case", _tile_cases(), ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("mode", ["f16", "split"])
def test_model_of_every_line_tile_case_stays_under_the_bound(mode, case):
    """Every case of tests/test_gpu_unet_f16_tiles.py, in both formats (the split tiles themselves are tested bit for bit against the
    GEMM in their own files)."""
    kind, dims = case[0], case[1:]
    got, ref, bnd = tile_case(kind, dims, mode)
    r = ratio(got, ref, bnd)
    print(f"TILEMODEL {mode} {kind} {dims}: worst |err|/bound {r:.3f}")
    assert r <= 1.0


def tile_case(kind, dims, mode, mutate=None):
    """(model output, fp64 reference, bound) of one line-tile case; ``mutate(args: dict)`` edits the model's operands only."""
    if kind == "upconv":
        xc, xs, wt, bt, wc, bc = R.upconv_data(*dims, mode=mode)
        ref = R.upconv_layer(xc, xs, wt, bt, wc, bc, (2, 1))
        A = R.upconv_layer(xc.abs(), xs.abs(), wt.abs(), bt.abs(), wc.abs(), bc.abs(), (2, 1))
        a = dict(x=xc, xs=xs, wt=wt.clone(), bt=bt.clone(), w=wc.clone(), b=bc.clone())
        if mutate:
            mutate(a)
        got = R.model_upconv(a["x"], a["xs"], a["wt"], a["bt"], a["w"], a["b"], (2, 1), mode=mode)
        return got, ref, R.bound(ref, A, R.K_UPCONV, mode)
    x, w, b = R.s21_data(*dims, mode=mode) if kind == "s21" else R.taps2d_data(*dims, mode=mode)
    geom = R.S21_GEOM if kind == "s21" else {}
    ref, A = R.conv_layer([x], w, b, **geom), R.conv_layer([x.abs()], w.abs(), b.abs(), **geom)
    a = dict(x=x, w=w.clone(), b=b.clone())
    if mutate:
        mutate(a)
    return R.model_conv([a["x"]], a["w"], a["b"], mode=mode, **geom), ref, R.bound(ref, A, w[0].numel(), mode)


# ------------------------------------------------------------------------------------------------ the bound has teeth
def swap_channels(a):
    a["w"][[3, 4]], a["b"][[3, 4]] = a["w"][[4, 3]], a["b"][[4, 3]]


def swap_taps(a):
    a["w"][..., [0, 1]] = a["w"][..., [1, 0]]


def zero_one_weight(a):
    """The weight of median magnitude among output channel 5's: a typical one, neither the easiest nor a near-zero one."""
    w5 = a["w"][5].reshape(-1)
    w5[w5.abs().argsort()[w5.numel() // 2]] = 0.0


def shift_input(a):
    a["x"] = torch.roll(a["x"], 1, dims=3)


def drop_bt(a):
    a["bt"] = a["bt"] * 0


MUTATIONS = {"swap": swap_channels, "taps": swap_taps, "zero": zero_one_weight, "shift": shift_input, "bt": drop_bt}
TEETH = [("s21", (3, 5, 15)), ("s21", (2, 33, 16)), ("upconv", (3, 8, 15)), ("upconv", (1, 16, 33))]


@pytest.mark.parametrize("name,kind,dims", [(n, k, d) for n in MUTATIONS for k, d in TEETH if n != "bt" or k == "upconv"])
def test_a_mutated_model_violates_the_bound(name, kind, dims):
    got, ref, bnd = tile_case(kind, dims, "f16", mutate=MUTATIONS[name])
    bad = (got - ref).abs() > bnd
    touched = bad[:, 5] if name == "zero" else (bad[:, 3:5] if name == "swap" else bad)
    print(f"TEETH {kind} {dims} {name}: violates at {100 * touched.double().mean():.1f} % of the elements it touches, {int(bad.sum())} in all")
    assert bad.any()
    if name in ("zero", "swap"):                                           # nothing outside the mutated channels moves
        keep = torch.ones(bad.shape[1], dtype=torch.bool)
        keep[[5] if name == "zero" else [3, 4]] = False
        assert not bad[:, keep].any()
