"""GPU: every layer of the inference U-Net (``HipUNet``, the forward of ``explain()``) against its own fp64 definition on the operands it
actually read, under the elementwise bound of tests/unet_layer_ref.py (pinned on the CPU by tests/test_unet_layer_ref_cpu.py).

After one forward the workspace keeps every launch (``steps``: plan, source map names, destination map name) and every map, so
each layer's inputs are read back as the kernel left them and the layer is recomputed from the state dict -- BatchNorm folded in fp64,
``F.conv2d`` / ``F.conv_transpose2d`` in fp64.  That covers the layer's planning, the fold, ``compose_upconv_weights``, the weight packing
and the kernel dispatch together, names the launch that is wrong, and leaves two errors no sigmoid to cancel through.  The stem, the
spectrogram pack and the mask head (also in its fused form, inside ``d1.block.3``'s epilogue) are checked the same way, and the halo of
every map is asserted to be the zero it was allocated as after two forwards.

Worst |err| / bound per destination map over the three shapes, measured on an MI355X (the line each layer prints; (line_tile, fuse_up)):

    map      f16 TT  f16 FT  f16 TF  f16 FF  f32 TT  f32 FT  f32 TF  f32 FF
    x1a       0.984   0.984   0.984   0.984   0.129   0.129   0.129   0.129     (stem, direct kernel)
    pack_x    0.975   0.975   0.975   0.975   0.222   0.222   0.222   0.222     (direct kernel)
    x1        0.277   0.277   0.277   0.277   0.005   0.005   0.005   0.005
    x2a       0.237   0.237   0.237   0.237   0.004   0.004   0.004   0.004
    x2        0.182   0.182   0.182   0.182   0.002   0.002   0.002   0.002
    x3a       0.189   0.189   0.189   0.189   0.003   0.003   0.003   0.003
    x3        0.175   0.175   0.175   0.175   0.002   0.002   0.002   0.002
    x4a       0.135   0.135   0.135   0.135   0.001   0.001   0.001   0.001
    x4        0.108   0.108   0.108   0.108   0.001   0.001   0.001   0.001
    b1        0.195   0.195   0.195   0.195   0.001   0.001   0.001   0.001
    b2        0.143   0.143   0.143   0.143   0.000   0.000   0.000   0.000
    u4           --      --   0.248   0.248      --      --   0.004   0.004
    y4a       0.028   0.028   0.085   0.085   0.000   0.000   0.000   0.000
    y4        0.116   0.116   0.125   0.125   0.001   0.001   0.001   0.001
    u3           --      --   0.313   0.313      --      --   0.007   0.007
    y3a       0.034   0.034   0.170   0.170   0.000   0.000   0.001   0.001
    y3        0.163   0.163   0.159   0.159   0.002   0.002   0.002   0.002
    u2           --      --   0.343   0.343      --      --   0.016   0.016
    y2a       0.053   0.053   0.162   0.162   0.000   0.000   0.002   0.002
    y2        0.252   0.252   0.257   0.257   0.004   0.004   0.003   0.003
    u1           --      --   0.459   0.459      --      --   0.035   0.035
    y1a       0.067   0.067   0.299   0.299   0.001   0.001   0.006   0.006
    y1        0.356   0.356   0.329   0.329      --   0.007      --   0.007
    logits    0.060   0.060   0.048   0.048   0.001   0.063   0.001   0.048     (direct kernel; f32 T*: in d1.block.3's epilogue)
    mask      0.052   0.052   0.055   0.055   0.001   0.059   0.001   0.055

The two ratios near 1 are fp16 stores of values that no operand rounding precedes (fp32 weights on the fp32 magnitude): there the bound is
little more than the half ulp of the store, and round-to-nearest reaches it.  In fp32-class mode the bound is led by its worst-case
accumulation term ``K 2^-24 A``, which fp32 sums of K terms stay far below; the line-tile and GEMM columns agree because they share the
rounding of the weights, the leading error.
"""
import numpy as np
import pytest
import torch

import unet_layer_ref as R
from addvisor_hip import synthetic as syn
from addvisor_hip.unet import HipUNet

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SHAPES = [(2, 32, 8), (3, 48, 20), (1, 64, 36)]
VARIANTS = [(True, True), (False, True), (True, False), (False, False)]    # (line_tile, fuse_up)
TAPS3X3 = ("x1", "x2", "y2", "y1")                                          # the 3 x 3 same-geometry 32- / 64-channel layers


def weights():
    """The synthetic state dict with the transposed convolutions' biases x8, so that the indicator path carries weight."""
    sd = {k: v.clone() for k, v in syn.unet_weights().items()}
    for n in ("up1", "up2", "up3", "up4"):
        sd[n + ".bias"] = sd[n + ".bias"] * 8.0
    return sd


def spectrogram(B, H, W, seed=0):
    r = np.random.Generator(np.random.PCG64(41 + B + H + W + seed))
    return torch.from_numpy(r.uniform(0, 3, size=(B, 1, H, W)).astype(np.float32))


def expected_plan(dst, precision, line_tile, fuse_up):
    tail = "Split" if precision == "f32" else ""
    if line_tile and dst in TAPS3X3:
        return f"Taps2d{tail}Plan"
    if line_tile and fuse_up and dst == "x2a":
        return f"ConvS21{tail}TilePlan"
    if line_tile and fuse_up and dst == "y1a":
        return f"Upconv{tail}TilePlan"
    return "PlanGroup" if fuse_up and dst in R.STAGE_OF else "GemmPlan"


def upconv_K(wt, wc, stride):
    """Reduction length of the fused stage: 2 x (2 or 3) coarse taps and 9 fine taps, each over its real channels and one 8-channel
    chunk for the indicator / padding."""
    Cs = wc.shape[1] - wt.shape[1]
    return 2 * (2 if stride[1] == 2 else 3) * (wt.shape[0] + 8) + 9 * (Cs + 8)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("line_tile,fuse_up", VARIANTS)
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_every_layer_forward_is_exact_on_its_own_operands(gpu_device, precision, line_tile, fuse_up, shape):
    B, H, W = shape
    mode = "split" if precision == "f32" else "f16"
    sd = weights()
    d = lambda k: sd[k].double()
    x = spectrogram(B, H, W)
    net = HipUNet(sd, gpu_device, line_tile=line_tile, fuse_up=fuse_up, precision=precision)
    mask, logits = net.forward(x[:, 0].to(gpu_device), H=H, W=W, want_logits=True)
    torch.cuda.synchronize()
    ws = net._workspace(B, H, W)
    m, x64 = ws["maps"], x.double()
    worst = {}

    def check(dst, got, ref, bnd, plan=None):
        assert ref.abs().max() > 0.1, f"{dst}: degenerate"
        r = float(((got - ref).abs() / bnd).max())
        worst[dst] = r
        print(f"UNETLAYER {precision} {dst} {type(plan).__name__ if plan is not None else 'direct'} worst |err|/bound {r:.3f}")
        assert r <= 1.0, (dst, r)

    # the stem: e1.block.0 on the fp32 magnitude (direct kernel, fp32 weights)
    cn, bn, st, pd, dl = R.CONVS["x1a"]
    w, b, ab = R.fold_bn(sd, cn, bn)
    ref, A = R.conv_layer([x64], w, b, st, pd, dl), R.conv_layer([x64.abs()], w.abs(), ab, st, pd, dl)
    check("x1a", R.read_map(m["x1a"]), ref, R.bound(ref, A, R.K_STEM, mode, operands="exact"))
    # the pack: (x, 1, 0 x 6) into xin, or behind up1's 32 channels in u1
    xcat, c0 = (m["xin"], 0) if fuse_up else (m["u1"], 32)
    chunk = R.read_map(xcat, slice(c0, c0 + 8))
    check("pack_x", chunk[:, :1], x64, R.bound(x64, x64.abs(), 0, mode, operands="exact"))
    assert (chunk[:, 1] == 1).all() and (chunk[:, 2:] == 0).all()

    for plan, srcs, dst in ws["steps"]:
        if dst not in R.UPS:
            assert type(plan).__name__ == expected_plan(dst, precision, line_tile, fuse_up), (dst, type(plan).__name__)
        if m[dst].t is None:                                                # y1 under the fused head: checked through the logits below
            assert dst == "y1" and net._fused_head
            continue
        if dst in R.UPS:                                                    # a ConvTranspose2d of the unfused network
            up, stride = R.UPS[dst]
            wt, bt = d(up + ".weight"), d(up + ".bias")
            src = R.read_map(m[srcs[0]], wt.shape[0])
            ref, A = R.convT_layer(src, wt, bt, stride), R.convT_layer(src.abs(), wt.abs(), bt.abs(), stride)
            check(dst, R.read_map(m[dst], wt.shape[1]), ref, R.bound(ref, A, wt.shape[0], mode), plan)
            continue
        cn, bn, st, pd, dl = R.CONVS[dst]
        w, b, ab = R.fold_bn(sd, cn, bn)
        if fuse_up and dst in R.STAGE_OF:                                   # ConvTranspose2d + the block's first convolution, one launch
            up, stride = R.STAGE_OF[dst]
            wt, bt = d(up + ".weight"), d(up + ".bias")
            coarse, skip = R.read_map(m[srcs[0]], wt.shape[0]), R.read_map(m[srcs[1]], w.shape[1] - wt.shape[1])
            ref = R.upconv_layer(coarse, skip, wt, bt, w, b, stride)
            A = R.upconv_layer(coarse.abs(), skip.abs(), wt.abs(), bt.abs(), w.abs(), ab, stride)
            check(dst, R.read_map(m[dst], w.shape[0]), ref, R.bound(ref, A, upconv_K(wt, w, stride), mode), plan)
            continue
        src = torch.cat([R.read_map(m[s]) for s in srcs], 1)[:, :w.shape[1]]  # unfused d1.block.0: 33 real channels of u1's 40
        ref, A = R.conv_layer([src], w, b, st, pd, dl), R.conv_layer([src.abs()], w.abs(), ab, st, pd, dl)
        check(dst, R.read_map(m[dst], w.shape[0]), ref, R.bound(ref, A, w[0].numel(), mode), plan)
    assert len(worst) == 2 + len(ws["steps"]) - net._fused_head

    # the head: logits (fp32) and mask
    hw, hb = d("mask_head.0.weight").reshape(32), d("mask_head.0.bias")
    head_A = lambda y: R.head(y, hw.abs(), hb.abs())
    if net._fused_head:                                                     # d1.block.3 + head in one launch: the two bounds chained
        cn, bn, st, pd, dl = R.CONVS["y1"]
        w, b, ab = R.fold_bn(sd, cn, bn)
        y1a = R.read_map(m["y1a"])
        y1 = R.conv_layer([y1a], w, b)
        e1 = R.bound(y1, R.conv_layer([y1a.abs()], w.abs(), ab), w[0].numel(), mode)
        ref = R.head(y1, hw, hb)
        bnd = R.head(e1, hw.abs(), hb * 0) + R.bound(ref, head_A(y1.abs() + e1), R.K_HEAD, mode, out="f32", operands="exact")
    else:
        y1 = R.read_map(m["y1"])
        ref = R.head(y1, hw, hb)
        bnd = R.bound(ref, head_A(y1.abs()), R.K_HEAD, mode, out="f32", operands="exact")
    check("logits", logits.cpu().double()[:, None], ref, bnd, ws["steps"][-1][0] if net._fused_head else None)
    check("mask", mask.cpu().double()[:, None], torch.sigmoid(ref), R.sigmoid_bound(bnd))
    print(f"UNETLAYER {precision} line_tile={line_tile} fuse_up={fuse_up} {shape}: worst {max(worst, key=worst.get)} {max(worst.values()):.3f}")


@pytest.mark.parametrize("line_tile,fuse_up", [(True, True), (False, False)])
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_halos_stay_zero(gpu_device, precision, line_tile, fuse_up):
    """``interior_only`` planning rests on it: every map's halo is the zero it was allocated as, forward after forward, in both planes of
    a split map; the in-image indicator channels hold 1 (hi 1, lo 0) at every interior pixel."""
    B, H, W = 2, 48, 20
    net = HipUNet(weights(), gpu_device, line_tile=line_tile, fuse_up=fuse_up, precision=precision)
    for seed in (0, 1):
        net.forward(spectrogram(B, H, W, seed)[:, 0].to(gpu_device), H=H, W=W)
    torch.cuda.synchronize()
    m = net._workspace(B, H, W)["maps"]
    stored = {k: f for k, f in m.items() if f.t is not None}
    assert set(m) - set(stored) == ({"y1"} if net._fused_head else set())
    for name, f in stored.items():
        halo = R.read_halo(f)
        assert f.PH + f.PW == 0 or halo.numel() > 0
        assert (halo == 0).all(), f"{name}: {int((halo != 0).sum())} halo element(s) written"
        assert R.read_map(f).abs().max() > 0.1, name                        # and the interior was
    indicators = {"b2": 512, "y4": 256, "y3": 128, "xin": 1} if fuse_up else {"u1": 33}
    for name, ch in indicators.items():
        t = m[name].t if m[name].split else m[name].t[None]
        inner = t[:, :, m[name].PH:m[name].PH + m[name].H, m[name].PW:m[name].PW + m[name].W, ch]
        assert (inner[0] == 1).all() and (inner[1:] == 0).all(), name
