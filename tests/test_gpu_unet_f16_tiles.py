"""GPU: the three fp16 LDS line tiles of the inference U-Net, each on its own operands against the fp64 layer definition of
tests/unet_layer_ref.py under that module's elementwise bound (pinned on the CPU by tests/test_unet_layer_ref_cpu.py):

  advh_conv53s21_tile_f16 (csrc/conv_s21_tile.hip, ``ConvS21TilePlan``)   e2.block.0, 8 x 16 tiles, at most 256 workgroups
  advh_upconv21_tile_f16  (csrc/upconv_tile.hip, ``UpconvTilePlan``)      up1 + d1.block.0, 16 x 16 tiles, at most 256 workgroups
  advh_conv_taps2d_f16    (csrc/conv_taps.hip, ``Taps2dPlan``)            3 x 3 same-geometry layers, 16 x 16 tiles, 512 / 256 workgroups

The first two are persistent double-buffered kernels: the cases with more tiles than workgroups make a workgroup walk a second and a
third tile (the patch buffer index flips and returns).  Every destination starts with NaN in its interior and 3.0 in its halo: the
kernels write every interior element and nothing else.  The implicit GEMM (``plan_conv2d`` / ``plan_upconv2d``) on the same maps is
held to the same bound; bit equality between tile and GEMM is not promised (other summation order).

Worst |err| / bound over each kernel's cases, measured on an MI355X (the line each case prints):

    kernel                    cases                                tile    implicit GEMM on the same maps
    advh_conv53s21_tile_f16   9 (416 and 520 tiles: 0.250, 0.244)  0.250   0.250
      act = ADVH_ACT_NONE     (2, 11, 21)                          0.210
    advh_upconv21_tile_f16    8 (520 and 416 tiles: 0.061, 0.060)  0.061   0.061
      bt = 0                  8                                    0.065
      act = ADVH_ACT_NONE     (2, 8, 21)                           0.055
    advh_conv_taps2d_f16 32   3 (546 tiles: 0.289)                 0.314   0.314
    advh_conv_taps2d_f16 64   3 (270 tiles: 0.230)                 0.230   0.230

Tile and GEMM agree to the third digit in every case: the error is the fp16 rounding of the weights, which both share, not the
order of summation.  The fused stage sits low because its ``A`` is the layer-by-layer one, an upper bound on ``sum |W_composed| |x|``;
tests/test_unet_layer_ref_cpu.py shows that a single zeroed weight still violates it.
"""
import ctypes as C

import pytest
import torch

import unet_layer_ref as R
from addvisor_hip import _lib, gemm as G

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENTINEL = 3.0


def src_map(dev, x, PH, PW, Cn=None):
    """A zero-haloed fp16 map holding ``x`` (NCHW, fp16-representable) in its first channels."""
    B, Cx, H, W = x.shape
    f = G.FMap(B, H, W, Cn or Cx, PH, PW).alloc(dev)
    f.interior()[..., :Cx] = R.to_nhwc(x).to(dev)
    return f


def dst_map(dev, B, H, W, Cn, PH, PW):
    """NaN in the interior, the sentinel in the halo."""
    f = G.FMap(B, H, W, Cn, PH, PW).alloc(dev)
    f.t.fill_(SENTINEL)
    f.interior()[:] = float("nan")
    return f


def check(what, f, ref, bnd):
    """``f``'s interior against ``ref`` under ``bnd`` at every element; its halo still the sentinel."""
    got = R.read_map(f)
    assert not torch.isnan(got).any(), f"{what}: an interior element was not written"
    r = float(((got - ref).abs() / bnd).max())
    print(f"UNETTILE f16 {what} worst |err|/bound {r:.3f}")
    assert r <= 1.0, (what, r)
    assert (R.read_halo(f) == SENTINEL).all(), f"{what}: the halo was written"
    return r


# ------------------------------------------------------------------------------------------------ advh_conv53s21_tile_f16
def s21_case(dev, B, Ho, W, pads):
    (phi, pwi), (pho, pwo) = pads
    x, w, b = R.s21_data(B, Ho, W)
    return src_map(dev, x, phi, pwi), (lambda: dst_map(dev, B, Ho, W, 64, pho, pwo)), x, w, b


@pytest.mark.parametrize("B,Ho,W,pads", R.S21_CASES)
def test_conv_s21_tile_f16(gpu_device, B, Ho, W, pads):
    _lib.init()
    src, mk, x, w, b = s21_case(gpu_device, B, Ho, W, pads)
    ref, A = R.conv_layer([x], w, b, **R.S21_GEOM), R.conv_layer([x.abs()], w.abs(), b.abs(), **R.S21_GEOM)
    bnd = R.bound(ref, A, R.K_S21, "f16")
    if Ho > 1:
        assert ref.abs().max() > 0.5                                        # not degenerate (one output row may be all padding)
    out, gemm = mk(), mk()
    assert G.conv_s21_supported([src], out, w, **R.S21_GEOM)
    G.ConvS21TilePlan(src, out, w, b, slope=R.SLOPE, device=gpu_device).run(src.t, out_h=out.t)
    G.plan_conv2d([src], gemm, w, b, slope=R.SLOPE, device=gpu_device, interior_only=True, **R.S21_GEOM).run(src.t, out_h=gemm.t)
    torch.cuda.synchronize()
    check(f"conv53s21 {(B, Ho, W)}", out, ref, bnd)
    check(f"conv53s21-gemm {(B, Ho, W)}", gemm, ref, bnd)


def test_conv_s21_tile_f16_entry_point(gpu_device):
    _lib.init()
    dev, lib = gpu_device, _lib.lib()
    B, Ho, W = 2, 11, 21
    src, mk, x, w, b = s21_case(dev, B, Ho, W, R.P1_S21)
    out = mk()
    plan = G.ConvS21TilePlan(src, out, w, b, slope=R.SLOPE, device=dev)
    plan.run(src.t, out_h=out.t)
    again = mk()
    plan.run(src.t, out_h=again.t)
    torch.cuda.synchronize()
    assert torch.equal(R.read_map(out), R.read_map(again))                  # the same plan twice: identical bits
    # act = ADVH_ACT_NONE: the layer without its LeakyReLU
    ref = R.conv_layer([x], w, b, slope=None, **R.S21_GEOM)
    bnd = R.bound(ref, R.conv_layer([x.abs()], w.abs(), b.abs(), **R.S21_GEOM), R.K_S21, "f16")
    assert (ref < -0.5).any()
    lin = mk()
    plan.desc.act = G.ACT["none"]
    plan.run(src.t, out_h=lin.t)
    torch.cuda.synchronize()
    check("conv53s21 act=none", lin, ref, bnd)
    plan.desc.act = G.ACT["leaky"]
    # bias = NULL is a zero bias, bit for bit
    zero, nob = mk(), mk()
    G.ConvS21TilePlan(src, zero, w, b * 0, slope=R.SLOPE, device=dev).run(src.t, out_h=zero.t)
    d = plan.desc
    d.X, d.W, d.bias, d.out_h = src.t.data_ptr(), plan.w.data_ptr(), None, nob.t.data_ptr()
    assert lib.advh_conv53s21_tile_f16(C.byref(d), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(nob.t, zero.t) and not torch.equal(nob.t, out.t)
    # geometry the kernel refuses: its patch starts two rows above and one column left of the interior
    d.bias = plan.bias.data_ptr()
    for field, bad in (("PHi", 1), ("PWi", 0), ("PHo", -1), ("Ho", 0), ("act", G.ACT["gelu"])):
        keep = getattr(d, field)
        setattr(d, field, bad)
        assert lib.advh_conv53s21_tile_f16(C.byref(d), None) == -1, field   # ADVH_EINVAL
        setattr(d, field, keep)
    assert not G.conv_s21_supported([G.FMap(B, 2 * Ho, W, 32, 1, 1)], out, w, **R.S21_GEOM)
    assert not G.conv_s21_supported([G.FMap(B, 2 * Ho, W, 32, 2, 0)], out, w, **R.S21_GEOM)
    torch.cuda.synchronize()
    assert (R.read_halo(nob) == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ advh_upconv21_tile_f16
def upconv_case(dev, B, Hc, W, pads):
    (phc, pwc), (phs, pws), (pho, pwo) = pads
    xc, xs, wt, bt, wc, bc = R.upconv_data(B, Hc, W)
    coarse = src_map(dev, xc, phc, pwc)
    skip = G.add_indicator(src_map(dev, xs, phs, pws, Cn=8), 1)
    return coarse, skip, (lambda: dst_map(dev, B, 2 * Hc, W, 32, pho, pwo)), (xc, xs), (wt, bt, wc, bc)


def upconv_ref(xc, xs, wt, bt, wc, bc, slope=R.SLOPE):
    ref = R.upconv_layer(xc, xs, wt, bt, wc, bc, (2, 1), slope=slope)
    A = R.upconv_layer(xc.abs(), xs.abs(), wt.abs(), bt.abs(), wc.abs(), bc.abs(), (2, 1))
    return ref, R.bound(ref, A, R.K_UPCONV, "f16")


UP_KW = dict(stride=(2, 1), coarse_C=64, skip_C=1, indicator=("skip", 1))


@pytest.mark.parametrize("B,Hc,W,pads", R.UPCONV_CASES)
def test_upconv_tile_f16(gpu_device, B, Hc, W, pads):
    _lib.init()
    coarse, skip, mk, xx, ww = upconv_case(gpu_device, B, Hc, W, pads)
    ref, bnd = upconv_ref(*xx, *ww)
    assert ref.abs().max() > 0.5
    out, gemm, nob = mk(), mk(), mk()
    assert G.upconv_tile_supported(coarse, skip, out, ww[0], ww[2], (2, 1), ("skip", 1))
    G.UpconvTilePlan(coarse, skip, out, *ww, slope=R.SLOPE, device=gpu_device).run(coarse.t, skip.t, out_h=out.t)
    G.plan_upconv2d(coarse, skip, gemm, *ww, slope=R.SLOPE, device=gpu_device, **UP_KW).run(coarse.t, skip.t, out_h=gemm.t)
    # the indicator path matters: the same stage without the transposed convolution's bias gives another map
    wt, bt, wc, bc = ww
    G.UpconvTilePlan(coarse, skip, nob, wt, bt * 0, wc, bc, slope=R.SLOPE, device=gpu_device).run(coarse.t, skip.t, out_h=nob.t)
    torch.cuda.synchronize()
    check(f"upconv21 {(B, Hc, W)}", out, ref, bnd)
    check(f"upconv21-gemm {(B, Hc, W)}", gemm, ref, bnd)
    assert not torch.equal(nob.t, out.t)
    ref0, bnd0 = upconv_ref(*xx, wt, bt * 0, wc, bc)
    check(f"upconv21 bt=0 {(B, Hc, W)}", nob, ref0, bnd0)


def test_upconv_tile_f16_entry_point(gpu_device):
    _lib.init()
    dev, lib = gpu_device, _lib.lib()
    B, Hc, W = 2, 8, 21
    coarse, skip, mk, xx, ww = upconv_case(dev, B, Hc, W, R.P1_UP)
    wt, bt, wc, bc = ww
    out, again = mk(), mk()
    plan = G.UpconvTilePlan(coarse, skip, out, *ww, slope=R.SLOPE, device=dev)
    plan.run(coarse.t, skip.t, out_h=out.t)
    plan.run(coarse.t, skip.t, out_h=again.t)
    torch.cuda.synchronize()
    assert torch.equal(R.read_map(out), R.read_map(again))                  # the same plan twice: identical bits
    ref, bnd = upconv_ref(*xx, *ww, slope=None)                             # act = ADVH_ACT_NONE
    assert (ref < -0.5).any()
    lin = mk()
    plan.desc.act = G.ACT["none"]
    plan.run(coarse.t, skip.t, out_h=lin.t)
    torch.cuda.synchronize()
    check("upconv21 act=none", lin, ref, bnd)
    plan.desc.act = G.ACT["leaky"]
    zero, nob = mk(), mk()                                                  # bias = NULL is a zero bias, bit for bit
    G.UpconvTilePlan(coarse, skip, zero, wt, bt, wc, bc * 0, slope=R.SLOPE, device=dev).run(coarse.t, skip.t, out_h=zero.t)
    d = plan.desc
    d.Xc, d.Xs, d.W, d.bias, d.out_h = coarse.t.data_ptr(), skip.t.data_ptr(), plan.w.data_ptr(), None, nob.t.data_ptr()
    assert lib.advh_upconv21_tile_f16(C.byref(d), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(nob.t, zero.t) and not torch.equal(nob.t, out.t)
    d.bias = plan.bias.data_ptr()
    for field in ("PHc", "PWc", "PHs", "PWs"):                              # a source halo below 1
        setattr(d, field, 0)
        assert lib.advh_upconv21_tile_f16(C.byref(d), None) == -1, field    # ADVH_EINVAL
        setattr(d, field, 1)
    for hc in (4, 12, 17):                                                  # tiles are 16 output rows = 8 coarse rows
        d.Hc = hc
        assert lib.advh_upconv21_tile_f16(C.byref(d), None) == -4           # ADVH_EUNSUPPORTED
        maps = [G.FMap(B, hc, W, 64, 1, 1), G.FMap(B, 2 * hc, W, 8, 1, 1), G.FMap(B, 2 * hc, W, 32, 1, 1)]
        assert not G.upconv_tile_supported(*maps, wt, wc, (2, 1), ("skip", 1))
    d.Hc = Hc
    assert not G.upconv_tile_supported(G.FMap(B, Hc, W, 64, 0, 1), skip, out, wt, wc, (2, 1), ("skip", 1))
    assert not G.upconv_tile_supported(coarse, G.FMap(B, 2 * Hc, W, 8, 1, 0), out, wt, wc, (2, 1), ("skip", 1))
    torch.cuda.synchronize()
    assert (R.read_halo(nob) == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ advh_conv_taps2d_f16
@pytest.mark.parametrize("Cn,B,H,W,PH,PW", R.TAPS2D_CASES)
def test_conv_taps2d_f16_past_its_grid(gpu_device, Cn, B, H, W, PH, PW):
    """The first two cases have more tiles than the launch has workgroups (546 > 512 with 32 channels, 270 > 256 with 64): a
    workgroup walks a second tile.  The other four are the shapes of tests/test_gpu_gemm.py::test_conv2d_line_tile, here under
    the elementwise bound instead of 2e-3 of the maximum."""
    _lib.init()
    x, w, b = R.taps2d_data(Cn, B, H, W)
    ref, A = R.conv_layer([x], w, b), R.conv_layer([x.abs()], w.abs(), b.abs())
    bnd = R.bound(ref, A, 9 * Cn, "f16")
    assert ref.abs().max() > 0.5
    src, out, gemm = src_map(gpu_device, x, PH, PW), dst_map(gpu_device, B, H, W, Cn, PH, PW), dst_map(gpu_device, B, H, W, Cn, PH, PW)
    assert G.taps2d_supported([src], out, w)
    G.Taps2dPlan(src, out, w, b, slope=R.SLOPE, device=gpu_device).run(src.t, out_h=out.t)
    G.plan_conv2d([src], gemm, w, b, slope=R.SLOPE, device=gpu_device, interior_only=True).run(src.t, out_h=gemm.t)
    torch.cuda.synchronize()
    check(f"taps2d C={Cn} {(B, H, W)}", out, ref, bnd)
    check(f"taps2d-gemm C={Cn} {(B, H, W)}", gemm, ref, bnd)
