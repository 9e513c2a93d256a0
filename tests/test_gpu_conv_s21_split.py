"""GPU: the fp32-class line tile of e2.block.0 (csrc/conv_s21_tile_x3.hip; Conv2d(32, 64, (5, 3), stride (2, 1), padding (2, 1)) +
bias + LeakyReLU on split maps) is bit-identical to the x3 implicit GEMM of ``gemm.plan_conv2d`` on the same maps -- both planes,
halo included -- at the production geometry and at ragged sizes, keeps the split format's range contract, and is what the fp32-class
``HipUNet`` dispatches with ``line_tile`` (``line_tile=False`` keeps the GEMM, the bit-for-bit reference)."""
import ctypes as C

import pytest
import torch

from addvisor_hip import _lib, gemm as G, synthetic as syn
from addvisor_hip.unet import HipUNet

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

KW = dict(stride=(2, 1), padding=(2, 1))


def split_map(B, H, W, Cn, PH, PW, dev, x=None):
    f = G.FMap(B, H, W, Cn, PH, PW, split=True).alloc(dev)
    if x is not None:
        f.t[:, :, PH:PH + H, PW:PW + W] = G.split_planes(x).to(dev)
    return f


def case(dev, B, Ho, W, pads=((2, 1), (1, 1))):
    g = torch.Generator().manual_seed(31 * B + 7 * Ho + W)
    (phi, pwi), (pho, pwo) = pads
    src = split_map(B, 2 * Ho, W, 32, phi, pwi, dev, torch.randn(B, 2 * Ho, W, 32, generator=g, dtype=torch.float64))
    w = torch.randn(64, 32, 5, 3, generator=g, dtype=torch.float64) / (15 * 32) ** 0.5
    b = torch.randn(64, generator=g, dtype=torch.float64) * 0.1
    return src, (lambda: split_map(B, Ho, W, 64, pho, pwo, dev)), w, b


# (B, Ho, W, (source halo, destination halo)): e2.block.0 at B = 2 (256 x 196 x 32 -> 128 x 196 x 64), then ragged sizes: widths 1, 15,
# 33, 50, B = 1 and 3, heights 1, 5, 17, 40 (not multiples of the 16-row tile), larger halos on either map, a destination without one
P1 = ((2, 1), (1, 1))
CASES = [(2, 128, 196, P1), (1, 1, 1, P1), (3, 5, 15, P1), (1, 17, 33, ((3, 2), (1, 1))), (3, 16, 50, ((2, 1), (2, 3))), (1, 40, 15, ((4, 4), (0, 0))),
         (1, 1, 50, P1), (2, 33, 16, P1), (5, 64, 200, P1)]             # the last: 260 tiles, so some workgroups walk two (ring across tiles)


@pytest.mark.parametrize("B,Ho,W,pads", CASES)
def test_conv_s21_split_tile_matches_implicit_gemm(gpu_device, B, Ho, W, pads):
    _lib.init()
    src, mk, w, b = case(gpu_device, B, Ho, W, pads)
    ref, out = mk(), mk()
    PH, PW = out.PH, out.PW
    out.t[:, :, PH:PH + Ho, PW:PW + W] = float("nan")                       # every interior element must be written
    assert G.conv_s21_split_supported([src], out, w, **KW)
    G.plan_conv2d([src], ref, w, b, slope=0.2, device=gpu_device, **KW).run(src.t, out_h=ref.t)
    G.ConvS21SplitTilePlan(src, out, w, b, slope=0.2, device=gpu_device).run(src.t, out_h=out.t)
    torch.cuda.synchronize()
    _lib.check_overflow("in-range layer")
    assert not torch.isnan(out.t).any()
    assert ref.t[0].abs().max() > 0.5                                       # the case is not degenerate
    assert torch.equal(out.t, ref.t)                                        # both planes, halo included
    halo = out.t.clone()
    halo[:, :, PH:PH + Ho, PW:PW + W] = 0
    assert (halo == 0).all()
    inner = mk()                                                            # and the GEMM in the enumeration HipUNet uses
    G.plan_conv2d([src], inner, w, b, slope=0.2, device=gpu_device, interior_only=True, **KW).run(src.t, out_h=inner.t)
    assert torch.equal(out.t, inner.t)


def test_conv_s21_split_tile_entry_point(gpu_device):
    _lib.init()
    src, mk, w, b = case(gpu_device, 1, 4, 16)
    out = mk()
    plan = G.ConvS21SplitTilePlan(src, out, w, b, device=gpu_device)
    d = plan.desc
    d.X, d.W, d.bias, d.out_h = src.t.data_ptr(), plan.w.data_ptr(), plan.bias.data_ptr(), out.t.data_ptr()
    lo = (src.t.stride(0), plan.w.stride(0), out.t.stride(0))
    lib = _lib.lib()
    assert lib.advh_conv53s21_tile_split(C.byref(d), 64, 64, *lo, None) == -4                    # ADVH_EUNSUPPORTED
    assert lib.advh_conv53s21_tile_split(C.byref(d), 32, 32, *lo, None) == -4
    assert lib.advh_conv53s21_tile_split(C.byref(d), 32, 64, 0, *lo[1:], None) == -1             # ADVH_EINVAL: no lo plane
    assert lib.advh_conv53s21_tile_split(C.byref(d), 32, 64, lo[0] + 4, *lo[1:], None) == -1     # not a multiple of 8
    assert lib.advh_conv53s21_tile_split(C.byref(d), 32, 64, *lo, None) == 0
    torch.cuda.synchronize()
    d.bias = None                                                           # a missing bias is a zero bias
    nob, ref = mk(), mk()
    d.out_h = nob.t.data_ptr()
    assert lib.advh_conv53s21_tile_split(C.byref(d), 32, 64, *lo, None) == 0
    G.plan_conv2d([src], ref, w, b * 0, slope=0.2, device=gpu_device, **KW).run(src.t, out_h=ref.t)
    torch.cuda.synchronize()
    assert torch.equal(nob.t, ref.t)


def flagged(launch) -> bool:
    lib = _lib.lib()
    torch.cuda.synchronize()
    lib.advh_split_overflow(1)
    raised = False
    try:
        launch()
    except _lib.SplitRangeError:
        raised = True
    torch.cuda.synchronize()
    return bool(lib.advh_split_overflow(1)) or raised


def test_conv_s21_split_tile_keeps_the_range_contract(gpu_device):
    """An activation above 65 504 reaching the kernel's store raises the sticky range flag exactly as the GEMM does, and both store the
    same saturated planes; the same layer in range leaves the flag clear."""
    _lib.init()
    src, mk, w, b = case(gpu_device, 1, 9, 20)
    out, ref = mk(), mk()
    assert not flagged(lambda: G.ConvS21SplitTilePlan(src, out, w, b, device=gpu_device).run(src.t, out_h=out.t))
    b = b.clone()
    b[7] = 1.0e5
    assert flagged(lambda: G.plan_conv2d([src], ref, w, b, slope=0.2, device=gpu_device, **KW).run(src.t, out_h=ref.t))
    plan = G.ConvS21SplitTilePlan(src, out, w, b, device=gpu_device)
    torch.cuda.synchronize()
    _lib.lib().advh_split_overflow(1)
    with pytest.raises(_lib.SplitRangeError):
        plan.run(src.t, out_h=out.t)
        torch.cuda.synchronize()
        _lib.check_overflow("e2.block.0")
    torch.cuda.synchronize()
    assert _lib.lib().advh_split_overflow(1) == 0
    assert torch.isfinite(out.t).all()                                      # saturated, not inf
    assert torch.equal(out.t, ref.t)


def test_split_unet_dispatches_the_tile_and_stays_bit_identical(gpu_device):
    sd = syn.unet_weights()
    mag = (torch.rand(2, 513, 199, generator=torch.Generator().manual_seed(12)) * 3).to(gpu_device)
    on = HipUNet(sd, gpu_device, precision="f32", line_tile=True)
    m_on, l_on = on.forward(mag, want_logits=True)
    steps = on._workspace(2, 512, 196)["steps"]
    assert [type(p).__name__ for p, _, dst in steps if dst == "x2a"] == ["ConvS21SplitTilePlan"]
    off = HipUNet(sd, gpu_device, precision="f32", line_tile=False)
    m_off, l_off = off.forward(mag, want_logits=True)
    assert [type(p).__name__ for p, _, dst in off._workspace(2, 512, 196)["steps"] if dst == "x2a"] == ["GemmPlan"]
    assert torch.equal(l_on, l_off) and torch.equal(m_on, m_off)
    assert torch.equal(on._workspace(2, 512, 196)["maps"]["x2a"].t, off._workspace(2, 512, 196)["maps"]["x2a"].t)
    f16 = HipUNet(sd, gpu_device, precision="f16", line_tile=True)
    f16.forward(mag)
    assert [type(p).__name__ for p, _, dst in f16._workspace(2, 512, 196)["steps"] if dst == "x2a"] == ["ConvS21TilePlan"]
