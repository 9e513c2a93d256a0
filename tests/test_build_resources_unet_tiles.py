"""CPU-only: every instantiation of the fp32-class U-Net line-tile kernels -- conv_taps2d_x3_kernel (csrc/conv_taps2d_x3.h: the two
plain ones of conv_taps2d_x3.hip and the one with the mask head of conv_taps2d_head_x3.hip) and upconv21_tile_x3_kernel
(csrc/upconv_tile_x3.hip) -- compiles for gfx950 without scratch at two wavefronts per SIMD (the second wavefront is what hides the
LDS latency there), and the new entry points reject bad arguments before any HIP call."""
import ctypes as C

import pytest

from addvisor_hip import _lib, gemm as G
from test_build_resources import resources


@pytest.mark.parametrize("src,count", [("conv_taps2d_x3.hip", 2), ("conv_taps2d_head_x3.hip", 1)])
def test_unet_tile_kernels_do_not_spill(src, count):
    res = resources(src)
    hit = {k: v for k, v in res.items() if "conv_taps2d_x3_kernel" in k}
    assert len(hit) == count, sorted(res)
    for k, v in hit.items():
        assert v["scratch"] == 0, (k, v)
        assert v["occupancy"] >= 2, (k, v)
    if count == 1:
        assert "Lb1E" in next(iter(hit)), sorted(hit)                      # the HEAD = true instantiation


def test_upconv_split_tile_kernel_does_not_spill():
    res = resources("upconv_tile_x3.hip")
    hit = {k: v for k, v in res.items() if "upconv21_tile_x3_kernel" in k}
    assert len(hit) == 1, sorted(res)
    for k, v in hit.items():
        assert v["scratch"] == 0, (k, v)
        assert v["occupancy"] >= 2, (k, v)                     # registers allow the eight wavefronts of the one workgroup per CU


def test_upconv_split_tile_argument_errors():
    _lib.build()
    lib = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -4
    assert 80 * 1024 < lib.advh_upconv21_tile_split_lds_bytes() <= 160 * 1024      # one workgroup (eight wavefronts) per CU
    buf = (C.c_float * 64)()
    p, q = C.addressof(buf), C.addressof(buf) + 64

    def desc(**kw):
        d = G.UpconvDesc()
        d.Xc, d.Xs, d.W, d.bias, d.out_h = p, p, p, None, q
        d.B, d.Hc, d.W_, d.PHc, d.PWc, d.PHs, d.PWs, d.PHo, d.PWo, d.act, d.slope = 1, 8, 16, 1, 1, 1, 1, 1, 1, G.ACT["leaky"], 0.2
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    pc, ps, po, pw = 10 * 18 * 64, 18 * 18 * 8, 18 * 18 * 32, 2 * 15 * 32 * 32
    ok = dict(xc_lo=pc, xs_lo=ps, w_lo=pw, o_lo=po)

    def call(d, Cc=64, N=32, **lo):
        a = {**ok, **lo}
        return lib.advh_upconv21_tile_split(C.byref(d), Cc, N, a["xc_lo"], a["xs_lo"], a["w_lo"], a["o_lo"], None)

    assert lib.advh_upconv21_tile_split(None, 64, 32, pc, ps, pw, po, None) == EINVAL
    for f in ("Xc", "Xs", "W", "out_h"):
        assert call(desc(**{f: None})) == EINVAL
    assert call(desc(out_h=p)) == EINVAL                                   # in place
    for f in ("B", "Hc", "W_", "PHc", "PWc", "PHs", "PWs"):
        assert call(desc(**{f: 0})) == EINVAL
    assert call(desc(PHo=-1)) == EINVAL
    assert call(desc(act=G.ACT["gelu"])) == EINVAL
    assert call(desc(), Cc=128, N=64) == EUNSUPPORTED                      # up2 + d2.block.0
    assert call(desc(), N=64) == EUNSUPPORTED
    for k, v in ok.items():
        assert call(desc(), **{k: 0}) == EINVAL                            # no lo plane
        assert call(desc(), **{k: v - 8}) == EINVAL                        # lo plane overlaps the hi plane
        assert call(desc(), **{k: v + 4}) == EINVAL                        # 16-byte alignment of the lo plane


def test_head_entry_point_argument_errors():
    _lib.build()
    lib = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -4
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def desc(**kw):
        d = G.Taps2dDesc()
        d.X, d.W, d.out_h = p, p, None                                     # out_h is not used by this entry point
        d.B, d.H, d.W_, d.PH, d.PW, d.act, d.slope = 1, 16, 16, 1, 1, G.ACT["leaky"], 0.2
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    plane, wplane = 18 * 18 * 32, 9 * 32 * 32

    def call(d, Cn=32, x_lo=plane, w_lo=wplane, hw=p, mask=p, logits=None):
        return lib.advh_conv_taps2d_split_head(C.byref(d), Cn, x_lo, w_lo, hw, 0.5, mask, logits, None)

    assert lib.advh_conv_taps2d_split_head(None, 32, plane, wplane, p, 0.5, p, None, None) == EINVAL
    assert call(desc(X=None)) == EINVAL
    assert call(desc(W=None)) == EINVAL
    assert call(desc(), hw=None) == EINVAL
    assert call(desc(), mask=None) == EINVAL
    assert call(desc(B=0)) == EINVAL
    assert call(desc(PW=0)) == EINVAL
    assert call(desc(act=G.ACT["gelu"])) == EINVAL
    assert call(desc(), Cn=64) == EUNSUPPORTED                             # the head belongs to the 32-channel layer
    assert call(desc(), Cn=48) == EUNSUPPORTED
    assert call(desc(), x_lo=0) == EINVAL                                  # no lo plane
    assert call(desc(), x_lo=plane - 8) == EINVAL                          # lo plane overlaps the hi plane
    assert call(desc(), x_lo=plane + 4) == EINVAL                          # 16-byte alignment of the lo plane
    assert call(desc(), w_lo=wplane - 8) == EINVAL
    assert call(desc(), w_lo=wplane + 4) == EINVAL
