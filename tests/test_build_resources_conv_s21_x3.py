"""CPU-only: the fp32-class line tile of e2.block.0, conv53s21_tile_x3_kernel (csrc/conv_s21_tile_x3.hip), compiles for gfx950 without
scratch at two wavefronts per SIMD (its one workgroup per CU is eight wavefronts; the second wavefront per SIMD is what hides the LDS
latency), its LDS plan fits a CU, its host-side weight packing is the implicit GEMM's K order, and the entry point rejects bad
arguments before any HIP call."""
import ctypes as C

import torch

from addvisor_hip import _lib, gemm as G
from test_build_resources import resources


def test_conv_s21_split_tile_kernel_does_not_spill():
    res = resources("conv_s21_tile_x3.hip")
    hit = {k: v for k, v in res.items() if "conv53s21_tile_x3_kernel" in k}
    assert len(hit) == 1, sorted(res)
    for k, v in hit.items():
        assert v["scratch"] == 0, (k, v)
        assert v["occupancy"] >= 2, (k, v)


def test_conv_s21_split_tile_weight_packing():
    """[2 planes][8 k-blocks][64 rows][64]: row R of a k-block carries output channel ``packed_row_channel``; the columns are the
    GEMM plan's K order (tap kh * 3 + kw, then channel) zero-padded to 512, i.e. the planes of the GEMM plan's own packed weight."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(64, 32, 5, 3, generator=g, dtype=torch.float64) * 0.1
    src, dst = G.FMap(1, 8, 5, 32, 2, 1, split=True), G.FMap(1, 4, 5, 64, 1, 1, split=True)
    assert G.conv_s21_split_supported([src], dst, w, (2, 1), (2, 1))
    assert not G.conv_s21_split_supported([src], dst, w, (2, 2), (2, 1))
    assert not G.conv_s21_split_supported([src], dst, w, (2, 1), (1, 1))
    assert not G.conv_s21_split_supported([G.FMap(1, 8, 5, 32, 2, 1)], G.FMap(1, 4, 5, 64, 1, 1), w, (2, 1), (2, 1))    # fp16 maps
    assert not G.conv_s21_split_supported([G.FMap(1, 8, 5, 32, 1, 1, split=True)], dst, w, (2, 1), (2, 1))            # row halo < 2
    assert not G.conv_s21_split_supported([src], dst, w[:, :, :3], (2, 1), (2, 1))
    tile = G.ConvS21SplitTilePlan(src, dst, w, torch.zeros(64))
    gemm = G.plan_conv2d([src], dst, w, torch.zeros(64), stride=(2, 1), padding=(2, 1))
    assert gemm.desc.wide and gemm.Kp == 512 and tuple(tile.w.shape) == (2, 8, 64, 64)
    # the GEMM's packed operand: [2 planes][1][256 rows (wide permutation)][512]
    assert torch.equal(tile.w.permute(0, 2, 1, 3).reshape(2, 64, 512), gemm.w[:, 0, :64])
    assert (tile.w[:, 7, :, 32:] == 0).all()                               # the padding step multiplies zero weights


def test_conv_s21_split_tile_argument_errors():
    _lib.build()
    lib = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -4
    assert 80 * 1024 < lib.advh_conv53s21_tile_split_lds_bytes() <= 160 * 1024      # one workgroup (eight wavefronts) per CU
    buf = (C.c_float * 64)()
    p, q = C.addressof(buf), C.addressof(buf) + 64

    def desc(**kw):
        d = G.ConvS21Desc()
        d.X, d.W, d.bias, d.out_h = p, p, None, q
        d.B, d.Ho, d.W_, d.PHi, d.PWi, d.PHo, d.PWo, d.act, d.slope = 1, 8, 16, 2, 1, 1, 1, G.ACT["leaky"], 0.2
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    px, pw, po = 20 * 18 * 32, 8 * 64 * 64, 10 * 18 * 64
    ok = dict(x_lo=px, w_lo=pw, o_lo=po)

    def call(d, Ci=32, N=64, **lo):
        a = {**ok, **lo}
        return lib.advh_conv53s21_tile_split(C.byref(d), Ci, N, a["x_lo"], a["w_lo"], a["o_lo"], None)

    assert lib.advh_conv53s21_tile_split(None, 32, 64, px, pw, po, None) == EINVAL
    for f in ("X", "W", "out_h"):
        assert call(desc(**{f: None})) == EINVAL
    assert call(desc(out_h=p)) == EINVAL                                   # in place
    for f in ("B", "Ho", "W_", "PWi"):
        assert call(desc(**{f: 0})) == EINVAL
    assert call(desc(PHi=1)) == EINVAL                                     # the 5-row window needs two halo rows
    assert call(desc(PHo=-1)) == EINVAL
    assert call(desc(PWo=-1)) == EINVAL
    assert call(desc(act=G.ACT["gelu"])) == EINVAL
    assert call(desc(), Ci=64) == EUNSUPPORTED
    assert call(desc(), N=32) == EUNSUPPORTED
    for k, v in ok.items():
        assert call(desc(), **{k: 0}) == EINVAL                            # no lo plane
        assert call(desc(), **{k: v - 8}) == EINVAL                        # lo plane overlaps the hi plane
        assert call(desc(), **{k: v + 4}) == EINVAL                        # 16-byte alignment of the lo plane
