"""CPU-only checks of the fp32-class 2-D line tile (csrc/conv_taps2d_x3.hip): it compiles without scratch at the designed occupancy,
its entry points reject bad arguments before any HIP call, and the planner routes exactly the 3x3 same-geometry split layers to it."""
import ctypes as C

import pytest
import torch

from addvisor_hip import _lib, gemm as G
from test_build_resources import resources


def test_taps2d_split_kernels_do_not_spill():
    res = resources("conv_taps2d_x3.hip")
    hit = {k: v for k, v in res.items() if "conv_taps2d_x3_kernel" in k}
    assert len(hit) == 2, sorted(res)
    for k, v in hit.items():
        assert v["scratch"] == 0, (k, v)
        assert v["occupancy"] >= 2, (k, v)                     # two wavefronts per SIMD (one CU: 2 x 4 or 1 x 8 wavefronts)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


def test_taps2d_split_lds_fits(lib):
    # 32 channels: two workgroups per CU; 64 channels: one (160 KiB of LDS per CU)
    assert 2 * lib.advh_conv_taps2d_split_lds_bytes(32) <= 160 * 1024
    assert 160 * 1024 // 2 < lib.advh_conv_taps2d_split_lds_bytes(64) <= 160 * 1024
    assert lib.advh_conv_taps2d_split_lds_bytes(48) == -1


def test_taps2d_split_argument_errors(lib):
    EINVAL, EUNSUPPORTED = -1, -4
    buf = (C.c_float * 64)()
    p, q = C.addressof(buf), C.addressof(buf) + 64

    def desc(**kw):
        d = G.Taps2dDesc()
        d.X, d.W, d.out_h = p, p, q
        d.B, d.H, d.W_, d.PH, d.PW, d.act, d.slope = 1, 16, 16, 1, 1, G.ACT["leaky"], 0.2
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    plane = 18 * 18 * 32
    ok = dict(x_lo=plane, w_lo=9 * 32 * 32, o_lo=plane)

    def call(d, Cn=32, **lo):
        a = {**ok, **lo}
        return lib.advh_conv_taps2d_split(C.byref(d), Cn, a["x_lo"], a["w_lo"], a["o_lo"], None)

    assert lib.advh_conv_taps2d_split(None, 32, plane, 9 * 32 * 32, plane, None) == EINVAL
    assert call(desc(X=None)) == EINVAL
    assert call(desc(W=None)) == EINVAL
    assert call(desc(out_h=None)) == EINVAL
    assert call(desc(out_h=p)) == EINVAL                                   # in place
    assert call(desc(B=0)) == EINVAL
    assert call(desc(H=0)) == EINVAL
    assert call(desc(W_=-3)) == EINVAL
    assert call(desc(PH=0)) == EINVAL
    assert call(desc(PW=0)) == EINVAL
    assert call(desc(act=G.ACT["gelu"])) == EINVAL
    assert call(desc(), Cn=48) == EUNSUPPORTED
    assert call(desc(), Cn=16) == EUNSUPPORTED
    assert call(desc(), x_lo=0) == EINVAL                                  # no lo plane
    assert call(desc(), x_lo=plane - 8) == EINVAL                          # lo plane overlaps the hi plane
    assert call(desc(), o_lo=plane - 8) == EINVAL
    assert call(desc(), w_lo=9 * 32 * 32 - 8) == EINVAL
    assert call(desc(), x_lo=plane + 4) == EINVAL                          # 16-byte alignment of the lo plane
    assert call(desc(), o_lo=plane + 4) == EINVAL
    assert call(desc(), w_lo=9 * 32 * 32 + 4) == EINVAL
    assert call(desc(), Cn=64) == EINVAL                                   # a 64-channel plane is twice as long


def test_taps2d_split_host_rule():
    w = torch.zeros(32, 32, 3, 3, dtype=torch.float64)
    s, d = G.FMap(2, 256, 196, 32, 2, 1, split=True), G.FMap(2, 256, 196, 32, 2, 1, split=True)
    assert G.taps2d_split_supported([s], d, w)
    f16s, f16d = G.FMap(2, 256, 196, 32, 2, 1), G.FMap(2, 256, 196, 32, 2, 1)
    assert not G.taps2d_split_supported([f16s], f16d, w)                  # fp16 maps: advh_conv_taps2d_f16's layers
    assert G.taps2d_supported([f16s], f16d, w)
    assert not G.taps2d_split_supported([s], G.FMap(2, 256, 196, 32, 1, 1, split=True), w)      # one halo geometry
    assert not G.taps2d_split_supported([s], d, w, stride=(2, 1))
    assert not G.taps2d_split_supported([G.FMap(2, 256, 196, 40, 1, 1, split=True)], G.FMap(2, 256, 196, 32, 1, 1, split=True),
                                        torch.zeros(32, 40, 3, 3))
    w64 = torch.zeros(64, 64, 3, 3)
    assert G.taps2d_split_supported([G.FMap(1, 128, 196, 64, 1, 1, split=True)], G.FMap(1, 128, 196, 64, 1, 1, split=True), w64)
    assert not G.taps2d_split_supported([G.FMap(1, 128, 196, 64, 1, 1, split=True)], G.FMap(1, 128, 196, 64, 1, 1, split=True),
                                        torch.zeros(64, 64, 5, 3), padding=(2, 1))
