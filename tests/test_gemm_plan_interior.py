"""CPU-only: ``gemm.plan_conv2d(..., interior_only=True)`` -- the enumeration of the U-Net's inference plans -- replayed in numpy with
the kernel's addressing rule (``gemm.replay_on_cpu``): it writes exactly the interior values of the padded plan and touches no halo
element (the destination starts NaN-filled: the halo stays NaN, the interior equals the padded plan's, value for value)."""
import pytest
import torch

from addvisor_hip import gemm as G

torch.manual_seed(0)


def fill(f: G.FMap, x_nchw: torch.Tensor):
    f.t = torch.zeros((f.B, f.Hp, f.Wp, f.C), dtype=torch.float16)
    f.interior()[:] = x_nchw.permute(0, 2, 3, 1).to(torch.float16)
    return f


# (source channels, Cout, kernel, stride, padding, dilation, H, W, source halo, destination halo)
CASES = [
    ([8], 8, (3, 3), (1, 1), (1, 1), (1, 1), 6, 5, (1, 1), (1, 1)),
    ([8], 8, (3, 3), (1, 1), (1, 1), (1, 1), 6, 5, (1, 1), (0, 0)),                # halo 0: both forms enumerate the same rows
    ([8], 16, (5, 3), (2, 1), (2, 1), (1, 1), 8, 5, (2, 1), (1, 1)),               # e2.block.0: stride (2, 1), 5 x 3, padding (2, 1)
    ([16], 8, (3, 3), (2, 2), (1, 1), (1, 1), 8, 6, (1, 1), (2, 2)),               # e3 / e4: stride (2, 2); e4.block.3's halo 2
    ([8], 8, (3, 3), (1, 1), (2, 2), (2, 2), 6, 7, (2, 2), (4, 4)),                # bottleneck.0: dilation 2 into a halo of 4
    ([8], 8, (3, 3), (1, 1), (4, 4), (4, 4), 6, 7, (4, 4), (1, 1)),                # bottleneck.3: dilation 4
    ([16, 8], 8, (3, 3), (1, 1), (1, 1), (1, 1), 4, 6, (1, 1), (1, 1)),            # two sources, concatenated by pointer
    ([8, 16], 8, (3, 3), (1, 1), (1, 1), (1, 1), 4, 6, (2, 3), (2, 1)),            # sources with a wider halo than the kernel needs
    ([8], 8, (3, 3), (2, 2), (1, 1), (1, 1), 6, 8, (3, 2), (4, 4)),                # stride (2, 2) with halos on both sides
]


@pytest.mark.parametrize("Cins,Cout,k,stride,pad,dil,H,W,halo_in,halo_out", CASES)
def test_interior_only_plan_writes_the_padded_plans_interior_and_nothing_else(Cins, Cout, k, stride, pad, dil, H, W, halo_in, halo_out):
    B = 2
    xs = [torch.randn(B, c, H, W) for c in Cins]
    w, b = torch.randn(Cout, sum(Cins), *k) * 0.2, torch.randn(Cout)
    srcs = [fill(G.FMap(B, H, W, c, *halo_in), x) for c, x in zip(Cins, xs)]
    Ho = (H + 2 * pad[0] - dil[0] * (k[0] - 1) - 1) // stride[0] + 1
    Wo = (W + 2 * pad[1] - dil[1] * (k[1] - 1) - 1) // stride[1] + 1
    dst = G.FMap(B, Ho, Wo, Cout, *halo_out)
    numel = B * dst.Hp * dst.Wp * Cout
    a1 = srcs[1].t if len(srcs) > 1 else None
    kw = dict(stride=stride, padding=pad, dilation=dil)
    padded = G.plan_conv2d(srcs, dst, w, b, **kw)
    inner = G.plan_conv2d(srcs, dst, w, b, interior_only=True, **kw)
    assert padded.desc.M == B * dst.Hp * dst.Wp and inner.desc.M == B * Ho * Wo
    assert inner.desc.halo_zero == 0 and (inner.desc.h0, inner.desc.h1, inner.desc.w0, inner.desc.w1) == (0, Ho, 0, Wo)
    assert (inner.tile, inner.Kp) == (padded.tile, padded.Kp) and (inner.ktab_host == padded.ktab_host).all()
    assert torch.equal(inner.w, padded.w)
    assert inner.flops == padded.flops * (Ho * Wo) / (dst.Hp * dst.Wp)          # interior rows only
    nan = torch.full((numel,), float("nan"))
    ref = G.replay_on_cpu(padded, srcs[0].t, a1, numel, out_init=nan).view(B, dst.Hp, dst.Wp, Cout)
    out = G.replay_on_cpu(inner, srcs[0].t, a1, numel, out_init=nan).view(B, dst.Hp, dst.Wp, Cout)
    PH, PW = dst.PH, dst.PW
    assert not torch.isnan(ref).any()                                       # the padded form produces the whole map
    assert torch.equal(out[:, PH:PH + Ho, PW:PW + Wo], ref[:, PH:PH + Ho, PW:PW + Wo])
    assert ref[:, PH:PH + Ho, PW:PW + Wo].abs().max() > 0.1
    halo = torch.ones(B, dst.Hp, dst.Wp, Cout, dtype=torch.bool)
    halo[:, PH:PH + Ho, PW:PW + Wo] = False
    assert torch.isnan(out[halo]).all()                                     # no halo element is touched
    assert (ref[halo] == 0).all()


def test_interior_only_is_off_by_default():
    src = fill(G.FMap(1, 4, 4, 8, 1, 1), torch.randn(1, 8, 4, 4))
    dst = G.FMap(1, 4, 4, 8, 1, 1)
    p = G.plan_conv2d([src], dst, torch.randn(8, 8, 3, 3), None)
    assert p.desc.halo_zero == 1 and p.desc.M == 36


def test_interior_only_with_a_channel_offset():
    """``dst_c0`` (a convolution writing into a slice of a wider map) moves with the interior origin."""
    B, H, W = 1, 3, 4
    src = fill(G.FMap(B, H, W, 8, 1, 1), torch.randn(B, 8, H, W))
    w, b = torch.randn(8, 8, 3, 3) * 0.2, torch.randn(8)
    dst = G.FMap(B, H, W, 24, 2, 1)
    numel = B * dst.Hp * dst.Wp * 24
    nan = torch.full((numel,), float("nan"))
    ref = G.replay_on_cpu(G.plan_conv2d([src], dst, w, b, dst_c0=8), src.t, None, numel, out_init=nan).view(B, dst.Hp, dst.Wp, 24)
    out = G.replay_on_cpu(G.plan_conv2d([src], dst, w, b, dst_c0=8, interior_only=True), src.t, None, numel, out_init=nan).view(B, dst.Hp, dst.Wp, 24)
    assert torch.equal(out[:, 2:2 + H, 1:1 + W, 8:16], ref[:, 2:2 + H, 1:1 + W, 8:16])
    out[:, 2:2 + H, 1:1 + W, 8:16] = float("nan")
    assert torch.isnan(out).all()
