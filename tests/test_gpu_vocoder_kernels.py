"""Every HIP kernel of the HiFi-GAN vocoder against a plain fp64 reference of its own operation (tests/vocoder_ops_ref.py, pinned by
tests/test_vocoder_ops_ref_cpu.py), at the sizes where such kernels break: clips shorter than the padding, M tails, clip edges judged on
their own, non-zero halos, and -- for the four persistent line-tile kernels -- more tiles than workgroups, so that a workgroup walks a
second tile.

Operands.  Split-format inputs are ``G.split_planes`` of random fp32 and the reference computes on ``G.join_planes`` of them in fp64;
fp16 inputs are rounded first and the reference computes on the rounded values, with intermediates rounded where the kernel stores fp16.
Weights go to the plans as fp32 (the fp16 reference rounds them as the plan does).

Tolerances.  Split-format kernels: ``TOL_KERNEL`` = 5e-6 of max|ref|, the stated tolerance of tests/test_gpu_split.py.  fp16 kernels:
tests/test_gpu_gemm.py's ``close()``, |err| <= 2e-3 * max|ref| + 2e-3 (3e-3 for the fused step).  Every named sub-block (a clip edge, one
phase of a transposed convolution, the rows of the second round of tiles) is judged against ITS OWN maximum.  The direct kernels carry
per-element bounds, derived at each test.  Outputs are NaN-filled first and must come out finite; halos that must stay zero are checked
in both planes."""
import numpy as np
import pytest
import torch

import vocoder_ops_ref as R
from addvisor_hip import _lib, gemm as G, synthetic as syn
from addvisor_hip.hifigan import HALO, HipHifigan
from oracle import hifigan_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_KERNEL = 5e-6            # tests/test_gpu_split.py: "split GEMM / convolution kernels 5e-6", relative to max|ref|
TOL_F16, TOL_F16_FUSED = 2e-3, 3e-3          # tests/test_gpu_gemm.py: close(), and its tol for test_fused_resblock_step
SPLIT = pytest.mark.parametrize("split", [True, False], ids=["x3", "f16"])
NAN = float("nan")


def rnd(g, *shape):
    return torch.randn(*shape, generator=g)


def stream():
    return torch.cuda.current_stream().cuda_stream


def pack(x, split):
    return G.split_planes(x) if split else x.half()


def value(t, split):
    """What a kernel read from / wrote to the map tensor ``t``, in fp64 on the host."""
    t = t.cpu()
    return (G.join_planes(t) if split else t).double()


def new_map(dev, B, T, C, split, interior=None, full=None, fill=None):
    """A zero-haloed map; ``interior [B, T, C]`` / ``full [B, P, C]``: its values (fp32); ``fill``: what the interior holds instead."""
    m = G.Map1D(B, T, C, HALO, split=split).alloc(dev)
    if full is not None:
        m.t.copy_(pack(full, split))
    elif interior is not None:
        m.t[..., HALO:HALO + T, :] = pack(interior, split).to(dev)
    elif fill is not None:
        m.t[..., HALO:HALO + T, :] = fill
    return m


def interior(m):
    return value(m.t, m.split)[:, HALO:HALO + m.T]


def halo_is_zero(m):
    """Every halo row of the map is zero, in both planes of a split map (a NaN is not zero)."""
    return bool((m.t[..., :HALO, :] == 0).all() and (m.t[..., HALO + m.T:, :] == 0).all())


def check(what, got, ref, split, blocks=(), tol16=TOL_F16):
    """``got`` / ``ref [N, rows, C]`` fp64: finite, and within the tolerance of the arithmetic class on the whole tensor and on
    every ``(name, rows)`` of ``blocks``, each relative to its own max|ref|."""
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    for name, rows in (("all", slice(None)),) + tuple(blocks):
        g_, r_ = got[:, rows], ref[:, rows]
        if r_.numel() == 0:
            continue
        err, mx = (g_ - r_).abs().max().item(), r_.abs().max().item()
        bound = TOL_KERNEL * mx if split else tol16 * mx + tol16
        print(f"{what} [{name}]: err {err:.2e}, max|ref| {mx:.2e}, err / bound {err / bound:.3f}")
        assert err <= bound, (what, name, err, mx)


def edges(pad, T):
    """The first and last ``pad`` positions of a clip: where taps reach into the halo."""
    return (("first pad", slice(0, min(pad, T))), ("last pad", slice(max(T - pad, 0), T)))


def walked_tiles(M, tile, cap):
    """(ntiles, grid) of a persistent line-tile launch: ``grid = min(ntiles, cap)`` workgroups loop ``tile += gridDim.x``.  A
    many-tile case needs ``ntiles > grid`` (some workgroup takes a second tile) and ``ntiles % grid != 0`` (not all of them do)."""
    ntiles = (M + tile - 1) // tile
    return ntiles, min(ntiles, cap)


def second_round(M, tile, grid):
    """The map rows (of the flat ``[M, C]`` view) that belong to tiles ``>= grid``."""
    return (("second round of tiles", slice(grid * tile, M)),)


# ------------------------------------------------------------------------------------------ 1. implicit GEMM, "same" Conv1d
GEMM_LAYERS = {"conv_pre": (80, 512, 7, 1),      # 10 chunks per row: not a whole 32-deep K step
               "conv1": (128, 128, 11, 5),       # bias + LeakyReLU, padding 25
               "conv2": (256, 256, 3, 1)}        # bias + residual, raw and pre-activated outputs


@pytest.mark.parametrize("T", [1, 5, 37])
@pytest.mark.parametrize("role", list(GEMM_LAYERS))
@SPLIT
def test_implicit_gemm_conv1d_same(gpu_device, split, role, T):
    """``plan_conv1d_same`` in both precisions: B = 3, so M = 3 * (T + 64) is an M tail; T smaller than the padding puts every tap but the
    centre in the halo.  Run once with zero halos and once with random ones (the "reflect" situation: the reference reads the same padded
    map), since a zero halo cannot show a wrong row offset at a clip edge."""
    _lib.init()
    Cin, Cout, k, d = GEMM_LAYERS[role]
    B, pad, conv2, dev = 3, (k - 1) * d // 2, role == "conv2", gpu_device
    g = torch.Generator().manual_seed(1000 * k + T)
    w, b = rnd(g, Cout, Cin, k) / (Cin * k) ** 0.5, rnd(g, Cout) * 0.1
    wr = w.double() if split else w.half().double()
    kw = dict(slope2=0.1) if conv2 else dict(act="leaky", slope=0.1)
    plan = None
    for halo in ("zero", "random"):
        xs = [rnd(g, B, T + 2 * HALO, Cin) for _ in range(2)]
        if halo == "zero":
            for x in xs:
                x[:, :HALO] = 0
                x[:, HALO + T:] = 0
        src = new_map(dev, B, T, Cin, split, full=xs[0])
        res = new_map(dev, B, T, Cout, split, full=xs[1][..., :Cout]) if conv2 else None
        dst, dst2 = new_map(dev, B, T, Cout, split), new_map(dev, B, T, Cout, split, fill=NAN)
        dst.t.fill_(NAN)                                          # the plan writes dst's halo rows itself, as zeros
        plan = plan or G.plan_conv1d_same(src, dst, w, b, dilation=d, device=dev, **kw)
        plan.run(src.t, out_h=dst.t, resid=res.t if conv2 else None, out_h2=dst2.t if conv2 else None)
        torch.cuda.synchronize()
        xv = value(src.t, split)
        y = R.conv1d_same(xv[:, HALO:HALO + T], wr, b, d, padded=xv)
        ref = y + interior(res) if conv2 else R.lrelu(y, 0.1)
        what = f"implicit GEMM {'x3' if split else 'f16'} {role} T={T} halo={halo}"
        check(what, interior(dst), ref, split, edges(pad, T))
        assert halo_is_zero(dst), what
        if conv2:
            check(what + " pre-activated", interior(dst2), R.lrelu(ref, 0.1), split, edges(pad, T))
            assert halo_is_zero(dst2), what


# ------------------------------------------------------------------------------------------ 2. implicit GEMM, ConvTranspose1d
@pytest.mark.parametrize("T", [1, 5, 37])
@pytest.mark.parametrize("Cin,Cout,r", [(128, 64, 8), (64, 32, 2), (16, 8, 2)])
@SPLIT
def test_implicit_gemm_convT1d(gpu_device, split, Cin, Cout, r, T):
    """``plan_convT1d`` (phase decomposition, K = 2 * Cin, pixel-shuffle store) with the pre-activated second output.  Judged per phase
    and on the first / last stride / 2 outputs, which see one input only.  The plan promises to write valid outputs only: the destination's
    pre-zeroed halo must still be zero."""
    _lib.init()
    B, dev = 3, gpu_device
    g = torch.Generator().manual_seed(100 * Cin + 10 * r + T)
    x = rnd(g, B, T, Cin)
    w, b = rnd(g, Cin, Cout, 2 * r) / (2 * Cin) ** 0.5, rnd(g, Cout) * 0.1
    src = new_map(dev, B, T, Cin, split, interior=x)
    dst, dst2 = (new_map(dev, B, T * r, Cout, split, fill=NAN) for _ in range(2))
    G.plan_convT1d(src, dst, w, b, stride=r, slope2=0.1, device=dev).run(src.t, out_h=dst.t, out_h2=dst2.t)
    torch.cuda.synchronize()
    ref = R.conv_transpose1d(interior(src), w.double() if split else w.half().double(), b, r)
    pad = r // 2
    blocks = tuple((f"phase {p}", slice((p - pad) % r, None, r)) for p in range(r))          # output t = q * r + phase - pad
    blocks += (("first r/2", slice(0, pad)), ("last r/2", slice(T * r - pad, T * r)))
    what = f"convT1d {'x3' if split else 'f16'} {Cin}->{Cout} r={r} T={T}"
    check(what, interior(dst), ref, split, blocks)
    check(what + " pre-activated", interior(dst2), R.lrelu(ref, 0.1), split, blocks)
    assert halo_is_zero(dst) and halo_is_zero(dst2), what


# ------------------------------------------------------------------------------------------ 3. advh_conv_taps_split
@pytest.mark.parametrize("k,dil,B,T", [(7, 3, 3, 700), (11, 5, 2, 1000), (11, 1, 1, 255), (7, 1, 5, 64), (3, 5, 2, 300),
                                       pytest.param(7, 3, 2, 33000, id="many-tiles")])
def test_conv_taps_split(gpu_device, k, dil, B, T):
    """``advh_conv_taps_split`` (64 channels, weights streamed through a four-slot LDS ring) against fp64 in both ResBlock roles, at the
    cases of ``test_split_line_tile_matches_implicit_gemm``.  The many-tile case has 259 tiles on 256 workgroups: the next tile's lines
    arrive under the epilogue and the weight ring wraps from tile to tile; its second round of tiles is judged on its own."""
    _lib.init()
    dev, C = gpu_device, 64
    g = torch.Generator().manual_seed(100 * k + dil)
    x, r = rnd(g, B, T, C), rnd(g, B, T, C)
    w, b = rnd(g, C, C, k) * (0.3 / k ** 0.5), rnd(g, C) * 0.1
    src, res = new_map(dev, B, T, C, True, interior=x), new_map(dev, B, T, C, True, interior=r)
    o1, o2, q2 = (new_map(dev, B, T, C, True) for _ in range(3))
    assert G.taps_split_supported(src, o1, w, dil, min_k=3)
    M, pad = B * src.P, (k - 1) * dil // 2
    tile = _lib.lib().advh_conv_taps_split_tile(C, k, (k - 1) * dil)
    ntiles, grid = walked_tiles(M, tile, 256)                      # advh_conv_taps_split: grid = ntiles < 256 ? ntiles : 256
    many = T > 10000
    if many:
        assert ntiles > grid and ntiles % grid != 0, (ntiles, grid)
    for m in (o1, o2, q2):
        m.t.fill_(NAN)                                             # the kernel zeroes the halo rows itself
    G.plan_conv1d_taps(src, o1, w, b, dilation=dil, act="leaky", slope=0.1, device=dev).run(src.t, out_h=o1.t)
    G.plan_conv1d_taps(src, o2, w, b, dilation=dil, slope2=0.1, device=dev).run(src.t, out_h=o2.t, resid=res.t, out_h2=q2.t)
    torch.cuda.synchronize()
    y = R.conv1d_same(interior(src), w, b, dil)
    ref2 = y + interior(res)
    what = f"conv_taps_split k={k} d={dil} B={B} T={T} ({ntiles} tiles on {grid} workgroups)"
    for name, m, ref in (("conv1", o1, R.lrelu(y, 0.1)), ("conv2", o2, ref2), ("conv2 pre-activated", q2, R.lrelu(ref2, 0.1))):
        check(f"{what} {name}", interior(m), ref, True, edges(pad, T))
        assert halo_is_zero(m), (what, name)
        if many:
            full = torch.zeros(B, src.P, C, dtype=torch.float64)
            full[:, HALO:HALO + T] = ref
            check(f"{what} {name}", value(m.t, True).reshape(1, M, C), full.reshape(1, M, C), True, second_round(M, tile, grid))


# ------------------------------------------------------------------------------------------ 4. advh_resblock_pair_x3
V1_KD = [(k, d) for k in (3, 7, 11) for d in (1, 3, 5)]
X3_MANY = {(3, 1): (65200, 512, 1),      # T, grid, nbuf: two workgroups per CU
           (7, 5): (32200, 256, 2),      # the prefetch ring
           (11, 5): (31600, 256, 1)}


def _resblock_weights(g, C, k):
    return (rnd(g, C, C, k) / (C * k) ** 0.5, rnd(g, C) * 0.1, rnd(g, C, C, k) / (C * k) ** 0.5, rnd(g, C) * 0.1)


@pytest.mark.parametrize("k,dil,B,T", [(k, d, B, T) for k, d in V1_KD for B, T in ((5, 40), (2, 700))]
                         + [pytest.param(k, d, 2, X3_MANY[k, d][0], id=f"{k}-{d}-many-tiles") for k, d in X3_MANY])
def test_resblock_pair_x3(gpu_device, k, dil, B, T):
    """``ResblockPairX3Plan`` (the fused split-format ResBlock step, 32 channels) against ``resblock_step`` in fp64: all nine (k, d) of V1
    with several clips inside one tile (B = 5, T = 40) and with clips spanning tiles (B = 2, T = 700), and one many-tile case per launch
    form of the kernel."""
    _lib.init()
    dev, C = gpu_device, 32
    g = torch.Generator().manual_seed(100 * k + dil + T)
    x = rnd(g, B, T, C)
    w1, b1, w2, b2 = _resblock_weights(g, C, k)
    src, dst = new_map(dev, B, T, C, True, interior=x), new_map(dev, B, T, C, True)
    dst.t.fill_(NAN)
    M, TO = B * src.P, 256 - (k - 1)
    lds = _lib.lib().advh_resblock_pair_x3_lds_bytes(C, k, dil)
    assert lds == G.resblock_pair_x3_lds_bytes(C, k, dil) > 0
    ntiles, grid = walked_tiles(M, TO, 256 * (2 if lds <= 80 * 1024 else 1))     # advh_resblock_pair_x3's launch rule
    many = T > 10000
    if many:
        buf = 2 * ((max(256 + (k - 1) * dil, 272) * 4 + 63) // 64 * 64) * 16     # one split line buffer
        assert (grid, (lds - 4 * k * C * C * 2) // buf) == X3_MANY[k, dil][1:], "not the launch form this case is for"
        assert ntiles > grid and ntiles % grid != 0, (ntiles, grid)
    G.ResblockPairX3Plan(src, dst, w1, b1, w2, b2, dilation=dil, slope=0.1, device=dev).run(src.t, out_h=dst.t)
    torch.cuda.synchronize()
    ref = R.resblock_step(interior(src), w1, b1, w2, b2, dil, 0.1)
    what = f"resblock_pair_x3 k={k} d={dil} B={B} T={T} ({ntiles} tiles on {grid} workgroups)"
    check(what, interior(dst), ref, True, edges((k - 1) * dil // 2 + (k - 1) // 2, T))
    assert halo_is_zero(dst), what
    if many:
        full = torch.zeros(B, src.P, C, dtype=torch.float64)
        full[:, HALO:HALO + T] = ref
        check(what, value(dst.t, True).reshape(1, M, C), full.reshape(1, M, C), True, second_round(M, TO, grid))


# ------------------------------------------------------------------------------------------ 5. the fp16 siblings, many tiles
@pytest.mark.parametrize("C,k,dil,B,T", [(32, 11, 5, 2, 65700), (64, 7, 3, 2, 33000)])
def test_conv_taps_f16_many_tiles(gpu_device, C, k, dil, B, T):
    """``advh_conv_taps_f16`` (weights resident in LDS, double-buffered lines) where a workgroup walks a second tile, with and without
    LeakyReLU inside the line buffer (``pre_slope``), bias + LeakyReLU + residual and the pre-activated second output.  A tile read twice
    or dropped moves outputs by O(1)."""
    _lib.init()
    dev, lib = gpu_device, _lib.lib()
    g = torch.Generator().manual_seed(C + k)
    x, r = rnd(g, B, T, C), rnd(g, B, T, C)
    w, b = rnd(g, C, C, k) / (C * k) ** 0.5, rnd(g, C) * 0.1
    src, res = new_map(dev, B, T, C, False, interior=x), new_map(dev, B, T, C, False, interior=r)
    M, span, pad = B * src.P, (k - 1) * dil, (k - 1) * dil // 2
    tile, lds = lib.advh_conv_taps_tile(C, k, span), lib.advh_conv_taps_lds_bytes(C, k, span)
    per_cu = 4 if lds <= 40 * 1024 else 3 if lds <= 53 * 1024 else 2 if lds <= 80 * 1024 else 1      # advh_conv_taps_f16's launch rule
    ntiles, grid = walked_tiles(M, tile, 256 * per_cu)
    assert tile > 0 and ntiles > grid and ntiles % grid != 0, (ntiles, grid)
    xv, wr = interior(src), w.half().double()
    for pre in (None, 0.3):
        o1, o2 = new_map(dev, B, T, C, False), new_map(dev, B, T, C, False)
        o1.t.fill_(NAN)
        o2.t.fill_(NAN)
        plan = G.plan_conv1d_taps(src, o1, w, b, dilation=dil, act="leaky", slope=0.1, slope2=0.2, device=dev, pre_slope=pre)
        plan.run(src.t, out_h=o1.t, resid=res.t, out_h2=o2.t)
        torch.cuda.synchronize()
        a = xv if pre is None else R.lrelu(xv, float(torch.tensor(pre).half())).half().double()      # activated in fp16, in place
        ref = R.lrelu(R.conv1d_same(a, wr, b, dil), 0.1) + interior(res)
        what = f"conv_taps_f16 C={C} k={k} d={dil} pre_slope={pre} ({ntiles} tiles on {grid} workgroups)"
        full = torch.zeros(B, src.P, C, dtype=torch.float64)
        full[:, HALO:HALO + T] = ref
        for name, m, rf in (("raw", o1, full), ("pre-activated", o2, R.lrelu(full, 0.2))):
            check(f"{what} {name}", interior(m), rf[:, HALO:HALO + T], False, edges(pad, T))
            check(f"{what} {name}", value(m.t, False).reshape(1, M, C), rf.reshape(1, M, C), False, second_round(M, tile, grid))
            assert halo_is_zero(m), (what, name)


@pytest.mark.parametrize("C,k,dil,B,T", [(32, 3, 1, 2, 65200), (64, 3, 5, 2, 32600)])
def test_resblock_pair_f16_many_tiles(gpu_device, C, k, dil, B, T):
    """``advh_resblock_pair_f16`` where a workgroup walks a second tile: 32 channels with one line buffer and two workgroups per CU
    (grid 512), 64 channels with the two-buffer prefetch ring (grid 256).  The reference rounds where the kernel stores fp16: the
    activated input and the intermediate map."""
    _lib.init()
    dev = gpu_device
    g = torch.Generator().manual_seed(C + k + dil)
    x = rnd(g, B, T, C)
    w1, b1, w2, b2 = _resblock_weights(g, C, k)
    src, dst = new_map(dev, B, T, C, False, interior=x), new_map(dev, B, T, C, False)
    dst.t.fill_(NAN)
    assert G.resblock_pair_supported(src, dst, w1, w2, dil)
    M, TO = B * src.P, 256 - (k - 1)
    lds = _lib.lib().advh_resblock_pair_lds_bytes(C, k, dil)
    ntiles, grid = walked_tiles(M, TO, 256 * (2 if lds <= 80 * 1024 else 1))     # advh_resblock_pair_f16's launch rule
    assert grid == (512 if C == 32 else 256) and ntiles > grid and ntiles % grid != 0, (ntiles, grid)
    G.ResblockPairPlan(src, dst, w1, b1, w2, b2, dilation=dil, slope=0.1, device=dev).run(src.t, out_h=dst.t)
    torch.cuda.synchronize()
    xv = interior(src)
    a = R.lrelu(xv, float(torch.tensor(0.1).half())).half().double()
    t = R.lrelu(R.conv1d_same(a, w1.half().double(), b1, dil), 0.1).half().double()
    ref = xv + R.conv1d_same(t, w2.half().double(), b2, 1)
    what = f"resblock_pair_f16 C={C} k={k} d={dil} ({ntiles} tiles on {grid} workgroups)"
    check(what, interior(dst), ref, False, edges((k - 1) * dil // 2 + (k - 1) // 2, T), tol16=TOL_F16_FUSED)
    full = torch.zeros(B, src.P, C, dtype=torch.float64)
    full[:, HALO:HALO + T] = ref
    check(what, value(dst.t, False).reshape(1, M, C), full.reshape(1, M, C), False, second_round(M, TO, grid), tol16=TOL_F16_FUSED)
    assert halo_is_zero(dst), what


# ------------------------------------------------------------------------------------------ 6. conv_post
@pytest.mark.parametrize("T", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("C", [8, 32, 64])
@SPLIT
def test_conv_post(gpu_device, split, C, T):
    """``advh_hifigan_conv_post`` / ``_split`` (Conv1d(C -> 1, k = 7) + tanh, 256 outputs per workgroup) on a map whose halo is random,
    either side of the workgroup boundary.  Per element |err| <= (k C + 2) 2^-24 mass + 2^-21: the first term is the fp32 fma chain of
    k C products and the bias (Higham's gamma_n on mass = sum |w| |x| + |b|; tanh' <= 1), the second allows the device tanhf a few
    ulp on |tanh| <= 1."""
    _lib.init()
    dev, lib, B, k = gpu_device, _lib.lib(), 3, 7
    g = torch.Generator().manual_seed(10 * C + T)
    m = new_map(dev, B, T, C, split, full=rnd(g, B, T + 2 * HALO, C))
    w = rnd(g, 1, C, k) * (0.8 / (k * C) ** 0.5)                    # pre-tanh values of std 0.8: outputs span about +-0.99
    bias = float(np.float32(0.05))
    wd = w[0].t().contiguous().to(dev)                              # [k][C]
    wav = torch.full((B, 1, T), NAN, dtype=torch.float32, device=dev)
    if split:
        _lib.check(lib.advh_hifigan_conv_post_split(m.t.data_ptr(), m.t.stride(0), wd.data_ptr(), bias, wav.data_ptr(), B, C, T, HALO, k, stream()),
                   "advh_hifigan_conv_post_split")
    else:
        _lib.check(lib.advh_hifigan_conv_post(m.t.data_ptr(), wd.data_ptr(), bias, wav.data_ptr(), B, C, T, HALO, k, stream()),
                   "advh_hifigan_conv_post")
    torch.cuda.synchronize()
    p = (k - 1) // 2
    ref, mass = R.conv_post(value(m.t, split)[:, HALO - p:HALO + T + p], w, bias, k)
    got = wav.cpu().double()[:, 0]
    assert bool(torch.isfinite(got).all())
    bound = (k * C + 2) * 2.0 ** -24 * mass + 2.0 ** -21
    ratio = ((got - ref).abs() / bound).max().item()
    print(f"conv_post {'split' if split else 'f16'} C={C} T={T}: worst |err| / bound {ratio:.3f}, max |err| {(got - ref).abs().max():.2e}, "
          f"outputs in [{ref.min():.3f}, {ref.max():.3f}]")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------ 7. MRF mix
def _mix_case(dev, split, shape, slope, seed):
    """Three maps of one sign per element and magnitudes within a factor 2 of a per-element scale, log-uniform over 1e-7 .. 1e2: the sum
    cannot cancel, so the kernel's fp32 roundings stay relative to the result (the bounds below say what the kernel's arithmetic can
    hold, not what cancellation does to any fp32 sum).  Generated on the host, checked on the device (plain torch in fp64): the
    large case has 17 M elements."""
    g = torch.Generator().manual_seed(seed)
    scale = 10.0 ** (torch.rand(shape, generator=g) * 9.0 - 7.0)
    scale = torch.where(torch.rand(shape, generator=g) < 0.5, -scale, scale)
    maps = [pack((scale * (0.5 + 0.5 * torch.rand(shape, generator=g))).float().to(dev), split) for _ in range(3)]
    y = torch.full_like(maps[0], NAN)
    lib, n = _lib.lib(), int(np.prod(shape))
    ptrs = [t.data_ptr() for t in maps + [y]]
    if split:
        assert y.stride(0) == n
        _lib.check(lib.advh_hifigan_mrf_mix_split(*ptrs, slope, n, n, stream()), "advh_hifigan_mrf_mix_split")
    else:
        _lib.check(lib.advh_hifigan_mrf_mix(*ptrs, slope, n, stream()), "advh_hifigan_mrf_mix")
    torch.cuda.synchronize()
    val = (lambda t: G.join_planes(t).double()) if split else (lambda t: t.double())
    ref, got = R.mrf_mix(*(val(t) for t in maps), slope), val(y)
    assert bool(torch.isfinite(got).all())
    # fp16: one rounding to 11 bits (2^-25 absolute where the result is an fp16 subnormal), the fp32 arithmetic in the 2^-10 on top.
    # split: four fp32 roundings (two adds, 1/3, slope) + the 22-bit store; 2^-24 is the absolute floor of test_split_small_magnitudes
    # (2^-25 per stored element) with the same allowance.
    bound = 2.0 ** -21 * ref.abs() + 2.0 ** -24 if split else 2.0 ** -11 * (1 + 2.0 ** -10) * ref.abs() + 2.0 ** -25
    ratio = ((got - ref).abs() / bound).max().item()
    print(f"mrf_mix {'split' if split else 'f16'} {tuple(shape)} slope {slope}: worst |err| / bound {ratio:.3f}; |ref| in "
          f"[{ref.abs().min():.1e}, {ref.abs().max():.1e}]")
    assert ratio <= 1.0 and ref.abs().min().item() < 1e-6 and ref.abs().max().item() > 10.0


@pytest.mark.parametrize("slope", [0.1, 0.01])
@SPLIT
def test_mrf_mix(gpu_device, split, slope):
    """``advh_hifigan_mrf_mix`` / ``_split`` on whole padded maps (B = 2, T = 100, 32 channels)."""
    _lib.init()
    _mix_case(gpu_device, split, (2, 100 + 2 * HALO, 32), slope, 7)


@SPLIT
def test_mrf_mix_grid_stride(gpu_device, split):
    """More than 8192 * 256 * 8 elements per map: the launcher caps the grid at 8192 workgroups and the kernel loops."""
    _lib.init()
    shape = (1, 262216 + 2 * HALO, 64)
    assert int(np.prod(shape)) > 8192 * 256 * 8
    _mix_case(gpu_device, split, shape, 0.1, 8)


# ------------------------------------------------------------------------------------------ 8. halo fill
@pytest.mark.parametrize("pair", [False, True], ids=["plain", "plane-pair"])
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("T", [1, 2, 32, 33, 40])
@pytest.mark.parametrize("mode", [0, 1])
def test_halo_fill(gpu_device, mode, T, C, pair):
    """``advh_halo_fill_f16`` is bit-equal to ``halo_fill``: zeros, or the mirrored interior for as many rows as the clip has
    reflections (T - 1; halo = 32) and zeros beyond; the interior untouched.  A plane pair is 2 B maps of the same geometry."""
    _lib.init()
    B = 3
    g = torch.Generator().manual_seed(T + C)
    t = rnd(g, *((2,) if pair else ()), B, T + 2 * HALO, C).half().to(gpu_device)          # the halo starts as garbage
    before = t.cpu().reshape(-1, T + 2 * HALO, C)
    _lib.check(_lib.lib().advh_halo_fill_f16(t.data_ptr(), before.shape[0], T, C, HALO, mode, stream()), "advh_halo_fill_f16")
    torch.cuda.synchronize()
    want = R.halo_fill(before, T, HALO, mode)
    assert torch.equal(t.cpu().reshape(want.shape), want)
    n = min(HALO, T - 1) if mode else 0
    assert (want[:, :HALO - n] == 0).all() and (want[:, HALO + T + n:] == 0).all() and torch.equal(want[:, HALO:HALO + T], before[:, HALO:HALO + T])


# ------------------------------------------------------------------------------------------ 9. mel packers
@pytest.mark.parametrize("T", [1, 9])
@pytest.mark.parametrize("kernel,pad", [("pack_mel", 0), ("pack_mel_pad", 0), ("pack_mel_pad", 5), ("pack_mel_split", 0), ("pack_mel_split", 5)])
def test_pack_mel(gpu_device, kernel, pad, T):
    """``advh_hifigan_pack_mel`` / ``_pad`` / ``_split``: the gathered (and replicated) frames as ``.half()``, or as the host's
    ``split_planes`` of them (host and device split agree bit for bit: test_split_planes_device_matches_host); the halo is left as it was."""
    _lib.init()
    dev, lib, B, C = gpu_device, _lib.lib(), 2, 80
    split = kernel == "pack_mel_split"
    g = torch.Generator().manual_seed(T + pad)
    mel = rnd(g, B, C, T) * 2.0 - 4.0
    Tp = T + 2 * pad
    out = rnd(g, *((2,) if split else ()), B, Tp + 2 * HALO, C).half().to(dev)               # garbage halo
    out[..., HALO:HALO + Tp, :] = NAN
    before = out.cpu()
    md = mel.to(dev)
    if kernel == "pack_mel":
        rc = lib.advh_hifigan_pack_mel(md.data_ptr(), out.data_ptr(), B, C, T, HALO, stream())
    elif kernel == "pack_mel_pad":
        rc = lib.advh_hifigan_pack_mel_pad(md.data_ptr(), out.data_ptr(), B, C, T, pad, HALO, stream())
    else:
        rc = lib.advh_hifigan_pack_mel_split(md.data_ptr(), out.data_ptr(), out.stride(0), B, C, T, pad, HALO, stream())
    _lib.check(rc, kernel)
    torch.cuda.synchronize()
    want = pack(R.pack_mel(mel, pad), split)
    got = out.cpu()
    assert torch.equal(got[..., HALO:HALO + Tp, :], want)
    assert torch.equal(got[..., :HALO, :], before[..., :HALO, :]) and torch.equal(got[..., HALO + Tp:, :], before[..., HALO + Tp:, :])


# ------------------------------------------------------------------------------------------ 10. end to end against the fp64 oracle
_E2E = {}


def _e2e_case(name):
    """Input, fp64 oracle waveform and E32 = max|oracle_fp32 - oracle_fp64|, computed once per configuration."""
    if name not in _E2E:
        cfg, T, seed = (syn.hifigan_tiny_config(), 9, 9) if name == "tiny" else (syn.HifiganConfig(), 24, 6)
        sd = syn.hifigan_weights(cfg)
        r = np.random.Generator(np.random.PCG64(seed))
        mel = torch.from_numpy(r.normal(-4.0, 2.0, size=(2, cfg.in_channels, T)).astype(np.float32))
        ref64 = hifigan_ref.generator(mel.double(), {k: v.double() for k, v in sd.items()}, cfg)
        e32 = (hifigan_ref.generator(mel, sd, cfg).double() - ref64).abs().max().item()
        _E2E[name] = (cfg, sd, mel, ref64, e32)
    return _E2E[name]


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "gemm-only"])
@pytest.mark.parametrize("name", ["tiny", "v1"])
def test_f32_mode_against_fp64_oracle(gpu_device, name, fuse):
    """The fp32-class vocoder against the oracle run in fp64, bounded by the fp32 oracle's own distance E32 from it:
    max|hip - oracle_fp64| <= 4 E32 -- a factor 2 for the format's unit roundoff (2^-23 of the split format against fp32's 2^-24) and a
    factor 2 for a different summation order.  (The 1e-4 of tests/test_gpu_hifigan.py is about 100 E32.)"""
    cfg, sd, mel, ref64, e32 = _e2e_case(name)
    net = HipHifigan(cfg, sd, gpu_device, fuse=fuse, precision="f32")
    kinds = {type(s.plan).__name__ for s in net._workspace(*mel.shape[::2])["steps"] if s.kind == "gemm"}
    assert ("ResblockPairX3Plan" in kinds) == fuse and ("TapsPlan" in kinds) == fuse
    wav = net.decode_batch(mel.to(gpu_device))
    assert wav.shape == ref64.shape
    err = (wav.cpu().double() - ref64).abs().max().item()
    print(f"hifigan f32 mode {name} fuse={fuse}: max|hip - fp64| {err:.3e}, E32 {e32:.3e}, ratio {err / e32:.2f}")
    assert err <= 4.0 * e32
