"""The split format's range contract (csrc/device_math.h, include/addvisor_hip.h advh_split_overflow) at every kind of producer:
NaN passes through as NaN planes and leaves the sticky flag clear; |x| > 65504 (+-inf included) saturates to +-65535.98 and
raises the flag; everything the specials cannot reach is bit-identical to the same launch without them.

Every case places the specials (tests/split_contract_ref.py) on the first and the last lane of a conversion vector, in one vector
that holds a NaN next to an out-of-range value, and in a ragged tail where the producer has one.  Expected planes come from
``split_ref``; the set of outputs a special reaches is computed by index arithmetic.  In-range outputs are also held against
an fp64 evaluation of the operation within TOL_KERNEL = 5e-6 of max|ref| (tests/test_gpu_split.py, split GEMM / convolution
kernels; the row kernels here are exact evaluations of the same fp32 arithmetic)."""
import math

import pytest
import torch
import torch.nn.functional as F

from addvisor_hip import _lib, gemm as G
from split_contract_ref import EDGE_IN_RANGE, EDGE_VALUES, same_bits, same_planes, split_ref, split_ref_planes

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_KERNEL = 5e-6
NAN, BIG = float("nan"), 1e5


def _stream():
    return torch.cuda.current_stream().cuda_stream


def flagged(launch) -> bool:
    """Run ``launch`` with the sticky flag cleared first; True iff the launch raised it (read after a synchronisation, or
    reported by the binding's own check at the end of the launch)."""
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


def rel64(got, ref):
    return float((got.double().cpu() - ref.double()).abs().max() / ref.double().abs().max())


def nan_planes(t: torch.Tensor, idx):
    """Write NaN into both planes of the split tensor ``t [2, ...]`` at ``idx`` (a tuple of the remaining dims)."""
    t[(0,) + idx] = NAN
    t[(1,) + idx] = NAN


# ------------------------------------------------------------------------------------------------ advh_split_f32 (C ABI)
@pytest.mark.parametrize("n", [64, 65, 66, 67])
def test_split_f32_kernel_contract(gpu_device, n):
    """store_h_rt<4> on the float4 groups, scalar split_f32 on the n % 4 tail (rowops.hip split_f32_kernel); the Python
    split_planes only takes n % 4 == 0, so the ABI is called directly."""
    _lib.init()
    lib = _lib.lib()
    g = torch.Generator().manual_seed(n)
    base = torch.randn(n, generator=g) * torch.logspace(-9, 4, n)
    tail = list(range(n - n % 4, n))
    lo = (n + 3) // 4 * 4

    def run(x):
        src = x.to(gpu_device).contiguous()
        dst = torch.full((2, lo), 7.0, dtype=torch.float16, device=gpu_device)
        f = flagged(lambda: _lib.check(lib.advh_split_f32(src.data_ptr(), dst.data_ptr(), lo, n, _stream()), "advh_split_f32"))
        return dst[:, :n].cpu(), f

    control, f = run(base)
    assert not f and same_bits(control, split_ref_planes(base))
    # the whole table, mixed lanes: first / last lane of a vector, a NaN next to an out-of-range value, the tail
    cases = {
        "nan only": {0: NAN, 7: NAN, 13: NAN, **{t: NAN for t in tail}},
        "in-range edges": {i + 20: v for i, v in enumerate(EDGE_IN_RANGE)},
        "table": {**{i: v for i, v in enumerate(EDGE_VALUES)}, 32: NAN, 33: BIG, 35: -math.inf, 36: 65520.0, 39: NAN,
                  **({tail[0]: NAN} if tail else {}), **({tail[-1]: -BIG} if len(tail) > 1 else {})},
        "nan next to out-of-range in the tail": {t: (NAN if i % 2 == 0 else BIG) for i, t in enumerate(tail)} or {60: NAN, 61: BIG},
    }
    for name, sp in cases.items():
        x = base.clone()
        for i, v in sp.items():
            x[i] = v
        got, f = run(x)
        hi, lo_, over = split_ref(x)
        assert same_planes(got, torch.stack([hi, lo_])), name
        assert f == bool(over.any()), name
        keep = torch.ones(n, dtype=torch.bool)
        keep[list(sp)] = False
        assert same_bits(got[:, keep], control[:, keep]), name


# ------------------------------------------------------------------------------------------------ HiFi-GAN row kernels
@pytest.mark.parametrize("pad", [0, 2])
def test_pack_mel_split_contract(gpu_device, pad):
    """store_h_rt<1> (hifigan.hip pack_mel_kernel / pack_mel_pad_kernel): every element its own conversion; the halo stays zero."""
    _lib.init()
    lib = _lib.lib()
    B, Cm, T, halo = 2, 80, 23, 32
    Tp = T + 2 * pad
    g = torch.Generator().manual_seed(40 + pad)
    base = torch.randn(B, Cm, T, generator=g) * 3

    def run(mel):
        m = mel.to(gpu_device).contiguous()
        out = torch.zeros(2, B, Tp + 2 * halo, Cm, dtype=torch.float16, device=gpu_device)
        f = flagged(lambda: _lib.check(lib.advh_hifigan_pack_mel_split(m.data_ptr(), out.data_ptr(), out.stride(0), B, Cm, T, pad, halo,
                                                                       _stream()), "advh_hifigan_pack_mel_split"))
        return out.cpu(), f

    def expect(mel):
        idx = (torch.arange(Tp) - pad).clamp(0, T - 1)
        return split_ref_planes(mel[:, :, idx].permute(0, 2, 1))            # [2, B, Tp, C]

    control, f = run(base)
    assert not f and same_bits(control[:, :, halo:halo + Tp], expect(base))
    pos = [(0, 0, 0), (1, Cm - 1, T - 1), (0, 7, T - 1), (1, 0, 0)]          # first / last sample and channel of each clip
    for name, vals in (("nan only", [NAN] * 4), ("table", EDGE_VALUES)):
        mel = base.clone()
        for i, v in enumerate(vals):
            b, c, t = pos[i] if i < len(pos) else (i % B, (5 * i) % Cm, (3 * i) % T)
            mel[b, c, t] = v
        got, f = run(mel)
        assert same_planes(got[:, :, halo:halo + Tp], expect(mel)), name
        assert f == (name == "table"), name
        assert not got[:, :, :halo].any() and not got[:, :, halo + Tp:].any(), name       # both planes of the halo stay zero


def _mix_ref32(a, b, c, slope):
    """The kernel's fp32 arithmetic (hifigan.hip mrf_mix_kernel) on joined planes."""
    v = ((G.join_planes(a) + G.join_planes(b)) + G.join_planes(c)) * torch.tensor(1.0 / 3.0, dtype=torch.float32)
    return torch.where(v > 0, v, slope * v)


def test_mrf_mix_split_contract(gpu_device):
    """store_h_rt<8> (hifigan.hip mrf_mix_kernel): NaN planes in chosen lanes; a = b = c = 65535.98 (an in-format input) mixes
    to a value above 65504."""
    _lib.init()
    lib = _lib.lib()
    n, slope = 8 * 40, 0.1
    g = torch.Generator().manual_seed(3)
    ins = [G.split_planes(torch.randn(n, generator=g) * 4) for _ in range(3)]
    sat = torch.tensor([65504.0, 65504.0], dtype=torch.float16)               # 65504 + 65504 / 2048 = 65535.98

    def run(a, b, c):
        a_, b_, c_ = (t.to(gpu_device).contiguous() for t in (a, b, c))
        y = torch.full((2, n), 9.0, dtype=torch.float16, device=gpu_device)
        f = flagged(lambda: _lib.check(lib.advh_hifigan_mrf_mix_split(a_.data_ptr(), b_.data_ptr(), c_.data_ptr(), y.data_ptr(), slope,
                                                                      n, n, _stream()), "advh_hifigan_mrf_mix_split"))
        return y.cpu(), f

    control, f = run(*ins)
    assert not f and same_bits(control, split_ref_planes(_mix_ref32(*ins, slope)))
    a64 = sum(G.join_planes(t).double() for t in ins) / 3
    assert rel64(G.join_planes(control), torch.where(a64 > 0, a64, slope * a64)) <= TOL_KERNEL
    for name, nans, overs, negs in (("nan only", [0, 15, 23, 39], [], []),
                                    ("overflow only", [], [8, 31, 47], [55]),
                                    ("mixed", [0, 17, 63], [20, 23, 64], [70])):
        a, b, c = (t.clone() for t in ins)
        for i, lane in enumerate(nans):
            nan_planes((a, b, c)[i % 3], (lane,))
        for lane in overs:
            for t in (a, b, c):
                t[:, lane] = sat
        for lane in negs:                                                        # -65535.98 mixes in range after the LeakyReLU
            for t in (a, b, c):
                t[:, lane] = -sat
        got, f = run(a, b, c)
        exp = split_ref_planes(_mix_ref32(a, b, c, slope))
        assert same_planes(got, exp), name
        assert all(math.isnan(float(got[0, i])) and math.isnan(float(got[1, i])) for i in nans), name
        assert all(float(G.join_planes(got[:, i])) == 65535.984375 for i in overs), name
        assert f == bool(overs), name
        keep = torch.ones(n, dtype=torch.bool)
        keep[nans + overs + negs] = False
        assert same_bits(got[:, keep], control[:, keep]), name


# ------------------------------------------------------------------------------------------------ layer norm (VW 4)
def test_layernorm_split_contract(gpu_device):
    """store_h_rt<4> (rowops.hip layernorm_kernel, fp32 rows in, split out): a NaN row; a gamma entry that pushes one channel past
    65504; a NaN gamma entry next to a large one (one 4-channel vector holding both)."""
    _lib.init()
    lib = _lib.lib()
    M, Cn, eps = 6, 64, 1e-5
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(M, Cn, generator=g)
    x0[:, 9] = 6.0 + torch.rand(M, generator=g)
    for c in (8, 9, 13):
        x0[:, c] = 6.0 + torch.rand(M, generator=g)                          # normalised value > 4 in channels 8, 9 and 13
    gamma0, beta0 = 1 + 0.1 * torch.randn(Cn, generator=g), 0.1 * torch.randn(Cn, generator=g)

    def run(x, gamma):
        x_, g_, b_ = (t.to(gpu_device).contiguous() for t in (x, gamma, beta0))
        out = torch.full((2, M, Cn), 5.0, dtype=torch.float16, device=gpu_device)
        f = flagged(lambda: _lib.check(lib.advh_layernorm_split(x_.data_ptr(), 1, Cn, 0, None, Cn, 0, g_.data_ptr(), b_.data_ptr(), None,
                                                                out.data_ptr(), Cn, out.stride(0), M, Cn, eps, 0, _stream()),
                                       "advh_layernorm_split"))
        return out.cpu(), f

    def ref64(x, gamma):
        x = x.double()
        return (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + eps) * gamma.double() + beta0.double()

    control, f = run(x0, gamma0)
    assert not f and rel64(G.join_planes(control), ref64(x0, gamma0)) <= TOL_KERNEL
    for name, row, gam in (("nan row", 2, {}), ("nan in the last row", M - 1, {}), ("overflowing gamma", None, {9: 60000.0}),
                           ("nan gamma next to a large one", None, {12: NAN, 13: 60000.0}), ("overflow on lane 0", None, {8: 60000.0})):
        x, gamma = x0.clone(), gamma0.clone()
        if row is not None:
            x[row, 5] = NAN
        for c, v in gam.items():
            gamma[c] = v
        got, f = run(x, gamma)
        ref = ref64(x, gamma).float()
        reach = torch.zeros(M, Cn, dtype=torch.bool)
        if row is not None:
            reach[row] = True
        for c in gam:
            reach[:, c] = True
        hi, lo, over = split_ref(ref)
        assert (torch.isnan(ref) | over)[reach].all(), name                    # every reached value is NaN or far out of range
        assert same_planes(got[:, reach], torch.stack([hi, lo])[:, reach]), name
        assert f == bool(over.any()) == (60000.0 in gam.values()), name
        assert same_bits(got[:, ~reach], control[:, ~reach]), name


# ------------------------------------------------------------------------------------------------ GEMM epilogues
def _linear_plans(monkeypatch, build):
    wide = build()
    monkeypatch.setattr(G, "WIDE_EPILOGUE", False)
    narrow = build()
    monkeypatch.undo()
    assert wide.desc.wide == 1 and narrow.desc.wide == 0
    return {"wide (VW 8)": wide, "narrow (VW 4)": narrow}


def test_gemm_epilogue_split_contract(gpu_device, monkeypatch):
    """store_h<VW, SPLIT> of gemm.hip in both forms: NaN rows of A (first and last row, the last in a ragged tile), an overflowing
    output column (first lane of a vector), a NaN bias column next to an overflowing one (one vector holding both)."""
    _lib.init()
    M, K, N = 200, 64, 72
    g = torch.Generator().manual_seed(21)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    w[[8, 16, 17]] = 0.0                                                          # these columns are their bias
    b0 = torch.randn(N, generator=g)
    A0 = G.split_planes(a)
    y64 = a.double() @ w.double().T + b0.double()
    nan_rows, over_cols = [0, M - 1, 77], [8, 17]
    b_sp = b0.clone()
    b_sp[8], b_sp[16], b_sp[17] = BIG, NAN, -BIG
    for bias_special in (False, True):
        bias = b_sp if bias_special else b0
        plans_c = _linear_plans(monkeypatch, lambda: G.plan_linear(M, w, b0, device=gpu_device, split=True))
        plans_s = _linear_plans(monkeypatch, lambda: G.plan_linear(M, w, bias, device=gpu_device, split=True))
        for form in plans_c:
            def run(p, A):
                out = torch.full((2, M, N), 3.0, dtype=torch.float16, device=gpu_device)
                f = flagged(lambda: p.run(A.to(gpu_device), out_h=out))
                return out.cpu(), f
            control, f = run(plans_c[form], A0)
            assert not f and rel64(G.join_planes(control), y64) <= TOL_KERNEL, form
            A = A0.clone()
            for r in nan_rows:
                nan_planes(A, (r, 5 + r % 7))
            got, f = run(plans_s[form], A)
            reach = torch.zeros(M, N, dtype=torch.bool)
            reach[nan_rows] = True
            if bias_special:
                reach[:, [8, 16, 17]] = True
            assert torch.isnan(got[:, nan_rows].float()).all(), form
            if bias_special:
                clean = torch.ones(M, dtype=torch.bool)
                clean[nan_rows] = False
                assert torch.isnan(got[:, clean][:, :, 16].float()).all(), form
                assert (G.join_planes(got[:, clean][:, :, 8]) == 65535.984375).all(), form
                assert (G.join_planes(got[:, clean][:, :, 17]) == -65535.984375).all(), form
            assert f == bias_special, form                                       # NaN rows alone leave the flag clear
            assert same_bits(got[:, ~reach], control[:, ~reach]), form


def test_conv2d_split_contract(gpu_device):
    """The GEMM epilogue on split-format maps with a halo (plan_conv2d, as in test_gpu_split.test_split_conv2d): a NaN input pixel
    reaches exactly the 3 x 3 outputs around it; an overflowing output channel saturates and raises the flag; the halo stays zero."""
    _lib.init()
    B, Cin, Cout, H, W = 2, 16, 24, 9, 11
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    w[9] = 0.0
    b0 = torch.randn(Cout, generator=g)
    src = G.FMap(B, H, W, Cin, 1, 1, split=True).alloc(gpu_device)
    planes = G.split_planes(x.permute(0, 2, 3, 1))
    src.t[:, :, 1:1 + H, 1:1 + W] = planes.to(gpu_device)
    ref = F.leaky_relu(F.conv2d(x.double(), w.double(), b0.double(), 1, 1), 0.2).permute(0, 2, 3, 1)

    def run(bias, X):
        dst = G.FMap(B, H, W, Cout, 1, 2, split=True).alloc(gpu_device)
        dst.t.fill_(3.0)
        p = G.plan_conv2d([src], dst, w, bias, device=gpu_device)
        f = flagged(lambda: p.run(X, out_h=dst.t))
        return dst.t.cpu(), f

    control, f = run(b0, src.t)
    assert not f and rel64(G.join_planes(control)[:, 1:1 + H, 2:2 + W], ref) <= TOL_KERNEL
    halo = torch.ones(B, H + 2, W + 4, dtype=torch.bool)
    halo[:, 1:1 + H, 2:2 + W] = False
    X = src.t.clone()
    pix = [(0, 0, W - 1), (1, H - 1, 0), (1, 4, 5)]                               # corners and an interior pixel
    for b, h, w_ in pix:
        nan_planes(X, (b, 1 + h, 1 + w_, 3))
    bsp = b0.clone()
    bsp[9] = BIG
    for name, bias in (("nan only", b0), ("nan + overflowing channel", bsp)):
        got, f = run(bias, X)
        reach = torch.zeros(B, H + 2, W + 4, Cout, dtype=torch.bool)
        for b, h, w_ in pix:
            for dh in (-1, 0, 1):
                for dw in (-1, 0, 1):
                    if 0 <= h + dh < H and 0 <= w_ + dw < W:
                        reach[b, 1 + h + dh, 2 + w_ + dw, :] = True
        assert torch.isnan(got[:, reach].float()).all(), name
        assert same_bits(got[:, halo], torch.zeros_like(got[:, halo])), name     # the halo is written as zeros, NaN or not
        if bias is bsp:
            over = torch.zeros_like(reach)
            over[:, 1:1 + H, 2:2 + W, 9] = True
            over &= ~reach
            assert (G.join_planes(got)[over] == 65535.984375).all(), name
            reach |= over
        assert f == (bias is bsp), name
        assert same_bits(got[:, ~reach], control[:, ~reach]), name


# ------------------------------------------------------------------------------------------------ 1-D line tiles
def _clip_rows(B, T, halo):
    P = T + 2 * halo
    return [(b * P + halo, b * P + halo + T) for b in range(B)]


def _taps_reach(s, B, T, halo, offsets):
    """Map rows (of the [B][T + 2 halo] geometry) whose outputs read row ``s`` through the tap offsets, inside their clip."""
    out = set()
    for lo, hi in _clip_rows(B, T, halo):
        for o in offsets:
            r = s - o
            if lo <= r < hi:
                out.add(r)
    return out


def test_conv_taps_split_contract(gpu_device):
    """advh_conv_taps_split (the 64-channel line tile; store_h_rt<8>): a NaN at the last sample of clip 0, whose neighbour clip shares
    the 256-position tile, reaches exactly the outputs whose taps cover it -- nothing leaks across the clip boundary, the halo stays
    zero; a NaN bias channel next to an overflowing one saturates and flags only the latter."""
    _lib.init()
    B, T, halo, k, dil = 2, 100, 32, 7, 3
    g = torch.Generator().manual_seed(12)
    src, res = (G.Map1D(B, T, 64, halo, split=True).alloc(gpu_device) for _ in range(2))
    xs = torch.randn(B, T, 64, generator=g)
    src.t[:, :, halo:halo + T] = G.split_planes(xs).to(gpu_device)
    res.t[:, :, halo:halo + T] = G.split_planes(torch.randn(B, T, 64, generator=g)).to(gpu_device)
    w = torch.randn(64, 64, k, generator=g) * (0.3 / k ** 0.5)
    w[9] = 0.0
    w[8] = 0.0
    b0 = torch.randn(64, generator=g) * 0.1
    bsp = b0.clone()
    bsp[8], bsp[9] = NAN, BIG
    P = T + 2 * halo
    s = halo + T - 1                                                              # the last sample of clip 0 (map row)
    offs = [j * dil - (k - 1) * dil // 2 for j in range(k)]
    interior = torch.zeros(B * P, dtype=torch.bool)
    for lo, hi in _clip_rows(B, T, halo):
        interior[lo:hi] = True
    ref = F.leaky_relu(F.conv1d(xs.permute(0, 2, 1).double(), w.double(), b0.double(), padding=(k - 1) * dil // 2, dilation=dil), 0.1)

    def run(bias, X, role):
        o1, o2 = (G.Map1D(B, T, 64, halo, split=True).alloc(gpu_device) for _ in range(2))
        if role == "conv1":
            p = G.plan_conv1d_taps(src, o1, w, bias, dilation=dil, act="leaky", slope=0.1, device=gpu_device)
            f = flagged(lambda: p.run(X, out_h=o1.t))
        else:
            p = G.plan_conv1d_taps(src, o1, w, bias, dilation=dil, slope2=0.1, device=gpu_device)
            f = flagged(lambda: p.run(X, out_h=o1.t, resid=res.t, out_h2=o2.t))
        return [o.t.cpu().reshape(2, B * P, 64) for o in (o1, o2)], f

    X = src.t.clone()
    nan_planes(X, (0, s, 5))
    reach = torch.zeros(B * P, 64, dtype=torch.bool)
    reach[sorted(_taps_reach(s, B, T, halo, offs))] = True
    assert reach[halo + T - 1 - 9].any() and not reach[P:].any()
    for role in ("conv1", "conv2"):
        control, f = run(b0, src.t, role)
        assert not f
        if role == "conv1":
            got_ref = G.join_planes(control[0]).reshape(B, P, 64)[:, halo:halo + T]
            assert rel64(got_ref, ref.permute(0, 2, 1)) <= TOL_KERNEL
        for name, bias in (("nan sample", b0), ("nan sample + nan / overflow channels", bsp)):
            outs, f = run(bias, X, role)
            r = reach.clone()
            if bias is bsp:
                r[interior, 8] = True
                r[interior, 9] = True
            for got, ctl in zip(outs, control):
                if role == "conv1" and got is outs[1]:
                    continue
                assert torch.isnan(got[:, reach].float()).all(), (role, name)
                assert not got[:, ~interior].any(), (role, name)                 # halo rows: zeros in both planes
                if bias is bsp:
                    clean = interior & ~reach.any(1)
                    assert torch.isnan(got[:, clean, 8].float()).all(), (role, name)
                    assert (G.join_planes(got[:, clean, 9]) == 65535.984375).all(), (role, name)
                assert same_bits(got[:, ~r], ctl[:, ~r]), (role, name)
            assert f == (bias is bsp), (role, name)


def test_resblock_pair_x3_contract(gpu_device):
    """advh_resblock_pair_x3 (the fused 32-channel ResBlock step): a NaN source sample at the end of clip 0 goes through the re-split of
    the LeakyReLU'd source (split_f32) and conv1 / conv2; it must reach exactly the outputs computed by index arithmetic, leak
    nothing into clip 1 or the halo, and leave the flag clear.  An overflow of conv1's output (a bias of 1e5 in one intermediate
    channel that conv2 does not read) goes through the intermediate re-split: it must raise the flag and change no output."""
    _lib.init()
    B, T, halo, k, dil, slope = 2, 100, 32, 7, 3, 0.1
    g = torch.Generator().manual_seed(13)
    src, dst = (G.Map1D(B, T, 32, halo, split=True).alloc(gpu_device) for _ in range(2))
    xs = torch.randn(B, T, 32, generator=g)
    src.t[:, :, halo:halo + T] = G.split_planes(xs).to(gpu_device)
    w1 = torch.randn(32, 32, k, generator=g) * (0.5 / (32 * k) ** 0.5)
    w2 = torch.randn(32, 32, k, generator=g) * (0.5 / (32 * k) ** 0.5)
    w2[:, 6] = 0.0                                                                # intermediate channel 6 feeds nothing
    b1, b2 = torch.randn(32, generator=g) * 0.1, torch.randn(32, generator=g) * 0.1
    P = T + 2 * halo
    s = halo + T - 1

    def run(bias1, X):
        d = G.Map1D(B, T, 32, halo, split=True).alloc(gpu_device)
        d.t.fill_(0.0)
        p = G.ResblockPairX3Plan(src, d, w1, bias1, w2, b2, dilation=dil, slope=slope, device=gpu_device)
        f = flagged(lambda: p.run(X, out_h=d.t))
        return d.t.cpu().reshape(2, B * P, 32), f

    control, f = run(b1, src.t)
    assert not f
    x64 = xs.permute(0, 2, 1).double()
    h = F.leaky_relu(F.conv1d(F.leaky_relu(x64, slope), w1.double(), b1.double(), padding=(k - 1) * dil // 2, dilation=dil), slope)
    ref = x64 + F.conv1d(h, w2.double(), b2.double(), padding=(k - 1) // 2)
    assert rel64(G.join_planes(control).reshape(B, P, 32)[:, halo:halo + T], ref.permute(0, 2, 1)) <= TOL_KERNEL
    interior = torch.zeros(B * P, dtype=torch.bool)
    for lo, hi in _clip_rows(B, T, halo):
        interior[lo:hi] = True
    # NaN: conv1 rows that read s, then conv2 rows that read any of them (both inside their clip), plus s itself (residual)
    mid = _taps_reach(s, B, T, halo, [j * dil - (k - 1) * dil // 2 for j in range(k)])
    rows = {s} | set().union(*(_taps_reach(m, B, T, halo, [j - (k - 1) // 2 for j in range(k)]) for m in mid))
    reach = torch.zeros(B * P, 32, dtype=torch.bool)
    reach[sorted(rows)] = True
    assert not reach[P:].any() and reach[s - 12].all() and not reach[s - 13].any()
    X = src.t.clone()
    nan_planes(X, (0, s, 11))
    got, f = run(b1, X)
    assert torch.isnan(got[:, reach].float()).all()
    assert not got[:, ~interior].any()                                           # the halo stays zero
    assert same_bits(got[:, ~reach], control[:, ~reach])
    assert not f
    # overflow of the intermediate only
    bo = b1.clone()
    bo[6] = BIG
    got, f = run(bo, src.t)
    assert f
    assert same_bits(got, control)
