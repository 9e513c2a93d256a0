"""Every training kernel of the U-Net mask decoder (csrc/unet_train.hip, csrc/unet_misc.hip) against fp64, called directly
through the C ABI on operands built as tensors -- not through HipUNetTrain, whose 22 layer geometries, near-zero-mean
pre-activations, zero halos and fresh buffers leave the edges below unreached.  References: tests/unet_train_ops_ref.py on the
values the kernel reads; cases and bars: tests/unet_train_kernel_cases.py (checked on the CPU by
tests/test_unet_train_ops_ref_cpu.py).

Conventions: halos that the contract says are never read hold a finite sentinel; every output buffer is pre-filled with a
sentinel and everything a kernel must not write keeps it; every ``partial`` buffer is pre-filled with NaN (a slot a first
stage forgets shows up in the sums) and, for the second launch of the bit-repeatability check, with 1e30.

Bars
  BatchNorm forward / backward     per value kind (N(0,1) | mu = 8 | mu = 64 | constant 1, channel by channel in turn):
                                   4 x the error of the fp32 two-pass numpy restatement + two fp32 roundings of the terms,
                                   backward never looser than the per-layer bars 2e-5 (split) / 4e-3 (fp16) of max|ref|
  LeakyReLU                        either branch where the fp64 pre-activation is within 2^-20 of zero relative to
                                   |scale z| + |shift|; at most 1e-4 of a case's elements
  advh_bn_coef on handed sums      elementwise, from the count of fp32 roundings (test_bn_coef_running_statistics)
  transpose_gather, pack_x (fp16)  bit equality
  head / stem forward              the row kernels' bounds (tests/test_gpu_rowops.py): fp32 and split outputs 5e-6 of max|ref|,
                                   fp16 outputs 2^-11 |ref| + 2^-25 + 5e-6 max|ref| elementwise
  33 / 480 / 288 weight sums       4 x an fp32 numpy restatement + 2^-22 of the sum of |terms|, never looser than 2e-5 / 4e-3 of the
                                   block's max|ref|
"""
import ctypes as C

import numpy as np
import pytest
import torch

import unet_train_kernel_cases as K
import unet_train_ops_ref as R
from addvisor_hip import _lib, gemm as G, unet_train as UT

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL = -1
TOL_KERNEL = 5e-6
NAN = float("nan")
S = K.OUT_SENTINEL
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"worst {k}: {WORST[k][0]:.2e} (bar {WORST[k][1]:.2e})")


def note(key, v, bar):
    """Record the worst value/bar ratio per key, then assert."""
    v, bar = float(v), float(bar)
    if key not in WORST or v * WORST[key][1] >= WORST[key][0] * bar:
        WORST[key] = (v, bar)
    assert v <= bar, (key, v, bar)


def lib():
    return _lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t if dtype is None else t.to(dtype)).cuda()


def full(shape, v, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), v, dtype=dtype, device="cuda")


def geom(B, H, W, Cn, PH, PW):
    return UT.MapGeom(B, H, W, Cn, PH, PW)


def values(t, fmt):
    """fp64 numpy values of a device tensor of format fmt (split: [2, ...] plane pair)."""
    return K.joined(t.cpu(), fmt)


def halo_mask(shape, PH, PW):
    m = np.ones(shape, bool)
    R.interior(m, PH, PW)[...] = False
    return m


def assert_keeps(t, fmt, mask, sentinel=S):
    """Every element of the map under ``mask`` still holds the sentinel (exact in fp16), in each plane."""
    a = t.cpu().float().numpy()
    for plane in (a if fmt == "split" else [a]):
        assert (plane[mask] == sentinel).all()


def twice(launch, outs, partial):
    """E: run ``launch`` with ``partial`` = NaN, then = 1e30; the outputs are bit-identical.  Returns the first outputs."""
    partial.fill_(NAN)
    assert launch() == 0
    first = [o.clone() for o in outs]
    partial.fill_(1e30)
    for o in outs:
        o.fill_(S)
    assert launch() == 0
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "not bit-repeatable, or depends on what partial held"
    return first


def err_f32(out, ref):
    return float(np.abs(out - ref).max() / max(np.abs(ref).max(), 1e-300))


def err_f16(out, ref):
    bound = 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + TOL_KERNEL * np.abs(ref).max()
    return float((np.abs(out - ref) / bound).max())


# ====================================================================================================== A. forward statistics
def bn_stats(z, fmt, gm, partial, sums):
    if fmt == "split":
        return lib().advh_bn_stats_split(z.data_ptr(), z.stride(0), C.byref(gm), partial.data_ptr(), sums.data_ptr(), st())
    return lib().advh_bn_stats(z.data_ptr(), C.byref(gm), partial.data_ptr(), sums.data_ptr(), st())


def bn_apply(z, fmt, gm, coef, a):
    if fmt == "split":
        return lib().advh_bn_apply_split(z.data_ptr(), z.stride(0), C.byref(gm), coef.data_ptr(), K.SLOPE, a.data_ptr(), a.stride(0), st())
    return lib().advh_bn_apply(z.data_ptr(), C.byref(gm), coef.data_ptr(), K.SLOPE, a.data_ptr(), st())


@pytest.mark.parametrize("case", K.BN_FWD_CASES, ids=K.case_id)
def test_bn_forward(gpu_device, case):
    """advh_bn_stats[_split] -> advh_bn_coef -> advh_bn_apply[_split]: sums, coef = [scale | shift | mean | invstd] and the activation
    against fp64, per value kind.  Measured worst value / bar over all cases (MI355X), by quantity:
    see the module's report and DESIGN.md's tolerance table."""
    Cn, tag, B, H, W, PH, PW, fmt = case
    d = K.bn_fwd_data(case)
    bars, _ = K.bn_fwd_bars(d)
    z, gm, n = dev(d["zt"]), geom(B, H, W, Cn, PH, PW), d["n"]
    partial, sums = full(K.NPART * 2 * Cn, NAN, torch.float64), full(2 * Cn + 8, S)            # advh_bn_stats' partials are fp64
    sums, = twice(lambda: bn_stats(z, fmt, gm, partial, sums), [sums], partial)
    sm = sums.cpu().double().numpy()
    assert (sm[2 * Cn:] == S).all()
    zi = d["zi"].reshape(-1, Cn)
    # sums[0..C) = sum z (also the up-convolutions' bias gradient), sums[C..2C) = sum (z - mean)^2: fp64 sums, one fp32 rounding each
    m2 = ((zi - zi.mean(0)) ** 2).sum(0)
    assert (np.abs(sm[:Cn] - zi.sum(0)) <= 2.0 ** -23 * np.abs(zi.sum(0))).all()
    assert (np.abs(sm[Cn:2 * Cn] - m2) <= 2.0 ** -23 * m2).all()
    assert (sm[Cn:2 * Cn] >= 0).all() and (sm[Cn:2 * Cn][3::4] == 0).all(), "a constant channel's variance is exactly 0"
    coef, gamma, beta = full(4 * Cn + 8, S), dev(d["gamma"]), dev(d["beta"])
    rc = lib().advh_bn_coef(sums.data_ptr(), gamma.data_ptr(), beta.data_ptr(), Cn, float(n), K.EPS, K.MOMENTUM,
                            None, None, None, coef.data_ptr(), st())
    assert rc == 0
    a = torch.full_like(z, S)
    assert bn_apply(z, fmt, gm, coef, a) == 0
    torch.cuda.synchronize()
    cf = coef.cpu().double().numpy()
    assert (cf[4 * Cn:] == S).all()
    av = values(a, fmt)
    e = K.bn_fwd_errors(d, cf[:4 * Cn].reshape(4, Cn), R.interior(av, PH, PW))
    for (q, k), v in e.items():
        note(f"A {q:6s} {K.KINDS[k]:7s} {fmt}", v, bars[q, k])
    assert d["band"].mean() <= K.BAND_CAP
    assert_keeps(a, fmt, halo_mask(av.shape, PH, PW))


@pytest.mark.parametrize("Cn", K.COEF_C)
def test_bn_coef_running_statistics(gpu_device, Cn):
    """advh_bn_coef alone on handed sums = [sum z | sum (z - mean)^2], two consecutive calls from non-trivial buffers, against the fp64
    nn.BatchNorm2d update (R.bn_running, pinned to it on the CPU) evaluated on the fp32 values the kernel reads (sums, n, eps, momentum
    as floats).  Bounds, u = 2^-24, counting the fp32 roundings of each formula (an fma only removes one):
      mean   = s0 / n                                  1 rounding                                   u |mean|
      var    = s1 / n                                  1
      invstd = rsqrt(var + eps)                        add 1, halved by the root, + 1 ulp = 2u rsqrt   3u invstd
      scale  = gamma * invstd                          + 1                                          4u |scale|
      shift  = beta - mean * scale                     mean 1 + scale 4 + product 1, + the subtraction   6u |mean scale| + u |shift|
      rmean' = (1 - m) rmean + m mean                  (1 - m) 1, product 1 | mean 1, product 1 | sum 1   4u (|(1-m) rmean| + |m mean|) per call
      rvar'  = (1 - m) rvar + m var n / (n - 1)        var 1, m var 1, n/(n-1) 1, product 1, sum 1     6u (|(1-m) rvar| + |m var_u|) per call
    and the first call's error enters the second times (1 - m): two calls <= 2 x the per-call bound at the larger magnitudes."""
    u = 2.0 ** -24
    rng = np.random.default_rng(100 + Cn)
    gamma, beta = rng.standard_normal(Cn).astype(np.float32), rng.standard_normal(Cn).astype(np.float32)
    rm = rng.standard_normal(Cn).astype(np.float32)
    rv = (0.5 + rng.random(Cn)).astype(np.float32)
    rm_d, rv_d, nbt_d, coef = dev(rm), dev(rv), torch.full((1,), 41, dtype=torch.int64, device="cuda"), full(4 * Cn + 8, S)
    g_d, b_d = dev(gamma), dev(beta)
    rm64, rv64, nbt = rm.astype(np.float64), rv.astype(np.float64), 41
    bound_m, bound_v = np.zeros(Cn), np.zeros(Cn)
    for n in (2.0, 35.0):
        mean_t = rng.standard_normal(Cn) * np.array([1.0, 8.0, 64.0, 1.0])[np.arange(Cn) % 4]
        var_t = (0.5 + rng.random(Cn)) * (np.arange(Cn) % 4 != 3)                       # every fourth channel: variance 0
        sums = np.concatenate([mean_t * n, var_t * n]).astype(np.float32)
        s64 = sums.astype(np.float64)
        mean, var = s64[:Cn] / n, s64[Cn:] / n
        invstd = 1.0 / np.sqrt(var + K.EPS)
        scale = gamma * invstd
        shift = beta - mean * scale
        new_m, new_v, nbt = R.bn_running(rm64, rv64, nbt, mean, var, n, K.MOMENTUM)
        bound_m = np.maximum(bound_m, 4 * u * (np.abs((1 - K.MOMENTUM) * rm64) + np.abs(K.MOMENTUM * mean)))
        bound_v = np.maximum(bound_v, 6 * u * (np.abs((1 - K.MOMENTUM) * rv64) + np.abs(new_v - (1 - K.MOMENTUM) * rv64)))
        rm64, rv64 = new_m, new_v
        coef.fill_(S)
        sums_d = dev(sums)
        rc = lib().advh_bn_coef(sums_d.data_ptr(), g_d.data_ptr(), b_d.data_ptr(), Cn, n, K.EPS, K.MOMENTUM,
                                rm_d.data_ptr(), rv_d.data_ptr(), nbt_d.data_ptr(), coef.data_ptr(), st())
        assert rc == 0
        cf = coef.cpu().double().numpy()
        assert (cf[4 * Cn:] == S).all()
        cf = cf[:4 * Cn].reshape(4, Cn)
        for name, got, ref, bound in (("scale", cf[0], scale, 4 * u * np.abs(scale)), ("mean", cf[2], mean, u * np.abs(mean)),
                                      ("shift", cf[1], shift, 6 * u * np.abs(mean * scale) + u * np.abs(shift)),
                                      ("invstd", cf[3], invstd, 3 * u * invstd)):
            note(f"coef {name} / bound", (np.abs(got - ref) / np.maximum(bound, 1e-300)).max(), 1.0)
        assert int(nbt_d.item()) == nbt
    for name, got, ref, bound in (("running_mean", rm_d, rm64, 2 * bound_m), ("running_var", rv_d, rv64, 2 * bound_v)):
        note(f"coef {name} / bound", (np.abs(got.cpu().double().numpy() - ref) / bound).max(), 1.0)
    # the all-NULL triple updates nothing; one of running_mean / running_var without the other is refused, nothing written
    before = (rm_d.clone(), rv_d.clone(), nbt_d.clone())
    assert lib().advh_bn_coef(sums_d.data_ptr(), g_d.data_ptr(), b_d.data_ptr(), Cn, 35.0, K.EPS, K.MOMENTUM, None, None, None, coef.data_ptr(), st()) == 0
    coef.fill_(S)
    for a, b in ((rm_d, None), (None, rv_d)):
        rc = lib().advh_bn_coef(sums_d.data_ptr(), g_d.data_ptr(), b_d.data_ptr(), Cn, 35.0, K.EPS, K.MOMENTUM, a.data_ptr() if a is not None else None,
                                b.data_ptr() if b is not None else None, nbt_d.data_ptr(), coef.data_ptr(), st())
        assert rc == EINVAL
    torch.cuda.synchronize()
    assert (coef == S).all() and all(torch.equal(x, y) for x, y in zip(before, (rm_d, rv_d, nbt_d)))


# ====================================================================================================== B. backward
def bn_bwd_sums(z, g, d, gm, coef, partial, sums):
    if d["gfmt"] == "split":
        return lib().advh_bn_bwd_sums_split(z.data_ptr(), z.stride(0), g.data_ptr(), g.stride(0), C.byref(gm), coef.data_ptr(), K.SLOPE,
                                            partial.data_ptr(), sums.data_ptr(), st())
    return lib().advh_bn_bwd_sums(z.data_ptr(), g.data_ptr(), int(d["gfmt"] == "f32"), C.byref(gm), coef.data_ptr(), K.SLOPE, partial.data_ptr(),
                                  sums.data_ptr(), st())


def bn_bwd_apply(z, g, d, gm, coef, coef_b, dz, sB, sH, sW, c0, z_lo=None, g_lo=None, dz_lo=None):
    if d["gfmt"] == "split":
        return lib().advh_bn_bwd_apply_split(z.data_ptr(), z.stride(0) if z_lo is None else z_lo, g.data_ptr(), g.stride(0) if g_lo is None else g_lo,
                                             C.byref(gm), coef.data_ptr(), coef_b.data_ptr(), K.SLOPE, dz.data_ptr(),
                                             dz.stride(0) if dz_lo is None else dz_lo, sB, sH, sW, c0, st())
    return lib().advh_bn_bwd_apply(z.data_ptr(), g.data_ptr(), int(d["gfmt"] == "f32"), C.byref(gm), coef.data_ptr(), coef_b.data_ptr(), K.SLOPE,
                                   dz.data_ptr(), sB, sH, sW, c0, st())


def kernel_branch(d, z, gm, coef, PH, PW):
    """The LeakyReLU branch the kernels take: the sign of advh_bn_apply's own value on the same coefficients.  Outside the band it must
    be the fp64 reference's."""
    a = torch.full_like(z, S)
    assert bn_apply(z, d["zfmt"], gm, coef, a) == 0
    act = R.interior(values(a, d["zfmt"]), PH, PW)
    positive = (act > 0) | ((act == 0) & (d["y"] > 0))                  # a positive value below the format's smallest stores as 0
    assert d["band"].mean() <= K.BAND_CAP
    assert ((positive == (d["y"] > 0)) | d["band"]).all(), "LeakyReLU branch differs from fp64 outside the band"
    return positive


def bn_backward_run(d, case_geom, positive_of):
    """sums -> coef_b, dgamma, dbeta checked against fp64; returns what advh_bn_bwd_apply needs."""
    Cn, B, H, W, PH, PW = case_geom
    z, g, gm = dev(d["zt"]), dev(d["gt"]), geom(B, H, W, Cn, PH, PW)
    coef = dev(d["coef32"].ravel())
    positive = positive_of(d, z, gm, coef, PH, PW)
    ref, bars, _ = K.bn_bwd_refs(d, positive)
    partial, sums = full(K.NPART * 2 * Cn, NAN), full(2 * Cn + 8, S)
    sums, = twice(lambda: bn_bwd_sums(z, g, d, gm, coef, partial, sums), [sums], partial)
    coef_b, dgam, dbet = full(3 * Cn + 8, S), full(Cn + 8, S), full(Cn + 8, S)
    assert lib().advh_bn_bwd_coef(sums.data_ptr(), coef.data_ptr(), Cn, float(d["n"]), d["inv_scale"], coef_b.data_ptr(), dgam.data_ptr(),
                                  dbet.data_ptr(), st()) == 0
    torch.cuda.synchronize()
    sm, cb = sums.cpu().double().numpy(), coef_b.cpu().double().numpy()
    assert (sm[2 * Cn:] == S).all() and (cb[3 * Cn:] == S).all() and (dgam[Cn:] == S).all() and (dbet[Cn:] == S).all()
    assert np.array_equal(cb[:Cn], d["coef32"][0].astype(np.float64)), "k1 is the forward scale"
    got = dict(s1=sm[:Cn], s2=sm[Cn:2 * Cn], m1=cb[Cn:2 * Cn], m2=cb[2 * Cn:3 * Cn], dbeta=dbet[:Cn].cpu().double().numpy(),
               dgamma=dgam[:Cn].cpu().double().numpy())
    for q, v in got.items():
        for k in range(4):
            note(f"B {q:6s} {K.KINDS[k]:7s} g={d['gfmt']}", K.kind_max(v - ref[q], k), bars[q, k])
    return z, g, gm, coef, coef_b, ref, bars


@pytest.mark.parametrize("case", K.BN_BWD_CASES, ids=K.case_id)
def test_bn_backward(gpu_device, case):
    """advh_bn_bwd_sums[_split] -> advh_bn_bwd_coef -> advh_bn_bwd_apply[_split] into a dense map of the same halo."""
    Cn, tag, B, H, W, PH, PW, gfmt, gkind = case
    d = K.bn_bwd_data(case)
    z, g, gm, coef, coef_b, ref, bars = bn_backward_run(d, (Cn, B, H, W, PH, PW), kernel_branch)
    dz = torch.full_like(z, S)
    Hp, Wp = H + 2 * PH, W + 2 * PW
    assert bn_bwd_apply(z, g, d, gm, coef, coef_b, dz, Hp * Wp * Cn, Wp * Cn, Cn, (PH * Wp + PW) * Cn) == 0
    torch.cuda.synchronize()
    dv = values(dz, d["zfmt"])
    for k in range(4):
        note(f"B dz     {K.KINDS[k]:7s} g={gfmt}", K.kind_max(R.interior(dv, PH, PW) - ref["dz"], k), bars["dz", k])
    assert_keeps(dz, d["zfmt"], halo_mask(dv.shape, PH, PW))


SCATTER_GEOM = (64, 2, 3, 5, 1, 1)


@pytest.mark.parametrize("form,gfmt", K.BN_SCATTER_CASES)
def test_bn_bwd_apply_scatter_forms(gpu_device, form, gfmt):
    """dz into a dense map of the same / another halo, into the zero-upsampled grid of a stride-(2,1) / (2,2) layer (d_sH, d_sW doubled)
    and into a channel slice of a wider map (d_c0 > 0): targets against fp64, every other element keeps its sentinel."""
    Cn, B, H, W, PH, PW = SCATTER_GEOM
    d = K.bn_bwd_data((Cn, "scatter", B, H, W, PH, PW, gfmt, "plain"))
    z, g, gm, coef, coef_b, ref, bars = bn_backward_run(d, SCATTER_GEOM, kernel_branch)
    sh, sw, Cd, cs, dPH, dPW = {"same": (1, 1, Cn, 0, PH, PW), "other_halo": (1, 1, Cn, 0, 2, 3), "up21": (2, 1, Cn, 0, 1, 1),
                                "up22": (2, 2, Cn, 0, 1, 2), "slice": (1, 1, Cn + 24, 16, 0, 1)}[form]
    Hd, Wd = sh * H + 2 * dPH, sw * W + 2 * dPW
    shape = (B, Hd, Wd, Cd)
    dz = full(((2,) + shape) if d["zfmt"] == "split" else shape, S, torch.float16)
    assert bn_bwd_apply(z, g, d, gm, coef, coef_b, dz, Hd * Wd * Cd, sh * Wd * Cd, sw * Cd, (dPH * Wd + dPW) * Cd + cs) == 0
    torch.cuda.synchronize()
    dv = values(dz, d["zfmt"])
    target = np.zeros(shape, bool)
    target[:, dPH:dPH + sh * H:sh, dPW:dPW + sw * W:sw, cs:cs + Cn] = True
    got = dv[target].reshape(B, H, W, Cn)
    for k in range(4):
        note(f"B dz scatter {K.KINDS[k]:7s} g={gfmt}", K.kind_max(got - ref["dz"], k), bars["dz", k])
    assert_keeps(dz, d["zfmt"], ~target)


def test_bn_einval(gpu_device):
    """A stride or d_c0 that is not a multiple of 8, or a lo-plane distance that is not one, is refused and nothing is written."""
    Cn, B, H, W, PH, PW = SCATTER_GEOM
    gm = geom(B, H, W, Cn, PH, PW)
    Hp, Wp = H + 2 * PH, W + 2 * PW
    for gfmt in ("f16", "split"):
        d = K.bn_bwd_data((Cn, "scatter", B, H, W, PH, PW, gfmt, "plain"))
        z, g, coef, coef_b = dev(d["zt"]), dev(d["gt"]), dev(d["coef32"].ravel()), full(3 * Cn, 0.0)
        dz = torch.full_like(z, S)
        good = [Hp * Wp * Cn, Wp * Cn, Cn, (PH * Wp + PW) * Cn]
        for i in range(4):
            bad = list(good)
            bad[i] += 4
            assert bn_bwd_apply(z, g, d, gm, coef, coef_b, dz, *bad) == EINVAL
        if gfmt == "split":
            lo = z.stride(0)
            for kw in (dict(z_lo=lo + 4), dict(g_lo=lo + 4), dict(dz_lo=lo + 4), dict(z_lo=0), dict(dz_lo=0)):
                assert bn_bwd_apply(z, g, d, gm, coef, coef_b, dz, *good, **kw) == EINVAL
            p64, partial, sums, a = full(K.NPART * 2 * Cn, NAN, torch.float64), full(K.NPART * 2 * Cn, NAN), full(2 * Cn, S), torch.full_like(z, S)
            L = lib()
            assert L.advh_bn_stats_split(z.data_ptr(), lo + 4, C.byref(gm), p64.data_ptr(), sums.data_ptr(), st()) == EINVAL
            assert L.advh_bn_stats_split(z.data_ptr(), lo, C.byref(gm), p64.data_ptr() + 4, sums.data_ptr(), st()) == EINVAL   # misaligned fp64 partials
            assert L.advh_bn_apply_split(z.data_ptr(), lo + 4, C.byref(gm), coef.data_ptr(), K.SLOPE, a.data_ptr(), lo, st()) == EINVAL
            assert L.advh_bn_apply_split(z.data_ptr(), lo, C.byref(gm), coef.data_ptr(), K.SLOPE, a.data_ptr(), lo + 4, st()) == EINVAL
            assert L.advh_bn_bwd_sums_split(z.data_ptr(), lo, g.data_ptr(), lo + 4, C.byref(gm), coef.data_ptr(), K.SLOPE, partial.data_ptr(),
                                            sums.data_ptr(), st()) == EINVAL
            torch.cuda.synchronize()
            assert (sums == S).all() and (a == S).all()
        torch.cuda.synchronize()
        assert (dz == S).all()
    assert lib().advh_bn_partial_count() == K.NPART


# ====================================================================================================== C. transpose_gather
def tr_struct(d):
    td = UT.TransposeDesc(**{k: v for k, v in d.items() if k not in ("oy", "ox")})
    for t in range(16):
        td.oy[t], td.ox[t] = d["oy"][t], d["ox"][t]
    return td


@pytest.mark.parametrize("name", list(K.TR_CASES))
def test_transpose_gather(gpu_device, name):
    """Pure data movement: the destination equals the numpy index restatement bit for bit -- zeros for taps outside the source interior
    although the source halo holds a sentinel; columns between M and ld, rows outside [r0, r0 + nC) of a tap, keep theirs."""
    d = K.TR_CASES[name]
    src, dst = K.tr_operands(d, 50 + len(name))
    want = R.transpose_gather(src.numpy(), d, dst.numpy())
    s_d, d_d = dev(src), dev(dst)
    td = tr_struct(d)
    assert lib().advh_transpose_gather(s_d.data_ptr(), d_d.data_ptr(), C.byref(td), st()) == 0
    torch.cuda.synchronize()
    got = d_d.cpu().numpy()
    assert np.array_equal(got.view(np.int16), want.view(np.int16))


@pytest.mark.parametrize("name", list(K.TR_EINVAL))
def test_transpose_gather_einval(gpu_device, name):
    d = dict(K.tr_desc(2, 5, 9, 0, 0, 5, 9, 1, 1, 40, 0, 40, 1, 1, [(1, -1), (1, 0), (1, 1)], ld=104, rpt=40), **K.TR_EINVAL[name])
    src, dst = K.tr_operands(d, 77)
    s_d, d_d = dev(src), dev(dst)
    td = tr_struct(d)
    assert lib().advh_transpose_gather(s_d.data_ptr(), d_d.data_ptr(), C.byref(td), st()) == EINVAL
    torch.cuda.synchronize()
    assert (d_d == S).all()


# ====================================================================================================== D. head, stem, skip, pack
def fmt_map(inter, PH, PW, fmt):
    t, v = K.make_map(inter, PH, PW, fmt)
    return dev(t), v


def weight_sum_bar(ref, f32, absum, fmt):
    """min(4 x fp32 restatement error + 2^-22 sum |terms|, per-layer bar x max|ref|), the block against its own maximum."""
    e2 = np.abs(f32.astype(np.float64) - ref).max()
    return min(4.0 * e2 + 2.0 ** -22 * absum.max(), K.PROJECT_BAR[fmt] * np.abs(ref).max())


@pytest.mark.parametrize("fmt", ["f16", "split"])
@pytest.mark.parametrize("case", K.HEAD_CASES, ids=K.case_id)
def test_head_forward_backward_wgrad(gpu_device, case, fmt):
    tag, B, H, W, Fq, Tq, PH, PW = case
    rng = np.random.default_rng(K._seed("head", tag))
    total = B * H * W
    y_d, yv = fmt_map(rng.standard_normal((B, H, W, 32)), PH, PW, fmt)
    w32 = (0.3 * rng.standard_normal(32)).astype(np.float32)
    bias = float(np.float32(0.1))
    w_d = dev(w32)
    mask_ref, logit_ref = R.head(yv, w32, bias)
    for with_logits in (True, False):                                    # `logits` NULL: the mask alone
        mask, logits = full(total + 64, S), full(total + 64, S)
        lp = logits.data_ptr() if with_logits else None
        if fmt == "split":
            rc = lib().advh_unet_head_split(y_d.data_ptr(), y_d.stride(0), B, H, W, PH, PW, w_d.data_ptr(), bias, mask.data_ptr(), lp, st())
        else:
            rc = lib().advh_unet_head(y_d.data_ptr(), B, H, W, PH, PW, w_d.data_ptr(), bias, mask.data_ptr(), lp, st())
        assert rc == 0
        torch.cuda.synchronize()
        note(f"D head mask {fmt}", err_f32(mask[:total].cpu().double().numpy(), mask_ref.ravel()), TOL_KERNEL)
        assert (mask[total:] == S).all() and (logits[total:] == S).all()     # the repeated tail lanes write nothing
        if with_logits:
            note(f"D head logits {fmt}", err_f32(logits[:total].cpu().double().numpy(), logit_ref.ravel()), TOL_KERNEL)
        else:
            assert (logits == S).all()
    # backward: dlogit, dy1 (fp16 | fp32 | split) on the kernel's own fp32 mask
    m32 = mask[:total].clone()
    dmask = rng.standard_normal(total).astype(np.float32)
    dm_d = dev(dmask)
    scale = 64.0
    dl_ref, dy_ref = R.head_bwd(dmask, m32.cpu().double().numpy(), w32, scale)
    for dfmt in (("f16", "f32") if fmt == "f16" else ("split",)):
        dlogit = full(total + 64, S)
        planes = (2,) if dfmt == "split" else ()
        dy1 = full(planes + (total + 2, 32), S, torch.float32 if dfmt == "f32" else torch.float16)
        if dfmt == "split":
            rc = lib().advh_unet_head_bwd_split(dm_d.data_ptr(), m32.data_ptr(), w_d.data_ptr(), scale, total, dlogit.data_ptr(), dy1.data_ptr(), dy1.stride(0), st())
        else:
            rc = lib().advh_unet_head_bwd(dm_d.data_ptr(), m32.data_ptr(), w_d.data_ptr(), scale, total, dlogit.data_ptr(), dy1.data_ptr(), int(dfmt == "f32"), st())
        assert rc == 0
        torch.cuda.synchronize()
        assert (dlogit[total:] == S).all()
        note("D head dlogit", err_f32(dlogit[:total].cpu().double().numpy(), dl_ref), TOL_KERNEL)
        assert ((dy1[:, total:] if dfmt == "split" else dy1[total:]) == S).all()
        got = K.joined(dy1.cpu(), dfmt)[:total]
        if dfmt == "f16":
            note("D head dy1 f16", err_f16(got, dy_ref), 1.0)
        else:
            note(f"D head dy1 {dfmt}", err_f32(got, dy_ref), TOL_KERNEL)
    # the 33 sums, y1 dense [total][32]
    y1_d, y1v = fmt_map(rng.standard_normal((1, 1, total, 32)), 0, 0, fmt)
    dl32 = dlogit[:total].clone()
    dlv = dl32.cpu().numpy()
    ref = R.head_wgrad(dlv, y1v)
    y32 = y1v.reshape(-1, 32).astype(np.float32)
    f32 = np.concatenate([np.ascontiguousarray(y32.T) @ dlv, [dlv.sum(dtype=np.float32)]]).astype(np.float32)
    absum = np.concatenate([np.abs(dlv.astype(np.float64)) @ np.abs(y1v.reshape(-1, 32)), [np.abs(dlv).sum(dtype=np.float64)]])
    partial, dw = full(K.NPART * 64, NAN), full(64 + 8, S)
    if fmt == "split":
        launch = lambda: lib().advh_unet_head_wgrad_split(dl32.data_ptr(), y1_d.data_ptr(), y1_d.stride(0), total, partial.data_ptr(), dw.data_ptr(), st())
    else:
        launch = lambda: lib().advh_unet_head_wgrad(dl32.data_ptr(), y1_d.data_ptr(), total, partial.data_ptr(), dw.data_ptr(), st())
    dw, = twice(launch, [dw], partial)
    assert (dw[64:] == S).all()
    note(f"D head 33 sums {fmt}", np.abs(dw[:33].cpu().double().numpy() - ref).max(), weight_sum_bar(ref, f32, absum, fmt))
    if fmt == "split":
        assert lib().advh_unet_head_split(y_d.data_ptr(), y_d.stride(0) + 4, B, H, W, PH, PW, w_d.data_ptr(), bias, mask.data_ptr(), None, st()) == EINVAL
        assert lib().advh_unet_head_bwd_split(dm_d.data_ptr(), m32.data_ptr(), w_d.data_ptr(), scale, total, dlogit.data_ptr(), dy1.data_ptr(), 12, st()) == EINVAL
        assert lib().advh_unet_head_wgrad_split(dl32.data_ptr(), y1_d.data_ptr(), 12, total, partial.data_ptr(), dw.data_ptr(), st()) == EINVAL


@pytest.mark.parametrize("fmt", ["f16", "split"])
@pytest.mark.parametrize("case", K.STEM_CASES, ids=K.case_id)
def test_stem_forward_and_wgrad(gpu_device, case, fmt):
    tag, B, H, W, Fq, Tq, PH, PW = case
    rng = np.random.default_rng(K._seed("stem", tag))
    mag = K.make_mag(B, H, W, Fq, Tq, K._seed("mag", tag))
    wgt, bias = (0.3 * rng.standard_normal((32, 15))).astype(np.float32), rng.standard_normal(32).astype(np.float32)
    mag_d, w_d, b_d = dev(mag), dev(wgt), dev(bias)
    Ho = H // 2
    shape = (B, Ho + 2 * PH, W + 2 * PW, 32)
    out = full(((2,) + shape) if fmt == "split" else shape, S, torch.float16)
    if fmt == "split":
        rc = lib().advh_unet_stem_split(mag_d.data_ptr(), Fq, Tq, B, H, W, w_d.data_ptr(), b_d.data_ptr(), out.data_ptr(), out.stride(0), PH, PW, K.SLOPE, st())
    else:
        rc = lib().advh_unet_stem(mag_d.data_ptr(), Fq, Tq, B, H, W, w_d.data_ptr(), b_d.data_ptr(), out.data_ptr(), PH, PW, K.SLOPE, st())
    assert rc == 0
    torch.cuda.synchronize()
    ref = R.stem(mag, H, W, wgt, bias, K.SLOPE)
    ov = values(out, fmt)
    got = R.interior(ov, PH, PW)
    if fmt == "f16":
        note("D stem f16", err_f16(got, ref), 1.0)
    else:
        note("D stem split", err_f32(got, ref), TOL_KERNEL)
    assert_keeps(out, fmt, halo_mask(shape, PH, PW))
    # odd H is refused, nothing written
    out.fill_(S)
    if fmt == "split":
        rc = lib().advh_unet_stem_split(mag_d.data_ptr(), Fq, Tq, B, H - 1, W, w_d.data_ptr(), b_d.data_ptr(), out.data_ptr(), out.stride(0), PH, PW, K.SLOPE, st())
    else:
        rc = lib().advh_unet_stem(mag_d.data_ptr(), Fq, Tq, B, H - 1, W, w_d.data_ptr(), b_d.data_ptr(), out.data_ptr(), PH, PW, K.SLOPE, st())
    assert rc == EINVAL
    # weight gradient: dz [B][Ho + 2PH][W + 2PW][32] with a sentinel halo
    dz_d, dzv = fmt_map(rng.standard_normal((B, Ho, W, 32)), PH, PW, fmt)
    ref = R.stem_wgrad(dzv, mag, H, W)
    win = R._windows(mag, H, W, 5, 3, 2, 2, 1)
    f32 = np.einsum("bhwc,bhwk->ck", dzv.astype(np.float32), win.astype(np.float32))
    absum = np.einsum("bhwc,bhwk->ck", np.abs(dzv), np.abs(win))
    partial, dw = full(K.NPART * 480, NAN), full(480 + 8, S)
    if fmt == "split":
        launch = lambda: lib().advh_unet_stem_wgrad_split(dz_d.data_ptr(), dz_d.stride(0), Fq, Tq, B, H, W, mag_d.data_ptr(), PH, PW, partial.data_ptr(), dw.data_ptr(), st())
    else:
        launch = lambda: lib().advh_unet_stem_wgrad(dz_d.data_ptr(), Fq, Tq, B, H, W, mag_d.data_ptr(), PH, PW, partial.data_ptr(), dw.data_ptr(), st())
    dw, = twice(launch, [dw], partial)
    assert (dw[480:] == S).all() and (out == S).all()
    note(f"D stem 32x15 sums {fmt}", np.abs(dw[:480].cpu().double().numpy().reshape(32, 15) - ref).max(), weight_sum_bar(ref, f32, absum, fmt))
    dw.fill_(S)
    if fmt == "split":
        rc = lib().advh_unet_stem_wgrad_split(dz_d.data_ptr(), dz_d.stride(0), Fq, Tq, B, H - 1, W, mag_d.data_ptr(), PH, PW, partial.data_ptr(), dw.data_ptr(), st())
    else:
        rc = lib().advh_unet_stem_wgrad(dz_d.data_ptr(), Fq, Tq, B, H - 1, W, mag_d.data_ptr(), PH, PW, partial.data_ptr(), dw.data_ptr(), st())
    torch.cuda.synchronize()
    assert rc == EINVAL and (dw == S).all()


@pytest.mark.parametrize("fmt", ["f16", "split"])
@pytest.mark.parametrize("case", K.SKIP_CASES, ids=K.case_id)
def test_skip_wgrad(gpu_device, case, fmt):
    tag, B, H, W, Fq, Tq, PH, PW = case
    rng = np.random.default_rng(K._seed("skip", tag))
    mag = K.make_mag(B, H, W, Fq, Tq, K._seed("mag", tag))
    mag_d = dev(mag)
    dz_d, dzv = fmt_map(rng.standard_normal((B, H, W, 32)), PH, PW, fmt)
    ref = R.skip_wgrad(dzv, mag, H, W)
    win = R._windows(mag, H, W, 3, 3, 1, 1, 1)
    f32 = np.einsum("bhwc,bhwk->ck", dzv.astype(np.float32), win.astype(np.float32))
    absum = np.einsum("bhwc,bhwk->ck", np.abs(dzv), np.abs(win))
    partial, dw = full(K.NPART * 288, NAN), full(288 + 8, S)
    if fmt == "split":
        launch = lambda: lib().advh_unet_skip_wgrad_split(dz_d.data_ptr(), dz_d.stride(0), Fq, Tq, B, H, W, mag_d.data_ptr(), PH, PW, partial.data_ptr(), dw.data_ptr(), st())
    else:
        launch = lambda: lib().advh_unet_skip_wgrad(dz_d.data_ptr(), Fq, Tq, B, H, W, mag_d.data_ptr(), PH, PW, partial.data_ptr(), dw.data_ptr(), st())
    dw, = twice(launch, [dw], partial)
    assert (dw[288:] == S).all()
    note(f"D skip 32x9 sums {fmt}", np.abs(dw[:288].cpu().double().numpy().reshape(32, 9) - ref).max(), weight_sum_bar(ref, f32, absum, fmt))


@pytest.mark.parametrize("fmt", ["f16", "split"])
@pytest.mark.parametrize("case", K.PACK_CASES, ids=K.case_id)
def test_pack_x(gpu_device, case, fmt):
    """(x, 1, 0, ..., 0) into channels [c0, c0 + 8) of a 40-channel map: the other 32 channels and the halo keep the sentinel."""
    tag, B, H, W, Fq, Tq, PH, PW, c0 = case
    mag = K.make_mag(B, H, W, Fq, Tq, K._seed("mag", tag))
    mag_d = dev(mag)
    shape = (B, H + 2 * PH, W + 2 * PW, 40)
    cat = full(((2,) + shape) if fmt == "split" else shape, S, torch.float16)
    if fmt == "split":
        rc = lib().advh_unet_pack_x_split(mag_d.data_ptr(), Fq, Tq, B, H, W, cat.data_ptr(), cat.stride(0), 40, c0, PH, PW, st())
    else:
        rc = lib().advh_unet_pack_x(mag_d.data_ptr(), Fq, Tq, B, H, W, cat.data_ptr(), 40, c0, PH, PW, st())
    assert rc == 0
    torch.cuda.synchronize()
    cv = values(cat, fmt)
    target = np.zeros(shape, bool)
    R.interior(target, PH, PW)[..., c0:c0 + 8] = True
    want = R.pack_x(mag, H, W, np.zeros(shape), c0, PH, PW)
    if fmt == "f16":
        assert np.array_equal(cv[target], want.astype(np.float16).astype(np.float64)[target])           # a conversion: exact
    else:
        assert (np.abs(cv[target] - want[target]) <= 2.0 ** -22 * np.abs(want[target]) + 2.0 ** -25).all()
    assert_keeps(cat, fmt, ~target)
    bad = dict(C=44, c0=c0), dict(C=40, c0=c0 + 4), dict(C=40, c0=40)
    for b in bad:
        if fmt == "split":
            rc = lib().advh_unet_pack_x_split(mag_d.data_ptr(), Fq, Tq, B, H, W, cat.data_ptr(), cat.stride(0), b["C"], b["c0"], PH, PW, st())
        else:
            rc = lib().advh_unet_pack_x(mag_d.data_ptr(), Fq, Tq, B, H, W, cat.data_ptr(), b["C"], b["c0"], PH, PW, st())
        assert rc == EINVAL


# ====================================================================================================== E. a second clip
@pytest.mark.parametrize("fmt", ["f16", "split"])
def test_first_clip_does_not_depend_on_the_second(gpu_device, fmt):
    """Adding a second, different clip to the batch changes no bit of what bn_apply, bn_bwd_apply and transpose_gather write for the
    first (same coefficients handed to both)."""
    Cn, _, H, W, PH, PW = SCATTER_GEOM
    gfmt = "split" if fmt == "split" else "f32"
    d2 = K.bn_bwd_data((Cn, "scatter", 2, H, W, PH, PW, gfmt, "plain"))
    coef, coef_b = dev(d2["coef32"].ravel()), dev(np.random.default_rng(3).standard_normal(3 * Cn).astype(np.float32))
    outs = []
    bdim = 1 if fmt == "split" else 0
    for B in (1, 2):
        z, g = dev(d2["zt"]).narrow(bdim, 0, B).contiguous(), dev(d2["gt"]).narrow(bdim, 0, B).contiguous()
        gm = geom(B, H, W, Cn, PH, PW)
        a, dz = torch.full_like(z, S), torch.full_like(z, S)
        assert bn_apply(z, fmt, gm, coef, a) == 0
        Hp, Wp = H + 2 * PH, W + 2 * PW
        assert bn_bwd_apply(z, g, d2, gm, coef, coef_b, dz, Hp * Wp * Cn, Wp * Cn, Cn, (PH * Wp + PW) * Cn) == 0
        d = K.tr_desc(B, H, W, 0, 0, H, W, PH, PW, Cn, 0, Cn, 1, 1, [(0, -1), (0, 0), (0, 1)], ld=2 * H * W + 10 + 8 - (2 * H * W + 10) % 8)
        src = z[0] if fmt == "split" else z
        dst = full((3 * Cn, d["ld"]), S, torch.float16)
        td = tr_struct(d)
        assert lib().advh_transpose_gather(src.data_ptr(), dst.data_ptr(), C.byref(td), st()) == 0
        torch.cuda.synchronize()
        outs.append((a.narrow(bdim, 0, 1).clone(), dz.narrow(bdim, 0, 1).clone(), dst[:, :H * W].clone()))
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
