"""Case lists, operand builders and tolerance bars of tests/test_gpu_unet_train_kernels.py, shared with the CPU tests that
check the bars (tests/test_unet_train_ops_ref_cpu.py).  ``ENTRY_CASES`` names every C entry point the GPU file calls.

Operands are built on the CPU as the tensors the kernels are handed: fp16 maps ``[B][H+2PH][W+2PW][C]`` or split plane
pairs (``split_planes``), halos filled with a sentinel; the reference reads the values the kernel reads (``.double()`` of
the fp16 values, ``join_planes`` of a pair).

Tolerance bars of the BatchNorm groups: per value kind, 4 x the error of the fp32 two-pass numpy restatement on the same
inputs against fp64, plus a floor of two fp32 roundings (2^-22) of the magnitudes the quantity is formed from -- without
it a case whose fp32 arithmetic happens to be exact (n = 2 of fp16 values, the constant kind) would demand bit equality with
fp64 from a kernel whose rsqrt is specified to 1 ulp.  The restatement's activation / gradient map is stored in the OUTPUT
format before its error is taken, so that rounding is in the 4 x already; only where that error is exactly 0 does the bar add one
rounding of the format (2^-11 fp16, 2^-22 split) of the largest value.  The one-pass restatement exceeds every such bar on the offset kinds (checked on the CPU)."""
import functools
import zlib

import numpy as np
import torch

import unet_train_ops_ref as R
from addvisor_hip import gemm as G

SLOPE = float(np.float32(0.2))      # the kernels take float arguments: the references use the values they read
EPS = float(np.float32(1e-5))
MOMENTUM = float(np.float32(0.1))
HALO_SENTINEL = 777.0            # finite, and far from every interior value
OUT_SENTINEL = -333.0
BAND = 2.0 ** -20                # LeakyReLU: relative distance of the pre-activation from 0 inside which either branch is accepted
BAND_CAP = 1e-4                  # share of a case's elements that may lie in the band
KINDS = ("N(0,1)", "mu=8", "mu=64", "const 1")
NPART = 1024

# ------------------------------------------------------------------------------------------------------ geometries
# (tag, B, H, W, PH, PW).  RL = 2048 / C row lanes per workgroup: "trip2" has more padded rows than 1024 * RL, so a
# thread's loop takes a second trip; "n2" pins the unbiased factor; "dozens" / "odd" leave most workgroups without a row.
_TRIP2 = {32: (2, 129, 259, 1, 1), 64: (2, 129, 127, 2, 1), 128: (1, 129, 129, 0, 0), 256: (3, 51, 53, 1, 1), 512: (1, 65, 63, 2, 1)}
C_LIST = (32, 64, 128, 256, 512)


def bn_geoms(C):
    return [("n2", 2, 1, 1, 1, 1), ("dozens", 1, 5, 7, 2, 1), ("odd", 2, 3, 5, 0, 0), ("trip2",) + _TRIP2[C]]


for _C in C_LIST:
    _B, _H, _W, _PH, _PW = _TRIP2[_C]
    assert _B * (_H + 2 * _PH) * (_W + 2 * _PW) > NPART * (2048 // _C)

BN_FWD_CASES = [(C,) + g + (fmt,) for C in C_LIST for g in bn_geoms(C) for fmt in ("f16", "split")]
# backward: g as fp16 / fp32 (fp16 z, fp16 dz) or as a split map (everything split); the "offset" kind of g has a per-channel
# mean of a thousand times its fluctuation (fp32 and split only: fp16 cannot carry it, include/addvisor_hip.h)
BN_BWD_CASES = [(C,) + g + (gfmt, gkind) for C in C_LIST for g in bn_geoms(C)
                for gfmt, gkind in (("f16", "plain"), ("f32", "plain"), ("f32", "offset"), ("split", "plain"), ("split", "offset"))
                if g[0] != "trip2" or gkind == "offset" or gfmt == "f16"]
SCATTER_FORMS = ("same", "other_halo", "up21", "up22", "slice")
BN_SCATTER_CASES = [(form, gfmt) for form in SCATTER_FORMS for gfmt in ("f16", "f32", "split")]
COEF_C = (1, 40, 256, 300, 512, 700)


def case_id(c):
    return "-".join(str(x) for x in c)


# ------------------------------------------------------------------------------------------------------ operands
def make_map(inter, PH, PW, fmt, sentinel=HALO_SENTINEL):
    """fp64 interior [B][H][W][C] -> (the CPU tensor the kernel is handed, the fp64 interior values it reads).
    fmt: "f16" | "split" | "f32"."""
    B, H, W, C = inter.shape
    full = np.full((B, H + 2 * PH, W + 2 * PW, C), sentinel, np.float64)
    R.interior(full, PH, PW)[...] = inter
    t = torch.from_numpy(full)
    if fmt == "f32":
        t = t.float()
        return t, R.interior(t.double().numpy(), PH, PW)
    if fmt == "f16":
        t = t.half()
        return t, R.interior(t.double().numpy(), PH, PW)
    t = G.split_planes(t)
    return t, R.interior(G.join_planes(t).double().numpy(), PH, PW)


def joined(t, fmt):
    """fp64 numpy values of a (CPU) tensor in format fmt."""
    return (G.join_planes(t) if fmt == "split" else t).double().numpy()


def bn_values(C, B, H, W, seed):
    """Each channel one value kind, in turn (KINDS)."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, H, W, C))
    z[..., 1::4] += 8.0
    z[..., 2::4] += 64.0
    z[..., 3::4] = 1.0
    return z


def _seed(*key):
    return zlib.crc32("|".join(str(k) for k in key).encode())


def band_of(coef, zi, y):
    """Elements whose fp64 pre-activation lies within BAND of zero relative to |scale z| + |shift|."""
    return np.abs(y) <= BAND * (np.abs(coef[0] * zi) + np.abs(coef[1]))


def kind_max(a, k):
    """max |a| over the channels of kind k (last axis = channel)."""
    s = np.abs(a[..., k::4])
    return float(s.max()) if s.size else 0.0


def quant(a, fmt):
    """fp32 values as the output format stores them."""
    return a.astype(np.float16).astype(np.float64) if fmt == "f16" else R.split_round(a.astype(np.float64))


OUT_Q = {"f16": 2.0 ** -11, "split": 2.0 ** -22, "f32": 2.0 ** -22}


@functools.lru_cache(maxsize=3)
def bn_fwd_data(case):
    C, tag, B, H, W, PH, PW, fmt = case
    for salt in range(8):       # the first seed for which the fp64 reference alone keeps the LeakyReLU band under its cap
        rng = np.random.default_rng(_seed("p", C, tag, salt))
        zt, zi = make_map(bn_values(C, B, H, W, _seed("z", C, tag, salt)), PH, PW, fmt)
        gamma = (1.0 + 0.5 * rng.standard_normal(C)).astype(np.float32)
        beta = rng.standard_normal(C).astype(np.float32)
        coef, var, y, act = R.bn_forward(zi, gamma.astype(np.float64), beta.astype(np.float64), EPS, SLOPE)
        band = band_of(coef, zi, y)
        c64 = coef.astype(np.float32).astype(np.float64)            # the backward cases hand the kernels these fp32 coefficients
        if max(band.mean(), band_of(c64, zi, c64[0] * zi + c64[1]).mean()) <= BAND_CAP:
            break
    d = dict(zt=zt, zi=zi, gamma=gamma, beta=beta, coef=coef, var=var, y=y, act=act, band=band, n=B * H * W, fmt=fmt)
    d["two"] = R.bn_forward_f32_two_pass(zi, gamma, beta, EPS, SLOPE)
    return d


def bn_fwd_errors(d, coef, act):
    """Per kind: the errors of (coef [4][C], activation [B][H][W][C], both fp64 numpy) against the fp64 reference; inside the
    LeakyReLU band either branch of the reference is accepted: the error there is the distance to the nearer of y and slope * y."""
    e = {}
    da = np.where(d["band"], np.minimum(np.abs(act - d["y"]), np.abs(act - SLOPE * d["y"])), np.abs(act - d["act"]))
    for k in range(4):
        for r, name in enumerate(("scale", "shift", "mean", "invstd")):
            e[name, k] = kind_max(coef[r] - d["coef"][r], k)
        e["act", k] = kind_max(da, k)
    return e


def bn_fwd_floor(d):
    scale, shift, mean, invstd = d["coef"]
    sd = np.sqrt(d["var"])
    f = {}
    for k in range(4):
        f["scale", k] = 2.0 ** -22 * kind_max(scale, k)
        f["shift", k] = 2.0 ** -22 * kind_max(np.abs(d["beta"]) + np.abs(mean * scale), k)
        f["mean", k] = 2.0 ** -22 * kind_max(np.abs(mean) + sd, k)
        f["invstd", k] = 2.0 ** -22 * kind_max(invstd, k)
        f["act", k] = 2.0 ** -22 * kind_max(np.abs(scale * d["zi"]) + np.abs(shift), k)
        f["act_exact", k] = OUT_Q[d["fmt"]] * kind_max(d["act"], k)
    return f


def bn_fwd_bars(d):
    """bar[quantity, kind] = 4 x (error of the fp32 two-pass restatement, its activation stored in the output format) + floor."""
    coef2, _, act2 = d["two"]
    e2 = bn_fwd_errors(d, coef2.astype(np.float64), quant(act2, d["fmt"]))
    fl = bn_fwd_floor(d)
    bars = {q: 4.0 * e2[q] + fl[q] for q in e2}
    for k in range(4):      # the restatement's stored activation happens to be exact: one rounding of the output format instead
        if e2["act", k] == 0.0:
            bars["act", k] += fl["act_exact", k]
    return bars, e2


# ------------------------------------------------------------------------------------------------------ backward
def g_values(C, B, H, W, gkind, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((B, H, W, C))
    if gkind == "offset":        # every other group of four channels (so each z kind meets both g kinds): mean = 1000 x fluctuation
        off = (np.arange(C) // 4) % 2 == 1
        g[..., off] = (rng.choice([-1.0, 1.0, 0.5], size=C) * (1.0 + 1e-3 * g))[..., off]
    return g


PROJECT_BAR = {"f16": 4e-3, "f32": 4e-3, "split": 2e-5}     # per-layer bars of tests/test_gpu_unet_train.py, of max|ref|


@functools.lru_cache(maxsize=3)
def bn_bwd_data(case):
    """Operands of a backward case.  The kernels are handed the fp64 reference's forward coefficients rounded to fp32, and the
    reference backward is evaluated on exactly those fp32 values."""
    C, tag, B, H, W, PH, PW, gfmt, gkind = case
    zfmt = "split" if gfmt == "split" else "f16"
    f = bn_fwd_data((C, tag, B, H, W, PH, PW, zfmt))
    gt, gi = make_map(g_values(C, B, H, W, gkind, _seed("g", C, tag, gkind)), PH, PW, gfmt)
    coef32 = f["coef"].astype(np.float32)
    c64 = coef32.astype(np.float64)
    y = c64[0] * f["zi"] + c64[1]
    return dict(zt=f["zt"], zi=f["zi"], gt=gt, gi=gi, coef32=coef32, y=y, band=band_of(c64, f["zi"], y), zfmt=zfmt, gfmt=gfmt,
                n=B * H * W, inv_scale=float(np.float32(1.0 / 64.0)))


BWD_QUANTITIES = ("s1", "s2", "m1", "m2", "dbeta", "dgamma", "dz")


def bn_bwd_refs(d, positive):
    """fp64 reference and fp32 restatement on the branch ``positive`` -> (ref, bars, restatement's errors), each a dict over
    BWD_QUANTITIES x kind.  bar = min(4 x restatement error + floor, the project's per-layer bar x max|ref| of the whole quantity, as
    tests/test_gpu_unet_train.py measures it); the floor of a sum is 2^-22 of its sum of |terms| (signed terms may cancel, their
    roundings do not), that of dz 2^-22 of its three terms' magnitudes (plus one rounding of the map's format where the restatement's error is 0).  Where dz is all
    cancellation -- n = 2 (z^ = +-1, dz = 0 up to eps), a constant channel under the offset g (one LeakyReLU branch, dy^ - m1 = the
    fluctuation: the fp32 rounding of m1 alone is 6e-5 of it) -- no fp32 evaluation meets a bar relative to that channel's own dz;
    the per-layer bar, relative to the map's max, still holds there and is what applies."""
    n, inv = d["n"], d["inv_scale"]

    def flat(r):
        return dict(s1=r["sums"][0], s2=r["sums"][1], m1=r["coef_b"][1], m2=r["coef_b"][2], dbeta=r["dbeta"], dgamma=r["dgamma"], dz=r["dz"])
    r64 = R.bn_backward(d["zi"], d["gi"], d["coef32"], SLOPE, inv, positive)
    r32 = R.bn_backward_f32(d["zi"], d["gi"], d["coef32"], SLOPE, inv, positive)
    ref, f32 = flat(r64), flat(r32)
    f32["dz"] = quant(f32["dz"], d["zfmt"])
    a1, a2 = r64["abs"]
    mag = dict(s1=a1, s2=a2, m1=a1 / n, m2=a2 / n, dbeta=a1 * inv, dgamma=a2 * inv, dz=r64["dz_terms"])
    bars, e2 = {}, {}
    for q in BWD_QUANTITIES:
        for k in range(4):
            e2[q, k] = kind_max(np.asarray(f32[q], np.float64) - ref[q], k)
            fl = 2.0 ** -22 * kind_max(mag[q], k) + (OUT_Q[d["zfmt"]] * kind_max(ref[q], k) if q == "dz" and e2[q, k] == 0.0 else 0.0)
            bars[q, k] = min(4.0 * e2[q, k] + fl, PROJECT_BAR[d["gfmt"]] * float(np.abs(ref[q]).max()))
    return ref, bars, e2


# ------------------------------------------------------------------------------------------------------ transpose_gather
def _taps(n, same_oy):
    return [(1 if same_oy else (t // 3) - (n // 6), (t % 3) - 1) for t in range(n)]


def tr_desc(B, Hg, Wg, GH, GW, Hs, Ws, PHs, PWs, Cs, c0, nC, sy, sx, taps, ld=None, col0=0, rpt=None, r0=0):
    M = B * Hg * Wg
    d = dict(B=B, Hg=Hg, Wg=Wg, GH=GH, GW=GW, H=Hg - 2 * GH, W=Wg - 2 * GW, Hs=Hs, Ws=Ws, PHs=PHs, PWs=PWs, Cs=Cs, c0=c0, nC=nC,
             sy=sy, sx=sx, ntap=len(taps), oy=[t[0] for t in taps] + [0] * (16 - len(taps)), ox=[t[1] for t in taps] + [0] * (16 - len(taps)),
             col0=col0, r0=r0)
    d["ld"] = ld if ld is not None else col0 + (M + 7) // 8 * 8 + 8
    d["rpt"] = rpt if rpt is not None else r0 + nC
    return d


# name -> descriptor.  M % 64 != 0 everywhere; "m8" has M % 8 != 0; B > 1 everywhere but "one".
TR_CASES = {
    "mag1": tr_desc(2, 5, 7, 0, 0, 5, 7, 1, 1, 40, 32, 1, 1, 1, [(0, 0)]),                                 # nC = 1: the magnitude channel
    "c8_m8": tr_desc(3, 3, 7, 0, 0, 3, 7, 2, 1, 8, 0, 8, 1, 1, [(0, 0)]),                                  # M = 63
    "c40_fuse3": tr_desc(2, 5, 9, 0, 0, 5, 9, 1, 1, 40, 0, 40, 1, 1, [(1, -1), (1, 0), (1, 1)], col0=16),  # fused form, col0 > 0
    "c64_tap9": tr_desc(2, 6, 11, 0, 0, 6, 11, 1, 1, 64, 0, 64, 1, 1, _taps(9, False)),                    # one workgroup per tap, M = 132
    "c72_tap15": tr_desc(2, 4, 9, 0, 0, 4, 9, 2, 1, 80, 8, 72, 1, 1, [(kh - 2, kw - 1) for kh in range(5) for kw in range(3)]),
    "c192_r0": tr_desc(2, 3, 5, 0, 0, 3, 5, 1, 1, 192, 0, 192, 1, 1, [(0, 0), (0, 1)], rpt=232, r0=24),      # three slabs; rows between keep
    "c72_s21": tr_desc(2, 9, 7, 2, 1, 10, 5, 1, 1, 72, 0, 72, 2, 1, [(0, 0), (1, 0)]),                      # stride (2,1), grid halo
    "c64_s22": tr_desc(2, 7, 8, 1, 2, 10, 8, 0, 0, 64, 0, 64, 2, 2, [(0, 0), (0, 1), (1, 0), (1, 1)]),      # stride (2,2), grid halo
    "c8_slice_one": tr_desc(1, 5, 13, 0, 0, 5, 13, 1, 1, 24, 8, 8, 1, 1, [(0, -1), (0, 0), (0, 1)], col0=8, rpt=16, r0=4),
}
TR_EINVAL = {
    "ld%8": dict(ld=100), "col0%8": dict(col0=4), "col0+M>ld": dict(col0=16, ld=72), "rpt<r0+nC": dict(r0=8, rpt=40),
    "c0+nC>Cs": dict(c0=8), "ntap>16": dict(ntap=17), "nC%8": dict(nC=12, rpt=40), "c0%8": dict(c0=4, nC=32, rpt=40), "Cs%8": dict(Cs=44),
}


def tr_operands(d, seed):
    """fp16 source with a non-zero halo sentinel, sentinel-filled destination [ntap*rpt][ld]."""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((d["B"], d["Hs"], d["Ws"], d["Cs"]))
    st, _ = make_map(src, d["PHs"], d["PWs"], "f16", sentinel=55.0)
    dst = torch.full((d["ntap"] * d["rpt"], d["ld"]), OUT_SENTINEL, dtype=torch.float16)
    return st, dst


# ------------------------------------------------------------------------------------------------------ head, stem, skip, pack
# (tag, B, H, W, Fq, Tq, PH, PW)
HEAD_CASES = [("min", 1, 2, 1, 3, 2, 0, 0), ("tail", 2, 5, 7, 9, 8, 2, 1), ("trip2", 1, 258, 255, 260, 256, 0, 0)]       # 65790 > 64 * 1024
STEM_CASES = [("min", 1, 2, 1, 3, 2, 2, 1), ("few", 1, 4, 1, 5, 3, 0, 0), ("odd", 2, 6, 7, 9, 8, 2, 1), ("trip2", 2, 128, 132, 130, 133, 0, 0)]  # 16896 > 8 * 1024
SKIP_CASES = [("min", 1, 2, 1, 3, 2, 0, 0), ("odd", 2, 5, 7, 9, 8, 2, 1), ("trip2", 2, 64, 132, 65, 133, 2, 1)]        # 16896 > 8 * 1024
PACK_CASES = [(tag, B, H, W, Fq, Tq, PH, PW, c0) for (tag, B, H, W, Fq, Tq, PH, PW) in HEAD_CASES[:2] for c0 in (0, 32)]
MAG_SENTINEL = 9e3


def make_mag(B, H, W, Fq, Tq, seed):
    """fp32 magnitude [B][Fq][Tq]: |N(0,1)| on the H x W crop, a sentinel outside it."""
    rng = np.random.default_rng(seed)
    m = np.full((B, Fq, Tq), MAG_SENTINEL, np.float32)
    m[:, :H, :W] = np.abs(rng.standard_normal((B, H, W))).astype(np.float32)
    return m


# ------------------------------------------------------------------------------------------------------ coverage
ENTRY_CASES = {
    "advh_bn_partial_count": ["properties"],
    "advh_bn_stats": BN_FWD_CASES, "advh_bn_stats_split": BN_FWD_CASES, "advh_bn_apply": BN_FWD_CASES, "advh_bn_apply_split": BN_FWD_CASES,
    "advh_bn_coef": list(COEF_C),
    "advh_bn_bwd_sums": BN_BWD_CASES, "advh_bn_bwd_sums_split": BN_BWD_CASES, "advh_bn_bwd_coef": BN_BWD_CASES,
    "advh_bn_bwd_apply": BN_BWD_CASES + BN_SCATTER_CASES, "advh_bn_bwd_apply_split": BN_BWD_CASES + BN_SCATTER_CASES,
    "advh_transpose_gather": list(TR_CASES) + list(TR_EINVAL),
    "advh_unet_head": HEAD_CASES, "advh_unet_head_split": HEAD_CASES,
    "advh_unet_head_bwd": HEAD_CASES, "advh_unet_head_bwd_split": HEAD_CASES,
    "advh_unet_head_wgrad": HEAD_CASES, "advh_unet_head_wgrad_split": HEAD_CASES,
    "advh_unet_stem": STEM_CASES, "advh_unet_stem_split": STEM_CASES,
    "advh_unet_stem_wgrad": STEM_CASES, "advh_unet_stem_wgrad_split": STEM_CASES,
    "advh_unet_skip_wgrad": SKIP_CASES, "advh_unet_skip_wgrad_split": SKIP_CASES,
    "advh_unet_pack_x": PACK_CASES, "advh_unet_pack_x_split": PACK_CASES,
}
ENTRY_PATTERNS = ("advh_bn_", "advh_unet_", "advh_transpose_gather")
