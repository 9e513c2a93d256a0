"""CPU-only checks of tests/gemm_desc_ref.py, the fp64 replay of ``advh_gemm_desc`` that tests/test_gpu_gemm_desc.py pins the
kernels to: the replay against torch fp64 on the planners' descriptors and against ``gemm.replay_on_cpu``; the case table
reaches every (kernel instance, epilogue form) pair and every addressing feature; every case tells each single descriptor
mistake apart; and the argument checks of ``advh_gemm_f16`` that precede any launch."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_desc_ref as R
from addvisor_hip import _lib, gemm as G


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)))


def fill(f, x_nchw):
    x = x_nchw.permute(0, 2, 3, 1)
    if f.split:
        f.t = torch.zeros((2, f.B, f.Hp, f.Wp, f.C), dtype=torch.float16)
        f.t[:, :, f.PH:f.PH + f.H, f.PW:f.PW + f.W, :x.shape[3]] = G.split_planes(x)
    else:
        f.t = torch.zeros((f.B, f.Hp, f.Wp, f.C), dtype=torch.float16)
        f.interior()[..., :x.shape[3]] = x.to(torch.float16)
    return f


def replay_plan(plan, A0, A1, out_numel, resid=None):
    """fp64 replay of a planner's plan writing ``out_h``; returns (value, mask)."""
    d = R.desc_fields(plan.desc)
    d.A0, d.A1, d.W, d.ktab, d.bias, d.out_h, d.resid = True, A1 is not None, True, True, plan.bias is not None, True, resid is not None
    bufs = {"A0": A0.reshape(-1).numpy(), "W": plan.w.reshape(-1).numpy(), "ktab": plan.ktab_host}
    if A1 is not None:
        bufs["A1"] = A1.reshape(-1).numpy()
    if plan.bias is not None:
        bufs["bias"] = plan.bias.reshape(-1).numpy()
    if plan.split:
        d.a_lo = [A0.stride(0) // 8, A1.stride(0) // 8 if A1 is not None else 0]
        d.o_lo = out_numel
    rep = R.replay(d, bufs, {"out_h": out_numel}, plan.BN)
    R.audit(rep, {"A0": A0.numel(), "A1": 0 if A1 is None else A1.numel(), "W": plan.w.numel(), "ktab": len(plan.ktab_host),
                  "bias": 0 if plan.bias is None else plan.bias.numel(), "out_h": out_numel * (2 if plan.split else 1)})
    return torch.from_numpy(rep.out["out_h"][0]), torch.from_numpy(rep.out["out_h"][1])


def against_fp32_replay(plan, A0, A1, n, val, mask):
    """Where ``replay_on_cpu`` applies it agrees with the fp64 replay to fp32 rounding, and writes the same elements."""
    old = G.replay_on_cpu(plan, A0, A1, n)
    assert torch.equal(~torch.isnan(old), mask)
    assert torch.allclose(old[mask].double(), val[mask], rtol=1e-5, atol=1e-5)


def test_linear_and_conv1d_against_torch():
    M, K, N = 37, 72, 20
    a, w, b = rnd(M, K).half(), rnd(N, K), rnd(N)
    p = G.plan_linear(M, w, b, act="gelu")
    val, mask = replay_plan(p, a, None, M * N)
    assert mask.all()
    ref = F.gelu(a.double() @ w.half().double().T + b.double())
    assert torch.allclose(val.view(M, N), ref, rtol=0, atol=1e-12)
    against_fp32_replay(p, a, None, M * N, val, mask)
    # overlapping-row Conv1d with written filler rows (window + halo_zero on a one-line grid)
    B, Cin, Cout, k, s, L_in, L_out, P_out, P_in = 2, 16, 24, 3, 2, 21, 10, 12, 24
    x, w, b = rnd(B, Cin, L_in), rnd(Cout, Cin, k), rnd(Cout)
    xin = torch.zeros(B, P_in, Cin, dtype=torch.float16)
    xin[:, :L_in] = x.transpose(1, 2).half()
    p = G.plan_conv1d_cl(B, P_in, P_out, L_out, w, b, s)
    val, mask = replay_plan(p, xin, None, B * P_out * Cout)
    ref = F.gelu(F.conv1d(xin[:, :L_in].double().transpose(1, 2), w.half().double(), b.double(), stride=s)).transpose(1, 2)
    v = val.view(B, P_out, Cout)
    assert mask.all() and torch.allclose(v[:, :L_out], ref, rtol=0, atol=1e-12) and (v[:, L_out:] == 0).all()
    against_fp32_replay(p, xin, None, B * P_out * Cout, val, mask)


@pytest.mark.parametrize("Cins,Cout,k,stride,pad,H,W,halo_in,halo_out", [
    ([8], 12, (3, 3), (1, 1), (1, 1), 6, 5, (1, 1), (1, 1)),
    ([8], 16, (5, 3), (2, 1), (2, 1), 8, 5, (2, 1), (1, 1)),
    ([16], 8, (3, 3), (2, 2), (1, 1), 8, 6, (1, 1), (2, 2)),
    ([16, 8], 8, (3, 3), (1, 1), (1, 1), 4, 6, (1, 1), (1, 1)),
    ([8, 16], 8, (3, 3), (2, 1), (1, 1), 6, 5, (1, 2), (0, 1)),
])
def test_conv2d_against_torch(Cins, Cout, k, stride, pad, H, W, halo_in, halo_out):
    B = 2
    xs = [rnd(B, c, H, W, seed=i) for i, c in enumerate(Cins)]
    w, b = rnd(Cout, sum(Cins), *k) * 0.2, rnd(Cout)
    srcs = [fill(G.FMap(B, H, W, c, *halo_in), x) for c, x in zip(Cins, xs)]
    ref = F.leaky_relu(F.conv2d(torch.cat([x.half().double() for x in xs], 1), w.half().double(), b.double(), stride=stride, padding=pad), 0.25)   # a slope fp32 holds exactly
    Ho, Wo = ref.shape[2:]
    dst = G.FMap(B, Ho, Wo, Cout + 8, *halo_out)                 # the plan writes channels [4, 4 + Cout) of a wider map
    p = G.plan_conv2d(srcs, dst, w, b, stride=stride, padding=pad, dst_c0=4, slope=0.25)
    n = B * dst.Hp * dst.Wp * dst.C
    val, mask = replay_plan(p, srcs[0].t, srcs[1].t if len(srcs) > 1 else None, n)
    v, mk = val.view(B, dst.Hp, dst.Wp, dst.C).clone(), mask.view(B, dst.Hp, dst.Wp, dst.C)
    assert mk[..., 4:4 + Cout].all() and not mk[..., :4].any() and not mk[..., 4 + Cout:].any()
    inner = v[:, dst.PH:dst.PH + Ho, dst.PW:dst.PW + Wo, 4:4 + Cout].permute(0, 3, 1, 2)
    assert torch.allclose(inner, ref, rtol=0, atol=1e-12)
    v[:, dst.PH:dst.PH + Ho, dst.PW:dst.PW + Wo] = 0
    assert (v == 0).all()
    against_fp32_replay(p, srcs[0].t, srcs[1].t if len(srcs) > 1 else None, n, val, mask)


@pytest.mark.parametrize("stride", [(2, 2), (2, 1)])
def test_conv_transpose2d_against_torch(stride):
    """kernel == stride: all sub-pixels in one launch (``n_sub``, stride (2, 2)) or row phases only (stride (2, 1))."""
    B, Cin, Cout, H, W = 2, 16, 8, 3, 4
    x, w, b = rnd(B, Cin, H, W), rnd(Cin, Cout, *stride) * 0.3, rnd(Cout)
    src = fill(G.FMap(B, H, W, Cin, 1, 2), x)
    ref = F.conv_transpose2d(x.half().double(), w.half().double(), b.double(), stride=stride)
    dst = G.FMap(B, H * stride[0], W * stride[1], Cout + 8, 1, 1)
    p = G.plan_convT2d(src, dst, w, b, stride=stride, dst_c0=4)
    assert (p.desc.n_sub > 1) == (stride[1] > 1)
    n = B * dst.Hp * dst.Wp * dst.C
    val, mask = replay_plan(p, src.t, None, n)
    v, mk = val.view(B, dst.Hp, dst.Wp, dst.C), mask.view(B, dst.Hp, dst.Wp, dst.C)
    assert torch.allclose(v[:, 1:1 + dst.H, 1:1 + dst.W, 4:4 + Cout].permute(0, 3, 1, 2), ref, rtol=0, atol=1e-12)
    want = torch.zeros_like(mk)
    want[:, 1:1 + dst.H, 1:1 + dst.W, 4:4 + Cout] = True
    assert torch.equal(mk, want)
    against_fp32_replay(p, src.t, None, n, val, mask)


@pytest.mark.parametrize("r", [2, 8])
def test_conv_transpose1d_phases_against_torch(r):
    B, T, Cc = 2, 13, 16
    x = rnd(B, Cc, T)
    src = G.Map1D(B, T, Cc, 6)
    src.t = torch.zeros(B, src.P, Cc, dtype=torch.float16)
    src.interior()[:] = x.transpose(1, 2).half()
    w, b = rnd(Cc, 8, 2 * r) * 0.2, rnd(8)
    dst = G.Map1D(B, T * r, 8, 5)
    p = G.plan_convT1d(src, dst, w, b, stride=r)
    val, mask = replay_plan(p, src.t, None, B * dst.P * 8)
    ref = F.conv_transpose1d(x.half().double(), w.half().double(), b.double(), stride=r, padding=r // 2)
    v, mk = val.view(B, dst.P, 8), mask.view(B, dst.P, 8)
    assert torch.allclose(v[:, 5:5 + T * r].transpose(1, 2), ref, rtol=0, atol=1e-12)
    assert mk[:, 5:5 + T * r].all() and not mk[:, :5].any() and not mk[:, 5 + T * r:].any()
    against_fp32_replay(p, src.t, None, B * dst.P * 8, val, mask)


@pytest.mark.parametrize("stride,Cb,Cu,Cs,N,Hc,Wc,where", [((2, 2), 16, 8, 8, 8, 3, 4, "coarse"), ((2, 1), 16, 8, 8, 16, 3, 5, "coarse"),
                                                          ((2, 1), 8, 8, 1, 8, 4, 3, "skip")])
def test_fused_upconv_against_torch(stride, Cb, Cu, Cs, N, Hc, Wc, where):
    """ConvTranspose2d -> cat -> Conv2d 3x3 -> LeakyReLU as one two-level batch (``nz_lo``, ``a_sZ2``, ``o_sZ2``, ``z_inner``), on
    split-format maps: the composed weights keep 22 bits, so the three torch fp64 ops are met to 1e-5."""
    B, (sh, sw) = 2, stride
    xb, xs = rnd(B, Cb, Hc, Wc), rnd(B, Cs, Hc * sh, Wc * sw)
    wt, bt = rnd(Cb, Cu, sh, sw) * 0.3, rnd(Cu)
    wc, bc = rnd(N, Cu + Cs, 3, 3) * 0.2, rnd(N)
    cC = G.round_up(Cb, 8) + (8 if where == "coarse" else 0)
    sC = G.round_up(Cs + (1 if where == "skip" else 0), 8)
    coarse = fill(G.FMap(B, Hc, Wc, cC, 1, 2, split=True), xb)
    skip = fill(G.FMap(B, Hc * sh, Wc * sw, sC, 2, 1, split=True), xs)
    ich = G.round_up(Cb, 8) if where == "coarse" else Cs
    G.add_indicator(coarse if where == "coarse" else skip, ich)
    dst = G.FMap(B, Hc * sh, Wc * sw, N, 1, 1, split=True)
    grp = G.plan_upconv2d(coarse, skip, dst, wt, bt, wc, bc, stride=stride, coarse_C=Cb, skip_C=Cs, indicator=(where, ich), slope=0.25)
    p = grp.plans[0]
    assert p.desc.nz == sh * sw and p.desc.nz_lo == sw and p.desc.z_inner == 1
    n = B * dst.Hp * dst.Wp * N
    val, mask = replay_plan(p, coarse.t, skip.t, n)
    xb64, xs64 = G.join_planes(G.split_planes(xb)).double(), G.join_planes(G.split_planes(xs)).double()
    up = F.conv_transpose2d(xb64, wt.double(), bt.double(), stride=stride)
    ref = F.leaky_relu(F.conv2d(torch.cat([up, xs64], 1), wc.double(), bc.double(), padding=1), 0.25)
    v, mk = val.view(B, dst.Hp, dst.Wp, N), mask.view(B, dst.Hp, dst.Wp, N)
    assert torch.allclose(v[:, 1:1 + dst.H, 1:1 + dst.W].permute(0, 3, 1, 2), ref, rtol=0, atol=1e-5)
    want = torch.zeros_like(mk)
    want[:, 1:1 + dst.H, 1:1 + dst.W] = True
    assert torch.equal(mk, want)


# ------------------------------------------------------------------------------------------------ the case table
@pytest.fixture(scope="module")
def prepared():
    """Every case of the table built once on the host: (case, plan, descriptor fields, buffers, planes, numel, replay)."""
    out = {}
    for case in R.CASES:
        plan = R.build_plan(case)
        bufs, tens, planes, numel = R.host_buffers(case, plan)
        d = R.case_desc(case, plan)
        rep = R.replay(d, bufs, planes, case.inst.BN)
        out[case.id] = (case, plan, d, bufs, planes, numel, rep)
    return out


def test_case_ids_are_unique():
    assert len(set(R.CASE_IDS)) == len(R.CASE_IDS)


def test_cases_are_valid_and_stay_inside_their_buffers(prepared):
    """``replay`` asserts the validity rules of the header on every case; ``audit`` the read / write ranges."""
    for case, plan, d, bufs, planes, numel, rep in prepared.values():
        R.audit(rep, numel)
        if case.inst.plain is not None:
            assert R.affine_loader(case.inst, d) == case.inst.plain, case.id
        for o, (val, mask) in rep.out.items():
            assert mask.any() and not mask.all(), (case.id, o)          # something is written and some sentinel is left to check


def test_case_table_reaches_every_form(prepared):
    reached = {name: set() for name in R.INSTANCES}
    for case, plan, d, *_ in prepared.values():
        reached[case.inst.name].add(R.form(case.inst, d))
    assert reached == R.EXPECTED_FORMS
    # the literal count: ten instances, 76 (instance, form) pairs
    assert len(R.EXPECTED_FORMS) == 10 and sum(len(v) for v in R.EXPECTED_FORMS.values()) == 76


GATHERED = {"padding_chunks", "two_sources", "halo_zero", "window", "nz", "nz_lo", "z_inner", "remap_remainder", "sc_ragged", "w_ld", "n_div",
            "n_sub", "phase", "ragged_m", "ragged_n"}
AFFINE = GATHERED - {"two_sources"}                          # the affine-row loader: one source, identity K table


def test_case_table_reaches_every_addressing_feature(prepared):
    seen = {name: set() for name in R.INSTANCES}
    for case, plan, d, *_ in prepared.values():
        seen[case.inst.name] |= R.features(case.inst, d)
    for name, inst in R.INSTANCES.items():
        assert seen[name] >= (AFFINE if inst.plain is True else GATHERED), (name, (AFFINE if inst.plain is True else GATHERED) - seen[name])


MUTATIONS = {"o_sNhi<->o_sNhh", "h0+1", "h1-1", "w0+1", "w1-1", "bit31_cleared", "a_sZ<->a_sZ2", "w_ld->Ktot", "ph_pad+1", "ph_pad-1", "bias_sZ->0",
             "slope2->slope", "drop_wide_permutation"}
SPLIT_MUTATIONS = {"A_lo_planes_dropped", "W_lo_plane_dropped"}


def test_every_case_tells_each_single_mistake_apart(prepared):
    """A mutation of a field the launch uses must move the reference, on some element, by more than the bound the GPU test
    allows there (or change the set of written elements): a kernel making that mistake cannot pass the case.  Mutations of
    fields a launch does not use (``ph_pad`` without phases, ...) cannot change anything and are counted per instance instead:
    every mutation applies to at least one case of every instance whose loader supports the feature.  Split cases must also see
    a lost lo plane of the activations or of the weights: the fp32-class bound has to stay below 2^-11-sized errors."""
    applied = {name: set() for name in R.INSTANCES}
    for case, plan, d, bufs, planes, numel, rep in prepared.values():
        for mname, fn in R.mutations(d):
            d2, bufs2, kw = copy.deepcopy(d), bufs, {}
            if fn == "ktab":
                kt = bufs["ktab"].copy()
                kt[np.nonzero(kt >> 31)[0][0]] &= 0x7FFFFFFF
                bufs2 = dict(bufs, ktab=kt)
            elif fn == "drop_wide":
                kw = {"drop_wide": True}
            elif fn in ("lo_A", "lo_W"):
                bufs2 = dict(bufs)
                for k, lo in ((("A0", d.a_lo[0] * 8), ("A1", d.a_lo[1] * 8)) if fn == "lo_A" else (("W", d.w_lo),)):
                    if k in bufs:
                        bufs2[k] = bufs[k].copy()
                        bufs2[k][lo:] = 0
            else:
                fn(d2)
            applied[case.inst.name].add(mname)
            try:
                rep2 = R.replay(d2, bufs2, planes, case.inst.BN, check=False, ranges=False, **kw)
            except (IndexError, AssertionError):
                continue                                   # the mistake leaves the buffers: told apart
            told = False
            for o, (val, mask) in rep.out.items():
                val2, mask2 = rep2.out[o]
                both = mask & mask2
                told |= bool((mask != mask2).any()) or bool((np.abs(val2 - val)[both] > R.bound(d, rep, o)[both]).any())
            assert told, (case.id, mname)
    for name, inst in R.INSTANCES.items():
        want = MUTATIONS - ({"bit31_cleared", "h0+1", "h1-1"} if inst.plain is True else set())     # one source, one-line grids
        want |= SPLIT_MUTATIONS if inst.split else set()
        assert applied[name] >= want, (name, want - applied[name])


# ------------------------------------------------------------------------------------------------ argument checks
EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


def _refused_desc(**over):
    """A descriptor over host memory that is valid except for ``over``: only ever passed to be refused before any launch."""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    d = G.GemmDesc()
    d.A0 = d.W = d.ktab = d.out_h = p
    d.M, d.N, d.Ktot, d.w_rows, d.Hg, d.Wg, d.h0, d.h1, d.w0, d.w1 = 16, 16, 64, 256, 1, 16, 0, 1, 0, 16
    d.o_sW, d.n_div, d.nz, d.wide = 16, 16, 1, 1
    for k, v in over.items():
        setattr(d, k, v)
    d._keep = buf
    return d


@pytest.mark.parametrize("over", [dict(N=12, n_div=12, w_rows=256), dict(N=24, n_div=12), dict(o_c0=4), dict(o_sB=4), dict(o_sH=12), dict(o_sW=20),
                                  dict(o_sNhi=4), dict(o_sZ=4), dict(o_sNhh=4, n_sub=2), dict(o_sZ2=12)])
@pytest.mark.parametrize("tile,split", [(G.TILE_AUTO, 0), (G.TILE_128x128, 0), (G.TILE_256x64, 0), (G.TILE_256x32, 0), (G.TILE_256x128_W8, 0),
                                        (G.TILE_128x256_W8, 0), (G.TILE_128x128, 1), (G.TILE_256x64, 1), (G.TILE_256x32, 1)])
def test_wide_needs_multiples_of_eight(lib, over, tile, split):
    """include/addvisor_hip.h, ``wide = 1``: N, n_div, o_c0 and every o_s* stride % 8 == 0, checked on the host: a wide lane
    stores 8 consecutive channels, so N % 8 == 4 would write 4 columns past N."""
    d = _refused_desc(split=split, **over)
    assert lib.advh_gemm_f16(C.byref(d), tile, None) == EINVAL


def test_other_refusals_precede_any_launch(lib):
    assert lib.advh_gemm_f16(C.byref(_refused_desc(split=1)), G.TILE_256x128_W8, None) == EUNSUPPORTED      # W8 tiles: fp16 operands only
    assert lib.advh_gemm_f16(C.byref(_refused_desc(split=1)), G.TILE_128x256_W8, None) == EUNSUPPORTED
    assert lib.advh_gemm_f16(C.byref(_refused_desc()), 7, None) == EINVAL
    assert lib.advh_gemm_f16(C.byref(_refused_desc(nz=4, nz_lo=3)), G.TILE_256x128_W8, None) == EINVAL       # nz % nz_lo
    assert lib.advh_gemm_f16(C.byref(_refused_desc(plain=1, ktab_identity=0)), G.TILE_256x64, None) == EINVAL
    assert lib.advh_gemm_f16(C.byref(_refused_desc(plain=1, ktab_identity=1, plain_out=1, w1=15)), G.TILE_256x64, None) == EINVAL
    assert lib.advh_gemm_f16(C.byref(_refused_desc(w_rows=16)), G.TILE_256x32, None) == EINVAL               # w_rows below the tile's BN multiple
