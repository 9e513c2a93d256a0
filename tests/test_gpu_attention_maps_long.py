"""Kernel-level suite of csrc/attention_maps_long.hip -- advh_attention_maps_long, advh_attention_bwd_value_long,
advh_rollout_step_long and advh_rollout_relevance_long -- against float64 evaluated on the CPU on the values the kernels read.
Cases, references and the numpy-fp32 restatement behind the row-sum bar: tests/attention_maps_long_cases.py
(tests/test_build_resources_attention_maps_long.py holds them against the compiled instances).

Buffers are those of tests/test_gpu_attention_bwd_long.py: PAD rows of NaN behind qkv and dctx, outputs prefilled with NaN (the
maps) or a NaN bit pattern no arithmetic produces (dqkv) with guard elements behind them, the workspace prefilled with NaN.

Bars, the project's: every returned map 5e-6 of its own max|ref| in both operand formats (the whole-clip maps kernel's bar); dV
5e-6 of max|ref| in split form and 5e-6 + 2^-11 in fp16 (tests/test_gpu_lrp.py); rows of P sum to 1 within max(1e-6, 4 x the
deviation of the numpy-fp32 restatement on the same inputs); rollout 2e-5 of max|ref|.  With frames the reference is each clip
cropped to its own Tv rows, alone.  Every figure is printed in front of its assertion; at T <= 256 the difference to the
whole-clip entries is printed (their softmax is another arithmetic; the rollout kernels are asserted bit-equal there, the tiles
and the k order being the same).

Measured on an MI355X, worst over all cases of a kind.  Maps (bar 5e-6): split random 1.15e-6, ordered 1.47e-6, peaked 5.3e-7,
uniform 4.5e-7, frames 7.4e-7; fp16 operands random 1.01e-6, ordered 9.7e-7, frames 7.9e-7.  Rows of P sum to 1 within 2.6e-7 (bar
1e-6; the numpy-fp32 restatement: 2.2e-7).  dV: split <= 1.23e-6 (bar 5e-6), fp16 <= 4.10e-4 (bar 4.93e-4, the half-ulp of the
store).  Rollout step 1.39e-6, relevance 1.43e-6 (bar 2e-5).  At T <= 256 the maps differ from the whole-clip entry by <= 2.6e-7
(bit-equal up to 128 frames, where there is one key block), dV by <= 6.0e-4 in fp16 (two roundings).  Every bit-identity held.
The gradient form of the peaked input on the peaked maker's own dctx measured 1.75e-4 (numpy fp32: 2.1e-4): an input no fp32
accumulation resolves (attention_maps_long_cases.maps_inputs), so that form runs on the random maker's dctx.
"""
import pytest
import torch

import attention_bwd_long_cases as C
import attention_maps_long_cases as M
import test_gpu_attention_bwd_long as BL
from addvisor_hip import _lib, gemm as G

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NAN = float("nan")
GUARD = 64                                      # fp32 elements behind a map
EINVAL, EUNSUPPORTED = -1, -4
pack, stream = BL.pack, BL.stream


def lo_of(entry, t):
    return 0 if (entry == "f16" or t is None) else t.stride(0)


def workspace(lib, B, T, heads, dev):
    return torch.full((lib.advh_attention_bwd_long_ws_bytes(B, T, heads) // 4,), NAN, dtype=torch.float32, device=dev)


def maps_launch(entry, qkv, dctx, dscale, fuse, frames, B, T, H, heads, dev, whole=False, expect=0):
    """One call of advh_attention_maps_long (``whole``: advh_attention_maps) on packed operands -> the fp32 map on the CPU."""
    _lib.init()
    lib = _lib.lib()
    qd = qkv.to(dev)
    dd = None if dctx is None else dctx.to(dev)
    n = B * T * T * (1 if fuse else heads)
    out = torch.full((n + GUARD,), NAN, dtype=torch.float32, device=dev)
    ws = workspace(lib, B, T, heads, dev)
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device=dev)
    dp = None if dd is None else dd.data_ptr()
    torch.cuda.synchronize()
    lib.advh_split_overflow(1)
    if whole:
        rc = lib.advh_attention_maps(qd.data_ptr(), lo_of(entry, qd), dp, lo_of(entry, dd), dscale, fuse, out.data_ptr(), B, T, H, heads, stream())
    else:
        rc = lib.advh_attention_maps_long(qd.data_ptr(), lo_of(entry, qd), dp, lo_of(entry, dd), dscale, fuse, out.data_ptr(), ws.data_ptr(),
                                          None if fr is None else fr.data_ptr(), B, T, H, heads, stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert lib.advh_split_overflow(1) == 0
    host = out.cpu()
    assert bool(torch.isnan(host[n:]).all()), "elements behind the map were written"
    return host[:n].view((B, T, T) if fuse else (B, heads, T, T))


def value_launch(entry, qkv, dctx, frames, B, T, H, heads, dev, whole=False, expect=0, flag=0):
    """One call of advh_attention_bwd_value_long (``whole``: advh_attention_bwd_value) -> dqkv bit patterns on the CPU."""
    _lib.init()
    lib = _lib.lib()
    qd, dd = qkv.to(dev), dctx.to(dev)
    rows = B * T
    shape = (rows + BL.GUARD, 3 * H) if entry == "f16" else (2, rows + BL.GUARD, 3 * H)
    out = torch.full(shape, BL.FILL, dtype=torch.int16, device=dev).view(torch.float16)
    ws = workspace(lib, B, T, heads, dev)
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lib.advh_split_overflow(1)
    args = (qd.data_ptr(), lo_of(entry, qd), dd.data_ptr(), lo_of(entry, dd), out.data_ptr(), lo_of(entry, out))
    if whole:
        rc = lib.advh_attention_bwd_value(*args, B, T, H, heads, stream())
    else:
        rc = lib.advh_attention_bwd_value_long(*args, ws.data_ptr(), None if fr is None else fr.data_ptr(), B, T, H, heads, stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert lib.advh_split_overflow(1) == flag
    bits = out.cpu().view(torch.int16)
    assert bool((bits[..., rows:, :] == BL.FILL).all()), "guard rows behind dqkv were written"
    return bits[..., :rows, :]


def relerr(got, ref):
    return ((got.double() - ref).abs().max() / (ref.abs().max() + 1e-300)).item()


def check_map(got, ref, what):
    assert torch.isfinite(got).all(), what
    e = relerr(got, ref)
    print(f"attention maps long {what}: rel err {e:.2e} (bar {M.TOL_MAPS:.0e})")
    assert e <= M.TOL_MAPS, (what, e)
    return e


def check_dv(entry, bits, ref_dv, H, what):
    assert bool((bits[..., :2 * H] == 0).all()), (what, "the Q and K thirds are not exactly zero in every plane")
    got = BL.values(entry, bits)[:, 2 * H:]
    assert torch.isfinite(got).all(), what
    e, bar = relerr(got, ref_dv), BL.bar_of(entry)
    print(f"attention bwd value long [{entry}] {what}: rel err dv {e:.2e} (bar {bar:.2e})")
    assert e <= bar, (what, e)
    return got


def variants():
    """(fuse, grad, dscale) of one case: the probabilities and the gradient form at both scales, under every fusion."""
    return [(f, g, s) for f in M.FUSIONS for g, s in ((False, 1.0), (True, M.DSCALES[0]), (True, M.DSCALES[1]))]


def run_maps_case(dev, kind, case):
    entry, T, heads, dm, B = case
    H = heads * dm
    qkv, dctx = M.maps_inputs(kind, entry, T, heads, dm, B)
    ref = M.maps_reference(kind, entry, T, heads, dm, B)
    q, d = pack(qkv, entry), pack(dctx, entry)
    for fuse, grad, dscale in variants():
        got = maps_launch(entry, q, d if grad else None, dscale, fuse, None, B, T, H, heads, dev)
        what = f"[{entry}] {kind} {M.case_id(case)} fuse={fuse} grad={grad} dscale={dscale:g}"
        check_map(got, M.maps_ref(ref, grad, dscale, fuse), what)
        if fuse == 0 and not grad:
            dev_sum = (got.double().sum(-1) - 1.0).abs().max().item()
            bar = M.rowsum_bar(qkv, B, T, heads, dm)
            print(f"  rows of P sum to 1 within {dev_sum:.2e} (bar {bar:.2e})")
            assert dev_sum <= bar, (what, dev_sum, bar)
        if T <= 256 and dscale == 1.0:
            other = maps_launch(entry, q, d if grad else None, dscale, fuse, None, B, T, H, heads, dev, whole=True)
            print(f"  vs the whole-clip entry at T={T}: {relerr(got, other.double()):.2e}")


@pytest.mark.parametrize("case", M.MAPS_CASES, ids=M.case_id)
def test_maps_parity(gpu_device, case):
    run_maps_case(gpu_device, "random", case)


@pytest.mark.parametrize("kind", ["uniform", "peaked", "ordered"])
@pytest.mark.parametrize("entry", M.ENTRIES)
@pytest.mark.parametrize("shape", M.KIND_SHAPES, ids=str)
def test_maps_adversarial(gpu_device, entry, shape, kind):
    """uniform: every probability exactly 1 / T; peaked: row maxima above 0.999 with scores spanning 60; ordered: the running
    maximum of the statistics kernel rises zero times, once and twice and alpha underflows.  The gradient form of the peaked
    input runs on the random maker's dctx (attention_maps_long_cases.maps_inputs says why)."""
    run_maps_case(gpu_device, kind, (entry,) + shape)


@pytest.mark.parametrize("case", M.MAPS_CASES, ids=M.case_id)
def test_value_parity(gpu_device, case):
    entry, T, heads, dm, B = case
    H = heads * dm
    qkv, dctx = C.inputs("random", entry, T, heads, dm, B)
    bits = value_launch(entry, pack(qkv, entry), pack(dctx, entry), None, B, T, H, heads, gpu_device)
    got = check_dv(entry, bits, M.reference("random", entry, T, heads, dm, B)["dv"], H, f"random {M.case_id(case)}")
    if T <= 256:
        other = BL.values(entry, value_launch(entry, pack(qkv, entry), pack(dctx, entry), None, B, T, H, heads, gpu_device, whole=True))
        print(f"  vs the whole-clip entry at T={T}: dv {relerr(got, other[:, 2 * H:]):.2e}")


@pytest.mark.parametrize("kind", ["uniform", "peaked", "ordered"])
@pytest.mark.parametrize("entry", M.ENTRIES)
@pytest.mark.parametrize("shape", M.KIND_SHAPES, ids=str)
def test_value_adversarial(gpu_device, entry, shape, kind):
    T, heads, dm, B = shape
    qkv, dctx = C.inputs(kind, entry, T, heads, dm, B)
    bits = value_launch(entry, pack(qkv, entry), pack(dctx, entry), None, B, T, heads * dm, heads, gpu_device)
    check_dv(entry, bits, M.reference(kind, entry, T, heads, dm, B)["dv"], heads * dm, f"{kind} {shape}")


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("case", M.FRAME_CASES, ids=M.case_id)
def test_frames(gpu_device, case, which):
    """Per-clip lengths at stride 513: frames = T against NULL, NaN / 1e30 past frames[b], a clip against its batch, stride 513
    against stride Tv -- all bit for bit -- exact zeros outside the Tv x Tv block and past Tv, and each clip against fp64 on the
    cropped clip alone; the maps (per head; mean of the gradient form) and the value backward."""
    entry, T, heads, dm, B = case
    frames = M.FRAMES[which]
    H, dev = heads * dm, gpu_device
    qkv, dctx = C.inputs("random", entry, T, heads, dm, B)
    forms = [("P", 0, False), ("GA mean", 1, True), ("GA max", 2, True)]
    for name, fuse, grad in forms:
        run = lambda q, d, fr, B_=B, T_=T: maps_launch(entry, q, d if grad else None, 1.0 / 4096.0, fuse, fr, B_, T_, H, heads, dev)
        eq = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
        full = run(pack(qkv, entry), pack(dctx, entry), None)
        assert eq(run(pack(qkv, entry), pack(dctx, entry), (T,) * B), full), "frames = T differs from frames = NULL"
        got = run(pack(qkv, entry), pack(dctx, entry), frames)
        for garbage in (NAN, float(torch.tensor(1e30).half())):
            other = run(pack(qkv, entry, T, frames, garbage), pack(dctx, entry, T, frames, garbage), frames)
            assert eq(other, got), f"rows past frames[b] = {garbage} changed the map"
        for b, f in enumerate(frames):
            assert bool((got[b, ..., f:, :] == 0).all()) and bool((got[b, ..., :, f:] == 0).all()), (b, "not zero outside the Tv x Tv block")
            rows = slice(b * T, (b + 1) * T)
            alone = run(pack(qkv[rows], entry), pack(dctx[rows], entry), (f,), 1)
            assert eq(alone[0], got[b]), (b, "a clip depends on its batch")
            cq, cd = qkv[b * T:b * T + f], dctx[b * T:b * T + f]
            tight = run(pack(cq, entry), pack(cd, entry), None, 1, f)
            assert eq(tight[0], got[b, ..., :f, :f].contiguous()), (b, f, "stride 513 differs from stride Tv")
            ref = M.maps_ref(M.reference_of(cq, cd, 1, f, heads, dm), grad, 1.0 / 4096.0, fuse)
            check_map(got[b:b + 1, ..., :f, :f], ref, f"frames [{entry}] {name} dm={dm} clip {b} Tv={f}")
    run = lambda q, d, fr, B_=B, T_=T: value_launch(entry, q, d, fr, B_, T_, H, heads, dev)
    full = run(pack(qkv, entry), pack(dctx, entry), None)
    assert torch.equal(run(pack(qkv, entry), pack(dctx, entry), (T,) * B), full)
    got = run(pack(qkv, entry), pack(dctx, entry), frames)
    for garbage in (NAN, float(torch.tensor(1e30).half())):
        assert torch.equal(run(pack(qkv, entry, T, frames, garbage), pack(dctx, entry, T, frames, garbage), frames), got)
    clip = lambda bits, b, lo, hi: bits[..., b * T + lo:b * T + hi, :]
    for b, f in enumerate(frames):
        assert bool((clip(got, b, f, T) == 0).all()), (b, "rows past frames[b] are not exactly zero in every plane")
        rows = slice(b * T, (b + 1) * T)
        assert torch.equal(run(pack(qkv[rows], entry), pack(dctx[rows], entry), (f,), 1), clip(got, b, 0, T)), (b, "a clip depends on its batch")
        cq, cd = qkv[b * T:b * T + f], dctx[b * T:b * T + f]
        assert torch.equal(run(pack(cq, entry), pack(cd, entry), None, 1, f), clip(got, b, 0, f)), (b, f, "stride 513 differs from stride Tv")
        check_dv(entry, clip(got, b, 0, f), M.reference_of(cq, cd, 1, f, heads, dm)["dv"], H, f"frames dm={dm} clip {b} Tv={f}")


@pytest.mark.parametrize("entry", M.ENTRIES)
def test_second_run_and_a_nan_in_one_head(gpu_device, entry):
    """A repeated launch repeats its bits.  One NaN in q of (clip 1, head 0, query 130): with fuse = 0 only that head's row of
    that clip changes; under every fusion the NaN wins that row and nothing else moves.  The value backward: only (clip 1, head 0)."""
    T, heads, dm, B = 273, M.HEADS, 40, 2
    H, dev = heads * dm, gpu_device
    qkv, dctx = C.inputs("random", entry, T, heads, dm, B)
    q, d = pack(qkv, entry), pack(dctx, entry)
    qn = pack(qkv, entry)
    qn[..., T + 130, 3] = NAN
    for fuse in M.FUSIONS:
        for grad in (False, True):
            run = lambda qq: maps_launch(entry, qq, d if grad else None, 1.0, fuse, None, B, T, H, heads, dev)
            clean = run(q)
            assert torch.equal(run(q), clean), "a second run differs"
            dirty = run(qn)
            hit = torch.zeros_like(clean, dtype=torch.bool)
            if fuse == 0:
                hit[1, 0, 130] = True
            else:
                hit[1, 130] = True
            assert bool(torch.isnan(dirty[hit]).all()), (fuse, grad, "the NaN did not win its row")
            assert torch.equal(dirty[~hit], clean[~hit]), (fuse, grad, "the NaN left its row")
    clean = value_launch(entry, q, d, None, B, T, H, heads, dev)
    assert torch.equal(value_launch(entry, q, d, None, B, T, H, heads, dev), clean)
    dirty = value_launch(entry, qn, d, None, B, T, H, heads, dev)
    hit = torch.zeros(B * T, 3 * H, dtype=torch.bool)
    hit[T:, 2 * H:2 * H + dm] = True                                             # dV of (clip 1, head 0)
    keep = ~(hit.expand_as(dirty) if dirty.dim() == 2 else hit[None].expand_as(dirty))
    assert torch.equal(dirty[keep], clean[keep]), "the NaN left its (clip, head)"
    assert bool(torch.isnan(dirty.view(torch.float16)[~keep].float()).any())


def test_value_range_contract(gpu_device):
    """A dV past 65 504 saturates, raises the sticky flag and leaves neither inf nor NaN in a plane (after
    tests/test_gpu_attention_bwd_long.py); the in-range launch of the same shape leaves the flag clear."""
    T, heads, dm, B = 273, 2, 16, 1
    H = heads * dm
    g = torch.Generator().manual_seed(5)
    qkv = G.join_planes(G.split_planes(torch.randn(B * T, 3 * H, generator=g) * 0.7)).double()
    d32 = torch.randn(B * T, H, generator=g)
    value_launch("split", pack(qkv, "split"), pack(d32.double(), "split"), None, B, T, H, heads, gpu_device, flag=0)
    big = d32.clone()
    big[:, 3] = 64000.0
    dctx = G.join_planes(G.split_planes(big)).double()
    ref = M.reference_of(qkv, dctx, B, T, heads, dm)["dv"]
    over = ref.abs() > BL.SPLIT_MAX * (1 + 1e-4)
    assert bool(over.any()) and bool((ref.abs() > BL.SAT_MAX * (1 + 1e-4)).any())
    bits = value_launch("split", pack(qkv, "split"), pack(dctx, "split"), None, B, T, H, heads, gpu_device, flag=1)
    planes = bits.view(torch.float16)
    assert bool(torch.isfinite(planes.float()).all()), "a saturating value left inf or NaN in a plane"
    assert bool((planes[0][:, 2 * H:][over].float().abs() == BL.SPLIT_MAX).all())
    check_dv("split", bits, ref.clamp(-BL.SAT_MAX, BL.SAT_MAX), H, "saturating dV against the clamped reference")


@pytest.mark.parametrize("entry", M.ENTRIES)
def test_refusals_leave_the_outputs_untouched(gpu_device, entry):
    T, B = 16, 1
    for H, heads, rc in ((20, 1, EUNSUPPORTED), (136, 1, EUNSUPPORTED), (40, 3, EINVAL)):
        qkv, dctx = torch.zeros(B * T, 3 * H, dtype=torch.float64), torch.zeros(B * T, H, dtype=torch.float64)
        bits = value_launch(entry, pack(qkv, entry), pack(dctx, entry), None, B, T, H, heads, gpu_device, expect=rc)
        assert bool((bits == BL.FILL).all()), (H, heads)
        out = maps_launch(entry, pack(qkv, entry), pack(dctx, entry), 1.0, 1, None, B, T, H, heads, gpu_device, expect=rc)
        assert bool(torch.isnan(out).all()), (H, heads)


# ----------------------------------------------------------------------------------------------------------- rollout
def rollout_launch(Mx, X, params, frames, dev, whole=False):
    _lib.init()
    lib = _lib.lib()
    B, T = X.shape[0], X.shape[1]
    md, xd = Mx.to(dev).contiguous(), X.to(dev).contiguous()
    y = torch.full((B * T * T + GUARD,), NAN, dtype=torch.float32, device=dev)
    rel = torch.full((B * T + GUARD,), NAN, dtype=torch.float32, device=dev)
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device=dev)
    fp = None if fr is None else fr.data_ptr()
    a, b, g, n = params
    if whole:
        rc = lib.advh_rollout_step(md.data_ptr(), xd.data_ptr(), y.data_ptr(), a, b, g, n, B, T, stream())
        rc2 = lib.advh_rollout_relevance(xd.data_ptr(), rel.data_ptr(), B, T, stream())
    else:
        rc = lib.advh_rollout_step_long(md.data_ptr(), xd.data_ptr(), y.data_ptr(), a, b, g, n, fp, B, T, stream())
        rc2 = lib.advh_rollout_relevance_long(xd.data_ptr(), rel.data_ptr(), fp, B, T, stream())
    torch.cuda.synchronize()
    assert rc == 0 and rc2 == 0, (rc, rc2)
    yh, rh = y.cpu(), rel.cpu()
    assert bool(torch.isnan(yh[B * T * T:]).all()) and bool(torch.isnan(rh[B * T:]).all()), "elements behind an output were written"
    return yh[:B * T * T].view(B, T, T), rh[:B * T].view(B, T)


@pytest.mark.parametrize("params", M.ROLLOUT_PARAMS, ids=str)
@pytest.mark.parametrize("T", M.ROLLOUT_T)
def test_rollout_step_and_relevance(gpu_device, T, params):
    """Both parameter sets, with and without frames, against fp64; NaN outside the Tv x Tv block changes no bit, the block at
    stride T is the block at stride Tv, and at T <= 256 with NULL frames both kernels are bit-equal to the whole-clip ones (the
    same 16 x 64 tiles and chunks of 64, so the same order of summation)."""
    Mx, X = M.rollout_inputs(T)
    B = X.shape[0]
    for frames in (None, M.ROLLOUT_FRAMES[T]):
        y, rel = rollout_launch(Mx, X, params, frames, gpu_device)
        ref_y, ref_r = M.rollout_step_ref(Mx, X, *params, frames=frames), M.rollout_relevance_ref(X, frames)
        ey, er = relerr(y, ref_y), relerr(rel, ref_r)
        print(f"rollout long T={T} {params} frames={frames}: step {ey:.2e} relevance {er:.2e} (bar {M.TOL_ROLLOUT:.0e})")
        assert torch.isfinite(y).all() and torch.isfinite(rel).all()
        assert ey <= M.TOL_ROLLOUT and er <= M.TOL_ROLLOUT
        if frames is None:
            if T <= 256:
                wy, wr = rollout_launch(Mx, X, params, None, gpu_device, whole=True)
                assert torch.equal(y, wy) and torch.equal(rel, wr), "differs from the whole-clip rollout kernels"
            continue
        Mg, Xg = Mx.clone(), X.clone()
        for b, f in enumerate(frames):
            assert bool((y[b, f:] == 0).all()) and bool((y[b, :, f:] == 0).all()) and bool((rel[b, f:] == 0).all())
            Mg[b, f:], Mg[b, :, f:], Xg[b, f:], Xg[b, :, f:] = NAN, NAN, NAN, NAN
            ty, tr = rollout_launch(Mx[b:b + 1, :f, :f], X[b:b + 1, :f, :f], params, None, gpu_device)
            assert torch.equal(ty[0], y[b, :f, :f]) and torch.equal(tr[0], rel[b, :f]), (b, f, "stride T differs from stride Tv")
        gy, gr = rollout_launch(Mg, Xg, params, frames, gpu_device)
        assert torch.equal(gy, y) and torch.equal(gr, rel), "NaN outside the Tv x Tv block changed the result"
