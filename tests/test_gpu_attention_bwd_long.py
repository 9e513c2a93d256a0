"""Kernel-level suite of the streamed attention backward (csrc/attention_bwd_long.hip): the six instances behind
advh_attention_bwd_long_f16 / advh_attention_bwd_long_split, against the float64 ``backward_ops_ref.attention_bwd`` evaluated on
the CPU on the values the kernels read.  Cases, the dispatch mirror and the inputs: tests/attention_bwd_long_cases.py
(tests/test_build_resources_attention_bwd_long.py holds them against the compiled instances and asserts the inputs' preconditions).

Buffers.  qkv and dctx have PAD rows of NaN behind them (per plane for the split entry).  dqkv is prefilled with a NaN bit pattern
no arithmetic produces and has GUARD rows behind it: every element of the rows must lose the pattern, every guard row keeps it.  The
statistics workspace is prefilled with NaN.  After every in-range launch the sticky range flag (advh_split_overflow) is clear.

Bars, the project's: split entry 5e-6 of the maximum of dq, dk and dv each; f16 entry 5e-6 + 2^-11, the one extra rounding of the
store (every product of both entries runs on the fp32-input matrix instruction).  With frames, the reference is each clip cropped to
its own Tv rows, alone.  Every figure is printed in front of its assertion; at T <= 256 the difference to the whole-clip entry
points is printed (bit-identity is not required: their arithmetic is another).

Worst rel err per instance (both kernels of a padded head dim D) over all its cases, measured on an MI355X: split D = 32 1.92e-6
(peaked), D = 64 1.34e-6 (ordered), D = 128 2.72e-6 (ordered); random inputs <= 1.15e-6, frames <= 1.11e-6, uniform <= 7.5e-7.  fp16
entry <= 4.74e-4 at every D (the half-ulp of the store).  Against the whole-clip entries at T <= 256: split <= 1.05e-6, fp16
<= 9.8e-4 (two fp16 roundings).  Every bit-identity held.  With the scaled score left to the compiler's contraction (one fma where
the product is not needed on its own) the ordered input measured dq 7.38e-6 at D = 128: csrc/attention_bwd_long.hip, bwl_score.
"""

import pytest
import torch

import attention_bwd_long_cases as C
from addvisor_hip import _lib, gemm as G

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PAD, GUARD = 16, 4
FILL = 0x7DAB                                   # an fp16 NaN whose payload neither the inputs nor any arithmetic carry
NAN = float("nan")
EINVAL, EUNSUPPORTED = -1, -4
SPLIT_MAX, SAT_MAX = 65504.0, 65504.0 + 65504.0 / 2048.0


def stream():
    return torch.cuda.current_stream().cuda_stream


def pack(vals, entry, T=None, frames=None, garbage=NAN):
    """float64 rows -> operand tensor on the CPU with PAD rows of NaN behind; rows >= frames[b] of clip b = garbage (every plane)."""
    rows, width = vals.shape
    if entry == "f16":
        t = torch.full((rows + PAD, width), NAN, dtype=torch.float16)
        t[:rows] = vals.half()
    else:
        t = torch.full((2, rows + PAD, width), NAN, dtype=torch.float16)
        t[:, :rows] = G.split_planes(vals)
    for b, f in enumerate(frames or ()):
        t[..., b * T + f:(b + 1) * T, :] = garbage
    return t


def launch(entry, qkv, dctx, frames, B, T, H, heads, dev, whole=False, expect=0, flag=0):
    """One call of the long entry (``whole``: of the whole-clip entry, T <= 256, no frames) on packed operands.  -> dqkv rows
    [.., B*T, 3H] on the CPU as int16 bit patterns, after checking the return code, the guard rows and the range flag."""
    _lib.init()
    lib = _lib.lib()
    qd, dd = qkv.to(dev), dctx.to(dev)
    rows = B * T
    shape = (rows + GUARD, 3 * H) if entry == "f16" else (2, rows + GUARD, 3 * H)
    out = torch.full(shape, FILL, dtype=torch.int16, device=dev).view(torch.float16)
    ws = torch.full((lib.advh_attention_bwd_long_ws_bytes(B, T, heads) // 4,), NAN, dtype=torch.float32, device=dev)
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device=dev)
    fp = None if fr is None else fr.data_ptr()
    torch.cuda.synchronize()
    lib.advh_split_overflow(1)
    if entry == "f16":
        rc = lib.advh_attention_bwd_f16(qd.data_ptr(), dd.data_ptr(), out.data_ptr(), B, T, H, heads, stream()) if whole else \
            lib.advh_attention_bwd_long_f16(qd.data_ptr(), dd.data_ptr(), out.data_ptr(), ws.data_ptr(), fp, B, T, H, heads, stream())
    else:
        rc = lib.advh_attention_bwd_split(qd.data_ptr(), qd.stride(0), dd.data_ptr(), dd.stride(0), out.data_ptr(), out.stride(0),
                                          B, T, H, heads, stream()) if whole else \
            lib.advh_attention_bwd_long_split(qd.data_ptr(), qd.stride(0), dd.data_ptr(), dd.stride(0), out.data_ptr(), out.stride(0),
                                              ws.data_ptr(), fp, B, T, H, heads, stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert lib.advh_split_overflow(1) == flag
    bits = out.cpu().view(torch.int16)
    assert bool((bits[..., rows:, :] == FILL).all()), "guard rows behind dqkv were written"
    return bits[..., :rows, :]


def values(entry, bits):
    """float64 [rows, 3H] of dqkv bit patterns; every element must have been written."""
    assert not bool((bits == FILL).any()), "an element of dqkv was not written"
    t = bits.contiguous().view(torch.float16)
    return t.double() if entry == "f16" else t[0].double() + t[1].double() / 2048.0


def bar_of(entry):
    return C.TOL_F16 if entry == "f16" else C.TOL_SPLIT


def check(entry, got, ref_rows, H, what):
    assert torch.isfinite(got).all(), what
    errs = C.third_errors(got, ref_rows, H)
    print(f"attention bwd long [{entry}] {what}: rel err dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e} (bar {bar_of(entry):.2e})")
    assert max(errs) <= bar_of(entry), (what, errs)
    return max(errs)


def whole_clip_gap(entry, qkv_vals, dctx_vals, got, B, T, heads, dm, dev):
    """T <= 256: the largest difference to the whole-clip entry point, each third against its maximum.  Printed only."""
    if T > 256 or (entry == "f16" and dm > 64 and T > 208):                   # the whole-clip f16 entry refuses wide heads there
        return
    H = heads * dm
    other = values(entry, launch(entry, pack(qkv_vals, entry), pack(dctx_vals, entry), None, B, T, H, heads, dev, whole=True))
    gaps = C.third_errors(got, other, H)
    print(f"  vs the whole-clip entry at T={T}: dq {gaps[0]:.2e} dk {gaps[1]:.2e} dv {gaps[2]:.2e}")


def run_case(dev, kind, case):
    entry, T, heads, dm, B = case
    qkv, dctx = C.inputs(kind, entry, T, heads, dm, B)
    H = heads * dm
    got = values(entry, launch(entry, pack(qkv, entry), pack(dctx, entry), None, B, T, H, heads, dev))
    ref = C.reference(kind, entry, T, heads, dm, B)
    errs = C.third_errors(got, ref["plain"], H)
    if max(errs) > bar_of(entry):
        np32 = C.third_errors(C.attention_bwd_np32(qkv, dctx, B, T, heads, dm), ref["plain"], H)
        print(f"  MISSED; numpy fp32 restatement on the same input: dq {np32[0]:.2e} dk {np32[1]:.2e} dv {np32[2]:.2e}")
    check(entry, got, ref["plain"], H, f"{kind} {C.case_id(case)} {C.instances_of(entry, T, dm)}")
    whole_clip_gap(entry, qkv, dctx, got, B, T, heads, dm, dev)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_long_backward_parity(gpu_device, case):
    """N(0, 0.7) q | k | v and N(0, 1) dO (backward_kernel_cases.att_inputs): every instance at one row, one tile, one row past a
    tile, every edge of one, two and three blocks of each streaming loop, every padded head dim, and the strides the whole-clip
    kernels take."""
    run_case(gpu_device, "random", case)


@pytest.mark.parametrize("kind", ["uniform", "peaked", "ordered"])
@pytest.mark.parametrize("entry", C.ENTRIES)
@pytest.mark.parametrize("shape", C.KIND_SHAPES, ids=str)
def test_long_backward_adversarial(gpu_device, entry, shape, kind):
    """uniform -- q = 0, every probability exactly 1 / T: a pad row that is counted or a row dropped at a block seam moves every
    element.  peaked -- row maxima above 0.999 and scores spanning 60: dS_ii = P_ii (dP_ii - delta_i) stands on the recomputed S
    and dP being those behind the statistics.  ordered -- the row maximum of query i in key block i % 3 with a margin of 40: the
    running maximum of sweep 1 rises zero times, once and twice and alpha underflows -- the rescale of l and of the delta sum."""
    run_case(gpu_device, kind, (entry,) + shape)


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("case", C.FRAME_CASES, ids=C.case_id)
def test_long_backward_frames(gpu_device, case, which):
    entry, T, heads, dm, B = case
    frames = C.FRAMES[which]
    H, dev = heads * dm, gpu_device
    qkv, dctx = C.inputs("random", entry, T, heads, dm, B)
    run = lambda q, d, fr, B_=B, T_=T: launch(entry, q, d, fr, B_, T_, H, heads, dev)
    full = run(pack(qkv, entry), pack(dctx, entry), None)
    assert torch.equal(run(pack(qkv, entry), pack(dctx, entry), (T,) * B), full), "frames = T differs from frames = NULL"
    got = run(pack(qkv, entry), pack(dctx, entry), frames)                                 # real values past frames[b]
    for garbage in (NAN, float(torch.tensor(1e30).half())):                               # 1e30 as fp16 holds it: +inf
        other = run(pack(qkv, entry, T, frames, garbage), pack(dctx, entry, T, frames, garbage), frames)
        assert torch.equal(other, got), f"rows past frames[b] = {garbage} changed the result"
    clip = lambda bits, b, lo, hi: bits[..., b * T + lo:b * T + hi, :]
    assert torch.equal(clip(got, 0, 0, T), clip(full, 0, 0, T)), "the full-length clip differs from the frames = NULL launch"
    worst = 0.0
    for b, f in enumerate(frames):
        assert bool((clip(got, b, f, T) == 0).all()), (b, "rows past frames[b] are not exactly zero in every plane")
        rows = slice(b * T, (b + 1) * T)
        alone = run(pack(qkv[rows], entry), pack(dctx[rows], entry), (f,), 1)
        assert torch.equal(alone, clip(got, b, 0, T)), (b, "a clip depends on its batch")
        body = clip(got, b, 0, f)
        crop_q, crop_d = qkv[b * T:b * T + f], dctx[b * T:b * T + f]
        out = values(entry, body)
        ref = C.reference_of(crop_q, crop_d, 1, f, heads, dm)
        worst = max(worst, check(entry, out, ref["plain"], H, f"frames {C.case_id(case)} clip {b} Tv={f}"))
        cropped = run(pack(crop_q, entry), pack(crop_d, entry), None, 1, f)                # the same clip at stride Tv
        assert torch.equal(cropped, body), (b, f, "valid rows differ from the launch on the cropped clip at stride Tv")
        whole_clip_gap(entry, crop_q, crop_d, out, 1, f, heads, dm, dev)
    print(f"attention bwd long frames [{entry}] dm={dm} frames={frames}: worst rel err {worst:.2e}")


@pytest.mark.parametrize("case", C.FRAME_CASES[:2], ids=C.case_id)
def test_out_of_range_frames_are_clamped(gpu_device, case):
    """frames outside [1, T] (0, negative, far above T) cannot move an access: they act as 1 and T."""
    entry, T, heads, dm, B = case
    qkv, dctx = C.inputs("random", entry, T, heads, dm, B)
    q, d = pack(qkv, entry), pack(dctx, entry)
    wild = launch(entry, q, d, (T + 1000, 0, -7), B, T, heads * dm, heads, gpu_device)
    tame = launch(entry, q, d, (T, 1, 1), B, T, heads * dm, heads, gpu_device)
    assert torch.equal(wild, tame)


@pytest.mark.parametrize("entry", C.ENTRIES)
@pytest.mark.parametrize("shape", C.STRIDE_SHAPES, ids=str)
def test_a_clip_at_stride_513_is_the_clip_at_its_own_stride(gpu_device, entry, shape):
    """Results depend on Tv only, not on T: frames = Tv at row stride 513 against the same rows at stride Tv, bit for bit."""
    Tv, heads, dm = shape
    H = heads * dm
    qkv, dctx = C.inputs("random", entry, 513, heads, dm, 2)
    wide = launch(entry, pack(qkv[:513], entry), pack(dctx[:513], entry), (Tv,), 1, 513, H, heads, gpu_device)
    tight = launch(entry, pack(qkv[:Tv], entry), pack(dctx[:Tv], entry), None, 1, Tv, H, heads, gpu_device)
    assert torch.equal(wide[..., :Tv, :], tight)
    assert bool((wide[..., Tv:, :] == 0).all())


@pytest.mark.parametrize("entry", C.ENTRIES)
def test_long_backward_does_not_depend_on_the_batch(gpu_device, entry):
    """Clip 0 of a two-clip launch equals, bit for bit, a one-clip launch on clip 0 alone; a repeated launch repeats its bits."""
    T, heads, dm = C.PROPERTY_SHAPE
    H = heads * dm
    qkv, dctx = C.inputs("random", entry, T, heads, dm, 2)
    q, d = pack(qkv, entry), pack(dctx, entry)
    two = launch(entry, q, d, None, 2, T, H, heads, gpu_device)
    again = launch(entry, q, d, None, 2, T, H, heads, gpu_device)
    one = launch(entry, pack(qkv[:T], entry), pack(dctx[:T], entry), None, 1, T, H, heads, gpu_device)
    assert torch.equal(two, again)
    assert torch.equal(two[..., :T, :], one)
    values(entry, one)


@pytest.mark.parametrize("entry", C.ENTRIES)
def test_long_backward_is_linear_in_the_gradient(gpu_device, entry):
    """Scaling dctx by 2^-2 and 2^+2 scales dq, dk and dv by exactly that factor, bit for bit (split: both planes), on inputs for
    which the fp64 reference shows that no output leaves its format's full-precision range (attention_bwd_long_cases)."""
    T, heads, dm, B = C.LINEAR_SHAPE
    H = heads * dm
    qkv, dctx = C.linear_inputs()
    lo, hi = C.linear_precondition(qkv, dctx)
    assert C.LINEAR_RANGE[0] <= lo and hi <= C.LINEAR_RANGE[1]
    q = pack(qkv, entry)
    base = launch(entry, q, pack(dctx, entry), None, B, T, H, heads, gpu_device)
    check(entry, values(entry, base), C.reference_of(qkv, dctx, B, T, heads, dm)["plain"], H, "linear")
    for shift in (-C.LINEAR_SHIFT, C.LINEAR_SHIFT):
        f = 2.0 ** shift
        d = pack(dctx * f, entry)
        rows = d[..., :B * T, :].double()
        assert torch.equal(rows if entry == "f16" else rows[0] + rows[1] / 2048.0, dctx * f)      # exact in both formats
        out = launch(entry, q, d, None, B, T, H, heads, gpu_device)
        values(entry, out)
        assert torch.equal(out.view(torch.float16).double(), base.view(torch.float16).double() * f), f"dctx * 2^{shift}"


@pytest.mark.parametrize("entry", C.ENTRIES)
@pytest.mark.parametrize("where", ["qkv", "dctx"])
def test_a_nan_stays_in_its_clip_and_head(gpu_device, entry, where):
    """One NaN in q (or dO) of (clip 1, head 0): every other (clip, head) keeps its bits."""
    T, heads, dm = C.PROPERTY_SHAPE
    H, B = heads * dm, 2
    qkv, dctx = C.inputs("random", entry, T, heads, dm, B)
    clean = launch(entry, pack(qkv, entry), pack(dctx, entry), None, B, T, H, heads, gpu_device)
    q, d = pack(qkv, entry), pack(dctx, entry)
    (q if where == "qkv" else d)[..., T + 130, 3] = NAN                          # clip 1, row 130, head 0's column 3 (q third / dO)
    dirty = launch(entry, q, d, None, B, T, H, heads, gpu_device)
    assert not bool((dirty == FILL).any())
    hit = torch.zeros(B * T, 3 * H, dtype=torch.bool)
    for third in range(3):
        hit[T:, third * H:third * H + dm] = True                                 # clip 1, head 0, all three thirds
    keep = ~hit.expand_as(dirty) if dirty.dim() == 2 else ~hit[None].expand_as(dirty)
    assert torch.equal(dirty[keep], clean[keep]), "the NaN left its (clip, head)"
    assert bool(torch.isnan(dirty.view(torch.float16)[~keep].float()).any())


def test_range_contract_of_the_split_store(gpu_device):
    """Split outputs go through the checked conversion: a dV past 65 504 saturates (hi = +-65504, lo the clamped remainder), raises
    the sticky flag and leaves neither inf nor NaN in a plane (after tests/test_gpu_lrp.py test_attention_bwd_value_range_contract);
    the in-range launch of the same shape leaves the flag clear."""
    T, heads, dm, B = 273, 2, 16, 1
    H = heads * dm
    g = torch.Generator().manual_seed(5)
    qkv = G.join_planes(G.split_planes(torch.randn(B * T, 3 * H, generator=g) * 0.7)).double()
    d32 = torch.randn(B * T, H, generator=g)
    launch("split", pack(qkv, "split"), pack(d32.double(), "split"), None, B, T, H, heads, gpu_device, flag=0)
    big = d32.clone()
    big[:, 3] = 64000.0                                     # dV[k, 3] = 64000 sum_q P[q, k]: past the range where a key's column sum > 1.0235
    dctx = G.join_planes(G.split_planes(big)).double()
    ref = C.reference_of(qkv, dctx, B, T, heads, dm)["plain"]
    over = ref.abs() > SPLIT_MAX * (1 + 1e-4)
    assert bool(over.any()) and bool((ref.abs() > SAT_MAX * (1 + 1e-4)).any()) and not bool(over[:, :2 * H].any())
    bits = launch("split", pack(qkv, "split"), pack(dctx, "split"), None, B, T, H, heads, gpu_device, flag=1)
    planes = bits.view(torch.float16)
    assert bool(torch.isfinite(planes.float()).all()), "a saturating value left inf or NaN in a plane"
    assert bool((planes[0][over].float().abs() == SPLIT_MAX).all())
    got = values("split", bits)
    print(f"saturating dV: {int(over.sum())} values past 65504 (max |ref| {ref.abs().max():.1f})")
    check("split", got, ref.clamp(-SAT_MAX, SAT_MAX), H, "saturating dV against the clamped reference")


@pytest.mark.parametrize("entry", C.ENTRIES)
def test_refusals_leave_dqkv_untouched(gpu_device, entry):
    """ADVH_EUNSUPPORTED (head dim 20 and 136) and ADVH_EINVAL (H % heads) with real buffers: no element of dqkv is written."""
    T, B = 16, 1                                            # T + PAD and T + GUARD rows keep every plane distance a multiple of 8
    for H, heads, rc in ((20, 1, EUNSUPPORTED), (136, 1, EUNSUPPORTED), (40, 3, EINVAL)):
        qkv, dctx = torch.zeros(B * T, 3 * H, dtype=torch.float64), torch.zeros(B * T, H, dtype=torch.float64)
        bits = launch(entry, pack(qkv, entry), pack(dctx, entry), None, B, T, H, heads, gpu_device, expect=rc)
        assert bool((bits == FILL).all()), (H, heads)
