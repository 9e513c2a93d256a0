"""Kernel-level suite of the streamed forward attention (csrc/attention_long.hip): the seven instances of attention_long_kernel
behind advh_attention_long_f16 / advh_attention_long_split, against the float64 ``embedder_ops_ref.attention`` evaluated on the CPU
on the operands the kernel saw.  Cases, the dispatch mirror and the ordered input: tests/attention_long_cases.py
(tests/test_build_resources_attention_long.py holds them against the compiled instances and asserts the inputs' preconditions).

Buffers.  q | k | v rows have PAD rows of NaN behind them (per plane for the split entry).  ctx is prefilled with a NaN bit pattern
no arithmetic produces and lies BETWEEN guard rows of the same pattern: every valid element must lose it, every guard row keeps it.
After every launch the sticky range flag (advh_split_overflow) is clear.

Bars: those of tests/attention_kernel_cases.py, unchanged.  Split entry: per (clip, head) block max|out - ref| <= 5e-6 max|ref|.
f16 entry, elementwise: |out - ref| <= 2^-11 (sum_j p_j |v_j| + |ref|) (1 + 2^-6) + 5e-6 max|v|.  A case that misses prints the
numpy fp32 restatement's own ratio on the same input next to the kernel's.

Worst |err| / bar per instance <NTB, D, NP, TR> over all its cases, measured on an MI355X: split <16, 32, 2, 0> 0.195,
<16, 64, 2, 0> 0.184 (ordered), <16, 64, 2, 1> 0.208, <7, 128, 2, 0> 0.225; fp16 <16, 32, 1, 0> 0.620, <16, 64, 1, 0> 0.692,
<16, 128, 1, 0> 0.643 (the fp16 half-ulps of P and of the store, as for the whole-clip kernels).  Every bit-identity of the frames
test held: frames = T against frames = NULL, NaN / inf past frames[b], a clip against its batch, a clip of m > 256 frames against
the launch on its cropped rows.
"""
import pytest
import torch

import attention_kernel_cases as K
import attention_long_cases as C
import backward_ops_ref as BR
import embedder_ops_ref
from addvisor_hip import _lib, gemm as G

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PAD, GUARD = 16, 4
FILL = 0x7DAB                                   # an fp16 NaN whose payload neither the inputs nor any arithmetic carry
NAN = float("nan")


def stream():
    return torch.cuda.current_stream().cuda_stream


def pack(vals, entry, T=None, frames=None, garbage=NAN):
    """float64 rows [B*T, 3H] -> operand tensor on the CPU with PAD rows of NaN behind; rows >= frames[b] of clip b = garbage."""
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


def launch(entry, qkv, frames, B, T, H, heads, dev, whole=False):
    """One call of the long entry (``whole``: of the whole-clip entry, T <= 256, no frames).  -> ctx rows [B*T] on the CPU as
    int16 bit patterns, after checking the guard rows in front of and behind them and the range flag."""
    _lib.init()
    lib = _lib.lib()
    qd = qkv.to(dev)
    rows = B * T
    shape = (rows + 2 * GUARD, H) if entry == "f16" else (2, rows + 2 * GUARD, H)
    ctx = torch.full(shape, FILL, dtype=torch.int16, device=dev).view(torch.float16)
    cp = ctx[..., GUARD:, :][(0,) * (ctx.dim() - 2)].data_ptr()                  # row GUARD of the (first) plane
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device=dev)
    fp = None if fr is None else fr.data_ptr()
    torch.cuda.synchronize()
    lib.advh_split_overflow(1)
    if entry == "f16":
        rc = lib.advh_attention_f16(qd.data_ptr(), cp, B, T, H, heads, stream()) if whole else \
            lib.advh_attention_long_f16(qd.data_ptr(), cp, fp, B, T, H, heads, stream())
    else:
        rc = lib.advh_attention_split(qd.data_ptr(), qd.stride(0), cp, ctx.stride(0), B, T, H, heads, stream()) if whole else \
            lib.advh_attention_long_split(qd.data_ptr(), qd.stride(0), cp, ctx.stride(0), fp, B, T, H, heads, stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert lib.advh_split_overflow(1) == 0
    bits = ctx.cpu().view(torch.int16)
    assert bool((bits[..., :GUARD, :] == FILL).all()) and bool((bits[..., GUARD + rows:, :] == FILL).all()), "guard rows were written"
    return bits[..., GUARD:GUARD + rows, :]


def values(entry, bits, B, T, heads, dm):
    """float64 [B, heads, T, dm] of ctx bit patterns [.., B*T, H]; every element must have been written."""
    assert not bool((bits == FILL).any()), "valid rows were not all written"
    t = bits.contiguous().view(torch.float16)
    rows = t.double() if entry == "f16" else G.join_planes(t).double()
    return BR.heads_of(rows, B, T, heads, dm)[0]


def ratio_of(entry, got, ref):
    return K.f16_ratio(got, ref) if entry == "f16" else K.split_ratio(got, ref["ctx"])


def run_case(dev, kind, case):
    entry, T, heads, dm, B = case
    vals = C.inputs(kind, entry, T, heads, dm, B)
    got = values(entry, launch(entry, pack(vals, entry), None, B, T, heads * dm, heads, dev), B, T, heads, dm)
    assert torch.isfinite(got).all()
    ref = C.reference(kind, entry, T, heads, dm, B)
    ratio = ratio_of(entry, got, ref)
    inst = C.instance_of(entry, T, dm)
    print(f"attention long [{entry}] {kind} T={T} heads={heads} dm={dm} B={B} {inst}: worst |err| / bar {ratio:.3f}")
    if ratio > 1.0:
        np32 = ratio_of(entry, K.attention_np32(ref["q"], ref["k"], ref["v"]), ref)
        print(f"  MISSED; numpy fp32 restatement on the same input: {np32:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_long_attention_parity(gpu_device, case):
    """N(0, 1) * 1.5 operands, V of head h scaled by 1, 1/4, 4: every instance with one key in its last block, a whole last block,
    one query row in its last tile and in its last query block, every padded head dim, and the strides the whole-clip kernels take."""
    run_case(gpu_device, "random", case)


@pytest.mark.parametrize("entry", C.ENTRIES)
@pytest.mark.parametrize("shape", C.UNIFORM_SHAPES, ids=str)
def test_long_attention_uniform(gpu_device, entry, shape):
    """q = 0: every probability is exactly 1 / T.  A pad key of the last block that is counted, or a key that is dropped at a
    block seam, moves every element by ~1 / T of itself."""
    run_case(gpu_device, "uniform", (entry,) + shape)


@pytest.mark.parametrize("entry", C.ENTRIES)
@pytest.mark.parametrize("shape", C.PEAKED_SHAPES, ids=str)
def test_long_attention_peaked(gpu_device, entry, shape):
    run_case(gpu_device, "peaked", (entry,) + shape)


@pytest.mark.parametrize("case", C.ORDERED_CASES, ids=C.case_id)
def test_long_attention_ordered(gpu_device, case):
    """Three key blocks of the instance's own size, query i's maximum in block i % 3 with a margin of 40: the running maximum
    rises zero times, once and twice, and alpha underflows -- the rescale branch, forced."""
    run_case(gpu_device, "ordered", case)


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("case", C.FRAME_CASES, ids=C.case_id)
def test_long_attention_frames(gpu_device, case, which):
    entry, T, heads, dm, B = case
    frames = C.FRAMES[T][which]
    H, dev = heads * dm, gpu_device
    vals = C.inputs("random", entry, T, heads, dm, B)
    full = launch(entry, pack(vals, entry), None, B, T, H, heads, dev)
    same = launch(entry, pack(vals, entry), (T,) * B, B, T, H, heads, dev)
    assert torch.equal(same, full), "frames = T differs from frames = NULL"
    got = launch(entry, pack(vals, entry), frames, B, T, H, heads, dev)                     # real values past frames[b]
    for garbage in (NAN, float(torch.tensor(1e30).half())):                               # 1e30 as fp16 holds it: +inf
        other = launch(entry, pack(vals, entry, T, frames, garbage), frames, B, T, H, heads, dev)
        assert torch.equal(other, got), f"rows past frames[b] = {garbage} changed the result"
    clip = lambda bits, b, lo, hi: bits[..., b * T + lo:b * T + hi, :]
    assert torch.equal(clip(got, 0, 0, T), clip(full, 0, 0, T)), "the full-length clip differs from the frames = NULL launch"
    worst = 0.0
    for b, f in enumerate(frames):
        assert bool((clip(got, b, f, T) == 0).all()), (b, "rows past frames[b] are not exactly zero in every plane")
        alone = launch(entry, pack(vals[b * T:(b + 1) * T], entry), (f,), 1, T, H, heads, dev)
        assert torch.equal(alone, clip(got, b, 0, T)), (b, "a clip depends on its batch")
        body = clip(got, b, 0, f)
        out = values(entry, body, 1, f, heads, dm)
        assert torch.isfinite(out).all()
        crop = vals[b * T:b * T + f]
        q, k, v = BR.heads_of(crop, 1, f, heads, dm)
        ctx, p = embedder_ops_ref.attention(q, k, v)
        ref = {"ctx": ctx, "p": p, "v": v}
        ratio = ratio_of(entry, out, ref)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (b, f, ratio)
        if f > 256:                                                                       # the same entry on the cropped rows, stride f
            cropped = launch(entry, pack(crop, entry), None, 1, f, H, heads, dev)
            assert torch.equal(cropped, body), (b, f, "valid rows differ from the launch on the cropped clip")
        else:                                                                             # the whole-clip entry on the cropped rows
            whole = values(entry, launch(entry, pack(crop, entry), None, 1, f, H, heads, dev, whole=True), 1, f, heads, dm)
            gap = ((out - whole).abs() / (K.f16_bound(ref) if entry == "f16" else (K.TOL_SPLIT * K.block_max(ctx)))).max().item()
            assert gap <= 2.0, (b, f, gap)
    print(f"attention long frames [{entry}] T={T} dm={dm} frames={frames} {C.instance_of(entry, T, dm)}: worst |err| / bar {worst:.3f}")


@pytest.mark.parametrize("case", C.FRAME_CASES, ids=C.case_id)
def test_out_of_range_frames_are_clamped(gpu_device, case):
    """frames outside [1, T] (0, negative, far above T) cannot move an access: they act as 1 and T."""
    entry, T, heads, dm, B = case
    qkv = pack(C.inputs("random", entry, T, heads, dm, B), entry)
    wild = launch(entry, qkv, (T + 1000, 0, -7), B, T, heads * dm, heads, gpu_device)
    tame = launch(entry, qkv, (T, 1, 1), B, T, heads * dm, heads, gpu_device)
    assert torch.equal(wild, tame)
