"""Kernel-level suite of the ragged forward attention (csrc/attention_ragged.hip): every compiled instance behind
advh_attention_f16_ragged / advh_attention_split_ragged.  Cases and the dispatch mirror: tests/attention_ragged_cases.py
(tests/test_build_resources_attention_ragged.py holds them against the compiled instances).

Each case is three clips of row stride T with frames = (T, 1, m), m one frame into a 16-frame tile (for the streaming kernel: at
the 112-key block edge).  Rows >= frames[b] of q | k | v are NaN in every plane, ctx is prefilled with a NaN bit pattern no
arithmetic produces and has guard rows behind it.  Required:
  valid rows      the float64 ``embedder_ops_ref.attention`` of the clip CROPPED to frames[b] rows, within the bar the sibling
                  instance has in tests/attention_kernel_cases.py (split: 5e-6 of max|ref| per (clip, head); f16: the elementwise
                  fp16 bound) -- a key or query past frames[b] that took part would put a NaN there;
  padded rows     rows [frames[b], T) of every plane are exactly +0;
  guard rows      untouched;
  full lengths    frames = (T, T, T) is bit-identical to the sibling entry point on the same operands;
  isolation       clip 0 (full length) is bit-identical to the sibling's clip 0 whatever the other clips' frames are.
Worst |err| / bar per case, measured on an MI355X: split instances 0.04 - 0.17, the streaming kernel 0.05 - 0.15, fp16 instances
0.63 - 0.78 (the fp16 half-ulps of P and of the store, which is their bound, as for the siblings).
"""
import pytest
import torch

import attention_kernel_cases as K
import attention_ragged_cases as C
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


def pack(vals, entry, T, frames=None):
    """float64 rows [B*T, 3H] -> operand tensor on the CPU with PAD rows of NaN behind; rows >= frames[b] of clip b NaN."""
    rows, width = vals.shape
    if entry == "f16":
        t = torch.full((rows + PAD, width), NAN, dtype=torch.float16)
        t[:rows] = vals.half()
    else:
        t = torch.full((2, rows + PAD, width), NAN, dtype=torch.float16)
        t[:, :rows] = G.split_planes(vals)
    for b, f in enumerate(frames or ()):
        t[..., b * T + f:(b + 1) * T, :] = NAN
    return t


def launch(entry, qkv, frames, B, T, H, heads, dev):
    """frames None: the sibling entry point.  -> (ctx on the CPU incl. guard rows as int16 bit patterns, range flag)."""
    _lib.init()
    lib = _lib.lib()
    qd = qkv.to(dev)
    shape = (B * T + GUARD, H) if entry == "f16" else (2, B * T + GUARD, H)
    ctx = torch.full(shape, FILL, dtype=torch.int16, device=dev).view(torch.float16)
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lib.advh_split_overflow(1)
    if entry == "f16":
        rc = (lib.advh_attention_f16(qd.data_ptr(), ctx.data_ptr(), B, T, H, heads, stream()) if fr is None else
              lib.advh_attention_f16_ragged(qd.data_ptr(), ctx.data_ptr(), fr.data_ptr(), B, T, H, heads, stream()))
    else:
        rc = (lib.advh_attention_split(qd.data_ptr(), qd.stride(0), ctx.data_ptr(), ctx.stride(0), B, T, H, heads, stream()) if fr is None else
              lib.advh_attention_split_ragged(qd.data_ptr(), qd.stride(0), ctx.data_ptr(), ctx.stride(0), fr.data_ptr(), B, T, H, heads, stream()))
    torch.cuda.synchronize()
    assert rc == 0, rc
    return ctx.cpu().view(torch.int16), lib.advh_split_overflow(1)


def clip_rows(bits, b, T, lo, hi):
    return bits[..., b * T + lo:b * T + hi, :]


def values(entry, bits):
    t = bits.view(torch.float16)
    return t.double() if entry == "f16" else G.join_planes(t).double()


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_ragged_attention(gpu_device, case):
    entry, T, heads, dm, B, is_stream = case
    H = heads * dm
    frames = C.frames_of(T, is_stream)
    vals = K.inputs("random", entry, T, heads, dm, B)
    full = pack(vals, entry, T)
    sib, flag0 = launch(entry, full, None, B, T, H, heads, gpu_device)
    same, flag1 = launch(entry, full, (T,) * B, B, T, H, heads, gpu_device)
    got, flag2 = launch(entry, pack(vals, entry, T, frames), frames, B, T, H, heads, gpu_device)
    assert flag0 == flag1 == flag2 == 0
    assert torch.equal(same, sib), "frames = T differs from the sibling entry point"
    for out in (same, got):
        assert bool((out[..., B * T:, :] == FILL).all()), "guard rows behind ctx were written"
    assert torch.equal(clip_rows(got, 0, T, 0, T), clip_rows(sib, 0, T, 0, T)), "clip 0 depends on the other clips' frames"
    worst = 0.0
    for b, f in enumerate(frames):
        assert bool((clip_rows(got, b, T, f, T) == 0).all()), (b, "padded rows are not exactly zero")
        body = clip_rows(got, b, T, 0, f)
        assert not bool((body == FILL).any()), (b, "valid rows were not all written")
        out = BR.heads_of(values(entry, body), 1, f, heads, dm)[0]
        q, k, v = BR.heads_of(vals[b * T:b * T + f], 1, f, heads, dm)
        ctx, p = embedder_ops_ref.attention(q, k, v)
        assert torch.isfinite(out).all(), (b, "a row past frames[b] took part")
        ratio = K.f16_ratio(out, {"ctx": ctx, "p": p, "v": v}) if entry == "f16" else K.split_ratio(out, ctx)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (b, f, ratio)
    print(f"ragged attention [{entry}] T={T} dm={dm} frames={frames} {C.instance_of(entry, T, dm)}: worst |err| / bar {worst:.3f}")


@pytest.mark.parametrize("entry,T,dm", [("f16", 65, 40), ("f16", 65, 64), ("f16", 129, 120), ("split", 65, 40), ("split", 65, 64), ("split", 225, 120)])
def test_out_of_range_frames_are_clamped(gpu_device, entry, T, dm):
    """frames outside [1, T] (0, negative, far above T) cannot move an access: they act as 1 and T."""
    heads, B = 2, 3
    H = heads * dm
    vals = K.inputs("random", entry, T, heads, dm, B)
    qkv = pack(vals, entry, T)
    wild, _ = launch(entry, qkv, (T + 1000, 0, -7), B, T, H, heads, gpu_device)
    tame, _ = launch(entry, qkv, (T, 1, 1), B, T, H, heads, gpu_device)
    assert torch.equal(wild, tame)
    assert bool((wild[..., B * T:, :] == FILL).all())
