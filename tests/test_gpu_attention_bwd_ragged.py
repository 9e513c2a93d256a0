"""Kernel-level suite of the ragged attention backward (the RAGGED instances of csrc/backward.hip, attention_bwd_x3.hip and
attention_bwd_f32.hip; the siblings are the batch instances of the same template arguments): every compiled instance at strides at both
edges of its tile-count class, three clips with ``frames = (T, 1, m)`` (``m % 16 == 1``: one frame into a tile), two heads.

Setup: NaN in the rows of qkv and dctx past ``frames[b]``, dqkv prefilled with NaN, NaN guard rows in front of and behind it.
Rows ``t < frames[b]`` are held against ``backward_ops_ref.attention_bwd`` on the clip's first ``frames[b]`` rows alone at the
sibling's bars (tests/test_gpu_backward_kernels.py: 5e-6 per third for the split entries, ``check_f16`` for the f16 entry); rows
``t >= frames[b]`` are exactly zero in every plane; the guards keep the prefill's bits; the ``frames = T`` clip is bit-identical
to the sibling's output; a clip's rows do not depend on the batch around it.  The cases and the dispatch mirror live in
tests/attention_bwd_ragged_cases.py; tests/test_build_resources_attention_bwd_ragged.py holds them against the compiled instances."""
import functools

import pytest
import torch

import attention_bwd_ragged_cases as C
import backward_kernel_cases as K
import backward_ops_ref as BR
from addvisor_hip import _lib
from test_gpu_backward_kernels import EUNSUPPORTED, GUARD, check_f16, check_split, launch_attention, pack, stream, untouched

pytestmark = pytest.mark.gpu
NAN = float("nan")


def fmt_of(entry):
    return "f16" if entry == "f16" else "split"


@functools.lru_cache(maxsize=4)
def operands(T, heads, dm, B, fmt):
    """(qkv tensor, dctx tensor, their fp64 values) with NaN in every row past the clip's frames.  Shared: never modify."""
    qv, dv = K.att_inputs(T, heads, dm, B, fmt)
    (q_t, q_v), (d_t, d_v) = pack(qv, fmt), pack(dv, fmt)
    q_t, d_t = q_t.clone(), d_t.clone()
    for b, f in enumerate(C.frames_of(T)[:B]):
        q_t[..., b * T + f:(b + 1) * T, :] = NAN
        d_t[..., b * T + f:(b + 1) * T, :] = NAN
    return q_t, d_t, q_v, d_v


def launch_ragged(entry, q_t, d_t, frames, B, T, heads, dm, dev):
    """One ragged launch into a NaN-prefilled buffer with GUARD rows on both sides: (rc, the whole buffer on the CPU)."""
    _lib.init()
    H, lib = heads * dm, _lib.lib()
    qd, dd = q_t.to(dev), d_t.to(dev)
    fr = torch.tensor(frames, dtype=torch.int32, device=dev)
    rows = GUARD + B * T + GUARD
    if entry == "f16":
        out = torch.full((rows, 3 * H), NAN, dtype=torch.float16, device=dev)
        rc = lib.advh_attention_bwd_f16_ragged(qd.data_ptr(), dd.data_ptr(), out[GUARD:].data_ptr(), fr.data_ptr(), B, T, H, heads, stream())
    else:
        out = torch.full((2, rows, 3 * H), NAN, dtype=torch.float16, device=dev)
        _lib.check(lib.advh_set_option(b"attention_bwd_mfma_f32", int(entry == "split_f32")), "advh_set_option")
        try:
            rc = lib.advh_attention_bwd_split_ragged(qd.data_ptr(), qd.stride(0), dd.data_ptr(), dd.stride(0), out[0, GUARD:].data_ptr(),
                                                     out.stride(0), fr.data_ptr(), B, T, H, heads, stream())
        finally:
            lib.advh_set_option(b"attention_bwd_mfma_f32", 0)
    torch.cuda.synchronize()
    return rc, out.cpu()


def body(entry, out, B, T):
    """(the B*T rows, the guard rows) of a launch's buffer."""
    if entry == "f16":
        return out[GUARD:GUARD + B * T], torch.cat([out[:GUARD], out[GUARD + B * T:]])
    return out[:, GUARD:GUARD + B * T], torch.cat([out[:, :GUARD], out[:, GUARD + B * T:]], 1)


def clip_reference(q_v, d_v, b, T, f, heads, dm, fmt):
    """The reference dict of tests/test_gpu_backward_kernels.py on rows [b*T, b*T + f) alone."""
    q, k, v = BR.heads_of(q_v[b * T:b * T + f], 1, f, heads, dm)
    (dO,) = BR.heads_of(d_v[b * T:b * T + f], 1, f, heads, dm)
    dq, dk, dv, P, dS = BR.attention_bwd(q, k, v, dO)
    ref = {"plain": BR.rows_of(dq, dk, dv), "q": q, "k": k, "v": v, "dO": dO}
    if fmt == "f16":
        ref["model"] = BR.attention_bwd_f16_model(q, k, v, dO)
        ref["np32"] = K.attention_bwd_f16_np32(q, k, v, dO)
    return ref


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_attention_bwd_ragged(gpu_device, case):
    entry, T, heads, dm, B = case
    fmt, H, frames = fmt_of(entry), heads * dm, C.frames_of(T)
    q_t, d_t, q_v, d_v = operands(T, heads, dm, B, fmt)
    rc, out = launch_ragged(entry, q_t, d_t, frames, B, T, heads, dm, gpu_device)
    assert rc == 0
    rows, guard = body(entry, out, B, T)
    assert untouched(guard), "guard rows around dqkv were written"
    from addvisor_hip import gemm as G
    got = rows.double() if entry == "f16" else G.join_planes(rows).double()
    inst = C.instance_of(entry, T, dm)
    for b, f in enumerate(frames):
        tail = rows[..., b * T + f:(b + 1) * T, :]
        assert bool((tail.view(torch.int16) == 0).all()), (b, "rows past the clip's frames are not exactly zero in every plane")
        g = got[b * T:b * T + f]
        assert torch.isfinite(g).all(), (b, "a valid row of dqkv was not written, or read a padded row")
        ref = clip_reference(q_v, d_v, b, T, f, heads, dm, fmt)
        if entry == "f16":
            check_f16(g, ref, 1, f, heads, dm, f"{inst} clip {b} ({f} of {T} frames)")
        else:
            check_split(entry, g, ref, H, f"{inst} clip {b} ({f} of {T} frames)")
    # the full-length clip: the sibling's bits (the sibling runs clip 0 alone: its operands have no NaN)
    cut = lambda t: t[..., :T, :].contiguous()
    rc1, sib = launch_attention(entry, cut(q_t), cut(d_t), 1, T, heads, dm, gpu_device)
    assert rc1 == 0
    sib = sib[:T] if entry == "f16" else sib[:, :T]
    assert torch.equal(rows[..., :T, :].view(torch.int16), sib.view(torch.int16)), "frames = T is not the sibling bit for bit"
    # the third clip alone (B = 1) and with its neighbours: the same bits
    sl = lambda t: t[..., 2 * T:3 * T, :].contiguous()
    rc2, alone = launch_ragged(entry, sl(q_t), sl(d_t), frames[2:], 1, T, heads, dm, gpu_device)
    assert rc2 == 0
    assert torch.equal(body(entry, alone, 1, T)[0].view(torch.int16), rows[..., 2 * T:3 * T, :].view(torch.int16)), "a clip depends on its batch"


@pytest.mark.parametrize("case", [c for c in C.CASES if c[1] in (65, 209)], ids=C.case_id)
def test_short_clip_is_the_sibling_on_its_cropped_rows(gpu_device, case):
    """The basis of the chain's bit-identity with the per-clip run: the m valid rows of the third clip equal, bit for bit, what the
    SIBLING gives for those m rows launched alone at T = m -- another instance class (m = 17: the 8-tile class against the 13- or
    16-tile class of the stride), whose extra tiles add exact zeros."""
    entry, T, heads, dm, B = case
    fmt, frames = fmt_of(entry), C.frames_of(T)
    m = frames[2]
    q_t, d_t, _, _ = operands(T, heads, dm, B, fmt)
    rc, out = launch_ragged(entry, q_t, d_t, frames, B, T, heads, dm, gpu_device)
    crop = lambda t: t[..., 2 * T:2 * T + m, :].contiguous()
    rc1, sib = launch_attention(entry, crop(q_t), crop(d_t), 1, m, heads, dm, gpu_device)
    assert rc == 0 and rc1 == 0
    rows = body(entry, out, B, T)[0][..., 2 * T:2 * T + m, :]
    sib = sib[:m] if entry == "f16" else sib[:, :m]
    assert torch.equal(rows.float(), sib.float()), "the valid rows differ from the sibling on the cropped clip"


@pytest.mark.parametrize("T,dm", C.REFUSED)
def test_attention_bwd_f16_ragged_refuses_wide_heads_above_208_frames(gpu_device, T, dm):
    """As the sibling: head dims above 64 with a stride above 208 frames need more than 160 KiB of LDS: ADVH_EUNSUPPORTED, dqkv untouched."""
    q_t, d_t, _, _ = operands(T, 2, dm, 3, "f16")
    rc, out = launch_ragged("f16", q_t, d_t, C.frames_of(T), 3, T, 2, dm, gpu_device)
    assert rc == EUNSUPPORTED and untouched(out)
    rc, _ = launch_attention("f16", q_t[:T].nan_to_num(0.0), d_t[:T].nan_to_num(0.0), 1, T, 2, dm, gpu_device)
    assert rc == EUNSUPPORTED


def test_frames_are_clamped_inside_the_kernel(gpu_device):
    """frames outside [1, T] cannot move an access: 0 and negative counts act as 1, counts above T as T (guards untouched)."""
    T, heads, dm, B = 65, 2, 24, 3
    for entry in ("f16", "split"):
        qv, dv = K.att_inputs(T, heads, dm, B, fmt_of(entry))
        (qq, _), (dd, _) = pack(qv, fmt_of(entry)), pack(dv, fmt_of(entry))
        rc_a, a = launch_ragged(entry, qq, dd, (T + 1000, 0, -7), B, T, heads, dm, gpu_device)
        rc_b, b_ = launch_ragged(entry, qq, dd, (T, 1, 1), B, T, heads, dm, gpu_device)
        assert rc_a == 0 and rc_b == 0
        assert torch.equal(a.view(torch.int16), b_.view(torch.int16))
        assert untouched(body(entry, a, B, T)[1])
