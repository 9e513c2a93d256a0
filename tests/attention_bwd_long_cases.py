"""Cases of tests/test_gpu_attention_bwd_long.py and the mirror of the host dispatch of csrc/attention_bwd_long.hip
(advh_attention_bwd_long_f16, advh_attention_bwd_long_split), free of GPU imports so that
tests/test_build_resources_attention_bwd_long.py can hold the cases against the compiled instances and assert every input's
preconditions on the CPU.

The operand format is a run-time argument of both kernels, so an instance is (kernel, D) with D = 32 | 64 | 128 the padded head
dim: six in all.  The four block sizes are the file's constants (BWL_QB, BWL_KB, BWL_KWB, BWL_SQB), the same at every D."""
import functools
import math

import torch

import attention_kernel_cases as AK
import attention_long_cases as AL
import backward_kernel_cases as BK
import backward_ops_ref as BR

ENTRIES = ("f16", "split")                                   # advh_attention_bwd_long_f16 | advh_attention_bwd_long_split
QUERY_KERNEL, KEY_KERNEL = "attention_bwd_long_query_kernel", "attention_bwd_long_key_kernel"
QB = 128                                                     # queries per query-kernel workgroup (eight 16-query tiles)
KB = 128                                                     # staged key block of the query kernel
KWB = 128                                                    # keys per key-kernel workgroup (eight 16-key tiles)
SQB = 128                                                    # staged query block of the key kernel
BLOCKS = tuple(sorted({QB, KB, KWB, SQB}))                   # the distinct block sizes
HEAD_DIMS = (24, 32, 40, 64, 72, 120, 128)                   # per padded width: a padded head dim and the exact one
B, HEADS = 2, 2
T_BLOCK = tuple(sorted({t for b in BLOCKS for t in (b, b + 1, 2 * b, 2 * b + 1, 2 * b + 17, 3 * b + 1)}))
T_FIXED = (1, 16, 17, 256, 257, 513)
T_ALL = tuple(sorted(set(T_BLOCK) | set(T_FIXED)))
TOL_SPLIT = 5e-6                                             # of the maximum of dq, dk and dv each (tests/test_gpu_backward_kernels.py)
TOL_F16 = TOL_SPLIT + 2.0 ** -11                             # plain fp16 output: the one extra rounding of the store (tests/test_gpu_lrp.py)


def padded(dm):
    return 32 if dm <= 32 else (64 if dm <= 64 else 128)


def lds_query(D):
    """K and V of one key block as fp32 [KB][D + 4]."""
    return 2 * KB * (D + 4) * 4


def lds_key(D):
    """Q and dO of one query block as fp32 [SQB][D + 4], and the block's (m, 1 / l, delta)."""
    return (2 * SQB * (D + 4) + 3 * SQB) * 4


def ws_bytes(B_, T, heads):
    return (3 * B_ * heads * T * 4 + 255) // 256 * 256


def instances_of(entry, T, dm):
    """[(kernel, D, blocks of its streaming loop, workgroups per (clip, head))] of the two launches for row stride ``T``; the
    entry picks no instance (the plane distance is a run-time argument)."""
    D = padded(dm)
    return [(QUERY_KERNEL, D, -(-T // KB), -(-T // QB)), (KEY_KERNEL, D, -(-T // SQB), -(-T // KWB))]


def _cases():
    out = [(entry, T, HEADS, dm, B) for dm in HEAD_DIMS for entry in ENTRIES for T in T_ALL]
    return out + [(entry, 273, 3, 40, 3) for entry in ENTRIES]            # three heads, three clips, padded head dim


CASES = _cases()                                             # (entry, T, heads, dm, B)
INSTANCE_DIMS = (24, 64, 120)                                # one head dim per padded width; with both kernels, all six instances
ADVERSARIAL_T = 273
KIND_SHAPES = [(ADVERSARIAL_T, 2, dm, 2) for dm in INSTANCE_DIMS]      # (T, heads, dm, B) of the uniform / peaked / ordered inputs
ORDERED_T = 2 * KB + 17                                      # three key blocks, the third a whole tile and one row
assert ORDERED_T == ADVERSARIAL_T
FRAMES_T = 513
FRAMES = ((513, 1, 257), (513, 256, 273), (513, 17, 129))    # three clips at stride 513
FRAME_CASES = [(entry, FRAMES_T, 2, dm, 3) for dm in (24, 40, 64, 120) for entry in ENTRIES]
PROPERTY_SHAPE = (273, 2, 40)                                # (T, heads, dm) of the batch-independence and NaN-isolation checks
STRIDE_SHAPES = [(273, 2, 40), (257, 2, 120)]                # (Tv, heads, dm): a clip at stride 513 against the same clip at stride Tv


def case_id(c):
    return "{}-T{}-h{}-d{}-B{}".format(*c)


def selected(cases=None):
    """{(kernel, D): [(case, loop blocks, workgroups), ...]} for the parity cases."""
    sel = {}
    for c in (CASES if cases is None else cases):
        for kernel, D, loops, wgs in instances_of(c[0], c[1], c[3]):
            sel.setdefault((kernel, D), []).append((c, loops, wgs))
    return sel


# ----------------------------------------------------------------------------------------------------------- inputs
def _uniform(T, heads, dm, B_, fmt):
    """backward_kernel_cases.att_inputs with q = 0: every probability is exactly 1 / Tv, dq = sum_j dS_ij k_j with dS = (dP - delta) / Tv."""
    qkv, dctx = BK.att_inputs(T, heads, dm, B_, fmt)
    qkv = qkv.clone()
    qkv[:, :heads * dm] = 0.0
    return qkv, dctx


PEAK_CHAIN = -0.8        # cosine of consecutive keys of the peaked input


def _peaked(T, heads, dm, B_, fmt):
    """backward_kernel_cases.peaked_inputs at T = 273 and every padded head dim: keys of one length, q_i = 4 k_i with
    q_i . k_i / sqrt(d) ~ 34, dO_i orthogonal to v_i, dctx scaled by 2^12.  Three things differ, each to keep the case inside what
    the formats and fp32 arithmetic can give at the suite's bars, whatever the kernel:
      * the key directions form a chain (attention_kernel_cases._peaked: random directions alone do not span 40 at head dims 64
        and 120): key j is PEAK_CHAIN of key j-1's direction plus a random direction orthogonal to keys j-1 and j-2.  Every row
        then has neighbours at a score of ~ -27 (a span of ~61) and, two keys away, at ~ +21.8 whatever the head dim: 1 - P_ii is
        ~ 2 e^-12.2 = 1e-5 in every row.  With the second neighbour at +8.5 as there, dq and dk at head dim 120 are ~1e-4 against
        dv ~ 1.6e4, and the split format's absolute floor (2^-26 below 2^-14) alone is 1e-4 of such a maximum;
      * q and k are multiples of 1/2 and 1/8, as the ordered input's: q . k is exact in fp32 in any order of summation.  A rounded
        fp32 dot product of 372 (head dim 120) carries ~1e-4 and the score ~1e-5, which is the relative error of every
        probability beside the diagonal -- and dq, dk consist of nothing else;
      * the bars are asserted to be within reach of a numpy fp32 restatement (tests/test_build_resources_attention_bwd_long.py)."""
    g = torch.Generator().manual_seed(1000 * T + 8 * dm + heads + 77)
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    r = torch.randn(B_, heads, T, dm, generator=g, dtype=torch.float64)
    k = torch.empty_like(r)
    k[..., 0, :] = unit(r[..., 0, :])
    for j in range(1, T):
        e1 = k[..., j - 1, :]
        u = r[..., j, :] - (r[..., j, :] * e1).sum(-1, keepdim=True) * e1
        if j >= 2:                                            # Gram-Schmidt: e1, e2 span keys j-1 and j-2
            e2 = unit(k[..., j - 2, :] - (k[..., j - 2, :] * e1).sum(-1, keepdim=True) * e1)
            u = u - (u * e2).sum(-1, keepdim=True) * e2
        k[..., j, :] = unit(PEAK_CHAIN * e1 + math.sqrt(1.0 - PEAK_CHAIN ** 2) * unit(u))
    k = torch.round(k * math.sqrt(AK.PEAK_SCORE * math.sqrt(dm) / 4.0) * 8.0) / 8.0
    v = torch.randn(B_, heads, T, dm, generator=g, dtype=torch.float64)
    dO = torch.randn(B_, heads, T, dm, generator=g, dtype=torch.float64)
    dO = dO - (dO * v).sum(-1, keepdim=True) / (v * v).sum(-1, keepdim=True) * v
    return AK.as_read(BR.rows_of(4.0 * k, k, v), fmt), AK.as_read(BR.rows_of(dO) * 4096.0, fmt)


def _ordered(T, heads, dm, B_, fmt):
    """attention_long_cases._ordered with the query kernel's key block: the row maximum of query i sits in key block i % 3, every
    other block's best score 40 below it, so the running maximum of sweep 1 rises zero times, once and twice.  Random dO."""
    g = torch.Generator().manual_seed(1000 * T + 8 * dm + heads + 700001)
    qkv = AL._ordered(T, heads, dm, B_, g, KB)
    dctx = torch.randn(B_ * T, heads * dm, generator=g, dtype=torch.float64)
    return AK.as_read(qkv, fmt), AK.as_read(dctx, fmt)


MAKERS = {"random": BK.att_inputs, "uniform": _uniform, "peaked": _peaked, "ordered": _ordered}


@functools.lru_cache(maxsize=4)
def inputs(kind, fmt, T, heads, dm, B_):
    """(qkv rows [B*T, 3H], dctx rows [B*T, H]) as the VALUES the kernel reads (float64).  Shared: never modify."""
    return MAKERS[kind](T, heads, dm, B_, fmt)


def reference_of(qkv, dctx, B_, T, heads, dm):
    q, k, v = BR.heads_of(qkv, B_, T, heads, dm)
    (dO,) = BR.heads_of(dctx, B_, T, heads, dm)
    dq, dk, dv, P, dS = BR.attention_bwd(q, k, v, dO)
    return {"plain": BR.rows_of(dq, dk, dv), "P": P, "q": q, "k": k}


@functools.lru_cache(maxsize=4)
def reference(kind, fmt, T, heads, dm, B_):
    """fp64 dq | dk | dv rows [B*T, 3H] (backward_ops_ref.attention_bwd) on the values the kernel read, with P, q and k."""
    return reference_of(*inputs(kind, fmt, T, heads, dm, B_), B_, T, heads, dm)


def scores(ref):
    return ref["q"] @ ref["k"].transpose(-1, -2) / math.sqrt(ref["q"].shape[-1])


def attention_bwd_np32(qkv, dctx, B_, T, heads, dm):
    """numpy fp32 restatement of backward_ops_ref.attention_bwd on fp32 roundings of the values: dq | dk | dv rows in float64.  What
    plain fp32 arithmetic gives on an input, whatever the kernel."""
    import numpy as np
    f = np.float32
    q, k, v = (t.numpy().astype(f) for t in BR.heads_of(qkv, B_, T, heads, dm))
    dO = BR.heads_of(dctx, B_, T, heads, dm)[0].numpy().astype(f)
    scale = f(1.0 / math.sqrt(dm))
    s = (q @ k.swapaxes(-1, -2)) * scale
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True, dtype=f)
    dp = dO @ v.swapaxes(-1, -2)
    delta = (p * dp).sum(-1, keepdims=True, dtype=f)
    ds = p * (dp - delta) * scale
    outs = (ds @ k, ds.swapaxes(-1, -2) @ q, p.swapaxes(-1, -2) @ dO)
    assert all(o.dtype == f for o in outs)
    return BR.rows_of(*(torch.from_numpy(o).double() for o in outs))


def third_errors(got, ref_rows, H):
    """max |got - ref| / max |ref| of the dq, dk and dv thirds, each against its OWN maximum."""
    return [((got[:, i * H:(i + 1) * H] - ref_rows[:, i * H:(i + 1) * H]).abs().max() /
             (ref_rows[:, i * H:(i + 1) * H].abs().max() + 1e-300)).item() for i in range(3)]


# ----------------------------------------------------------------------------------------------------------- linearity
LINEAR_SHAPE = (273, 1, 8, 1)            # (T, heads, dm, B): three blocks of every loop, 18 tiles
LINEAR_SEED = 1                          # a seed that meets linear_precondition (tests/test_build_resources_attention_bwd_long.py asserts it)
LINEAR_SHIFT = 2                         # dctx is scaled by 2^-2 and 2^+2
LINEAR_DCTX = 3072.0                     # the largest |dctx| * 2^2 stays an fp16 value, the smallest output * 2^-2 above the range's floor
# Every intermediate of the two kernels is fp32 and every operation on the gradient is a product with it or a sum of such
# products, so a power-of-two factor on dctx commutes with every rounding as long as nothing leaves fp32's normal range; the only
# narrower roundings are the stores.  fp16 output: normal range, [2^-14, 65504].  Split output: the lo plane holds
# (x - hi) * 2^11 on fp16's subnormal grid of 2^-24 exactly as long as x >= 2^-12 (backward_kernel_cases.linear_precondition).
# With a factor 2 of margin on both sides, over the nonzero outputs of the fp64 reference at both scaled launches:
LINEAR_RANGE = (2.0 ** -11, 32752.0)


def linear_inputs():
    """backward_kernel_cases.linear_inputs at T = 273: fp16-exact q | k | v and dctx (lo planes zero, so both formats read the
    same values), small q and k so that P stays near uniform and no output sits far below the others."""
    T, heads, dm, B_ = LINEAR_SHAPE
    g = torch.Generator().manual_seed(LINEAR_SEED)
    H = heads * dm
    qkv = torch.randn(B_ * T, 3 * H, generator=g)
    qkv[:, :2 * H] *= 0.25
    dctx = torch.randn(B_ * T, H, generator=g) * LINEAR_DCTX
    return qkv.half().double(), dctx.half().double()


def linear_precondition(qkv, dctx):
    """(smallest, largest) magnitude of the nonzero outputs of the fp64 reference over the two scaled launches.  The scaled dctx
    itself must stay among fp16's normal values (asserted here): it is an input of both formats."""
    T, heads, dm, B_ = LINEAR_SHAPE
    d = dctx.abs()[dctx != 0]
    assert d.max().item() * 2.0 ** LINEAR_SHIFT <= 65504.0 and d.min().item() * 2.0 ** -LINEAR_SHIFT >= 2.0 ** -14
    mags = reference_of(qkv, dctx, B_, T, heads, dm)["plain"].abs().flatten()
    mags = mags[mags > 0]
    return mags.min().item() * 2.0 ** -LINEAR_SHIFT, mags.max().item() * 2.0 ** LINEAR_SHIFT


def all_input_sets():
    """Every (kind, entry, T, heads, dm, B) the GPU module launches for parity."""
    out = [("random",) + c for c in CASES]
    return out + [(kind, entry) + s for kind in ("uniform", "peaked", "ordered") for s in KIND_SHAPES for entry in ENTRIES]
