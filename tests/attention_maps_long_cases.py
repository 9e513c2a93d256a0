"""Cases of tests/test_gpu_attention_maps_long.py and the mirror of the host dispatch of csrc/attention_maps_long.hip
(advh_attention_maps_long, advh_attention_bwd_value_long, advh_rollout_step_long, advh_rollout_relevance_long), free of GPU
imports so that tests/test_build_resources_attention_maps_long.py can hold the cases against the compiled instances.

The operand format and ``fuse`` are run-time arguments; an instance is (kernel, D[, GRAD]) with D = 32 | 64 | 128 the padded head
dim: three statistics kernels, six maps kernels (probabilities / gradient form) and three value kernels.  The inputs are those of
tests/attention_bwd_long_cases.py (random, uniform, peaked, ordered / forced rescale), which this module only imports."""
import functools
import math

import numpy as np
import torch

import attention_bwd_long_cases as C
import backward_ops_ref as BR

ENTRIES = C.ENTRIES                                          # operand formats: plain fp16 (qkv_lo == 0) | split plane pairs
STATS_KERNEL, MAPS_KERNEL, VALUE_KERNEL = "attention_stats_long_kernel", "attention_maps_long_kernel", "attention_bwd_value_long_kernel"
BLOCK = 128                                                  # rows a workgroup owns and rows of a staged block, every kernel
HEAD_DIMS = C.HEAD_DIMS
INSTANCE_DIMS = C.INSTANCE_DIMS                              # 24, 64, 120: one head dim per padded width
T_ALL = (1, 16, 17, 128, 129, 256, 257, 273, 385, 513)
HEADS, B = 3, 2                                              # an odd head count, so that the fold order of the fusions shows
FUSIONS = (0, 1, 2, 3)
DSCALES = (1.0, 1.0 / 4096.0)
ADVERSARIAL_T = C.ADVERSARIAL_T
FRAMES_T, FRAMES = C.FRAMES_T, C.FRAMES                      # (513, 1, 257), (513, 256, 273), (513, 17, 129) at stride 513
TOL_MAPS = 5e-6                                              # of max|ref| per returned tensor: the whole-clip maps kernel's bar
TOL_SPLIT, TOL_F16 = C.TOL_SPLIT, C.TOL_F16                  # dV: tests/test_gpu_lrp.py
TOL_ROLLOUT = 2e-5                                           # tests/test_gpu_attention_rollout.py
ROLLOUT_T = (1, 17, 64, 65, 257, 513)
ROLLOUT_PARAMS = ((1.0, 1.0, 0.0, 1), (1.0, 1.0, 1.0, 0))    # (alpha, beta, gamma, normalize): plain | gradient rollout
ROLLOUT_FRAMES = {257: (257, 1, 130), 513: (513, 256, 273), 65: (65, 64, 17), 17: (17, 1, 16), 64: (64, 63, 1), 1: (1, 1, 1)}
# |rowsum(P) - 1| of stats_np32 below over the parity and adversarial inputs, measured by
# tests/test_build_resources_attention_maps_long.py (which asserts it stays under this figure): the row-sum bar of the GPU suite is
# max(ROWSUM_FLOOR, 4 x the restatement's deviation on the same inputs), the 4 for the MFMA's other summation order.
ROWSUM_FLOOR = 1e-6
ROWSUM_NP32_WORST = 3e-7                                     # measured 2.24e-7 (random, split, T = 513, head dim 120)

MAPS_CASES = [(entry, T, HEADS, dm, B) for dm in INSTANCE_DIMS for entry in ENTRIES for T in T_ALL]
MAPS_CASES += [(entry, 273, HEADS, dm, B) for dm in HEAD_DIMS if dm not in INSTANCE_DIMS for entry in ENTRIES]
KIND_SHAPES = [(ADVERSARIAL_T, HEADS, dm, B) for dm in INSTANCE_DIMS]
FRAME_CASES = [(entry, FRAMES_T, HEADS, dm, 3) for dm in INSTANCE_DIMS for entry in ENTRIES]


def case_id(c):
    return "{}-T{}-h{}-d{}-B{}".format(*c)


def padded(dm):
    return C.padded(dm)


def lds_stats(D):
    return BLOCK * (D + 4) * 4


def lds_maps(D, grad):
    return (2 if grad else 1) * BLOCK * (D + 4) * 4


def lds_value(D):
    return (2 * BLOCK * (D + 4) + 2 * BLOCK) * 4


def instances_of(T, dm):
    """{(kernel, D) | (MAPS_KERNEL, D, grad)} a parity case launches: every form of both entries, with and without dctx."""
    D = padded(dm)
    return {(STATS_KERNEL, D), (MAPS_KERNEL, D, False), (MAPS_KERNEL, D, True), (VALUE_KERNEL, D)}


def blocks(T):
    return -(-T // BLOCK)


# ----------------------------------------------------------------------------------------------------------- references
def reference_of(qkv, dctx, B_, T, heads, dm):
    """fp64 on the values read: P [B, heads, T, T], dP = dO V^T, dv rows [B*T, H]."""
    q, k, v = BR.heads_of(qkv, B_, T, heads, dm)
    (dO,) = BR.heads_of(dctx, B_, T, heads, dm)
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dm), -1)
    return {"P": P, "dP": dO @ v.transpose(-1, -2), "dv": BR.rows_of(P.transpose(-1, -2) @ dO)}


@functools.lru_cache(maxsize=4)
def reference(kind, fmt, T, heads, dm, B_):
    """Of the maker's own (qkv, dctx): what the value backward is held against."""
    return reference_of(*C.inputs(kind, fmt, T, heads, dm, B_), B_, T, heads, dm)


def maps_inputs(kind, fmt, T, heads, dm, B_):
    """(qkv, dctx) of the maps cases: the maker's, except that the peaked qkv goes with the RANDOM maker's dctx.  The peaked
    maker builds dO_i orthogonal to v_i and scales it by 2^12 (for dS_ii of the full backward).  In exact arithmetic
    dP_ii = dO_i . v_i would be 0; on the values the kernel reads (rounded to fp16 or 22 bits) it is the small residue, of order
    1 to 10, of dm products of magnitude ~4096 |dO||v| that cancel.  P_ii ~ 1 on that diagonal and P_ij ~ 1e-5 off it, so these
    residues ARE the maximum of the gradient-weighted map P * dP (~10).  An fp32 accumulator's partial sums in that dot product
    are ~1e4 (ulp 1e-3), that is 1e-4 of the map's maximum and twenty times the 5e-6 bar: no arithmetic on the fp32-input
    matrix instruction resolves it, whatever the kernel.
    tests/test_build_resources_attention_maps_long.py asserts both halves of this on the CPU with numpy fp32 (``ga_np32``); the
    streamed kernel measured 1.75e-4 on that combination at head dim 24.  The probabilities of the peaked input, which are what
    it is peaked for, are checked under every fusion, and the value backward runs on the maker's own dctx."""
    qkv, dctx = C.inputs(kind, fmt, T, heads, dm, B_)
    if kind == "peaked":
        dctx = C.inputs("random", fmt, T, heads, dm, B_)[1]
    return qkv, dctx


@functools.lru_cache(maxsize=4)
def maps_reference(kind, fmt, T, heads, dm, B_):
    return reference_of(*maps_inputs(kind, fmt, T, heads, dm, B_), B_, T, heads, dm)


def ga_np32(qkv, dctx, B_, T, heads, dm):
    """numpy fp32 restatement of the per-head gradient-weighted map max(P * dP, 0) [B, heads, T, T] (float32)."""
    f = np.float32
    v = BR.heads_of(qkv, B_, T, heads, dm)[2].numpy().astype(f)
    dO = BR.heads_of(dctx, B_, T, heads, dm)[0].numpy().astype(f)
    P = stats_np32(qkv, B_, T, heads, dm)[2]
    return np.maximum(P * (dO @ v.swapaxes(-1, -2)).astype(f), f(0))


def fused(t, fuse):
    """[B, heads, T, T] -> the output of ``fuse``."""
    return t if fuse == 0 else (t.mean(1) if fuse == 1 else (t.max(1).values if fuse == 2 else t.min(1).values))


def maps_ref(ref, grad, dscale, fuse):
    m = (ref["P"] * (ref["dP"] * dscale)).clamp_min(0) if grad else ref["P"]
    return fused(m, fuse)


def stats_np32(qkv, B_, T, heads, dm, block=BLOCK):
    """numpy fp32 restatement of the statistics kernel's recurrences -- the scaled score one rounded product, keys in blocks of
    ``block`` with a running maximum m (log2 domain) and a running sum l rescaled by 2^(m_old - m_new) -- and of the maps kernel's
    P = exp2(s c2 - m) (1 / l): ``(m, 1 / l, P)`` as float32 arrays.  What plain fp32 gives on an input, whatever the kernel."""
    f = np.float32
    q, k, _ = (t.numpy().astype(f) for t in BR.heads_of(qkv, B_, T, heads, dm))
    c2 = f(f(1.0 / math.sqrt(dm)) * f(1.4426950408889634))
    s = ((q @ k.swapaxes(-1, -2)).astype(f) * c2).astype(f)
    m = np.full(s.shape[:-1], -np.inf, dtype=f)
    l = np.zeros(s.shape[:-1], dtype=f)
    for k0 in range(0, T, block):
        blk = s[..., k0:k0 + block]
        m_new = np.maximum(m, blk.max(-1))
        alpha = np.exp2(m - m_new).astype(f)
        l = (l * alpha + np.exp2(blk - m_new[..., None]).astype(f).sum(-1, dtype=f)).astype(f)
        m = m_new
    inv = (f(1.0) / l).astype(f)
    P = (np.exp2(s - m[..., None]).astype(f) * inv[..., None]).astype(f)
    return m, inv, P


def rowsum_deviation(P):
    """max |sum_j P[.., i, j] - 1| with the sum in float64."""
    return float(np.abs(np.asarray(P, dtype=np.float64).sum(-1) - 1.0).max())


def rowsum_bar(qkv, B_, T, heads, dm):
    return max(ROWSUM_FLOOR, 4.0 * rowsum_deviation(stats_np32(qkv, B_, T, heads, dm)[2]))


# ----------------------------------------------------------------------------------------------------------- rollout
def rollout_inputs(T, B_=3):
    """(M, X) fp32 [B, T, T]: M rows of a softmax (an attention map), X a product of two such maps plus the identity."""
    g = torch.Generator().manual_seed(4000 + T)
    M = torch.softmax(torch.randn(B_, T, T, generator=g, dtype=torch.float64) * 2.0, -1)
    X = torch.softmax(torch.randn(B_, T, T, generator=g, dtype=torch.float64), -1) + torch.eye(T, dtype=torch.float64)
    return M.float(), X.float()


def rollout_step_ref(M, X, alpha, beta, gamma, normalize, frames=None):
    """fp64 on the fp32 values; with frames, clip b is its top-left Tv x Tv block alone, zeros elsewhere."""
    M, X = M.double(), X.double()
    Y = torch.zeros_like(X)
    for b in range(X.shape[0]):
        tv = X.shape[1] if frames is None else frames[b]
        m, x = M[b, :tv, :tv], X[b, :tv, :tv]
        y = alpha * x + beta * (m @ x) + gamma * m
        Y[b, :tv, :tv] = y / (alpha + beta * m.sum(-1, keepdim=True)) if normalize else y
    return Y


def rollout_relevance_ref(X, frames=None):
    X = X.double()
    rel = torch.zeros(X.shape[0], X.shape[1], dtype=torch.float64)
    for b in range(X.shape[0]):
        tv = X.shape[1] if frames is None else frames[b]
        rel[b, :tv] = X[b, :tv, :tv].sum(0) / tv
    return rel
