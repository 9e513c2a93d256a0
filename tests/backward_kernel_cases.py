"""Cases of tests/test_gpu_backward_kernels.py and a mirror of the host dispatch that picks the kernel instance, kept free of
GPU imports so that tests/test_build_resources_backward.py can hold the case lists against the compiled instances on the CPU.

Dispatch mirrored from csrc/backward.hip (advh_attention_bwd_f16, layernorm_bwd_launch), csrc/attention_bwd_f32.hip
(advh_attention_bwd_split) and csrc/attention_bwd_x3.hip (advh_attention_bwd_x3_launch)."""
import functools
import itertools
import math

import torch

import backward_ops_ref as BR

# ----------------------------------------------------------------------------------------------------------- attention
ENTRIES = ("f16", "split", "split_f32")        # advh_attention_bwd_f16 | advh_attention_bwd_split | the same with attention_bwd_mfma_f32 = 1
T_EDGES = (1, 16, 17, 64, 65, 128, 129, 208, 209, 256)      # both edges of every tile-count class, one frame, one whole tile
HEAD_DIMS = (8, 24, 32, 40, 56, 64, 72, 120, 128)           # per padded width D = 32 | 64 | 128: two padded head dims and the exact one


def instance_of(entry, T, dm, forced_f32=False, ragged=False):
    """(kernel, NT, D, TR | NW, RAGGED) the host code launches for this shape; ``ragged``: the entry point with per-clip frames,
    which picks by the row stride T as the batch entry point does by T."""
    nt = (T + 15) // 16
    D = 32 if dm <= 32 else (64 if dm <= 64 else 128)
    cls = 4 if nt <= 4 else (8 if nt <= 8 else (13 if nt <= 13 else 16))
    if entry == "f16":
        if D == 128 and cls == 8:
            cls = 13                                               # head dim 128 has no 8-tile instance
        return ("attention_bwd_kernel", cls, D, dm == 64, ragged)
    if dm <= 64 and not forced_f32:
        return ("attention_bwd_x3_kernel", cls, D, 4 if cls == 16 else 8, ragged)
    return ("attention_bwd_f32_kernel", cls, D, 8 if D <= 64 else 4, ragged)


def refused_f16(T, dm):
    """advh_attention_bwd_f16 refuses head dims above 64 with more than 13 key tiles: attention_bwd_kernel<16, 128, false, *>
    would need 2 * 128 * 320 * 2 + 3 * 256 * 4 = 166 912 bytes of LDS, above the CU's 160 KiB."""
    return dm > 64 and T > 208


def _att_cases():
    out = []
    for (T, dm), entry in itertools.product(itertools.product(T_EDGES, HEAD_DIMS), ENTRIES):      # entries of one shape side by side
        if entry == "split_f32" and dm > 64:
            continue                                               # head dims > 64 run the fp32-MFMA kernel by default ("split")
        if entry == "f16" and refused_f16(T, dm):
            continue                                               # REFUSED_CASES
        out.append((entry, T, 2, dm, 2))
    return out + [(entry, 65, 3, 40, 3) for entry in ENTRIES]      # three heads, three clips, padded head dim


ATT_CASES = _att_cases()                                           # (entry, T, heads, dm, B)
REFUSED_CASES = [(T, dm) for dm in (72, 120, 128) for T in (209, 256)]
PROPERTY_SHAPES = {"f16": (65, 2, 40), "split": (65, 2, 40), "split_f32": (65, 2, 40)}      # (T, heads, dm) of the B-independence check
LINEAR_SHAPE = (17, 1, 8, 1)                                       # (T, heads, dm, B) of the linearity check: two query tiles
PEAKED_SHAPE = (65, 2, 32, 2)


def att_selected(cases=None):
    """{instance: [case, ...]} for the parity cases."""
    sel = {}
    for c in (ATT_CASES if cases is None else cases):
        entry, T, heads, dm, B = c
        sel.setdefault(instance_of("f16" if entry == "f16" else "split", T, dm, entry == "split_f32"), []).append(c)
    return sel


@functools.lru_cache(maxsize=2)
def att_inputs(T, heads, dm, B, fmt):
    """(qkv rows [B*T, 3H], dctx rows [B*T, H]) as the VALUES the kernel reads (float64): fp16 values for the f16 entry,
    22-bit split values for the split entries.  One generator per shape, so the two split entries share inputs and reference."""
    from addvisor_hip import gemm as G
    g = torch.Generator().manual_seed(1000 * T + dm + heads)
    H = heads * dm
    qkv, dctx = torch.randn(B * T, 3 * H, generator=g) * 0.7, torch.randn(B * T, H, generator=g)
    if fmt == "f16":
        return qkv.half().double(), dctx.half().double()
    return G.join_planes(G.split_planes(qkv)).double(), G.join_planes(G.split_planes(dctx)).double()


def peaked_inputs(fmt):
    """Every query attends to its own key: keys of one length in random directions and q_i = 4 k_i with q_i . k_i / sqrt(d) = 34,
    so the row maxima of P exceed 0.999 and the scores span > 40 (asserted from the fp64 reference by the tests).  Two choices keep
    the case inside what fp32 arithmetic can give at the suite's bars, whatever the kernel:
      * the scores are no larger than the span asks for: a score s carries an fp32 error of ~|s| 2^-24, which is the RELATIVE error of
        every small probability and of dS (unscaled random keys gave a plain fp32 evaluation 3e-4 of max|dq|, these give 1e-6);
      * dO_i is orthogonal to v_i: with P_ii ~ 1, dP_ii - delta_i is a difference of nearly equal numbers whose fp32 rounding error,
        eps |dP_ii|, would be eps / (1 - P_ii) of the result.
    With P that peaked every dS is below 1e-3 |dO|: dctx carries a loss scale of 2^12, as the chain's gradients do, or dS would
    sit among fp16's subnormals and dq, dk near the split format's absolute floor of 2^-25."""
    from addvisor_hip import gemm as G
    T, heads, dm, B = PEAKED_SHAPE
    g = torch.Generator().manual_seed(77)
    k = torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64)
    k = k / k.norm(dim=-1, keepdim=True) * math.sqrt(34.0 * math.sqrt(dm) / 4.0)
    v = torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64)
    dO = torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64)
    dO = dO - (dO * v).sum(-1, keepdim=True) / (v * v).sum(-1, keepdim=True) * v
    qkv, dctx = BR.rows_of(4.0 * k, k, v), BR.rows_of(dO) * 4096.0
    if fmt == "f16":
        return qkv.half().double(), dctx.half().double()
    return G.join_planes(G.split_planes(qkv)).double(), G.join_planes(G.split_planes(dctx)).double()


LINEAR_SEED = 2          # set by a search over seeds for one that meets linear_precondition (tests/test_backward_ops_ref_cpu.py asserts it)
LINEAR_SHIFT = 4         # dctx is scaled by 2^-4 and 2^+4


def linear_inputs():
    """fp16-exact q | k | v and dctx (their lo planes are zero, so both formats read the same values and scaling dctx by a power
    of two is exact).  Small q, k keep P near uniform, so no dS sits far below the others."""
    T, heads, dm, B = LINEAR_SHAPE
    g = torch.Generator().manual_seed(LINEAR_SEED)
    H = heads * dm
    qkv = torch.randn(B * T, 3 * H, generator=g)
    qkv[:, :2 * H] *= 0.25
    dctx = torch.randn(B * T, H, generator=g) * 64.0
    return qkv.half().double(), dctx.half().double()


def linear_precondition(qkv, dctx):
    """(smallest, largest) magnitude, over the nonzero dS * scale and the three outputs of the fp64 reference, at the two scaled
    launches.  Scaling by 2^k commutes with every rounding of the kernels iff no rounded quantity leaves the range where its
    format has a full significand: fp16 normal (>= 2^-14, <= 65504) for the fp16 dS and outputs of the f16 entry; for the split
    format, whose lo plane holds (x - hi) * 2^11 -- a multiple of ulp32(x) * 2^11 -- exactly as long as that multiple is on fp16's
    subnormal grid of 2^-24, x >= 2^-12.  The test asks for a factor 2 of margin on both sides: [2^-11, 32752]."""
    T, heads, dm, B = LINEAR_SHAPE
    q, k, v = BR.heads_of(qkv, B, T, heads, dm)
    (dO,) = BR.heads_of(dctx, B, T, heads, dm)
    dq, dk, dv, _, ds = BR.attention_bwd(q, k, v, dO)
    mags = torch.cat([t.abs().flatten() for t in (ds, dq, dk, dv)])
    mags = mags[mags > 0]
    return mags.min().item() * 2.0 ** -LINEAR_SHIFT, mags.max().item() * 2.0 ** LINEAR_SHIFT


LINEAR_RANGE = (2.0 ** -11, 32752.0)

# ----------------------------------------------------------------------------------------------------------- LayerNorm
LN_C = (4, 32, 120, 512, 516, 768, 1024, 1028, 1920, 2048)        # MAXV boundaries (512 | 516, 1024 | 1028), partial last rounds
LN_M = (37, 1, 5)
LN_EPS = 1e-5


def ln_instance_of(x_fmt, dy_fmt, C):
    """(X32, DY32, MAXV) of layernorm_bwd_kernel; fp16 and split operands share an instance (the lo distance is a run-time argument)."""
    return (x_fmt == "f32", dy_fmt == "f32", 2 if C <= 512 else (4 if C <= 1024 else 8))


def _ln_cases():
    """A pruned product: every (C, X32, DY32) with the half-precision operands once as plain fp16 (advh_layernorm_bwd) and once as
    split planes (advh_layernorm_bwd_split); gelu_fwd, dact_src, add, the output form and M rotate with the running count per
    instance, so that each of the 12 instances meets both gelu_fwd values, a dact_src, an add and every output form."""
    out, count = [], {}
    for C, x32, dy32, half in itertools.product(LN_C, (True, False), (True, False), ("f16", "split")):
        x_fmt, dy_fmt = ("f32" if x32 else half), ("f32" if dy32 else half)
        k = count.get(ln_instance_of(x_fmt, dy_fmt, C), 0)
        count[ln_instance_of(x_fmt, dy_fmt, C)] = k + 1
        out.append(dict(C=C, M=LN_M[(k + k // 3) % 3], x=x_fmt, dy=dy_fmt, half=half, gelu=k % 2,
                        dact=half if k % 4 in (1, 2) else None, add=k % 4 in (2, 3), out=("f", "h", "fh")[k % 3]))
    return out


LN_CASES = _ln_cases()
LN_REMAP_CASES = [dict(C=120, B=3, T=5, P=7, half="f16"), dict(C=768, B=2, T=3, P=8, half="split"), dict(C=1920, B=2, T=4, P=5, half="split")]


def ln_case_id(c):
    return "C{C}-M{M}-x_{x}-dy_{dy}-{half}-gelu{gelu}-dact_{dact}-add{add:d}-out_{out}".format(**c)


def offset_rows(ratio=64.0, M=5, C=768, seed=5):
    """fp32 rows mu + sigma * noise with |mu| / sigma = ``ratio``: E[x^2] - mean^2 loses ~ratio^2 * eps of the variance."""
    g = torch.Generator().manual_seed(seed)
    x = (ratio + torch.randn(M, C, generator=g, dtype=torch.float64)).float()
    dy = torch.randn(M, C, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    return x, dy, gamma


def ln_dx_np32(x, dy, gamma, eps, one_pass):
    """numpy fp32 restatement of dx = rstd (g - mean g - xhat mean(g xhat)), g = dy gamma, with the variance either from the
    centred values (two passes, what the kernel does) or as E[x^2] - mean^2 (one pass)."""
    import numpy as np
    f = np.float32
    x, dy, gamma = x.numpy().astype(f), dy.numpy().astype(f), gamma.numpy().astype(f)
    C = f(x.shape[-1])
    mean = x.sum(-1, keepdims=True, dtype=f) / C
    if one_pass:
        var = (x * x).sum(-1, keepdims=True, dtype=f) / C - mean * mean
    else:
        var = ((x - mean) ** 2).sum(-1, keepdims=True, dtype=f) / C
    rstd = f(1.0) / np.sqrt(var + f(eps), dtype=f)
    xhat = (x - mean) * rstd
    g = dy * gamma
    dx = rstd * (g - g.sum(-1, keepdims=True, dtype=f) / C - xhat * ((g * xhat).sum(-1, keepdims=True, dtype=f) / C))
    assert dx.dtype == f
    return torch.from_numpy(dx)


def attention_bwd_f16_np32(q, k, v, dO):
    """numpy fp32 restatement of ``backward_ops_ref.attention_bwd_f16_model``: the same formula and the same fp16 rounding points,
    every sum and product in float32.  Returns the three sums in front of the output conversion."""
    import numpy as np
    f = np.float32
    q, k, v, dO = (t.numpy().astype(f) for t in (q, k, v, dO))
    scale = f(1.0 / math.sqrt(q.shape[-1]))
    s = (q @ k.swapaxes(-1, -2)) * scale
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True, dtype=f)
    dp = dO @ v.swapaxes(-1, -2)
    delta = (p * dp).sum(-1, keepdims=True, dtype=f)
    ds = (p * (dp - delta) * scale).astype(np.float16).astype(f)
    p16 = p.astype(np.float16).astype(f)
    outs = (ds @ k, ds.swapaxes(-1, -2) @ q, p16.swapaxes(-1, -2) @ dO)
    assert all(o.dtype == f for o in outs)
    return tuple(torch.from_numpy(o).double() for o in outs)
