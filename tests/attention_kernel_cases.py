"""Cases of tests/test_gpu_attention_kernels.py and a mirror of the host dispatch that picks the forward attention kernel
instance, kept free of GPU imports so that tests/test_build_resources_attention.py can hold the case lists against the
compiled instances and tests/test_attention_kernel_cases_cpu.py can assert every input's preconditions on the CPU.

Dispatch mirrored from csrc/attention.hip (advh_attention_f16, advh_attention_split)."""
import functools
import itertools
import math

import numpy as np
import torch

import backward_ops_ref as BR
import embedder_ops_ref

ENTRIES = ("f16", "split")                                   # advh_attention_f16 | advh_attention_split
T_EDGES = (1, 16, 17, 64, 65, 128, 129, 208, 209, 256)       # both edges of every tile-count class, one frame, one whole tile
HEAD_DIMS = (8, 24, 32, 40, 56, 64, 72, 120, 128)            # per padded width D = 32 | 64 | 128: two padded head dims and the exact one
STREAM_T = (112, 113, 224, 225)                              # the edges of the streaming kernel's key blocks of 112
STREAM_KB = 112
TOL_SPLIT = 5e-6                                             # tests/test_gpu_split.py TOL_KERNEL, here per (clip, head) block
CLASSES = {4: (1, 64), 8: (65, 128), 13: (129, 208), 16: (209, 256)}      # T range of each tile-count class NT


def instance_of(entry, T, dm):
    """(kernel, template arguments ...) the host code launches for this shape; for the streaming kernel the tuple also carries
    (key blocks, query rounds) behind the template arguments."""
    nt = (T + 15) // 16
    cls = 4 if nt <= 4 else (8 if nt <= 8 else (13 if nt <= 13 else 16))
    if dm == 64:
        return ("attention_tr_kernel" if entry == "f16" else "attention_x3_tr_kernel", cls)
    D = 32 if dm <= 32 else (64 if dm <= 64 else 128)
    if entry == "f16":
        if D == 128 and cls == 8:
            cls = 13                                         # head dim 128 has no 8-tile instance
        return ("attention_kernel", cls, D)
    if D == 128:
        return ("attention_x3_stream_kernel", 7, 128, -(-T // STREAM_KB), -(-nt // 8))
    return ("attention_x3_kernel", cls, D)


def compiled_name(inst):
    """The instance without the run-time figures of the streaming kernel: what the compiler instantiates."""
    return inst[:3] if inst[0] == "attention_x3_stream_kernel" else inst


def _att_cases():
    out = [(entry, T, 2, dm, 2) for (T, dm), entry in itertools.product(itertools.product(T_EDGES, HEAD_DIMS), ENTRIES)]
    out += [(entry, 65, 3, 40, 3) for entry in ENTRIES]      # three heads, three clips, padded head dim
    return out + [(entry, T, 2, dm, 2) for (T, dm), entry in itertools.product(itertools.product(STREAM_T, (72, 120, 128)), ENTRIES)]


ATT_CASES = _att_cases()                                     # (entry, T, heads, dm, B)
UNIFORM_SHAPES = [(T, 2, dm, 2) for T in (17, 113, 209, 225) for dm in (40, 64, 120)]      # (T, heads, dm, B): every template of both entries
PEAKED_SHAPES = [(65, 2, 40, 2), (65, 2, 64, 2), (129, 2, 120, 2)]
ORDERED_SHAPE = (256, 2, 120, 2)
BATCH_SHAPES = [(65, 2, 40), (65, 2, 64), (129, 2, 120)]     # (T, heads, dm): clip 0 of three against a launch of its own
ISOLATION_SHAPES = [(17, 2, 40, 2), (17, 2, 72, 2), (17, 2, 64, 2)]
NAN_SHAPES = [(65, 2, 40, 2), (65, 2, 64, 2), (129, 2, 120, 2)]
TEMPLATES = {"f16": {"attention_kernel", "attention_tr_kernel"},
             "split": {"attention_x3_kernel", "attention_x3_tr_kernel", "attention_x3_stream_kernel"}}

PEAK_SCORE, PEAK_SPAN = 34.0, 40.0                           # q_i . k_i / sqrt(d); what the scores of every row must span
ORDERED_SCORE, ORDERED_GAP = 21.0, 40.0                      # |score| of a key block's direction; margin of the target block


def att_selected(cases=None):
    """{compiled instance: [case, ...]} for the parity cases."""
    sel = {}
    for c in (ATT_CASES if cases is None else cases):
        sel.setdefault(compiled_name(instance_of(c[0], c[1], c[3])), []).append(c)
    return sel


def stream_reach(cases=None):
    """{(key blocks, query rounds)} the parity cases give the streaming kernel."""
    insts = (instance_of(c[0], c[1], c[3]) for c in (ATT_CASES if cases is None else cases))
    return {i[3:] for i in insts if i[0] == "attention_x3_stream_kernel"}


def att_id(c):
    return "{}-T{}-h{}-d{}-B{}".format(*c)


# ----------------------------------------------------------------------------------------------------------- input makers
HEAD_SCALE = (1.0, 0.25, 4.0)          # exact powers of two on the V columns of head 0, 1, 2: no head hides behind a larger one


def as_read(rows, fmt):
    """float64 values of ``rows`` as the kernel reads them: fp16 values for the f16 entry, joined 22-bit values for split."""
    from addvisor_hip import gemm as G
    if fmt == "f16":
        return rows.half().double()
    return G.join_planes(G.split_planes(rows)).double()


def _scale_v(v):
    """v [B, heads, T, dm] with head h multiplied by HEAD_SCALE[h]."""
    return v * torch.tensor(HEAD_SCALE[:v.shape[1]], dtype=v.dtype).view(1, -1, 1, 1)


def _random(T, heads, dm, B, g):
    q, k, v = (torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64) * 1.5 for _ in range(3))
    return BR.rows_of(q, k, _scale_v(v))


def _uniform(T, heads, dm, B, g):
    """q = 0: every score is exactly 0, every probability exactly 1 / T, ctx the mean of V over the T real keys."""
    rows = _random(T, heads, dm, B, g)
    rows[:, :heads * dm] = 0.0
    return rows


def _peaked(T, heads, dm, B, g):
    """As backward_kernel_cases.peaked_inputs: keys of one length, q_i = 4 k_i, q_i . k_i / sqrt(d) = 34.  The scores are no
    larger than the span of 40 asks for: a score s carries an fp32 error of ~|s| 2^-24, which is the relative error of every
    small probability.  Random directions alone do not span 40 at head dims 64 and 120 (their cosines are ~1 / sqrt(d)), so the
    directions form a chain: key j is -1/2 of key j-1's direction plus sqrt(3)/2 of a random direction orthogonal to it.  Every
    row then has a neighbour at a score of -17 (a span of 51), its second neighbour at +8.5, the rest near 0."""
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    r = torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64)
    k = torch.empty_like(r)
    k[..., 0, :] = unit(r[..., 0, :])
    for j in range(1, T):
        prev = k[..., j - 1, :]
        k[..., j, :] = -0.5 * prev + math.sqrt(0.75) * unit(r[..., j, :] - (r[..., j, :] * prev).sum(-1, keepdim=True) * prev)
    k = unit(k) * math.sqrt(PEAK_SCORE * math.sqrt(dm) / 4.0)
    v = torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64) * 1.5
    return BR.rows_of(4.0 * k, k, _scale_v(v))


def ordered_target(T):
    """Key block that holds the row maximum of query i: i % 3, so every query tile carries all three kinds in its lanes."""
    return torch.arange(T) % 3


def ordered_block(T):
    """Key block (of 112) of key j."""
    return torch.arange(T) // STREAM_KB


ORDERED_WEIGHTS = ((1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.2, -1.0, 1.0))      # per target block: q's weight on each block's direction


def _ordered(T, heads, dm, B, g):
    """Three key blocks, three orthogonal directions e_0, e_1, e_2 (the first three coordinates): key j = a e_block(j) + noise,
    query i = a (w_0 e_0 + w_1 e_1 + w_2 e_2) + noise with w = ORDERED_WEIGHTS[i % 3] and a^2 / sqrt(d) = 21; the noise lives in
    the other coordinates and moves a score by ~0.6.  So the scores of query i are ~+21 in its target block and ~-21 (-25 for
    block 0 of target 2) in the others: the row maximum sits in block i % 3 and the best score of each other block is more
    than 40 below it.  For the streaming kernel that is: target 0 -- the first block dominates, the later ones add terms of
    e^-40; target 1 -- the maximum rises once and alpha = e^-42 wipes the first block's sums out of fp32's sight; target 2 -- the
    maximum rises twice (-25 -> -21 -> +21).  |score| stays at what the margin of 40 needs (see _peaked), and every q and k is
    a multiple of 1/8: the products are multiples of 2^-6 and their partial sums stay below 2^11, so q . k is EXACT in fp32 in
    any order of summation and the score carries the one rounding of its scaling.  (With unrounded noise a plain fp32 dot
    product rounds ~120 times at |q . k| ~ 230; a numpy fp32 evaluation then missed the split bar by itself.)  Multiples of
    1/8 are fp16 values, so both entries read the same q and k."""
    grid = lambda t: torch.round(t * 8.0) / 8.0
    a = grid(torch.tensor(math.sqrt(ORDERED_SCORE * math.sqrt(dm)), dtype=torch.float64))
    sigma = math.sqrt(0.6)
    blk, tgt = ordered_block(T), ordered_target(T)
    k = torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64) * sigma
    q = torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64) * sigma
    k[..., :3], q[..., :3] = 0.0, 0.0
    k[..., torch.arange(T), blk] = a
    q[..., :3] = a * torch.tensor(ORDERED_WEIGHTS, dtype=torch.float64)[tgt]
    v = torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64) * 1.5
    return BR.rows_of(grid(q), grid(k), _scale_v(v))


MAKERS = {"random": _random, "uniform": _uniform, "peaked": _peaked, "ordered": _ordered}
KIND_SHAPES = {"uniform": UNIFORM_SHAPES, "peaked": PEAKED_SHAPES, "ordered": [ORDERED_SHAPE]}      # (T, heads, dm, B) per adversarial kind


@functools.lru_cache(maxsize=8)
def inputs(kind, fmt, T, heads, dm, B):
    """qkv rows [B*T, 3H] (q | k | v side by side, heads side by side in each) as the VALUES the kernel reads (float64).  One
    generator per (kind, shape), so the two entries draw the same numbers and differ by their format's rounding alone.  Cached
    and shared: never modify the result."""
    g = torch.Generator().manual_seed(1000 * T + 8 * dm + heads + 100003 * sorted(MAKERS).index(kind))
    return as_read(MAKERS[kind](T, heads, dm, B, g), fmt)


@functools.lru_cache(maxsize=8)
def reference(kind, fmt, T, heads, dm, B):
    """{"ctx": [B, heads, T, dm], "p": [B, heads, T, T], "q" | "k" | "v"} in float64, from tests/embedder_ops_ref.py."""
    q, k, v = BR.heads_of(inputs(kind, fmt, T, heads, dm, B), B, T, heads, dm)
    ctx, p = embedder_ops_ref.attention(q, k, v)
    return {"ctx": ctx, "p": p, "q": q, "k": k, "v": v}


def scores(ref):
    return ref["q"] @ ref["k"].transpose(-1, -2) / math.sqrt(ref["q"].shape[-1])


def all_input_sets():
    """Every (kind, entry, T, heads, dm, B) the GPU module launches for parity."""
    out = [("random",) + c for c in ATT_CASES]
    for kind, shapes in KIND_SHAPES.items():
        out += [(kind, entry) + s for s in shapes for entry in ENTRIES]
    return out


def set_id(s):
    return "{}-{}-T{}-h{}-d{}-B{}".format(*s)


# ----------------------------------------------------------------------------------------------------------- bars
def block_max(t):
    """max|t| per (clip, head) block of [B, heads, T, dm], NaN entries left out (0 for a block that is all NaN)."""
    return torch.nan_to_num(t.abs(), nan=0.0).amax((-1, -2), keepdim=True)


def split_ratio(got, ref):
    """Worst |got - ref| / (5e-6 max|ref| of the (clip, head) block) over the elements where ref is a number."""
    err = torch.nan_to_num((got - ref).abs() / (TOL_SPLIT * block_max(ref)).clamp_min(1e-300), nan=0.0)
    return err.masked_fill(torch.isnan(ref), 0.0).max().item()


def f16_bound(ref):
    """|out - ref| <= 2^-11 (sum_j p_j |v_j| + |ref|) (1 + 2^-6) + 5e-6 max|v| elementwise: the bound of
    tests/test_gpu_split.py test_attention_f16_kernel (the kernel rounds the probabilities to fp16 in front of P V and the
    result to fp16), with max|v| taken per (clip, head)."""
    return 2.0 ** -11 * (ref["p"] @ ref["v"].abs() + ref["ctx"].abs()) * (1 + 2.0 ** -6) + TOL_SPLIT * block_max(ref["v"])


def f16_ratio(got, ref):
    """Worst |err| / bound over the elements where the reference is a number."""
    ratio = (got - ref["ctx"]).abs() / f16_bound(ref)
    return torch.nan_to_num(ratio, nan=0.0).masked_fill(torch.isnan(ref["ctx"]), 0.0).max().item()


def attention_np32(q, k, v):
    """numpy fp32 restatement of softmax(Q K^T / sqrt(d)) V: every sum and product in float32."""
    f = np.float32
    q, k, v = (t.numpy().astype(f) for t in (q, k, v))
    s = (q @ k.swapaxes(-1, -2)) * f(1.0 / math.sqrt(q.shape[-1]))
    e = np.exp(s - s.max(-1, keepdims=True))
    out = (e / e.sum(-1, keepdims=True, dtype=f)) @ v
    assert out.dtype == f
    return torch.from_numpy(out).double()
