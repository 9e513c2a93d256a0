"""Cases of tests/test_gpu_attention_long.py and the mirror of the host dispatch of csrc/attention_long.hip
(advh_attention_long_f16, advh_attention_long_split), free of GPU imports so that tests/test_build_resources_attention_long.py
can hold the cases against the compiled instances and assert every input's preconditions on the CPU.

The makers, the float64 reference and the bars are those of tests/attention_kernel_cases.py; what is new is the ordered input
with key blocks of the instance's own size."""
import functools
import itertools
import math

import torch

import attention_kernel_cases as K
import backward_ops_ref as BR
import embedder_ops_ref

ENTRIES = K.ENTRIES
KERNEL = "attention_long_kernel"
QB = 128                                                     # queries per workgroup: eight tiles of 16
T_KB256 = (257, 272, 273, 512, 513)                          # one key in the last block | whole last tile | one query row in the
T_KB112 = (257, 336, 337, 448, 449)                          # last tile | whole last block | one key and one query row past it
SHORT = (1, 16, 17, 113, 256)                                # strides the whole-clip kernels take too; 113: two blocks of 112
HEAD_DIMS = (24, 32, 40, 64, 72, 120, 128)                   # per padded width D = 32 | 64 | 128: a padded head dim and the exact one
DMA_DIM = 64                                                 # split entry: the DMA-staged instance; 40 keeps the register-staged one
B, HEADS = 2, 2


def instance_of(entry, T, dm):
    """(kernel, NTB, D, NP, TR, key blocks, query blocks) the host code launches for row stride ``T`` and head dim ``dm``.  TR: the
    split instance for head dim 64 exactly, staged by the LDS DMA."""
    D = 32 if dm <= 32 else (64 if dm <= 64 else 128)
    NP = 1 if entry == "f16" else 2
    NTB = 7 if (NP == 2 and D == 128) else 16
    return (KERNEL, NTB, D, NP, NP == 2 and dm == 64, -(-T // (NTB * 16)), -(-T // QB))


def compiled_name(inst):
    return inst[:5]


def key_block(entry, dm):
    return instance_of(entry, 1, dm)[1] * 16


def long_strides(entry, dm):
    return T_KB112 if key_block(entry, dm) == 112 else T_KB256


def _cases():
    out = [(entry, T, HEADS, dm, B) for dm in HEAD_DIMS for entry in ENTRIES for T in long_strides(entry, dm)]
    out += [(entry, 273, 3, 40, 3) for entry in ENTRIES]     # three heads, three clips, padded head dim
    return out + [(entry, T, HEADS, dm, B) for T, dm, entry in itertools.product(SHORT, HEAD_DIMS, ENTRIES)]


CASES = _cases()                                             # (entry, T, heads, dm, B)
INSTANCE_DIMS = (32, 40, 64, 120)                            # with both entries, all seven instances (f16: 40 and 64 share one)
UNIFORM_SHAPES = [(273, 2, dm, 2) for dm in (24, 40, 64, 120)] + [(513, 2, 64, 2), (449, 2, 72, 2)]
PEAKED_SHAPES = [(273, 2, dm, 2) for dm in INSTANCE_DIMS]


def ordered_T(entry, dm):
    """Three key blocks of the instance's size, the third 17 keys long: a whole tile and one row."""
    return 2 * key_block(entry, dm) + 17


ORDERED_CASES = [(entry, ordered_T(entry, dm), 2, dm, 2) for dm in INSTANCE_DIMS for entry in ENTRIES]
# frames of three clips of row stride T: (T, a, m) with m % 16 == 1
FRAMES = {513: ((513, 1, 257), (513, 256, 273), (513, 17, 129)), 449: ((449, 1, 257), (449, 256, 273), (449, 17, 113))}
FRAME_CASES = [(entry, T, 2, dm, 3) for T, dms in ((513, (24, 40, 64, 120)), (449, (120,))) for dm in dms for entry in ENTRIES
               if (T == 449) == (key_block(entry, dm) == 112)]


def selected(cases=None):
    """{compiled instance: [case, ...]} for the parity cases."""
    sel = {}
    for c in (CASES if cases is None else cases):
        sel.setdefault(compiled_name(instance_of(c[0], c[1], c[3])), []).append(c)
    return sel


def case_id(c):
    return "{}-T{}-h{}-d{}-B{}".format(*c)


def ordered_block(T, KB):
    return torch.arange(T) // KB


def _ordered(T, heads, dm, B, g, KB):
    """attention_kernel_cases._ordered with key blocks of ``KB``: key j = a e_block(j) + noise, query i = a (w . e) + noise with
    w = ORDERED_WEIGHTS[i % 3] and a^2 / sqrt(d) = 21, noise of variance 0.45, every q and k a multiple of 1/8 (q . k exact in
    fp32).  The row maximum of query i sits in block i % 3, the best score of each other block more than 40 below it: the
    running maximum of the online softmax rises zero times, once (alpha = e^-42 wipes the first block out) and twice."""
    grid = lambda t: torch.round(t * 8.0) / 8.0
    a = grid(torch.tensor(math.sqrt(K.ORDERED_SCORE * math.sqrt(dm)), dtype=torch.float64))
    sigma = math.sqrt(0.45)                                  # 0.6 there; three times the keys and head dim 32 ask for less
    blk, tgt = ordered_block(T, KB), K.ordered_target(T)
    k = torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64) * sigma
    q = torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64) * sigma
    k[..., :3], q[..., :3] = 0.0, 0.0
    k[..., torch.arange(T), blk] = a
    q[..., :3] = a * torch.tensor(K.ORDERED_WEIGHTS, dtype=torch.float64)[tgt]
    v = torch.randn(B, heads, T, dm, generator=g, dtype=torch.float64) * 1.5
    return BR.rows_of(grid(q), grid(k), K._scale_v(v))


@functools.lru_cache(maxsize=4)
def inputs(kind, fmt, T, heads, dm, B):
    """As attention_kernel_cases.inputs (shared, never modified); ``ordered`` is this module's, by the instance's key block."""
    if kind != "ordered":
        return K.inputs(kind, fmt, T, heads, dm, B)
    g = torch.Generator().manual_seed(1000 * T + 8 * dm + heads + 700001)
    return K.as_read(_ordered(T, heads, dm, B, g, key_block(fmt, dm)), fmt)


@functools.lru_cache(maxsize=4)
def reference(kind, fmt, T, heads, dm, B):
    q, k, v = BR.heads_of(inputs(kind, fmt, T, heads, dm, B), B, T, heads, dm)
    ctx, p = embedder_ops_ref.attention(q, k, v)
    return {"ctx": ctx, "p": p, "q": q, "k": k, "v": v}


def all_input_sets():
    """Every (kind, entry, T, heads, dm, B) the GPU module launches for parity."""
    out = [("random",) + c for c in CASES]
    out += [("uniform", entry) + s for s in UNIFORM_SHAPES for entry in ENTRIES]
    out += [("peaked", entry) + s for s in PEAKED_SHAPES for entry in ENTRIES]
    return out + [("ordered",) + c for c in ORDERED_CASES]
