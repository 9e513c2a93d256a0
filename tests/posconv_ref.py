"""The positional convolution of wav2vec2 (modeling_wav2vec2.py:326-379: ``Conv1d(H, H, K, padding K/2, groups G)``, last frame
dropped, GELU, residual add) in fp64, a mirror of the host arithmetic of csrc/posconv_tile.hip and of the gather launch of
csrc/rowops.hip, and the case tables of tests/test_gpu_posconv.py.  Kept free of GPU imports so that
tests/test_posconv_ref_cpu.py can hold the tables against their claims on the CPU.

Plain torch, written from the formulas -- not from the kernels, and not through ``addvisor_hip.embedder``.  The operands a
function is handed are the values the path under test reads (``h.half()`` for the fp16 paths, ``planes_value(split_planes(h))``
for the split paths); everything is computed in float64.

Integer data: with small-integer operands every product and every partial sum is exact in fp32 whatever the summation order,
``gelu_fast(z)`` (csrc/device_math.h) is exactly ``z`` for ``z >= 6`` and exactly ``-0`` for ``z <= -6``, and GELU'(z) is exactly
1 / 0 at ``z = +-16, +-24`` -- so the outputs can be compared bit for bit."""
import functools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from addvisor_hip import gemm as G

K_TILE = 128                                   # taps of the line tile (PC_K)
EXACT_Z = 6.0                                  # |z| from which gelu_fast returns z / -0 exactly


# ------------------------------------------------------------------------------------------------------- fp64 references
def gelu_erf(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(z):
    """d/dz GELU(z) = Phi(z) + z * phi(z)."""
    z = z.double()
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def planes_value(p):
    """fp64 value of a split-format pair ``[2, ...]``: hi + lo * 2^-11, exactly."""
    return p[0].double() + p[1].double() * 2.0 ** -11


def conv_ref(x, w, bias, G_):
    """x [B, T, H], w [H, Cg, K], bias [H] or None -> z [B, T, H]: the grouped convolution with padding K/2, last frame dropped."""
    K, T = w.shape[-1], x.shape[1]
    z = F.conv1d(x.double().transpose(1, 2), w.double(), None if bias is None else bias.double(), padding=K // 2, groups=G_)
    return z[:, :, :T].transpose(1, 2).contiguous()


def forward_ref(h, w, bias, G_, resid=None):
    """``(resid + gelu_erf(z), z)`` with ``z = conv1d(h, w, bias, padding = K // 2, groups = G)[..., :T]``; ``h [B, T, H]``,
    ``w [H, Cg, K]``, ``bias [H]``.  ``resid`` (default ``h``): the fp32 rows the kernel adds to, where they are not the rounded
    operand of the convolution."""
    z = conv_ref(h, w, bias, G_)
    return (h if resid is None else resid).double() + gelu_erf(z), z


def backward_ref(dh, pc, w, G_):
    """Gradient of ``h + gelu_erf(conv(h))`` with respect to ``h`` for the output gradient ``dh`` at pre-activation ``pc``:
    ``dh + conv^T(dh * gelu'(pc))``.  The transposed convolution is written as a correlation with the taps reversed and the
    channel roles swapped: out[t][g, ci] = sum_{k', co} a[t + k' - (K/2 - 1)][g, co] * w[g, co, ci, K - 1 - k']."""
    H, Cg, K = w.shape
    a = (dh.double() * gelu_grad(pc)).transpose(1, 2)                              # [B, H, T]
    wt = w.double().view(G_, Cg, Cg, K).flip(3).transpose(1, 2).reshape(H, Cg, K)  # [g][ci][co][k']
    a = F.pad(a, (K // 2 - 1, K // 2))
    return dh.double() + F.conv1d(a, wt, None, groups=G_).transpose(1, 2)


def tile_weights(w, G_):
    """``w [H, Cg, K]`` -> fp16 ``[g][k-step][n][32]``: the line tile's weight stream, K order (tap, channel):
    element ``(g, s, n, j)`` is ``w[g * Cg + n, ci, k]`` with ``k * Cg + ci = 32 s + j``."""
    H, Cg, K = w.shape
    kk = torch.arange(K * Cg)
    k, ci = kk // Cg, kk % Cg
    flat = w.view(G_, Cg, Cg, K)[:, :, ci, k]                                      # [g][n][(k, ci)]
    return flat.view(G_, Cg, K * Cg // 32, 32).transpose(1, 2).contiguous().half()


def gather_ref(x, G_, K, pad_left):
    """x [B, T, H] -> [G, B, T + K, Cg]: data rows [pad_left, pad_left + T), zeros elsewhere (advh_posconv_gather's layout)."""
    B, T, H = x.shape
    Cg = H // G_
    out = torch.zeros(G_, B, T + K, Cg, dtype=x.dtype)
    out[:, :, pad_left:pad_left + T] = x.view(B, T, G_, Cg).permute(2, 0, 1, 3)
    return out


# ---------------------------------------------------------------------------------------- mirrors of the host arithmetic
def lds_bytes(Cg, T):
    """advh_posconv_tile_lds_bytes: a three-slot ring of four-k-step weight blocks, then the clip's T + 127 staged rows of eight
    16-byte slots rounded up to whole-wave loads; -1 where the tile does not run."""
    if T <= 0 or T > 256 or Cg not in (48, 64):
        return -1
    nX = ((T + K_TILE - 1) * 8 + 63) & ~63
    b = 3 * 4 * Cg * 64 + nX * 16
    return b if b <= 160 * 1024 else -1


def per_cu(Cg, T):
    return 2 if lds_bytes(Cg, T) <= 80 * 1024 else 1


def grid(Cg, T, G_, B):
    return min(256 * per_cu(Cg, T), G_ * B)


def nj_of(T):
    """Frame tiles of each of the four wavefronts: tiles wv, wv + 4, ... below nt."""
    nt = (T + 15) // 16
    return tuple(max(0, min(4, (nt - wv + 3) // 4)) for wv in range(4))


GATHER_TRIP = 4096 * 256                        # items (four channels) one trip of the gather's grid-stride loop covers


def gather_items(Cg, G_, B, T, K):
    return G_ * B * (T + K) * (Cg // 4)


# ------------------------------------------------------------------------------------------------------ the case tables
T_EDGES = tuple(sorted({t for nt in range(1, 17) for t in (16 * (nt - 1) + 1, 16 * nt)}))       # both ends of every tile count
CG = (48, 64)
SWEEP = tuple((Cg, 2, 2, T) for Cg in CG for T in T_EDGES)                                      # (Cg, G, B, T)
NAMED = ((64, 16, 17, 130),        # 272 tiles on a grid of 256: a second trip on another group; one workgroup per CU; gather's second trip
         (48, 16, 33, 17),         # 528 tiles on a grid of 512: a second trip at two workgroups per CU
         (64, 2, 3, 129), (48, 2, 3, 225), (48, 2, 3, 226),                                    # the per_cu edges
         (48, 1, 1, 1), (64, 16, 1, 256))
TILE_CASES = SWEEP + NAMED
IDENTICAL_CASES = tuple((Cg, 2, 2, T) for Cg in CG for T in (1, 17, 49, 199, 256)) + ((48, 16, 33, 17),)

GEMM_T = (1, 16, 17, 199, 256, 257, 300)
GEMM_CG = ((32, 16), (48, 128), (64, 128), (120, 128))                                          # (Cg, K); 32 / 16: the tiny config
GEMM_CASES = tuple((Cg, 2, 3, T, K) for Cg, K in GEMM_CG for T in GEMM_T)                       # (Cg, G, B, T, K)
SECOND_TRIP = (64, 16, 17, 130)


# --------------------------------------------------------------------------------------------------------- data makers
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def int_forward(Cg, G_, B, T, K=K_TILE):
    """h in {-2..2}, w in {-2..2}, bias in {-3..3} as fp32 tensors (h [B, T, H], w [H, Cg, K], bias [H]).  With 16 taps of 32
    channels (the tiny config) uniform weights leave z a standard deviation of 45 and 11 % of the elements inside (-6, 6);
    there the weights are +-2 only (deviation 64), which keeps the bit-exact class above 90 % of the elements."""
    g = _gen("int_fwd", Cg, G_, B, T, K)
    H = Cg * G_
    h = _ints(g, -2, 2, B, T, H)
    w = _ints(g, -2, 2, H, Cg, K) if K >= K_TILE else 4 * _ints(g, 0, 1, H, Cg, K) - 2
    return h, w, _ints(g, -3, 3, H)


@functools.lru_cache(maxsize=None)
def rand_forward(Cg, G_, B, T, K=K_TILE):
    """The distribution of tests/test_gpu_gemm.py::test_posconv_line_tile."""
    g = _gen("rand_fwd", Cg, G_, B, T, K)
    H = Cg * G_
    return (torch.randn(B, T, H, generator=g), torch.randn(H, Cg, K, generator=g) / (K * Cg) ** 0.5,
            torch.randn(H, generator=g) * 0.1)


@functools.lru_cache(maxsize=None)
def int_backward(Cg, G_, B, T, K=K_TILE):
    """dh in {-1, 0, 1}, pc in {+-16, +-24} (GELU' exactly 1 or 0), w in {-2..2}."""
    g = _gen("int_bwd", Cg, G_, B, T, K)
    H = Cg * G_
    pc = torch.tensor([-24.0, -16.0, 16.0, 24.0])[torch.randint(0, 4, (B, T, H), generator=g)]
    return _ints(g, -1, 1, B, T, H), pc, _ints(g, -2, 2, H, Cg, K)


@functools.lru_cache(maxsize=None)
def rand_backward(Cg, G_, B, T, K=K_TILE):
    """dh ~ N(0, 1), pc ~ 1.5 N(0, 1) (the spread of tests/gemm_desc_ref.py's dact_src), w as in ``rand_forward``."""
    g = _gen("rand_bwd", Cg, G_, B, T, K)
    H = Cg * G_
    return (torch.randn(B, T, H, generator=g), torch.randn(B, T, H, generator=g) * 1.5,
            torch.randn(H, Cg, K, generator=g) / (K * Cg) ** 0.5)


def operand(x, split):
    """(the fp16-side tensor a path is handed for fp32 values ``x``, the fp64 values it reads from it)."""
    if split:
        p = G.split_planes(x)
        return p, planes_value(p)
    return x.half(), x.half().double()


@functools.lru_cache(maxsize=None)
def forward_case(kind, split, Cg, G_, B, T, K=K_TILE):
    """(h, w, bias, ref, z) of one case: fp32 data, and the fp64 reference on the operands the path reads.  Shared between the
    tests that use it; never modified."""
    h, w, bias = (int_forward if kind == "int" else rand_forward)(Cg, G_, B, T, K)
    ref, z = forward_ref(operand(h, split)[1], operand(w, split)[1], bias, G_, resid=h)
    return h, w, bias, ref, z


@functools.lru_cache(maxsize=None)
def backward_case(kind, split, Cg, G_, B, T, K=K_TILE):
    """(dh, pc fp16-side tensor, w, ref): ``pc`` as stored (fp16 or plane pair), the reference on the stored values."""
    dh, pc, w = (int_backward if kind == "int" else rand_backward)(Cg, G_, B, T, K)
    pcs, pcv = operand(pc, split)
    return dh, pcs, w, backward_ref(dh, pcv, operand(w, split)[1], G_)


def exact_expected(h, z):
    """Where |z| >= 6: h + max(z, 0), the value an exact-GELU kernel must produce bit for bit (fp64; integers below 2^24)."""
    return h.double() + z.clamp_min(0.0)


def np_gelu_fast(x):
    """csrc/device_math.h's gelu_fast in numpy fp32 (rcp as a correctly rounded 1 / x, exp2 as numpy's)."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    u = (x * f(0.70710678118654752440)).astype(f)
    ax = np.abs(u)
    t = (f(1) / (f(0.3275911) * ax + f(1)).astype(f)).astype(f)
    p = (f(1.061405429) * t + f(-1.453152027)).astype(f)
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = (p * t + f(c)).astype(f)
    e = np.exp2((f(-1.4426950408889634) * ax * ax).astype(f)).astype(f)
    r = np.copysign((f(1) - (p * t).astype(f) * e).astype(f), u)
    return ((f(0.5) * x).astype(f) * (f(1) + r).astype(f)).astype(f)
