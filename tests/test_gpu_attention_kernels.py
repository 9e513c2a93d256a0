"""Kernel-level suite of the forward attention (csrc/attention.hip): every compiled instance of its five kernel templates, behind
advh_attention_f16 and advh_attention_split, against the float64 ``embedder_ops_ref.attention`` evaluated on the CPU on the
operands the kernel saw.  The case lists, the input makers and the mirror of the host dispatch live in
tests/attention_kernel_cases.py; tests/test_build_resources_attention.py holds them against the compiled instances and
tests/test_attention_kernel_cases_cpu.py asserts the preconditions of every input from the reference.

Buffers.  q | k | v rows sit in one allocation with PAD rows of NaN behind row B*T (per plane for the split entry, whose plane
distance is the plane stride): legal to read, so a tail tile that reads them unmasked poisons ctx.  ctx is prefilled with a NaN
bit pattern no arithmetic produces and has GUARD rows behind it: every element of the body must lose the pattern, every guard row
must keep it.  After every in-range launch the sticky range flag (advh_split_overflow) is clear.

Bars.  Split entry: per (clip, head) block, max|out - ref| <= 5e-6 max|ref| of that block (the project's TOL_KERNEL, per block
and not once per launch).  f16 entry, elementwise: |out - ref| <= 2^-11 (sum_j p_j |v_j| + |ref|) (1 + 2^-6) + 5e-6 max|v|,
max|v| per (clip, head) (tests/test_gpu_split.py test_attention_f16_kernel).  The adversarial inputs keep the same bars.

Worst |err| / bar per instance over all its cases (random, uniform, peaked, ordered, NaN), measured on an MI355X.  The f16
instances sit at the fp16 half-ulps of P and of the store, which is their bound; the split instances at 8 - 20 % of theirs.  What
that margin still sees, measured once with three mistakes compiled in: a pad key counted by attention_x3_kernel's mask fails
every T below the instance's NT * 16 keys (uniform: 1 / T of every element); the streaming kernel rescaling only its main
accumulator by alpha gives ~100 bars at two or three key blocks and passes at one; attention_kernel storing one 4-column group past a
padded head dim fails on the neighbouring head's columns or the guard rows, and passes at head dims 32 and 128.
  attention_tr_kernel<4>              0.730  random T=17 dm=64      attention_x3_tr_kernel<4>           0.089  random T=64 dm=64
  attention_tr_kernel<8>              0.776  random T=65 dm=64      attention_x3_tr_kernel<8>           0.111  random T=128 dm=64
  attention_tr_kernel<13>             0.707  random T=129 dm=64     attention_x3_tr_kernel<13>          0.079  random T=208 dm=64
  attention_tr_kernel<16>             0.703  random T=256 dm=64     attention_x3_tr_kernel<16>          0.111  random T=209 dm=64
  attention_kernel<4, 32>             0.677  random T=16 dm=24      attention_x3_kernel<4, 32>          0.084  random T=64 dm=8
  attention_kernel<8, 32>             0.717  random T=65 dm=32      attention_x3_kernel<8, 32>          0.120  random T=65 dm=24
  attention_kernel<13, 32>            0.759  random T=208 dm=32     attention_x3_kernel<13, 32>         0.163  random T=208 dm=24
  attention_kernel<16, 32>            0.767  random T=209 dm=24     attention_x3_kernel<16, 32>         0.144  random T=209 dm=32
  attention_kernel<4, 64>             0.755  random T=16 dm=40      attention_x3_kernel<4, 64>          0.089  random T=17 dm=56
  attention_kernel<8, 64>             0.755  random T=128 dm=40     attention_x3_kernel<8, 64>          0.152  random T=65 dm=40 heads=3 B=3
  attention_kernel<13, 64>            0.750  random T=129 dm=56     attention_x3_kernel<13, 64>         0.098  random T=208 dm=40
  attention_kernel<16, 64>            0.703  random T=256 dm=40     attention_x3_kernel<16, 64>         0.125  random T=209 dm=56
  attention_kernel<4, 128>            0.764  random T=17 dm=128     attention_x3_stream_kernel<7, 128>  0.192  ordered T=256 dm=120
  attention_kernel<13, 128>           0.796  random T=112 dm=120
  attention_kernel<16, 128>           0.794  random T=256 dm=128
"""
import pytest
import torch

import attention_kernel_cases as K
import backward_ops_ref as BR
import embedder_ops_ref
from addvisor_hip import _lib, gemm as G

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PAD = 16                                        # NaN rows behind the last q | k | v row
GUARD = 4                                       # rows allocated behind ctx, which no kernel may touch
EINVAL, EUNSUPPORTED = -1, -4
FILL = 0x7DAB                                   # an fp16 NaN whose payload neither the inputs nor any arithmetic carry
NAN = float("nan")


def stream():
    return torch.cuda.current_stream().cuda_stream


def pack(vals, entry, nan_at=()):
    """float64 rows [B*T, 3H] -> (operand tensor on the CPU with its PAD rows of NaN, float64 values it holds in its first B*T
    rows).  ``nan_at``: index tuples (row, column), slices allowed, set to NaN after the conversion (in both planes)."""
    rows, width = vals.shape
    if entry == "f16":
        t = torch.full((rows + PAD, width), NAN, dtype=torch.float16)
        t[:rows] = vals.half()
    else:
        t = torch.full((2, rows + PAD, width), NAN, dtype=torch.float16)
        t[:, :rows] = G.split_planes(vals)
    for idx in nan_at:
        t[(Ellipsis,) + tuple(idx)] = NAN
    seen = t[:rows].double() if entry == "f16" else G.join_planes(t[:, :rows]).double()
    return t, seen


def launch(entry, qkv, B, T, H, heads, dev, rows=None, qkv_lo=None, ctx_lo=None, null=None):
    """One call of the entry's C function on an operand tensor from ``pack``.  Returns (rc, ctx on the CPU with its guard rows,
    flag): ctx is [rows + GUARD, H] fp16 or [2, rows + GUARD, H] planes, prefilled with FILL; flag is the sticky range flag after
    the launch (cleared in front of it)."""
    _lib.init()
    lib = _lib.lib()
    rows = B * T if rows is None else rows
    qd = qkv.to(dev)
    shape = (rows + GUARD, H) if entry == "f16" else (2, rows + GUARD, H)
    ctx = torch.full(shape, FILL, dtype=torch.int16, device=dev).view(torch.float16)
    qp, cp = (None if null == "qkv" else qd.data_ptr()), (None if null == "ctx" else ctx.data_ptr())
    torch.cuda.synchronize()
    lib.advh_split_overflow(1)
    if entry == "f16":
        rc = lib.advh_attention_f16(qp, cp, B, T, H, heads, stream())
    else:
        rc = lib.advh_attention_split(qp, qd.stride(0) if qkv_lo is None else qkv_lo, cp, ctx.stride(0) if ctx_lo is None else ctx_lo,
                                      B, T, H, heads, stream())
    torch.cuda.synchronize()
    return rc, ctx.cpu(), lib.advh_split_overflow(1)


def untouched(t):
    return bool((t.contiguous().view(torch.int16) == FILL).all())


def body_of(entry, out, rows):
    """The first ``rows`` rows of a launch's output ([rows, H] or [2, rows, H]), after checking that every element of them was
    written and no guard row was."""
    body, guard = out[..., :rows, :], out[..., rows:, :]
    assert untouched(guard), "guard rows behind ctx were written"
    missed = int((body.contiguous().view(torch.int16) == FILL).sum())
    assert missed == 0, f"{missed} element(s) of ctx were not written"
    return body


def values_of(entry, out, B, T, heads, dm):
    """float64 [B, heads, T, dm] of a launch's output (``body_of`` checks included)."""
    body = body_of(entry, out, B * T)
    rows = body.double() if entry == "f16" else G.join_planes(body).double()
    return BR.heads_of(rows, B, T, heads, dm)[0]


def ratio_of(entry, got, ref):
    return K.f16_ratio(got, ref) if entry == "f16" else K.split_ratio(got, ref["ctx"])


def run_case(dev, kind, case):
    """Launch one (entry, T, heads, dm, B) on the cached inputs of ``kind`` and hold it against the cached reference."""
    entry, T, heads, dm, B = case
    vals = K.inputs(kind, entry, T, heads, dm, B)
    t, seen = pack(vals, entry)
    assert torch.equal(seen, vals)                                   # the reference's values are the kernel's operands
    rc, out, flag = launch(entry, t, B, T, heads * dm, heads, dev)
    assert rc == 0 and flag == 0
    got = values_of(entry, out, B, T, heads, dm)
    assert torch.isfinite(got).all()
    ratio = ratio_of(entry, got, K.reference(kind, entry, T, heads, dm, B))
    print(f"attention fwd [{entry}] {kind} T={T} heads={heads} dm={dm} B={B} {K.compiled_name(K.instance_of(entry, T, dm))}: "
          f"worst |err| / bar {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", K.ATT_CASES, ids=K.att_id)
def test_attention_parity(gpu_device, case):
    """N(0, 1) * 1.5 operands, the V columns of head h scaled by 1, 1/4, 4: every instance at both edges of its tile-count class,
    every padded head dim, the streaming kernel at the edges of its key blocks."""
    run_case(gpu_device, "random", case)


@pytest.mark.parametrize("entry", K.ENTRIES)
@pytest.mark.parametrize("shape", K.UNIFORM_SHAPES, ids=str)
def test_attention_uniform(gpu_device, entry, shape):
    """q = 0: every probability is exactly 1 / T and ctx is the mean of V over the T real keys.  A pad key that is counted (l = T
    would become T + 1 .. 16 ceil(T / 16)), or a real key that is dropped, moves every element by ~1 / T of itself."""
    run_case(gpu_device, "uniform", (entry,) + shape)


@pytest.mark.parametrize("entry", K.ENTRIES)
@pytest.mark.parametrize("shape", K.PEAKED_SHAPES, ids=str)
def test_attention_peaked(gpu_device, entry, shape):
    """Every row of P has one entry above 0.999 and scores that span more than 40 (tests/test_attention_kernel_cases_cpu.py):
    without the subtraction of the row maximum exp overflows or the small probabilities vanish."""
    run_case(gpu_device, "peaked", (entry,) + shape)


@pytest.mark.parametrize("entry", K.ENTRIES)
def test_attention_ordered(gpu_device, entry):
    """The streaming kernel's online softmax over three key blocks, each query's maximum in block i % 3 with a margin of 40: the
    first block dominates | the maximum rises once and the rescale wipes the first block out | the maximum rises twice."""
    run_case(gpu_device, "ordered", (entry,) + K.ORDERED_SHAPE)


@pytest.mark.parametrize("entry", K.ENTRIES)
@pytest.mark.parametrize("shape", K.BATCH_SHAPES, ids=str)
def test_attention_does_not_depend_on_the_batch(gpu_device, entry, shape):
    """Clip 0 of a three-clip launch equals, bit for bit, a one-clip launch on clip 0 alone; a repeated launch repeats its bits."""
    T, heads, dm = shape
    vals = K.inputs("random", entry, T, heads, dm, 3)
    t3, _ = pack(vals, entry)
    t1, _ = pack(vals[:T], entry)
    rc3, out3, f3 = launch(entry, t3, 3, T, heads * dm, heads, gpu_device)
    rc3b, out3b, f3b = launch(entry, t3, 3, T, heads * dm, heads, gpu_device)
    rc1, out1, f1 = launch(entry, t1, 1, T, heads * dm, heads, gpu_device)
    assert rc3 == rc3b == rc1 == 0 and f3 == f3b == f1 == 0
    bits = lambda x: x.contiguous().view(torch.int16)
    assert torch.equal(bits(out3), bits(out3b))
    assert torch.equal(bits(body_of(entry, out3, 3 * T)[..., :T, :]), bits(body_of(entry, out1, T)))


@pytest.mark.parametrize("entry", K.ENTRIES)
@pytest.mark.parametrize("shape", K.ISOLATION_SHAPES, ids=str)
def test_attention_isolation(gpu_device, entry, shape):
    """A head (padded head dims 40 and 72: its columns are the neighbours of the other head's zero-filled chunks; 64: the
    transposing kernels) or a clip (T = 17: its rows are what the other clip's tail tile would read) made of NaN turns its own
    ctx into NaN and leaves the other's bits alone."""
    T, heads, dm, B = shape
    H = heads * dm
    vals = K.inputs("random", entry, T, heads, dm, B)
    bits = lambda x: x.contiguous().view(torch.int16)

    def run(nan_at):
        rc, out, flag = launch(entry, pack(vals, entry, nan_at)[0], B, T, H, heads, gpu_device)
        assert rc == 0 and flag == 0
        return body_of(entry, out, B * T)

    clean = run(())
    assert torch.isfinite(clean.float()).all()
    for bad in range(heads):
        cols = [slice(i * H + bad * dm, i * H + (bad + 1) * dm) for i in range(3)]       # q, k and v of that head
        got = run([(slice(0, B * T), c) for c in cols])
        for h in range(heads):
            mine = slice(h * dm, (h + 1) * dm)
            if h == bad:
                assert torch.isnan(got[..., mine].float()).all(), f"head {h} of NaN"
            else:
                assert torch.equal(bits(got[..., mine]), bits(clean[..., mine])), f"head {h} next to a head of NaN"
    for bad in range(B):
        got = run([(slice(bad * T, (bad + 1) * T), slice(0, 3 * H))])
        for b in range(B):
            mine = slice(b * T, (b + 1) * T)
            if b == bad:
                assert torch.isnan(got[..., mine, :].float()).all(), f"clip {b} of NaN"
            else:
                assert torch.equal(bits(got[..., mine, :]), bits(clean[..., mine, :])), f"clip {b} next to a clip of NaN"


@pytest.mark.parametrize("entry", K.ENTRIES)
@pytest.mark.parametrize("where", ["q", "k", "v"])
@pytest.mark.parametrize("shape", K.NAN_SHAPES, ids=str)
def test_attention_nan_propagation(gpu_device, entry, where, shape):
    """One NaN in one q row (clip 1, head 0, a middle row), one k row (the LAST key, which the tail tile shares with the masked pad
    keys) or one v element (last key, last dim): the output is NaN exactly where the fp64 reference is, elsewhere finite and
    within the bar, and the range flag stays clear (NaN is no range error: tests/test_gpu_split_contract.py)."""
    T, heads, dm, B = shape
    H = heads * dm
    row, col = {"q": (T + T // 2, 3), "k": (2 * T - 1, H + 5), "v": (2 * T - 1, 2 * H + dm - 1)}[where]
    t, seen = pack(K.inputs("random", entry, T, heads, dm, B), entry, [(row, col)])
    assert int(torch.isnan(seen).sum()) == 1
    q, k, v = BR.heads_of(seen, B, T, heads, dm)
    ctx, p = embedder_ops_ref.attention(q, k, v)
    ref = {"ctx": ctx, "p": torch.nan_to_num(p, nan=0.0), "v": torch.nan_to_num(v, nan=0.0)}
    want = torch.isnan(ctx)
    expect = torch.zeros_like(want)
    if where == "q":
        expect[1, 0, T // 2, :] = True
    elif where == "k":
        expect[1, 0] = True
    else:
        expect[1, 0, :, dm - 1] = True
    assert torch.equal(want, expect)                                 # the reference's NaN set is the one the arithmetic implies
    rc, out, flag = launch(entry, t, B, T, H, heads, gpu_device)
    assert rc == 0 and flag == 0
    got = values_of(entry, out, B, T, heads, dm)
    assert torch.equal(torch.isnan(got), want)
    assert torch.isfinite(got[~want]).all()
    ratio = ratio_of(entry, got, ref)                                # over the elements where the reference is a number
    print(f"attention fwd [{entry}] nan-{where} T={T} heads={heads} dm={dm} B={B} {K.compiled_name(K.instance_of(entry, T, dm))}: "
          f"worst |err| / bar {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("entry", K.ENTRIES)
def test_attention_arguments(gpu_device, entry):
    """What the two entries refuse, and that a refused call leaves ctx alone."""
    dev = gpu_device

    def call(B=2, T=17, H=80, heads=2, alloc=None, **kw):
        aB, aT = alloc or (max(B, 1), max(T, 1))
        t, _ = pack(torch.zeros(aB * aT, 3 * H, dtype=torch.float64), entry)
        rc, out, flag = launch(entry, t, B, T, H, heads, dev, rows=aB * aT, **kw)
        assert untouched(out) and flag == 0
        return rc

    assert call(T=257) == EUNSUPPORTED
    assert call(H=24, heads=2) == EUNSUPPORTED                       # head dim 12: no multiple of 8
    assert call(H=136, heads=1) == EUNSUPPORTED                      # head dim 136 > 128
    assert call(null="qkv") == EINVAL
    assert call(null="ctx") == EINVAL
    assert call(H=80, heads=3) == EINVAL                             # H % heads
    assert call(heads=0) == EINVAL
    for B, T in ((0, 17), (-1, 17), (2, 0), (2, -3)):
        assert call(B=B, T=T, alloc=(2, 17)) == EINVAL
    if entry == "split":
        lo, clo = (2 * 17 + PAD) * 240, (2 * 17 + GUARD) * 80
        assert lo % 8 == 0 and clo % 4 == 0
        assert call(qkv_lo=0) == EINVAL
        assert call(qkv_lo=lo + 4) == EINVAL                         # qkv_lo % 8
        assert call(ctx_lo=0) == EINVAL
        assert call(ctx_lo=clo + 2) == EINVAL                        # ctx_lo % 4
    # the same call, in range, computes
    t, _ = pack(K.inputs("random", entry, 17, 2, 40, 2), entry)
    rc, out, flag = launch(entry, t, 2, 17, 80, 2, dev)
    assert rc == 0 and flag == 0
    body_of(entry, out, 34)
