"""Kernel-level suite of the input-gradient chain's attention and LayerNorm backward (csrc/backward.hip,
attention_bwd_x3.hip, attention_bwd_f32.hip): every compiled instance against the float64 restatement of
tests/backward_ops_ref.py, evaluated on the CPU on the operands the kernel saw.  The case lists and the mirror of the host
dispatch live in tests/backward_kernel_cases.py; tests/test_build_resources_backward.py holds them against the compiled
instances.

Bars.  Split entries (both kernels): 5e-6 of the maximum of dq, dk and dv EACH (the project's kernel-level bar of the
fp32-class mode).  LayerNorm fp32 output: 2e-5 of max|ref|.  The f16 attention entry: see ``test_attention_bwd_f16``."""
import functools

import pytest
import torch

import backward_kernel_cases as K
import backward_ops_ref as BR
from addvisor_hip import _lib, gemm as G

pytestmark = pytest.mark.gpu

TOL_SPLIT = 5e-6
TOL_LN = 2e-5
GUARD = 4                                       # rows allocated behind every output, which no kernel may touch
EINVAL, EUNSUPPORTED = -1, -4
NAN16 = torch.full((1,), float("nan"), dtype=torch.float16).view(torch.int16).item()


def stream():
    return torch.cuda.current_stream().cuda_stream


def pack(vals, fmt):
    """float64 values -> the CPU tensor in the kernel's operand format, and the float64 values that tensor holds."""
    if fmt == "f32":
        t = vals.float()
        return t, t.double()
    if fmt == "f16":
        t = vals.half()
        return t, t.double()
    t = G.split_planes(vals)
    return t, G.join_planes(t).double()


def untouched(t):
    """Every element still has the bit pattern of the NaN prefill."""
    return bool((t.cpu().view(torch.int16 if t.dtype == torch.float16 else torch.int32) ==
                 (NAN16 if t.dtype == torch.float16 else torch.full((1,), float("nan")).view(torch.int32).item())).all())


# =========================================================================================================== attention
def launch_attention(entry, qkv, dctx, B, T, heads, dm, dev):
    """One launch on operand tensors already in the entry's format.  Returns (rc, output tensor on the CPU, guard rows included):
    [B*T + GUARD, 3H] fp16 for the f16 entry, [2, B*T + GUARD, 3H] planes for the split entries, prefilled with NaN."""
    _lib.init()
    H, lib = heads * dm, _lib.lib()
    qd, dd = qkv.to(dev), dctx.to(dev)
    if entry == "f16":
        out = torch.full((B * T + GUARD, 3 * H), float("nan"), dtype=torch.float16, device=dev)
        rc = lib.advh_attention_bwd_f16(qd.data_ptr(), dd.data_ptr(), out.data_ptr(), B, T, H, heads, stream())
    else:
        out = torch.full((2, B * T + GUARD, 3 * H), float("nan"), dtype=torch.float16, device=dev)
        _lib.check(lib.advh_set_option(b"attention_bwd_mfma_f32", int(entry == "split_f32")), "advh_set_option")
        try:
            rc = lib.advh_attention_bwd_split(qd.data_ptr(), qd.stride(0), dd.data_ptr(), dd.stride(0), out.data_ptr(), out.stride(0),
                                              B, T, H, heads, stream())
        finally:
            lib.advh_set_option(b"attention_bwd_mfma_f32", 0)
    torch.cuda.synchronize()
    return rc, out.cpu()


def values_of(entry, out, rows):
    """float64 [rows, 3H] of a launch's output, after checking that every element was written and the guard rows were not."""
    body, guard = (out[:rows], out[rows:]) if entry == "f16" else (out[:, :rows], out[:, rows:])
    assert untouched(guard), "guard rows behind dqkv were written"
    got = body.double() if entry == "f16" else G.join_planes(body).double()
    assert torch.isfinite(body.float()).all(), "an element of dqkv was not written"
    return got


@functools.lru_cache(maxsize=4)
def packed_inputs(T, heads, dm, B, fmt, kind="random"):
    """(qkv tensor, dctx tensor, qkv values, dctx values): built once per shape and format, shared by the entries and never modified."""
    vals = {"random": lambda: K.att_inputs(T, heads, dm, B, fmt), "peaked": lambda: K.peaked_inputs(fmt),
            "linear": K.linear_inputs}[kind]()
    (q_t, q_v), (d_t, d_v) = pack(vals[0], fmt), pack(vals[1], fmt)
    return q_t, d_t, q_v, d_v


@functools.lru_cache(maxsize=4)
def reference(T, heads, dm, B, fmt, kind="random"):
    """fp64 results on the values the kernel reads: plain (dq | dk | dv rows) and, for fp16 operands, the kernel's rounding model
    with the error of its fp32 restatement."""
    _, _, qv, dv_ = packed_inputs(T, heads, dm, B, fmt, kind)
    q, k, v = BR.heads_of(qv, B, T, heads, dm)
    (dO,) = BR.heads_of(dv_, B, T, heads, dm)
    dq, dk, dv, P, dS = BR.attention_bwd(q, k, v, dO)
    ref = {"plain": BR.rows_of(dq, dk, dv), "P": P, "dS": dS, "q": q, "k": k, "v": v, "dO": dO}
    if fmt == "f16":
        ref["model"] = BR.attention_bwd_f16_model(q, k, v, dO)
        ref["np32"] = K.attention_bwd_f16_np32(q, k, v, dO)
    return ref


def thirds(rows, H):
    return (("dq", rows[:, :H]), ("dk", rows[:, H:2 * H]), ("dv", rows[:, 2 * H:]))


def check_split(entry, got, ref, H, what):
    worst = 0.0
    for (name, a), (_, b) in zip(thirds(got, H), thirds(ref["plain"], H)):
        err = ((a - b).abs().max() / (b.abs().max() + 1e-300)).item()          # each third against its OWN maximum
        print(f"attention bwd [{entry}] {what} {name}: rel err {err:.2e}")
        assert err <= TOL_SPLIT, name
        worst = max(worst, err)
    return worst


def check_f16(got, ref, B, T, heads, dm, what):
    """See test_attention_bwd_f16 for the bound."""
    H = heads * dm
    m, (q, k, dO) = ref["model"], (ref["q"], ref["k"], ref["dO"])
    ds16, p16 = m["ds"].half().double().abs(), m["p"].half().double().abs()
    amax = lambda t, d: t.abs().amax(d, keepdim=True)
    flip = {"dq": amax(ds16, -1) * amax(k, -2),                 # dq[i, d] = sum_j dS[i, j] k[j, d]
            "dk": amax(ds16, -2).transpose(-1, -2) * amax(q, -2),          # dk[j, d] = sum_i dS[i, j] q[i, d]
            "dv": amax(p16, -2).transpose(-1, -2) * amax(dO, -2)}          # dv[j, d] = sum_i P[i, j] dO[i, d]
    worst = 0.0
    for i, ((name, a), (_, plain)) in enumerate(zip(thirds(got, H), thirds(ref["plain"], H))):
        model, pre = BR.rows_of(m[name]), m[name + "_pre"]
        slack = 4.0 * (ref["np32"][i] - pre).abs().max().item()
        bound = 2.0 ** -10 * (1 + 2.0 ** -6) * model.abs() + 2 * 2.0 ** -10 * BR.rows_of(flip[name].expand_as(pre)) + slack
        err = (a - model).abs()
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        rel_plain = ((a - plain).abs().max() / (plain.abs().max() + 1e-300)).item()
        print(f"attention bwd [f16] {what} {name}: worst |err| / bound vs the fp16 model {ratio:.3f} (fp32 slack {slack:.2e}), "
              f"rel err vs plain fp64 {rel_plain:.2e}")
        assert ratio <= 1.0, name
        assert rel_plain < 1e-2, name
        worst = max(worst, ratio)
    return worst


def att_id(c):
    return "{}-T{}-h{}-d{}-B{}".format(*c)


@pytest.mark.parametrize("case", [c for c in K.ATT_CASES if c[0] != "f16"], ids=att_id)
def test_attention_bwd_split(gpu_device, case):
    """advh_attention_bwd_split, by default (attention_bwd_x3_kernel for head dims <= 64, attention_bwd_f32_kernel above) and under
    ``attention_bwd_mfma_f32`` (attention_bwd_f32_kernel for every head dim), against fp64 on the joined planes: 5e-6 per third."""
    entry, T, heads, dm, B = case
    q_t, d_t, _, _ = packed_inputs(T, heads, dm, B, "split")
    rc, out = launch_attention(entry, q_t, d_t, B, T, heads, dm, gpu_device)
    assert rc == 0
    check_split(entry, values_of(entry, out, B * T), reference(T, heads, dm, B, "split"), heads * dm, K.instance_of("split", T, dm, entry == "split_f32"))


@pytest.mark.parametrize("case", [c for c in K.ATT_CASES if c[0] == "f16"], ids=att_id)
def test_attention_bwd_f16(gpu_device, case):
    """advh_attention_bwd_f16 against ``backward_ops_ref.attention_bwd_f16_model``, elementwise, and against plain fp64 (1e-2 of
    each third's maximum, the bar of tests/test_gpu_backward.py, there over the three thirds at once).

    The kernel and the model round at the same points -- dS * scale and P to fp16 in front of the three output products, the
    outputs to fp16 -- and differ in what lies between them: the kernel evaluates S, P, dP, delta and the output sums in fp32.
    For an output element with the model's unrounded sum ``pre``:
      * the kernel's sum differs from ``pre`` by its fp32 arithmetic.  Its size depends on the MFMA's summation order, so it is
        not derived but taken as 4x the largest error that a numpy fp32 restatement of the same formula, roundings included,
        shows against the float64 model on the same inputs, over that third (``slack``);
      * an fp16 operand whose fp32 value lies within that fp32 error of a rounding boundary may round the other way than in the
        model, by one fp16 ulp <= 2^-10 of itself.  That happens to a few operands in a thousand; two such flips of the LARGEST
        term of the sum are allowed per output element: 2 * 2^-10 max|dS or P| max|k, q or dO| over the summed index;
      * two sums that close round to fp16 values at most one ulp further apart: 2^-10 |model| (1 + 2^-6).
    |out - model| <= 2^-10 |model| (1 + 2^-6) + 2^-9 max|operand| max|operand| + slack; the test asserts worst |err| / bound <= 1."""
    entry, T, heads, dm, B = case
    q_t, d_t, _, _ = packed_inputs(T, heads, dm, B, "f16")
    rc, out = launch_attention(entry, q_t, d_t, B, T, heads, dm, gpu_device)
    assert rc == 0
    check_f16(values_of(entry, out, B * T), reference(T, heads, dm, B, "f16"), B, T, heads, dm, K.instance_of("f16", T, dm))


@pytest.mark.parametrize("T,dm", K.REFUSED_CASES)
def test_attention_bwd_f16_refuses_wide_heads_above_208_frames(gpu_device, T, dm):
    """Head dims above 64 with T > 208 select attention_bwd_kernel<16, 128, false>, whose 166 912 bytes of LDS exceed the CU's
    160 KiB: ADVH_EUNSUPPORTED, dqkv untouched (include/addvisor_hip.h states the limit).  T = 208 computes: ATT_CASES."""
    assert ("f16", 208, 2, dm, 2) in K.ATT_CASES
    q_t, d_t, _, _ = packed_inputs(T, 2, dm, 2, "f16")
    rc, out = launch_attention("f16", q_t, d_t, 2, T, 2, dm, gpu_device)
    assert rc == EUNSUPPORTED
    assert untouched(out)


@pytest.mark.parametrize("entry", K.ENTRIES)
def test_attention_bwd_does_not_depend_on_the_batch(gpu_device, entry):
    """Clip 0 of a three-clip launch equals, bit for bit, a one-clip launch on clip 0 alone; a repeated launch repeats its bits."""
    T, heads, dm = K.PROPERTY_SHAPES[entry]
    fmt = "f16" if entry == "f16" else "split"
    q_t, d_t, _, _ = packed_inputs(T, heads, dm, 3, fmt)
    rc3, out3 = launch_attention(entry, q_t, d_t, 3, T, heads, dm, gpu_device)
    rc3b, out3b = launch_attention(entry, q_t, d_t, 3, T, heads, dm, gpu_device)
    rc1, out1 = launch_attention(entry, q_t[..., :T, :].contiguous(), d_t[..., :T, :].contiguous(), 1, T, heads, dm, gpu_device)
    assert rc3 == rc3b == rc1 == 0
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(out3), bits(out3b))
    assert torch.equal(bits(out3[..., :T, :]), bits(out1[..., :T, :]))
    values_of(entry, out1, T)


@pytest.mark.parametrize("entry", K.ENTRIES)
def test_attention_bwd_is_linear_in_the_gradient(gpu_device, entry):
    """csrc/backward.hip: "the whole chain is linear in the gradient", which is what makes the power-of-two loss scale exact.
    Scaling dctx by 2^-4 and 2^+4 scales dq, dk and dv by exactly that factor, bit for bit (for the split entries: both planes),
    on inputs for which the fp64 reference shows that no rounded quantity leaves its format's full-precision range
    (backward_kernel_cases.linear_precondition)."""
    T, heads, dm, B = K.LINEAR_SHAPE
    fmt = "f16" if entry == "f16" else "split"
    lo, hi = K.linear_precondition(*K.linear_inputs())
    assert K.LINEAR_RANGE[0] <= lo and hi <= K.LINEAR_RANGE[1]
    q_t, d_t, q_v, d_v = packed_inputs(T, heads, dm, B, fmt, "linear")
    assert torch.equal(q_v, K.linear_inputs()[0]) and torch.equal(d_v, K.linear_inputs()[1])        # fp16-exact in both formats
    rc, base = launch_attention(entry, q_t, d_t, B, T, heads, dm, gpu_device)
    assert rc == 0
    got = values_of(entry, base, B * T)
    ref = reference(T, heads, dm, B, fmt, "linear")
    if entry == "f16":
        check_f16(got, ref, B, T, heads, dm, "linear")
    else:
        check_split(entry, got, ref, heads * dm, "linear")
    for shift in (-K.LINEAR_SHIFT, K.LINEAR_SHIFT):
        f = 2.0 ** shift
        ds_t, ds_v = pack(d_v * f, fmt)
        assert torch.equal(ds_v, d_v * f)
        rc, out = launch_attention(entry, q_t, ds_t, B, T, heads, dm, gpu_device)
        assert rc == 0
        values_of(entry, out, B * T)
        assert torch.equal(out[..., :B * T, :].double(), base[..., :B * T, :].double() * f), f"dctx * 2^{shift}"


@pytest.mark.parametrize("entry", K.ENTRIES)
def test_attention_bwd_peaked_softmax(gpu_device, entry):
    """Every row of P has one entry above 0.999 and scores that span more than 40 (asserted from the reference): without the
    subtraction of the row maximum, in either pass, exp overflows or the small probabilities vanish.  Same bars."""
    T, heads, dm, B = K.PEAKED_SHAPE
    fmt = "f16" if entry == "f16" else "split"
    q_t, d_t, _, _ = packed_inputs(T, heads, dm, B, fmt, "peaked")
    ref = reference(T, heads, dm, B, fmt, "peaked")
    s = ref["q"] @ ref["k"].transpose(-1, -2) / dm ** 0.5
    assert ref["P"].max(-1).values.min().item() > 0.999 and (s.max(-1).values - s.min(-1).values).min().item() > 40
    rc, out = launch_attention(entry, q_t, d_t, B, T, heads, dm, gpu_device)
    assert rc == 0
    got = values_of(entry, out, B * T)
    if entry == "f16":
        check_f16(got, ref, B, T, heads, dm, "peaked")
    else:
        check_split(entry, got, ref, heads * dm, "peaked")


# =========================================================================================================== LayerNorm
def ln_operands(M, C, x_fmt, dy_fmt, dact_fmt, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, dy, z, add = r(M, C) * 1.5 + 0.3, r(M, C) * 2.0, r(M, C) * 1.5, r(M, C)
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, r(C) * 0.1
    return {"x": pack(x, x_fmt), "dy": pack(dy, dy_fmt), "z": pack(z, dact_fmt) if dact_fmt else None, "add": pack(add, "f32"),
            "gamma": pack(gamma, "f32"), "beta": pack(beta, "f32")}


def launch_layernorm(dev, half, ops, M, C, gelu, use_add, out, remap=(0, 0), out_rows=None, beta=True, lo_override=None):
    """One launch of advh_layernorm_bwd (``half`` = "f16") or advh_layernorm_bwd_split ("split").  Returns (rc, out_f, out_h) on the
    CPU, NaN-prefilled with GUARD rows behind ``out_rows``; out_h is fp16 [rows, C] or split planes [2, rows, C]."""
    _lib.init()
    lib = _lib.lib()
    rows = (M if out_rows is None else out_rows) + GUARD
    keep = {n: (None if v is None else v[0].to(dev)) for n, v in ops.items()}
    ptr = lambda t: None if t is None else t.data_ptr()
    lo = lambda t: t.stride(0) if t is not None and t.dim() == 3 else 0
    out_f = torch.full((rows, C), float("nan"), device=dev) if "f" in out else None
    out_h = None
    if "h" in out:
        out_h = torch.full(((2, rows, C) if half == "split" else (rows, C)), float("nan"), dtype=torch.float16, device=dev)
    x, dy, z = keep["x"], keep["dy"], keep["z"]
    x32, dy32 = int(x.dtype == torch.float32), int(dy.dtype == torch.float32)
    add = keep["add"] if use_add else None
    bt = keep["beta"] if beta else None
    if half == "split":
        los = dict(x=lo(x), dy=lo(dy), z=lo(z), out=lo(out_h))
        los.update(lo_override or {})
        rc = lib.advh_layernorm_bwd_split(ptr(x), x32, los["x"], ptr(dy), dy32, los["dy"], ptr(keep["gamma"]), ptr(bt), gelu, ptr(add),
                                          ptr(z), los["z"], ptr(out_f), ptr(out_h), los["out"], M, C, K.LN_EPS, remap[0], remap[1], stream())
    else:
        rc = lib.advh_layernorm_bwd(ptr(x), x32, ptr(dy), dy32, ptr(keep["gamma"]), ptr(bt), gelu, ptr(add), ptr(z), ptr(out_f), ptr(out_h),
                                    M, C, K.LN_EPS, remap[0], remap[1], stream())
    torch.cuda.synchronize()
    return rc, (None if out_f is None else out_f.cpu()), (None if out_h is None else out_h.cpu())


def ln_reference(ops, gelu, use_add):
    return BR.layernorm_bwd(ops["x"][1], ops["dy"][1], ops["gamma"][1], ops["beta"][1], K.LN_EPS, gelu,
                            None if ops["z"] is None else ops["z"][1], ops["add"][1] if use_add else None)


def check_ln_outputs(half, out_f, out_h, ref, what):
    """out_f: 2e-5 of max|ref|.  out_h next to out_f: the SAME values converted once -- plain fp16: out_f.half(); split planes:
    gemm.split_planes(out_f), the host restatement of device_math.h's conversion (tests/test_gpu_split.py holds the two
    together).  out_h alone: the bar of out_f plus the format's own rounding (2^-11 of the element, 2^-22 for a plane pair)."""
    top = ref.abs().max().item()
    if out_f is not None:
        err = (out_f.double() - ref).abs().max().item() / top
        print(f"layernorm bwd {what}: out_f rel err {err:.2e}")
        assert err <= TOL_LN
        if out_h is not None:
            want = G.split_planes(out_f) if half == "split" else out_f.half()
            assert torch.equal(out_h, want)
    else:
        got = (G.join_planes(out_h) if half == "split" else out_h).double()
        assert torch.isfinite(got).all()
        bound = TOL_LN * top + (2.0 ** -22 if half == "split" else 2.0 ** -11) * ref.abs() * (1 + 2.0 ** -6)
        ratio = ((got - ref).abs() / bound).max().item()
        print(f"layernorm bwd {what}: out_h alone, worst |err| / bound {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("case", K.LN_CASES, ids=K.ln_case_id)
def test_layernorm_bwd(gpu_device, case):
    """advh_layernorm_bwd / advh_layernorm_bwd_split against fp64 on the values the kernel read, for every instance
    <X32, DY32, MAXV>, across the MAXV boundaries and with partial last 64-lane rounds."""
    c = case
    M, C = c["M"], c["C"]
    ops = ln_operands(M, C, c["x"], c["dy"], c["dact"], seed=C + M)
    rc, out_f, out_h = launch_layernorm(gpu_device, c["half"], ops, M, C, c["gelu"], c["add"], c["out"])
    assert rc == 0
    for t in (out_f, out_h):
        if t is not None:
            assert untouched(t[..., M:, :]), "guard rows were written"
    cut = lambda t: None if t is None else t[..., :M, :]
    check_ln_outputs(c["half"], cut(out_f), cut(out_h), ln_reference(ops, c["gelu"], c["add"]), K.ln_instance_of(c["x"], c["dy"], C))


@pytest.mark.parametrize("case", K.LN_REMAP_CASES, ids=lambda c: "C{C}-B{B}-T{T}-P{P}-{half}".format(**c))
def test_layernorm_bwd_remap(gpu_device, case):
    """remap = (T, P), P > T (the feature encoder's per-clip padded layout): row b*T + t lands at b*P + t in out_f and out_h, the pad
    rows keep the prefill."""
    C, B, T, P, half = (case[n] for n in ("C", "B", "T", "P", "half"))
    M = B * T
    ops = ln_operands(M, C, half, half, half, seed=C + P)
    rc, out_f, out_h = launch_layernorm(gpu_device, half, ops, M, C, 1, True, "fh", remap=(T, P), out_rows=B * P)
    assert rc == 0
    real = torch.zeros(B * P + GUARD, dtype=torch.bool)
    for b in range(B):
        real[b * P:b * P + T] = True
    assert untouched(out_f[~real]) and untouched(out_h[..., ~real, :])
    check_ln_outputs(half, out_f[real], out_h[..., real, :], ln_reference(ops, 1, True), f"remap {T}->{P}")


def test_layernorm_bwd_offset_rows(gpu_device):
    """Rows mu + sigma * noise with |mu| / sigma = 64: a variance taken as E[x^2] - mean^2 in fp32 loses ~64^2 eps of it.  The bar
    is 4x the error of a numpy fp32 TWO-pass restatement against fp64 on the same rows; a numpy fp32 ONE-pass restatement
    misses it (asserted here and in tests/test_backward_ops_ref_cpu.py), so the case separates the two."""
    x, dy, gamma = K.offset_rows()
    M, C = x.shape
    ref = BR.layernorm_bwd(x, dy, gamma, None, K.LN_EPS, 0)
    two = (K.ln_dx_np32(x, dy, gamma, K.LN_EPS, one_pass=False).double() - ref).abs().max().item()
    one = (K.ln_dx_np32(x, dy, gamma, K.LN_EPS, one_pass=True).double() - ref).abs().max().item()
    bar = 4.0 * two
    assert one > bar
    ops = {"x": pack(x.double(), "f32"), "dy": pack(dy.double(), "f32"), "z": None, "add": pack(torch.zeros(M, C), "f32"),
           "gamma": pack(gamma.double(), "f32"), "beta": pack(torch.zeros(C), "f32")}
    rc, out_f, _ = launch_layernorm(gpu_device, "f16", ops, M, C, 0, False, "f")
    assert rc == 0
    err = (out_f[:M].double() - ref).abs().max().item()
    print(f"layernorm bwd offset rows: |err| {err:.3e}, bar {bar:.3e} (fp32 two-pass {two:.3e}, one-pass {one:.3e}), max|ref| {ref.abs().max().item():.3e}")
    assert err <= bar


def test_layernorm_bwd_arguments(gpu_device):
    """What the two entries refuse, and that a refused call leaves both outputs alone."""
    M = 5

    def call(C, half="f16", out="fh", **kw):
        ops = ln_operands(M, C, half, half, half, seed=C)
        rc, out_f, out_h = launch_layernorm(gpu_device, half, ops, M, C, 1, True, out, **kw)
        assert (out_f is None or untouched(out_f)) and (out_h is None or untouched(out_h))
        return rc

    assert call(6) == EINVAL                                     # C % 4
    assert call(6, "split") == EINVAL
    assert call(32, remap=(5, 3), out_rows=M) == EINVAL          # remap_P < remap_T
    assert call(32, out="") == EINVAL                            # neither out_f nor out_h
    assert call(32, beta=False) == EINVAL                        # gelu_fwd without beta
    for name in ("x", "dy", "z", "out"):
        assert call(32, "split", lo_override={name: 0}) == EINVAL          # a missing plane distance
        assert call(32, "split", lo_override={name: (M + GUARD) * 32 + 2}) == EINVAL      # not a multiple of 4
    assert call(2052) == EUNSUPPORTED                            # more than 8 rounds of 64 lanes x 4 channels
    assert call(2052, "split") == EUNSUPPORTED
