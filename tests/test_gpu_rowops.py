"""The embedder's row kernels against fp64, called directly through the C ABI: LayerNorm (csrc/rowops.hip), time pool +
logistic regression, the positional-conv gathers, and the small backward / attribution kernels of csrc/backward.hip.
The references are tests/embedder_ops_ref.py, evaluated on the values the kernel read (``.float()`` of an fp16 tensor,
``join_planes`` of a split pair).

Stated bounds (no element is left out of any comparison):
  fp32 and split-format outputs    max|out - ref| <= 5e-6 * max|ref|                                  (TOL_KERNEL)
  fp16 outputs, elementwise        |out - ref| <= 2^-11 |ref| + 2^-25 + 5e-6 * max|ref|               (fp16 rounding on top)
  single fp32 operations           |out - expr| <= 2^-22 |expr| against the same expression in fp32 torch
  conversions                      fp16: exact;  split: |join - x| <= 2^-22 |x| + 2^-25              (csrc/device_math.h)
"""
import functools

import pytest
import torch

import embedder_ops_ref as R
from addvisor_hip import _lib, gemm as G

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_KERNEL = 5e-6
EINVAL, EUNSUPPORTED = -1, -4
SENTINEL = 777.0
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"worst {k}: {WORST[k]:.2e}")


def note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def err_f32(out, ref):
    """max|out - ref| / max|ref| (fp32 and split outputs; bound TOL_KERNEL)."""
    return ((out.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def err_f16(out, ref):
    """Worst ratio of |out - ref| to the fp16 bound 2^-11 |ref| + 2^-25 + 5e-6 max|ref| (must be <= 1)."""
    bound = 2.0 ** -11 * ref.abs() + 2.0 ** -25 + TOL_KERNEL * ref.abs().max()
    return ((out.double().cpu() - ref).abs() / bound).max().item()


# ------------------------------------------------------------------------------------------------------------ LayerNorm
LN_C = [4, 64, 252, 256, 260, 512, 516, 768, 1024, 1028, 1920, 2048]      # both sides of every MAXV class, ragged last vector
LN_M = [1, 3, 4, 5, 9]                                                    # a block handles four rows
LN_ROWS = 9
EPS = 1e-5


def _fmt(x, fmt):
    """fp32 values -> (the tensor the kernel is handed, the fp64 values it reads from it)."""
    if fmt == "f32":
        return x, x.double()
    if fmt == "f16":
        return x.half(), x.half().double()
    p = G.split_planes(x)
    return p, G.join_planes(p).double()


@functools.lru_cache(maxsize=None)
def ln_bank(C, fin, fadd):
    """Nine rows, kinds in turn: Gaussian | mean 100, std 0.01 | std 3e-3 | constant 1.0.  With an addend the kinds describe
    the SUM in + add.  The kernel forms that sum in fp32 (as the oracle's residual add does); on the mean-100 rows its rounding
    (2^-24 * 100 against a std of 0.01) would alone exceed the bound, so there the operands are multiples of 2^-17 (in ~ 60) and
    2^-16 / 2^-5 (add ~ 40) whose fp32 sum is exact -- checked below -- and the fp64 sum is the reference of both."""
    g = torch.Generator().manual_seed(1000 + C)
    x = torch.randn(LN_ROWS, C, generator=g)
    add = None if fadd is None else torch.randn(LN_ROWS, C, generator=g)
    for r in range(LN_ROWS):
        kind = r % 4
        if kind == 1:
            if fadd is None:
                x[r] = 100.0 + 0.01 * x[r]
            else:
                x[r] = torch.round((60.0 + 0.01 * x[r]) * 2.0 ** 17) * 2.0 ** -17
                add[r] = torch.round((40.0 + (0.02 if fadd == "f16" else 0.003) * add[r]) * 2.0 ** 16) * 2.0 ** -16
        elif kind == 2:
            x[r] *= 3e-3 if fadd is None else 2e-3
            if fadd is not None:
                add[r] *= 2e-3
        elif kind == 3:
            x[r] = 1.0 if fadd is None else 0.25
            if fadd is not None:
                add[r] = 0.75
    xt, xs = _fmt(x, fin)
    at, as_ = (None, None) if fadd is None else _fmt(add, fadd)
    if fadd is not None:
        tight = [r for r in range(LN_ROWS) if r % 4 == 1]
        assert torch.equal((xs[tight].float() + as_[tight].float()).double(), xs[tight] + as_[tight])
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    return xt, xs, at, as_, gamma, beta


@functools.lru_cache(maxsize=None)
def ln_ref(C, fin, fadd, gelu):
    _, xs, _, as_, gamma, beta = ln_bank(C, fin, fadd)
    return R.layernorm(xs, gamma, beta, EPS, add=as_, act=bool(gelu))


def ln_call(entry, fin, x, in_ld, add, add_ld, gamma, beta, out_f, out_h, out_ld, M, C, gelu, in_lo=0, add_lo=0, out_lo=0):
    lib = _lib.lib()
    f32 = int(fin == "f32")
    if entry == "plain":
        return lib.advh_layernorm(ptr(x), f32, in_ld, ptr(gamma), ptr(beta), ptr(out_f), ptr(out_h), out_ld, M, C, EPS, gelu, stream())
    if entry == "add":
        return lib.advh_layernorm_add(ptr(x), f32, in_ld, ptr(add), add_ld, ptr(gamma), ptr(beta), ptr(out_f), ptr(out_h), out_ld,
                                      M, C, EPS, gelu, stream())
    return lib.advh_layernorm_split(ptr(x), f32, in_ld, in_lo, ptr(add), add_ld, add_lo, ptr(gamma), ptr(beta), ptr(out_f),
                                    ptr(out_h), out_ld, out_lo, M, C, EPS, gelu, stream())


LN_CASES = [("plain", "f32", None), ("plain", "f16", None), ("add", "f32", None), ("add", "f32", "f16"), ("add", "f16", None),
            ("add", "f16", "f16"), ("split", "f32", None), ("split", "f32", "split"), ("split", "split", None),
            ("split", "split", "split")]


def lo_of(t, fmt):
    return t.stride(0) if fmt == "split" else 0


@pytest.mark.parametrize("outs", ["f", "h", "fh"])
@pytest.mark.parametrize("gelu", [0, 1])
@pytest.mark.parametrize("entry,fin,fadd", LN_CASES)
def test_layernorm(gpu_device, entry, fin, fadd, gelu, outs):
    """Every entry point x input format x addend x GELU x output set, at every C of LN_C and M of LN_M.  Rows behind the M-th
    keep their sentinel."""
    _lib.init()
    fout = "split" if entry == "split" else "f16"
    worst_f = worst_h = 0.0
    for C in LN_C:
        xt, _, at, _, gamma, beta = ln_bank(C, fin, fadd)
        ref_all = ln_ref(C, fin, fadd, gelu)
        xd, ad = xt.to(gpu_device), None if at is None else at.to(gpu_device)
        gd, bd = gamma.to(gpu_device), beta.to(gpu_device)
        for M in LN_M:
            out_f = torch.full((LN_ROWS, C), SENTINEL, device=gpu_device) if "f" in outs else None
            out_h = None
            if "h" in outs:
                out_h = torch.full(((2,) if fout == "split" else ()) + (LN_ROWS, C), SENTINEL, dtype=torch.float16, device=gpu_device)
            rc = ln_call(entry, fin, xd, C, ad, C, gd, bd, out_f, out_h, C, M, C, gelu, lo_of(xd, fin),
                         0 if ad is None else lo_of(ad, fadd), 0 if out_h is None else lo_of(out_h, fout))
            _lib.check(rc, f"layernorm {entry} C={C} M={M}")
            ref = ref_all[:M]
            if out_f is not None:
                o = out_f.cpu()
                assert (o[M:] == SENTINEL).all()
                e = err_f32(o[:M], ref)
                worst_f = max(worst_f, e)
                assert e <= TOL_KERNEL, (C, M, e)
            if out_h is not None:
                o = out_h.cpu()
                assert (o[..., M:, :] == SENTINEL).all()
                if fout == "split":
                    e = err_f32(G.join_planes(o)[:M], ref)
                    assert e <= TOL_KERNEL, (C, M, e)
                    worst_f = max(worst_f, e)
                else:
                    e = err_f16(o[:M], ref)
                    assert e <= 1.0, (C, M, e)
                    worst_h = max(worst_h, e)
    print(f"layernorm {entry} in={fin} add={fadd} gelu={gelu} outs={outs}: fp32/split rel {worst_f:.2e}, fp16 bound ratio {worst_h:.2f}")
    note("layernorm fp32/split rel", worst_f)
    note("layernorm fp16 bound ratio", worst_h)


@pytest.mark.parametrize("fin", ["f32", "f16", "split"])
def test_layernorm_leading_dimensions(gpu_device, fin):
    """in_ld, add_ld and out_ld larger than C: the gap columns keep their sentinel in every buffer."""
    _lib.init()
    C, M = 252, 5
    in_ld, add_ld, out_ld = 260, 264, 268
    entry, fadd = ("split", "split") if fin == "split" else ("add", "f16")
    xt, _, at, _, gamma, beta = ln_bank(C, fin, fadd)
    ref = ln_ref(C, fin, fadd, 1)[:M]

    def wide(t, ld):
        w = torch.full(tuple(t.shape[:-1]) + (ld,), SENTINEL, dtype=t.dtype)
        w[..., :C] = t
        return w.to(gpu_device)
    xd, ad = wide(xt, in_ld), wide(at, add_ld)
    x0, a0 = xd.clone(), ad.clone()
    out_f = torch.full((LN_ROWS, out_ld), SENTINEL, device=gpu_device)
    out_h = torch.full(((2,) if fin == "split" else ()) + (LN_ROWS, out_ld), SENTINEL, dtype=torch.float16, device=gpu_device)
    rc = ln_call(entry, fin, xd, in_ld, ad, add_ld, gamma.to(gpu_device), beta.to(gpu_device), out_f, out_h, out_ld, M, C, 1,
                 lo_of(xd, fin), lo_of(ad, fadd), lo_of(out_h, "split" if fin == "split" else "f16"))
    _lib.check(rc, "layernorm ld")
    assert torch.equal(xd, x0) and torch.equal(ad, a0)
    of, oh = out_f.cpu(), out_h.cpu()
    assert (of[:, C:] == SENTINEL).all() and (of[M:] == SENTINEL).all()
    assert (oh[..., C:] == SENTINEL).all() and (oh[..., M:, :] == SENTINEL).all()
    assert err_f32(of[:M, :C], ref) <= TOL_KERNEL
    if fin == "split":
        assert err_f32(G.join_planes(oh)[:M, :C], ref) <= TOL_KERNEL
    else:
        assert err_f16(oh[:M, :C], ref) <= 1.0


@pytest.mark.parametrize("fin", ["f16", "split"])
def test_layernorm_in_place(gpu_device, fin):
    """out_h aliasing the fp16 (split) input, with GELU: the layer-mode feature extractor's use (a row is read whole before it
    is written)."""
    _lib.init()
    for C in (512, 1028):
        xt, _, _, _, gamma, beta = ln_bank(C, fin, None)
        ref = ln_ref(C, fin, None, 1)
        buf = xt.to(gpu_device).clone()
        rc = ln_call("split" if fin == "split" else "plain", fin, buf, C, None, 0, gamma.to(gpu_device), beta.to(gpu_device), None,
                     buf, C, LN_ROWS, C, 1, lo_of(buf, fin), 0, lo_of(buf, fin))
        _lib.check(rc, "layernorm in place")
        if fin == "split":
            assert err_f32(G.join_planes(buf.cpu()), ref) <= TOL_KERNEL
        else:
            assert err_f16(buf.cpu(), ref) <= 1.0


# -------------------------------------------------------------------------------------------------------- pool + logreg
POOL_T = [1, 2, 4, 5, 8, 9, 12, 13, 199]            # the row kernels take frames t and t + 4 and step by 8


@pytest.mark.parametrize("H", [4, 768, 1024, 1028, 1920, 2048, 30, 2052])       # 30 / 2052: the any-H fallback
def test_pool_logreg(gpu_device, H):
    _lib.init()
    lib, B = _lib.lib(), 3
    g = torch.Generator().manual_seed(H)
    coef = (torch.randn(H, generator=g) / H ** 0.5)
    cd, icpt = coef.to(gpu_device), 0.5
    worst = 0.0
    for T in POOL_T:
        h = torch.randn(B, T, H, generator=g) + 0.3
        hd = h.to(gpu_device)
        ref_logit, ref_prob, ref_pooled = R.pool_logreg(h, coef, icpt)

        def run(hh, nb, want_pooled=True):
            logit = torch.full((nb,), SENTINEL, device=gpu_device)
            prob = torch.full((nb,), SENTINEL, device=gpu_device)
            pooled = torch.full((nb, H), SENTINEL, device=gpu_device) if want_pooled else None
            _lib.check(lib.advh_pool_logreg(hh.data_ptr(), cd.data_ptr(), icpt, logit.data_ptr(), prob.data_ptr(), ptr(pooled),
                                            nb, T, H, stream()), f"pool_logreg H={H} T={T}")
            return logit.cpu(), prob.cpu(), None if pooled is None else pooled.cpu()
        logit, prob, pooled = run(hd, B)
        e = max(err_f32(logit, ref_logit), err_f32(prob, ref_prob), err_f32(pooled, ref_pooled))
        worst = max(worst, e)
        assert e <= TOL_KERNEL, (T, e)
        l2, p2, pooled2 = run(hd, B)                                       # deterministic
        assert torch.equal(l2, logit) and torch.equal(p2, prob) and torch.equal(pooled2, pooled)
        l3, p3, _ = run(hd, B, want_pooled=False)                          # pooled is optional
        assert torch.equal(l3, logit) and torch.equal(p3, prob)
        l1, p1, pooled1 = run(hd[1:2].contiguous(), 1)                     # batch invariance, bit for bit
        assert torch.equal(l1[0], logit[1]) and torch.equal(p1[0], prob[1]) and torch.equal(pooled1[0], pooled[1])
    print(f"pool_logreg H={H}: worst rel over logit / prob / pooled {worst:.2e}")
    note("pool_logreg fp32 rel", worst)


# ------------------------------------------------------------------------------------------------------- posconv gather
GATHER = [(48, 16, 2, 199, 128), (8, 2, 3, 17, 4), (120, 2, 1, 40, 128)]       # (Cg, G, B, T, K)


def _gather_layout(h, G_, Cg, pad_left, P):
    """h [B, T, H] -> the expected [G, B, P, Cg] with data rows [pad_left, pad_left + T) and zeros elsewhere."""
    B, T, _ = h.shape
    exp = torch.zeros(G_, B, P, Cg, dtype=h.dtype)
    exp[:, :, pad_left:pad_left + T] = h.view(B, T, G_, Cg).permute(2, 0, 1, 3)
    return exp


@pytest.mark.parametrize("Cg,G_,B,T,K", GATHER)
def test_posconv_gather_forward(gpu_device, Cg, G_, B, T, K):
    _lib.init()
    lib, H, P = _lib.lib(), Cg * G_, T + K
    h = torch.randn(B, T, H, generator=torch.Generator().manual_seed(T)) * torch.logspace(-7, 2, H)[None, None, :]
    hd = h.to(gpu_device)
    inside = _gather_layout(torch.ones(B, T, H), G_, Cg, K // 2, P).bool()
    xg = torch.full((G_, B, P, Cg), SENTINEL, dtype=torch.float16, device=gpu_device)
    _lib.check(lib.advh_posconv_gather(hd.data_ptr(), xg.data_ptr(), B, T, H, G_, K, K // 2, None, stream()), "posconv_gather")
    assert torch.equal(xg.cpu(), _gather_layout(h.half(), G_, Cg, K // 2, P))                  # fp16 conversion: exact; zeros exact
    xs = torch.full((2, G_, B, P, Cg), SENTINEL, dtype=torch.float16, device=gpu_device)
    _lib.check(lib.advh_posconv_gather_split(hd.data_ptr(), xs.data_ptr(), xs.stride(0), B, T, H, G_, K, K // 2, stream()),
               "posconv_gather_split")
    xs = xs.cpu()
    assert (xs[:, ~inside] == 0).all()                                                         # every plane of every other row
    exp = _gather_layout(h, G_, Cg, K // 2, P).double()
    d = (G.join_planes(xs).double() - exp).abs()
    assert (d <= 2.0 ** -22 * exp.abs() + 2.0 ** -25).all()
    note("posconv gather split join rel", (d / exp.abs().clamp_min(1e-3)).max())


@pytest.mark.parametrize("Cg,G_,B,T,K", GATHER)
def test_posconv_gather_bwd_split(gpu_device, Cg, G_, B, T, K):
    """xg = dh * GELU'(z) at pad_left = K/2 - 1 against the fp64 derivative, z spread over [-6, 6]."""
    _lib.init()
    lib, H, P = _lib.lib(), Cg * G_, T + K
    g = torch.Generator().manual_seed(T + 1)
    dh = torch.randn(B, T, H, generator=g)
    z = G.split_planes((torch.rand(B, T, H, generator=g) * 12 - 6))
    zd, dd = z.to(gpu_device), dh.to(gpu_device)
    xs = torch.full((2, G_, B, P, Cg), SENTINEL, dtype=torch.float16, device=gpu_device)
    _lib.check(lib.advh_posconv_gather_bwd_split(dd.data_ptr(), xs.data_ptr(), xs.stride(0), B, T, H, G_, K, K // 2 - 1,
                                                 zd.data_ptr(), zd.stride(0), stream()), "posconv_gather_bwd_split")
    xs = xs.cpu()
    inside = _gather_layout(torch.ones(B, T, H), G_, Cg, K // 2 - 1, P).bool()
    assert (xs[:, ~inside] == 0).all()
    ref = _gather_layout(dh.double() * R.gelu_grad(G.join_planes(z)), G_, Cg, K // 2 - 1, P)
    e = err_f32(G.join_planes(xs), ref)
    print(f"posconv gather bwd {(Cg, G_, B, T, K)}: rel {e:.2e}")
    note("posconv gather bwd split rel", e)
    assert e <= TOL_KERNEL


# ----------------------------------------------------------------------------------------------- backward odds and ends
def close_f32(out, expr):
    """A single fp32 operation against the same expression in fp32 torch: 2^-22 relative, elementwise."""
    out, expr = out.double().cpu(), expr.double().cpu()
    return bool(((out - expr).abs() <= 2.0 ** -22 * expr.abs()).all())


@pytest.mark.parametrize("outs", ["f", "h", "fh"])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("T", [1, 199])
@pytest.mark.parametrize("H", [4, 768, 1920])
def test_pool_logreg_bwd(gpu_device, H, T, split, outs):
    """dh[b][t][:] = coef * (dlogit[b] / T) as fp32, as fp16 and as a split pair, each alone and together."""
    _lib.init()
    lib, B = _lib.lib(), 3
    g = torch.Generator().manual_seed(H + T)
    coef, dlogit = torch.randn(H, generator=g).to(gpu_device), (torch.randn(B, generator=g) * 1024).to(gpu_device)
    expr = (coef[None, None, :] * (dlogit / T)[:, None, None]).expand(B, T, H)
    dh = torch.full((B, T, H), SENTINEL, device=gpu_device) if "f" in outs else None
    dh16 = torch.full(((2,) if split else ()) + (B, T, H), SENTINEL, dtype=torch.float16, device=gpu_device) if "h" in outs else None
    if split:
        rc = lib.advh_pool_logreg_bwd_split(coef.data_ptr(), dlogit.data_ptr(), ptr(dh), ptr(dh16), 0 if dh16 is None else dh16.stride(0),
                                            B, T, H, stream())
    else:
        rc = lib.advh_pool_logreg_bwd(coef.data_ptr(), dlogit.data_ptr(), ptr(dh), ptr(dh16), B, T, H, stream())
    _lib.check(rc, "pool_logreg_bwd")
    if dh is not None:
        assert close_f32(dh, expr)
    if dh16 is not None:
        e = expr.double().cpu()
        if split:                                         # the operation's 2^-22 and the format's 2^-22 + 2^-25
            assert ((G.join_planes(dh16.cpu()).double() - e).abs() <= 2.0 ** -21 * e.abs() + 2.0 ** -25).all()
        else:                                             # fp16 rounding of a value within 2^-22 of expr
            assert ((dh16.cpu().double() - e).abs() <= (2.0 ** -11 + 2.0 ** -21) * e.abs() + 2.0 ** -25).all()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows,x_rows", [(5, 5), (5, 2), (7, 1)])
def test_scale_rows(gpu_device, rows, x_rows, accumulate):
    """y[r] = alpha[r] * x[r % x_rows] (+ y[r]); n is not a multiple of the 256-thread block."""
    _lib.init()
    n = 1000
    g = torch.Generator().manual_seed(rows + x_rows)
    x, alpha = torch.randn(x_rows, n, generator=g).to(gpu_device), torch.randn(rows, generator=g).to(gpu_device)
    y0 = torch.randn(rows + 1, n, generator=g).to(gpu_device)                  # one row behind: must stay
    y = y0.clone()
    _lib.check(_lib.lib().advh_scale_rows(x.data_ptr(), x_rows, alpha.data_ptr(), y.data_ptr(), rows, n, accumulate, stream()), "scale_rows")
    v = alpha[:, None] * x[torch.arange(rows) % x_rows]
    if accumulate:                                                             # y + v is one more fp32 rounding: of the sum
        s = (y0[:rows] + v).double()
        assert ((y[:rows].double() - s).abs() <= 2.0 ** -22 * (y0[:rows].abs() + v.abs()).double()).all()
    else:
        assert close_f32(y[:rows], v)
    assert torch.equal(y[rows], y0[rows])


def test_attr_finalize(gpu_device):
    _lib.init()
    total = 3 * 1000 + 7
    g = torch.Generator().manual_seed(8)
    grad, x = torch.randn(total, generator=g).to(gpu_device), torch.randn(total, generator=g).to(gpu_device)
    for mode, expr in ((0, grad.abs()), (1, x * grad)):
        out = torch.full((total + 1,), SENTINEL, device=gpu_device)
        _lib.check(_lib.lib().advh_attr_finalize(grad.data_ptr(), None if mode == 0 else x.data_ptr(), out.data_ptr(), mode, total, stream()),
                   "attr_finalize")
        assert close_f32(out[:total], expr) and out[total].item() == SENTINEL
        if mode == 0:
            assert torch.equal(out[:total], expr)


@pytest.mark.parametrize("with_wave", [False, True])
@pytest.mark.parametrize("n", [5, 1023, 1025, 16000])
def test_time_mask(gpu_device, n, with_wave):
    """mask = |attr| / (max|attr| + 1e-8) per clip: a clip of all zeros gives 0 (not NaN) next to normal ones; negative
    attributions; wave_in = wave * mask, wave_out = wave * (1 - mask) (from the kernel's own mask: each operation on its own)."""
    _lib.init()
    B = 3
    g = torch.Generator().manual_seed(n)
    attr = torch.randn(B, n, generator=g)
    attr[1] = 0.0
    attr[2] = -attr[2].abs() * 1e-3                                            # all negative, small
    attr, wave = attr.to(gpu_device), torch.randn(B, n, generator=g).to(gpu_device)
    mask = torch.full((B, n), SENTINEL, device=gpu_device)
    win = torch.full((B, n), SENTINEL, device=gpu_device) if with_wave else None
    wout = torch.full((B, n), SENTINEL, device=gpu_device) if with_wave else None
    _lib.check(_lib.lib().advh_time_mask(attr.data_ptr(), mask.data_ptr(), ptr(win), ptr(wout), wave.data_ptr() if with_wave else None,
                                         B, n, stream()), "time_mask")
    expr = attr.abs() / (attr.abs().amax(1, keepdim=True) + 1e-8)
    assert torch.isfinite(mask).all() and (mask[1] == 0).all()
    assert close_f32(mask, expr)
    assert mask.max().item() <= 1.0 and (mask[2] >= 0).all() and abs(mask[2].max().item() - 1.0) < 1e-4
    if with_wave:
        assert close_f32(win, wave * mask) and close_f32(wout, wave * (1.0 - mask))
        assert torch.equal(win[1], torch.zeros_like(win[1])) and torch.equal(wout[1], wave[1])


# ------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks(gpu_device):
    """Arguments the entry points reject before launching anything: the documented code, and the output keeps its sentinel.
    Every buffer is large enough for the call as stated."""
    _lib.init()
    lib, dev = _lib.lib(), gpu_device
    M, Cmax = 4, 2052
    x = torch.zeros(M, Cmax + 4, device=dev)
    x16 = torch.zeros(2, M, Cmax + 4, dtype=torch.float16, device=dev)
    gamma, beta = torch.ones(Cmax + 4, device=dev), torch.zeros(Cmax + 4, device=dev)
    out_f = torch.full((M, Cmax + 4), SENTINEL, device=dev)
    out_h = torch.full((2, M, Cmax + 4), SENTINEL, dtype=torch.float16, device=dev)
    ld = Cmax + 4

    def ln(C, in_ld=ld, out_ld=ld):
        return lib.advh_layernorm(x.data_ptr(), 1, in_ld, gamma.data_ptr(), beta.data_ptr(), out_f.data_ptr(), out_h.data_ptr(), out_ld,
                                  M, C, EPS, 0, stream())
    assert ln(6) == EINVAL                                                     # C % 4
    assert ln(8, in_ld=ld - 2) == EINVAL                                       # in_ld % 4
    assert ln(2052) == EUNSUPPORTED                                            # above the widest register class
    assert lib.advh_layernorm_split(x16.data_ptr(), 0, ld, x16.stride(0), None, 0, 0, gamma.data_ptr(), beta.data_ptr(), None,
                                    out_h.data_ptr(), ld, 0, M, 8, EPS, 0, stream()) == EINVAL      # out_h without out_lo
    # front end: C0 = 24 (3 channel groups do not divide the block), T0 inconsistent with L
    B, L, T0, C0 = 2, 330, 65, 32
    wave = torch.zeros(B, L, device=dev)
    w0 = torch.zeros(512 + 8, 10, device=dev)
    ws = torch.zeros(B * 2 * (512 + 8) * 2, device=dev)                        # stats / norm / mr / part / sums: each fits in here
    fe_out = torch.full((2, B, T0 + 1, 512 + 8), SENTINEL, dtype=torch.float16, device=dev)

    def fe(C0_, T0_):
        return lib.advh_w2v2_frontend(wave.data_ptr(), wave.stride(0), L, B, L, w0.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(), 0, 1,
                                      ws.data_ptr(), ws.data_ptr(), ws.data_ptr(), fe_out.data_ptr(), T0_, T0 + 1, C0_, stream())
    assert fe(24, T0) == EINVAL and fe(C0, T0 - 1) == EINVAL
    assert lib.advh_w2v2_frontend_split(wave.data_ptr(), wave.stride(0), L, B, L, w0.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(), 0, 1,
                                        ws.data_ptr(), ws.data_ptr(), ws.data_ptr(), fe_out.data_ptr(), fe_out.stride(0), T0 - 1, T0 + 1, C0,
                                        stream()) == EINVAL
    # front-end backward: C0 odd, C0 above 512
    dy = torch.zeros(2, B, T0 + 1, 512 + 8, dtype=torch.float16, device=dev)

    def fb(C0_):
        return lib.advh_w2v2_frontend_bwd_group(wave.data_ptr(), wave.stride(0), L, B, L, w0.data_ptr(), gamma.data_ptr(), ws.data_ptr(),
                                                ws.data_ptr(), ws.data_ptr(), dy.data_ptr(), ws.data_ptr(), ws.data_ptr(), fe_out.data_ptr(),
                                                T0, T0 + 1, C0_, stream())
    assert fb(7) == EINVAL and fb(520) == EINVAL
    torch.cuda.synchronize()
    assert (out_f == SENTINEL).all() and (out_h == SENTINEL).all() and (fe_out == SENTINEL).all()
