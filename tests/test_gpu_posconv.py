"""The positional convolution on each of its code paths, called as the model calls it, against tests/posconv_ref.py (fp64):
the line tile (csrc/posconv_tile.hip), the implicit-GEMM fallback in fp16 and split form (``embedder.plan_posconv``), the
gathers (csrc/rowops.hip) and the backward (gather with GELU', flipped-weight GEMM).

Two kinds of data.  Integer operands, where every product and partial sum is exact in fp32 and ``gelu_fast`` is exact from
|z| = 6 on: the output must equal the reference bit for bit there, which a dropped, doubled or misplaced product cannot
survive.  Random operands in the distribution of tests/test_gpu_gemm.py::test_posconv_line_tile, to the tolerance stated there.

Stated bounds (no element is left out of any comparison):
  integer data, |z| >= 6          out == h + max(z, 0) exactly; out_pre == z exactly; backward: out_f == out_h == ref exactly
  integer data, |z| < 6           |out - ref| <= 6 * GELU_TOL[True] + 2^-23 |ref|     (gelu_fast at an fp32 output, |z| < 6)
  random data, forward            |out - ref| <= 1e-4;  out_pre: the format's rounding on top (fp16 2^-11 |z|, pair 2^-22 |z| + 2^-25)
  random data, backward           |out_f - ref| <= DACT_TOL[split] * max|ref|;  out_h: the format's rounding on top
  gathers                         fp16 conversion exact; fp16 x GELU': err_f16 of tests/test_gpu_rowops.py; split: TOL_KERNEL
Every output buffer is a window inside a larger sentinel-filled buffer; nothing outside the window may change."""
import ctypes

import pytest
import torch

import posconv_ref as R
from gemm_desc_ref import DACT_TOL, GELU_TOL
from test_gpu_rowops import TOL_KERNEL, err_f16, err_f32
from addvisor_hip import _lib, embedder

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PAD = 64                                     # sentinel elements on both sides of every window (keeps 16-byte alignment)
SENT_H, SENT_F = 3.0, -7.0
TOL_RANDOM = 1e-4
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


def window(dev, shape, dtype, planes=False):
    """(whole buffer, the window as a tensor of ``shape``, or ``[2, *shape]`` plane pair with the planes' windows)."""
    n = 1
    for s in shape:
        n *= s
    lead = (2,) if planes else ()
    full = torch.full(lead + (n + 2 * PAD,), SENT_F if dtype == torch.float32 else SENT_H, dtype=dtype, device=dev)
    return full, full[..., PAD:PAD + n].view(lead + tuple(shape))


def untouched(full):
    s = SENT_F if full.dtype == torch.float32 else SENT_H
    return bool((full[..., :PAD] == s).all() and (full[..., full.shape[-1] - PAD:] == s).all())


def gather(dev, x, G_, K, pad_left, split, dact=None):
    """The model's gather launch for fp32 rows ``x [B, T, H]`` (a device tensor): (whole buffer, xg window)."""
    lib = _lib.lib()
    B, T, H = x.shape
    full, xg = window(dev, (G_, B, T + K, H // G_), torch.float16, planes=split)
    if split and dact is not None:
        rc = lib.advh_posconv_gather_bwd_split(x.data_ptr(), xg.data_ptr(), xg.stride(0), B, T, H, G_, K, pad_left,
                                               dact.data_ptr(), dact.stride(0), stream())
    elif split:
        rc = lib.advh_posconv_gather_split(x.data_ptr(), xg.data_ptr(), xg.stride(0), B, T, H, G_, K, pad_left, stream())
    else:
        rc = lib.advh_posconv_gather(x.data_ptr(), xg.data_ptr(), B, T, H, G_, K, pad_left, None if dact is None else dact.data_ptr(), stream())
    _lib.check(rc, "posconv gather")
    assert untouched(full)
    return full, xg


def run_tile(xg, wt, bias, resid, out, Cg, G_, B, T):
    d = embedder.PosconvDesc()
    d.xg, d.W, d.bias, d.resid, d.out = xg.data_ptr(), wt.data_ptr(), bias.data_ptr(), resid.data_ptr(), out.data_ptr()
    d.B, d.T, d.H, d.G, d.K = B, T, Cg * G_, G_, R.K_TILE
    _lib.check(_lib.lib().advh_posconv_tile_f16(ctypes.byref(d), stream()), "advh_posconv_tile_f16")


def check_exact(out, h, z, ref, what):
    """Integer data: bit for bit where |z| >= 6, the gelu_fast bound elsewhere."""
    out = out.double().cpu().view(ref.shape)
    big = z.abs() >= R.EXACT_Z
    want = R.exact_expected(h, z)
    bad = big & (out != want)
    assert not bad.any(), (what, int(bad.sum()), bad.nonzero()[:4].tolist(), out[bad][:4].tolist(), want[bad][:4].tolist())
    e = (out - ref).abs()
    assert (e <= 6 * GELU_TOL[True] + 2.0 ** -23 * ref.abs())[~big].all(), (what, e[~big].max().item())


def check_random(out, ref, what, key):
    e = (out.double().cpu().view(ref.shape) - ref).abs().max().item()
    note(key, e)
    assert e <= TOL_RANDOM, (what, e)


# -------------------------------------------------------------------------------------------------------- the line tile
def tile_case(dev, kind, Cg, G_, B, T, check):
    """Gather, then the tile into a buffer of its own and in place (``out == resid == h``, the embedder's call)."""
    _lib.init()
    h, w, bias, ref, z = R.forward_case(kind, False, Cg, G_, B, T)
    assert embedder.posconv_tile_selected(Cg, T, B, R.K_TILE, False)
    hd, bd = h.to(dev), bias.to(dev)
    _, xg = gather(dev, hd, G_, R.K_TILE, R.K_TILE // 2, False)
    assert torch.equal(xg.cpu(), R.gather_ref(h.half(), G_, R.K_TILE, R.K_TILE // 2))
    wt = embedder.pack_posconv_tile(w, G_).to(dev)
    full, out = window(dev, h.shape, torch.float32)
    run_tile(xg, wt, bd, hd, out, Cg, G_, B, T)
    check(out, "out != resid")
    assert untouched(full) and torch.equal(hd.cpu(), h)
    full, io = window(dev, h.shape, torch.float32)
    io.copy_(hd)
    run_tile(xg, wt, bd, io, io, Cg, G_, B, T)
    check(io, "in place")
    assert untouched(full)
    return h, z, ref


@pytest.mark.parametrize("Cg,G_,B,T", R.TILE_CASES, ids=lambda v: str(v))
def test_tile_exact(gpu_device, Cg, G_, B, T):
    h, _, _, ref, z = R.forward_case("int", False, Cg, G_, B, T)
    tile_case(gpu_device, "int", Cg, G_, B, T, lambda out, what: check_exact(out, h, z, ref, (what, Cg, G_, B, T)))


@pytest.mark.parametrize("Cg,G_,B,T", R.TILE_CASES, ids=lambda v: str(v))
def test_tile_random(gpu_device, Cg, G_, B, T):
    ref = R.forward_case("rand", False, Cg, G_, B, T)[3]
    tile_case(gpu_device, "rand", Cg, G_, B, T, lambda out, what: check_random(out, ref, (what, Cg, G_, B, T), f"tile Cg={Cg} random abs"))


# ---------------------------------------------------------------------------------------------------- the GEMM fallback
@pytest.mark.parametrize("kind", ["int", "rand"])
@pytest.mark.parametrize("split", [False, True], ids=["f16", "split"])
@pytest.mark.parametrize("Cg,G_,B,T,K", R.GEMM_CASES, ids=lambda v: str(v))
def test_gemm_forward(gpu_device, Cg, G_, B, T, K, split, kind):
    """``plan_posconv`` as ``HipEmbedder.forward`` runs it (``out_f == resid == h``) and as ``EmbedderGrad.forward`` does (a
    second fp32 buffer, ``out_pre`` = the pre-activation)."""
    _lib.init()
    dev, H = gpu_device, Cg * G_
    h, w, bias, ref, z = R.forward_case(kind, split, Cg, G_, B, T, K)
    mode = "split" if split else "f16"
    plan = embedder.plan_posconv(B, T, H, G_, K, w, bias, device=dev, split=split)
    hd = h.to(dev)
    _, xg = gather(dev, hd, G_, K, K // 2, split)

    def check(out, what):
        if kind == "int":
            check_exact(out, h, z, ref, (what, mode, Cg, T))
        else:
            check_random(out, ref, (what, mode, Cg, T), f"gemm {mode} random abs")
    full, io = window(dev, (B * T, H), torch.float32)
    io.copy_(hd.view(B * T, H))
    plan.run(xg, out_f=io, resid=io)
    check(io, "in place")
    assert untouched(full)
    full, out = window(dev, (B * T, H), torch.float32)
    pfull, pre = window(dev, (B * T, H), torch.float16, planes=split)
    plan.run(xg, out_f=out, resid=hd.view(B * T, H), out_pre=pre)
    check(out, "with out_pre")
    assert untouched(full) and untouched(pfull) and torch.equal(hd.cpu(), h)
    pv = (R.planes_value(pre.cpu()) if split else pre.cpu().double()).view(z.shape)
    if kind == "int":
        assert torch.equal(pv, z)
    else:
        e = (pv - z).abs()
        fmt = 2.0 ** -22 * z.abs() + 2.0 ** -25 if split else 2.0 ** -11 * z.abs()
        note(f"gemm {mode} random out_pre abs", e.max())
        assert (e <= TOL_RANDOM + fmt).all(), (mode, Cg, T, e.max().item())


@pytest.mark.parametrize("Cg,G_,B,T", R.IDENTICAL_CASES, ids=lambda v: str(v))
def test_tile_and_gemm_bit_identical(gpu_device, Cg, G_, B, T):
    """One gathered buffer, integer data: the tile and the fp16 GEMM hold the same exact sums and run the same gelu_fast."""
    _lib.init()
    dev, K, H = gpu_device, R.K_TILE, Cg * G_
    h, w, bias, _, _ = R.forward_case("int", False, Cg, G_, B, T)
    hd, bd = h.to(dev), bias.to(dev)
    _, xg = gather(dev, hd, G_, K, K // 2, False)
    f1, a = window(dev, h.shape, torch.float32)
    run_tile(xg, embedder.pack_posconv_tile(w, G_).to(dev), bd, hd, a, Cg, G_, B, T)
    f2, b = window(dev, h.shape, torch.float32)
    embedder.plan_posconv(B, T, H, G_, K, w, bias, device=dev).run(xg, out_f=b.view(B * T, H), resid=hd.view(B * T, H))
    assert untouched(f1) and untouched(f2)
    assert torch.equal(a, b), int((a != b).sum())


# ----------------------------------------------------------------------------------------------------------- the gathers
@pytest.mark.parametrize("Cg,G_,B,T,K", [(48, 2, 2, 17, 128), (32, 2, 3, 5, 16), (120, 2, 1, 40, 128), R.SECOND_TRIP + (128,)],
                         ids=lambda v: str(v))
def test_gather_dact_f16(gpu_device, Cg, G_, B, T, K):
    """advh_posconv_gather with a ``dact_src``: xg = fp16(dh * GELU'(z)) at pad_left = K/2 - 1, z spread over [-6, 6]; the last
    case takes the grid-stride loop's second trip."""
    _lib.init()
    H = Cg * G_
    g = torch.Generator().manual_seed(T + Cg)
    dh = torch.randn(B, T, H, generator=g)
    z = (torch.rand(B, T, H, generator=g) * 12 - 6).half()
    _, xg = gather(gpu_device, dh.to(gpu_device), G_, K, K // 2 - 1, False, dact=z.to(gpu_device))
    xg = xg.cpu()
    inside = R.gather_ref(torch.ones(B, T, H), G_, K, K // 2 - 1).bool()
    assert (xg[~inside] == 0).all()
    ref = R.gather_ref(dh.double() * R.gelu_grad(z), G_, K, K // 2 - 1)
    e = err_f16(xg, ref)
    note("gather dact f16 bound ratio", e)
    assert e <= 1.0, e


def test_gathers_second_trip(gpu_device):
    """All three entry points where the grid-stride loop (4096 blocks of 256 items) takes a second trip."""
    _lib.init()
    Cg, G_, B, T = R.SECOND_TRIP
    K, H, dev = R.K_TILE, Cg * G_, gpu_device
    assert R.gather_items(Cg, G_, B, T, K) > R.GATHER_TRIP
    g = torch.Generator().manual_seed(1)
    h = torch.randn(B, T, H, generator=g)
    hd = h.to(dev)
    inside = R.gather_ref(torch.ones(B, T, H), G_, K, K // 2).bool()
    _, xg = gather(dev, hd, G_, K, K // 2, False)
    assert torch.equal(xg.cpu(), R.gather_ref(h.half(), G_, K, K // 2))
    _, xs = gather(dev, hd, G_, K, K // 2, True)
    xs = xs.cpu()
    assert (xs[:, ~inside] == 0).all()
    exp = R.gather_ref(h.double(), G_, K, K // 2)
    assert ((R.planes_value(xs) - exp).abs() <= 2.0 ** -22 * exp.abs() + 2.0 ** -25).all()
    zs, zv = R.operand(torch.rand(B, T, H, generator=g) * 12 - 6, True)
    _, xb = gather(dev, hd, G_, K, K // 2 - 1, True, dact=zs.to(dev))
    xb = xb.cpu()
    inside = R.gather_ref(torch.ones(B, T, H), G_, K, K // 2 - 1).bool()
    assert (xb[:, ~inside] == 0).all()
    e = err_f32(R.planes_value(xb), R.gather_ref(h.double() * R.gelu_grad(zv), G_, K, K // 2 - 1))
    note("gather bwd split second trip rel", e)
    assert e <= TOL_KERNEL, e


# ---------------------------------------------------------------------------------------------------------- the backward
@pytest.mark.parametrize("kind", ["int", "rand"])
@pytest.mark.parametrize("split", [False, True], ids=["f16", "split"])
@pytest.mark.parametrize("Cg,G_,B,T,K", R.GEMM_CASES, ids=lambda v: str(v))
def test_backward(gpu_device, Cg, G_, B, T, K, split, kind):
    """``EmbedderGrad.backward``'s two launches: the gather of ``dh * GELU'(pc)`` at pad_left = K/2 - 1, then the flipped plan
    with ``resid = dh``, ``out_f`` and ``out_h``."""
    _lib.init()
    dev, H = gpu_device, Cg * G_
    dh, pcs, w, ref = R.backward_case(kind, split, Cg, G_, B, T, K)
    mode = "split" if split else "f16"
    plan = embedder.plan_posconv(B, T, H, G_, K, w, flip=True, device=dev, split=split)
    dd = dh.to(dev)
    _, xg = gather(dev, dd, G_, K, K // 2 - 1, split, dact=pcs.to(dev))
    ffull, of = window(dev, (B * T, H), torch.float32)
    hfull, oh = window(dev, (B * T, H), torch.float16, planes=split)
    plan.run(xg, out_f=of, out_h=oh, resid=dd.view(B * T, H))
    assert untouched(ffull) and untouched(hfull) and torch.equal(dd.cpu(), dh)
    of = of.double().cpu().view(ref.shape)
    ohv = (R.planes_value(oh.cpu()) if split else oh.cpu().double()).view(ref.shape)
    if kind == "int":
        pcv = R.planes_value(pcs) if split else pcs.double()
        a = R.gather_ref(dh.double() * (pcv > 0), G_, K, K // 2 - 1)
        assert torch.equal(R.planes_value(xg.cpu()) if split else xg.cpu().double(), a)
        assert ref.abs().max().item() < 2048
        assert torch.equal(of, ref.float().double()), int((of != ref.float().double()).sum())
        assert torch.equal(ohv, ref.float().double()), int((ohv != ref.float().double()).sum())
        return
    mx = ref.abs().max().item()
    e = (of - ref).abs().max().item()
    note(f"backward {mode} random out_f / max|ref|", e / mx)
    assert e <= DACT_TOL[split] * mx, (mode, Cg, T, e, mx)
    eh = (ohv - ref).abs()
    fmt = 2.0 ** -22 * ref.abs() + 2.0 ** -25 if split else 2.0 ** -11 * ref.abs() + 2.0 ** -25
    note(f"backward {mode} random out_h / max|ref|", eh.max().item() / mx)
    assert (eh <= DACT_TOL[split] * mx + fmt).all(), (mode, Cg, T, eh.max().item(), mx)
