"""The waveform front end (csrc/frontend.hip: clip normaliser, GroupNorm statistics from the 10 x 10 Gram matrix, conv0) and
its backward (csrc/frontend_bwd.hip: GroupNorm-over-time backward from per-tile partials, the stride-5 overlap gather, the
normaliser's Jacobian) against the fp64 restatement of tests/embedder_ops_ref.py, called directly through the C ABI.

The clips of one batch are the edges real data brings: Gaussian, three quarters zero-padded, amplitude 1e4 and 1e-6, a DC
offset of 4 std (|mean| / std <= 5 keeps the fp32 rounding of the stored mean at 5 * 2^-24 of xhat), digital silence (forward
only: the reference's own gradient is NaN at sigma = 0).  ``wave`` is a view of a wider buffer at storage offset 1 with an odd
row stride (= 1 mod 4), so the rows start at every 4-byte phase of a 16-byte line.

Stated bounds, per clip b (amplitudes differ by 1e10) and never above the whole tensor's:
  split output       |out - ref| <= min(5e-6 max|ref|, 5e-6 max|ref[b]| + 2^-25)         (2^-25: the format's absolute floor)
  fp16 output        |out - ref| <= 2^-11 |ref| + 2^-25 + 5e-6 max|ref[b]|               elementwise
  stats, norm, mr    5e-6, in the units in which they act (see ``check_saved``)
  backward dz0, dx   max(5e-6 max|ref[b]|, 4 x the error of fp32 torch autograd through the same stage, measured in the test)
                     (+ the fp16 rounding for an fp16 dz0); the kernels reduce in another order than torch
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import embedder_ops_ref as R
from addvisor_hip import _lib, gemm as G
from oracle import signal_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_KERNEL = 5e-6
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


def n_in_of(L, rel):
    return {"<": max(1, L * 3 // 4), "=": L, ">": L + 37}[rel]


@functools.lru_cache(maxsize=None)
def clips(n, normalize, silence):
    g = torch.Generator().manual_seed(n)
    unit = torch.randn(n, generator=g)
    padded = torch.randn(n, generator=g)
    padded[max(1, n // 4):] = 0.0
    big = unit * (1e4 if normalize else 30.0)          # without the normaliser 1e4 would leave the fp16 / split range behind conv0
    dc = torch.randn(n, generator=g) * 0.5 + 2.0
    rows = [unit, padded, big, unit * 1e-6, dc] + ([torch.zeros(n)] if silence else [])
    return torch.stack(rows)


def strided(wave, dev):
    """The clips as a view of a wider device buffer: storage offset 1, row stride odd and = 1 mod 4, garbage in the gaps."""
    B, n = wave.shape
    W = n + 1
    while W % 4 != 1:
        W += 1
    buf = torch.full((B * W + 1,), 1e3, device=dev)
    view = buf[1:].view(B, W)[:, :n]
    view.copy_(wave)
    assert view.stride(0) % 2 == 1 and view.data_ptr() % 16 == 4
    return view


@functools.lru_cache(maxsize=None)
def weights(C0):
    g = torch.Generator().manual_seed(C0)
    return (torch.randn(C0, 10, generator=g) * 0.45, torch.rand(C0, generator=g) + 0.5, torch.randn(C0, generator=g) * 0.5,
            torch.randn(C0, generator=g) * 0.1)          # w0, gamma, beta, bias


@functools.lru_cache(maxsize=None)
def fwd_ref(C0, mode, has_bias, L, n_in, normalize):
    w0, gamma, beta, bias = weights(C0)
    return R.frontend(clips(n_in, normalize, True), L, w0, mode, bool(normalize), gamma, beta, bias if has_bias else None)


def run_forward(dev, split, wave, n_in, L, C0, mode, has_bias, normalize, P0):
    """-> (out planes or fp16 [.., B, P0, C0], stats [B, 2], norm [B, C0, 2], mr [B, C0, 2]) on the device."""
    lib = _lib.lib()
    w0, gamma, beta, bias = (t.to(dev) for t in weights(C0))
    B, T0 = wave.shape[0], (L - 10) // 5 + 1
    out = torch.full(((2,) if split else ()) + (B, P0, C0), SENTINEL, dtype=torch.float16, device=dev)
    stats = torch.full((B, 2), SENTINEL, device=dev)
    norm, mr = torch.full((B, C0, 2), SENTINEL, device=dev), torch.full((B, C0, 2), SENTINEL, device=dev)
    head = (wave.data_ptr(), wave.stride(0), n_in, B, L, w0.data_ptr(), bias.data_ptr() if has_bias else None, gamma.data_ptr(),
            beta.data_ptr(), mode, normalize, stats.data_ptr(), norm.data_ptr(), mr.data_ptr(), out.data_ptr())
    if split:
        rc = lib.advh_w2v2_frontend_split(*head, out.stride(0), T0, P0, C0, stream())
    else:
        rc = lib.advh_w2v2_frontend(*head, T0, P0, C0, stream())
    _lib.check(rc, f"frontend C0={C0} L={L} n_in={n_in} P0={P0} mode={mode} normalize={normalize}")
    return out, stats, norm, mr


def check_rows(got, ref, split):
    """Data rows [B, T0, C0] against the reference, per clip; returns the worst ratio to the bound."""
    worst = 0.0
    top = ref.abs().max()
    for b in range(ref.shape[0]):
        d = (got[b].double() - ref[b]).abs()
        mb = ref[b].abs().max()
        if split:
            bound = torch.minimum(TOL_KERNEL * top, TOL_KERNEL * mb + 2.0 ** -25)
            worst = max(worst, (d.max() / bound).item())
        else:
            worst = max(worst, (d / (2.0 ** -11 * ref[b].abs() + 2.0 ** -25 + TOL_KERNEL * mb)).max().item())
    return worst


def check_saved(stats, norm, mr, ref, C0, mode):
    """stats = (mean, rho): the mean's error acts on xhat as err * rho, rho's relatively.  mr = (mean_c, rstd_c): likewise on the
    normalised activation.  norm = (scale, shift) = (gamma rstd_c, beta - mean_c gamma rstd_c): 5e-6 of the clip's largest."""
    _, gamma, beta, _ = weights(C0)
    s, rs = stats.double().cpu(), ref["stats"]
    e = max(((s[:, 0] - rs[:, 0]).abs() * rs[:, 1]).max().item(), ((s[:, 1] - rs[:, 1]).abs() / rs[:, 1]).max().item())
    if mode == 0:
        m, rm = mr.double().cpu(), ref["mr"]
        unit = (rm[..., 0].abs() * rm[..., 1]).amax(1, keepdim=True).clamp_min(1.0)
        e = max(e, ((m[..., 0] - rm[..., 0]).abs() * rm[..., 1] / unit).max().item(), ((m[..., 1] - rm[..., 1]).abs() / rm[..., 1]).max().item())
        scale = gamma.double() * rm[..., 1]
        shift = beta.double() - rm[..., 0] * scale
        nn = norm.double().cpu()
        e = max(e, ((nn[..., 0] - scale).abs() / scale.abs().amax(1, keepdim=True)).max().item(),
                ((nn[..., 1] - shift).abs() / torch.maximum(shift.abs(), (rm[..., 0] * scale).abs()).amax(1, keepdim=True)).max().item())
    return e


FWD_L = [10, 325, 330, 16000]                                          # T0 = 1, 64, 65, 3199


def fwd_combos(L):
    """(P0 - T0, n_in relation, normalize): the whole product at the 64 / 65-frame sizes, every value at the others."""
    if L in (325, 330):
        return [(p, r, nz) for p in (1, 70) for r in "<=>" for nz in (0, 1)]
    return [(1, "=", 1), (70, "<", 1), (70, ">", 0), (1, "<", 0)] if L == 10 else [(1, "<", 1), (70, ">", 1), (1, "=", 0)]


@pytest.mark.parametrize("C0", [8, 32, 512])                            # 1, 4, 64 channel groups: 256, 64, 4 frame lanes
@pytest.mark.parametrize("mode,has_bias", [(0, False), (1, False), (1, True)])
@pytest.mark.parametrize("split", [False, True])
def test_frontend_forward(gpu_device, split, mode, has_bias, C0):
    _lib.init()
    worst = worst_saved = 0.0
    for L in FWD_L:
        T0 = (L - 10) // 5 + 1
        for extra, rel, normalize in fwd_combos(L):
            n_in, P0 = n_in_of(L, rel), T0 + extra
            ref = fwd_ref(C0, mode, has_bias, L, n_in, normalize)
            wave = strided(clips(n_in, normalize, True), gpu_device)
            out, stats, norm, mr = run_forward(gpu_device, split, wave, n_in, L, C0, mode, has_bias, normalize, P0)
            out = out.cpu()
            assert (out[..., T0:, :] == 0).all(), (L, P0, "filler rows")                     # every plane
            got = G.join_planes(out) if split else out.float()
            w = check_rows(got[:, :T0], ref["out"], split)
            s = check_saved(stats, norm, mr, ref, C0, mode)
            worst, worst_saved = max(worst, w), max(worst_saved, s)
            assert w <= 1.0, (L, n_in, P0, normalize, w)
            assert s <= TOL_KERNEL, (L, n_in, P0, normalize, s)
            if normalize:                                                                   # the normaliser removes the amplitude
                assert check_rows(got[2:3, :T0], ref["out"][0:1], split) <= 2.0
            silent = ref["out"][5]                                                          # digital silence: GELU(beta) / bias / 0
            _, _, beta, bias = weights(C0)
            expect = R.gelu(beta) if mode == 0 else (bias.double() if has_bias else torch.zeros(C0, dtype=torch.float64))
            assert torch.allclose(silent, expect.expand_as(silent), rtol=0, atol=1e-12)
    print(f"frontend forward {'split' if split else 'f16'} mode={mode} bias={has_bias} C0={C0}: worst ratio to the bound {worst:.3f}, "
          f"saved statistics {worst_saved:.2e}")
    note(f"frontend forward {'split' if split else 'f16'} ratio to bound", worst)
    note("frontend saved statistics", worst_saved)


# ------------------------------------------------------------------------------------------------------------- backward
BWD_COMBOS = [  # L, n_in relation, normalize, out_scale, P0 - T0
    (325, "=", 1, 1.0, 1), (330, "<", 1, 1.0 / 1024, 70), (330, ">", 0, 1.0, 1), (4103, ">", 1, 1.0 / 1024, 1),
    (4103, "<", 0, 1.0, 70), (16000, "<", 1, 1.0 / 1024, 1), (330, "=", 1, 1.0, 1),
]


@pytest.mark.parametrize("C0", [8, 32, 512])
@pytest.mark.parametrize("split", [False, True])
def test_frontend_backward(gpu_device, split, C0):
    """Forward, advh_w2v2_frontend_bwd_group[_split], then g = dz0 . w0 formed in fp64 from the kernel's own dz0 and
    advh_wave_bwd: dz0 against autograd of the fp64 forward, dx against autograd applied to that same dz0."""
    _lib.init()
    lib, dev = _lib.lib(), gpu_device
    w0, gamma, beta, _ = weights(C0)
    w0d, gd = w0.to(dev), gamma.to(dev)
    for L, rel, normalize, out_scale, extra in BWD_COMBOS:
        T0 = (L - 10) // 5 + 1
        n_in, P0 = n_in_of(L, rel), T0 + extra
        cl = clips(n_in, normalize, False)
        B = cl.shape[0]
        wave = strided(cl, dev)
        _, stats, norm, mr = run_forward(dev, split, wave, n_in, L, C0, 0, False, normalize, P0)
        gen = torch.Generator().manual_seed(L + C0)
        dy = torch.randn(B, P0, C0, generator=gen)
        dy[:, T0:] = 123.0                                                                   # finite garbage in the filler rows
        dyk = G.split_planes(dy) if split else dy.half()
        dy_seen = (G.join_planes(dyk) if split else dyk.float()).double()[:, :T0]
        dyd = dyk.to(dev)
        dz = torch.full_like(dyd, SENTINEL)
        ntile = (P0 + 63) // 64
        part, sums = torch.zeros(B, ntile, C0, 2, device=dev), torch.zeros(B, C0, 2, device=dev)
        head = (wave.data_ptr(), wave.stride(0), n_in, B, L, w0d.data_ptr(), gd.data_ptr(), stats.data_ptr(), norm.data_ptr(), mr.data_ptr())
        if split:
            rc = lib.advh_w2v2_frontend_bwd_group_split(*head, dyd.data_ptr(), dyd.stride(0), part.data_ptr(), sums.data_ptr(), dz.data_ptr(),
                                                        dz.stride(0), T0, P0, C0, stream())
        else:
            rc = lib.advh_w2v2_frontend_bwd_group(*head, dyd.data_ptr(), part.data_ptr(), sums.data_ptr(), dz.data_ptr(), T0, P0, C0, stream())
        _lib.check(rc, "frontend_bwd_group")
        dz = dz.cpu()
        assert (dz[..., T0:, :] == 0).all()
        dz_seen = (G.join_planes(dz) if split else dz.float()).double()                      # [B, P0, C0]
        # ---- stage 1: dz0 against fp64 autograd of GroupNorm-over-time + GELU, and the same stage in fp32 torch
        with torch.enable_grad():
            f = R.frontend(cl, L, w0, 0, bool(normalize), gamma, beta)
            z64 = f["z0"].detach().requires_grad_(True)
            o64, _, _ = R.frontend_tail(z64, 0, gamma, beta)
            ref_dz, = torch.autograd.grad(o64, z64, dy_seen)
            x32 = signal_ref.pad_or_crop(cl, L)
            x32 = signal_ref.zero_mean_unit_var_norm(x32) if normalize else x32
            z32 = F.conv1d(x32[:, None], w0[:, None], stride=5).detach().requires_grad_(True)
            o32 = F.gelu(F.group_norm(z32, C0, gamma, beta, eps=1e-5))
            dz32, = torch.autograd.grad(o32, z32, dy_seen.float().transpose(1, 2))
        dz32 = dz32.transpose(1, 2).double()
        for b in range(B):
            e32 = (dz32[b] - ref_dz[b]).abs().max().item()
            bound = max(TOL_KERNEL * ref_dz[b].abs().max().item(), 4 * e32)
            d = (dz_seen[b, :T0] - ref_dz[b]).abs()
            if not split:
                d = (d - (2.0 ** -11 * ref_dz[b].abs() + 2.0 ** -25)).clamp_min(0.0)         # the fp16 rounding of dz0
            ek = d.max().item()
            print(f"dz0 {'split' if split else 'f16'} C0={C0} L={L} n_in={n_in} nz={normalize} clip {b}: kernel {ek:.2e} fp32 {e32:.2e} "
                  f"max|ref| {ref_dz[b].abs().max().item():.2e}")
            note(f"frontend dz0 {'split' if split else 'f16'} rel", ek / ref_dz[b].abs().max().item())
            assert ek <= bound, ("dz0", L, n_in, normalize, b, ek, bound)
        # ---- stage 2: g = dz0 . w0 in fp64 from the kernel's own dz0, 16 columns in fp32 with garbage in 10..15
        g16 = torch.full((B, P0, 16), 55.0)
        g16[..., :10] = (dz_seen @ w0.double()).float()
        nt = (L + 2047) // 2048
        dxh, wpart = torch.zeros(B, L, device=dev), torch.zeros(B, nt, 2, device=dev)
        dx_stride = n_in + 5
        dx = torch.full((B, dx_stride), SENTINEL, device=dev)
        g16d = g16.to(dev)
        _lib.check(lib.advh_wave_bwd(g16d.data_ptr(), wave.data_ptr(), wave.stride(0), n_in, B, L, stats.data_ptr(), dxh.data_ptr(),
                                     wpart.data_ptr(), normalize, out_scale, dx.data_ptr(), dx_stride, T0, P0, stream()), "wave_bwd")
        dx = dx.cpu()
        assert (dx[:, n_in:] == SENTINEL).all()
        if n_in > L:
            assert (dx[:, L:n_in] == 0).all()
        gg = g16[:, :T0, :10]
        with torch.enable_grad():
            w64 = cl.double().requires_grad_(True)
            xh, _, _ = R.normalise(R.pad_or_crop(w64, L), bool(normalize))
            ref_dx, = torch.autograd.grad((xh.unfold(-1, 10, 5) * gg.double()).sum(), w64)
            w32 = cl.clone().requires_grad_(True)
            x32 = signal_ref.pad_or_crop(w32, L)
            x32 = signal_ref.zero_mean_unit_var_norm(x32) if normalize else x32
            dx32, = torch.autograd.grad((x32.unfold(-1, 10, 5) * gg).sum(), w32)
        ref_dx = ref_dx * out_scale
        dx32 = dx32.double() * out_scale
        for b in range(B):
            e32 = (dx32[b] - ref_dx[b]).abs().max().item()
            bound = max(TOL_KERNEL * ref_dx[b].abs().max().item(), 4 * e32)
            ek = (dx[b, :n_in].double() - ref_dx[b]).abs().max().item()
            print(f"dx  {'split' if split else 'f16'} C0={C0} L={L} n_in={n_in} nz={normalize} clip {b}: kernel {ek:.2e} fp32 {e32:.2e} "
                  f"max|ref| {ref_dx[b].abs().max().item():.2e}")
            note("frontend dx rel", ek / ref_dx[b].abs().max().item())
            assert ek <= bound, ("dx", L, n_in, normalize, b, ek, bound)
