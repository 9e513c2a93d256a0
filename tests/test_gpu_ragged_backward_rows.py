"""Kernel-level suite of the row and waveform-end kernels of the ragged gradient chain (csrc/backward.hip, csrc/frontend_bwd.hip):
advh_pool_logreg_bwd_ragged / _split_ragged, advh_zero_tail_rows_h, advh_w2v2_frontend_bwd_group_ragged / _split_ragged and
advh_wave_bwd_ragged, each against a float64 restatement on every clip CROPPED to its length (autograd through
tests/embedder_ops_ref.py for the two front-end kernels), bit-identical to its sibling at full lengths, and with NaN in every
sample / row past a length, so that a kernel that reads one for its value fails.

Bars.  The pool backward is one division and one product in fp32: 2^-22 of the value (fp32 output), plus the output format's
rounding (2^-11 fp16, 2^-21 split).  The GroupNorm and waveform backward are normalisation backwards in fp32 with the chain's
erf approximation, the class of the LayerNorm backward: its bar, 2e-5 of the clip's max|ref| (tests/test_gpu_backward_kernels.py
TOL_LN), plus the elementwise rounding of an fp16 output."""
import pytest
import torch

import embedder_ops_ref as R
import ragged_ref as RR
from addvisor_hip import _lib, gemm as G
from test_gpu_ragged_rows import L, LENS, clips, run_frontend, weights

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_NORM = 2e-5
NAN = float("nan")
SENTINEL = 777.0
GUARD = 3
FRAMES = tuple(T for _, T, _ in RR.TABLE)            # 12, 12, 7, 3, 2, 1, 1 of T = 12


def stream():
    return torch.cuda.current_stream().cuda_stream


def i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------------------------ pool + logreg backward
@pytest.mark.parametrize("H", [32, 36, 768])
@pytest.mark.parametrize("split", [False, True])
def test_pool_logreg_bwd_ragged(gpu_device, split, H):
    _lib.init()
    lib, dev = _lib.lib(), gpu_device
    B, T = len(FRAMES), 12
    g = torch.Generator().manual_seed(H)
    coef, dlogit = torch.randn(H, generator=g), torch.randn(B, generator=g) * 64.0
    cd, dd = coef.to(dev), dlogit.to(dev)

    def launch(frames):
        dh = torch.full((B * T + GUARD, H), NAN, device=dev)
        d16 = torch.full(((2,) if split else ()) + (B * T + GUARD, H), NAN, dtype=torch.float16, device=dev)
        if frames is None:
            rc = (lib.advh_pool_logreg_bwd_split(cd.data_ptr(), dd.data_ptr(), dh.data_ptr(), d16.data_ptr(), d16.stride(0), B, T, H, stream())
                  if split else lib.advh_pool_logreg_bwd(cd.data_ptr(), dd.data_ptr(), dh.data_ptr(), d16.data_ptr(), B, T, H, stream()))
        else:
            fr = i32(frames, dev)
            rc = (lib.advh_pool_logreg_bwd_split_ragged(cd.data_ptr(), dd.data_ptr(), dh.data_ptr(), d16.data_ptr(), d16.stride(0),
                                                        fr.data_ptr(), B, T, H, stream())
                  if split else lib.advh_pool_logreg_bwd_ragged(cd.data_ptr(), dd.data_ptr(), dh.data_ptr(), d16.data_ptr(), fr.data_ptr(),
                                                                B, T, H, stream()))
        torch.cuda.synchronize()
        assert rc == 0
        return dh.cpu(), d16.cpu()
    dh, d16 = launch(FRAMES)
    assert torch.isnan(dh[B * T:]).all() and torch.isnan(d16[..., B * T:, :].float()).all()          # guards
    h16 = (G.join_planes(d16[:, :B * T]) if split else d16[:B * T].float()).double().view(B, T, H)
    dh = dh[:B * T].double().view(B, T, H)
    for b, f in enumerate(FRAMES):
        ref = coef.double() * (dlogit[b].double() / f)
        assert bool((dh[b, f:] == 0).all()) and bool((d16[..., b * T + f:(b + 1) * T, :].view(torch.int16) == 0).all())
        assert ((dh[b, :f] - ref).abs() <= 2.0 ** -22 * ref.abs()).all()
        assert ((h16[b, :f] - ref).abs() <= (2.0 ** -21 if split else 2.0 ** -11) * ref.abs() + 2.0 ** -22 * ref.abs() + 2.0 ** -25).all()
    full, sib = launch((T,) * B), launch(None)
    assert all(torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                           b.view(torch.int32 if b.dtype == torch.float32 else torch.int16)) for a, b in zip(full, sib))
    clamped = launch((T + 5,) * 3 + (0, -3, 1, 1))
    assert torch.equal(clamped[0][:3 * T], sib[0][:3 * T]) and torch.equal(clamped[0][3 * T:5 * T], launch((T, T, T, 1, 1, 1, 1))[0][3 * T:5 * T])


# ------------------------------------------------------------------------------------------------ zeroing fp16 / plane-pair rows
@pytest.mark.parametrize("H,offset", [(32, 0), (32, 3), (6, 0), (36, 0), (40, 8)])
@pytest.mark.parametrize("split", [False, True])
def test_zero_tail_rows_h(gpu_device, split, H, offset):
    """fp16 rows (lo = 0) and a plane pair, 16-byte aligned and not (``offset`` halfs into the allocation), H % 8 and H % 4 != 0."""
    _lib.init()
    dev = gpu_device
    B, T = len(FRAMES), 12
    frames = (12, 0, 7, 3, 2, 1, 20)                  # 0: the whole clip; 20: clamped to T, nothing zeroed
    n = B * T * H
    plane = -(-(offset + n + GUARD * H) // 8) * 8       # the lo plane starts 16-byte aligned relative to the hi plane
    buf = torch.full((2 if split else 1, plane), SENTINEL, dtype=torch.float16, device=dev)
    fr = i32(frames, dev)
    rc = _lib.lib().advh_zero_tail_rows_h(buf[0, offset:].data_ptr(), plane if split else 0, fr.data_ptr(), B, T, H, stream())
    torch.cuda.synchronize()
    assert rc == 0
    out = buf.cpu()
    assert bool((out[:, :offset] == SENTINEL).all()) and bool((out[:, offset + n:] == SENTINEL).all())      # in front and behind, every plane
    rows = out[:, offset:offset + n].reshape(-1, B, T, H)
    for b, f in enumerate(frames):
        f = min(max(f, 0), T)
        assert bool((rows[:, b, :f] == SENTINEL).all()), (b, "a valid row was written")
        assert bool((rows[:, b, f:].view(torch.int16) == 0).all()), (b, "a padded row is not zero in every plane")


# ------------------------------------------------------------------------------------------------ GroupNorm backward of layer 0
def saved(dev, split, wave, lens, C0, P0):
    """The per-clip statistics the ragged front end saves (mode 0), back on the device."""
    out, stats, norm, mr = run_frontend(dev, split, wave, lens, C0, 0, False, 1, P0)
    return stats.to(dev), norm.to(dev), mr.to(dev)


def gn0_launch(dev, split, wave, lens, C0, P0, dy, st):
    """lens None: the sibling.  dy: fp16 [B, P0, C0] or planes [2, B, P0, C0].  -> dz0 on the CPU (NaN prefill)."""
    lib = _lib.lib()
    w0, gamma, _, _ = (t.to(dev) for t in weights(C0))
    B, T0 = wave.shape[0], (L - 10) // 5 + 1
    wd, dyd = wave.to(dev), dy.to(dev)
    ntile = -(-P0 // 64)
    part, sums = torch.full((B, ntile, C0, 2), NAN, device=dev), torch.full((B, C0, 2), NAN, device=dev)
    dz = torch.full(dy.shape, NAN, dtype=torch.float16, device=dev)
    ld = None if lens is None else i32(lens, dev)
    head = (wd.data_ptr(), wd.stride(0), L, B, L, w0.data_ptr(), gamma.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
            dyd.data_ptr()) + ((dyd.stride(0),) if split else ()) + (part.data_ptr(), sums.data_ptr(), dz.data_ptr())
    tail = ((dz.stride(0),) if split else ()) + (T0, P0, C0) + (() if lens is None else (ld.data_ptr(),)) + (stream(),)
    name = "advh_w2v2_frontend_bwd_group" + ("_split" if split else "") + ("" if lens is None else "_ragged")
    rc = getattr(lib, name)(*head, *tail)
    torch.cuda.synchronize()
    _lib.check(rc, name)
    return dz.cpu()


@pytest.mark.parametrize("C0", [32, 512])
@pytest.mark.parametrize("split", [False, True])
def test_frontend_bwd_group_ragged(gpu_device, split, C0):
    _lib.init()
    dev = gpu_device
    w0, gamma, beta, _ = weights(C0)
    wave = clips()
    B, T0, P0 = len(LENS), (L - 10) // 5 + 1, (L - 10) // 5 + 1 + 3
    poisoned = wave.clone()
    g = torch.Generator().manual_seed(C0 + 1)
    dyv = torch.randn(B, P0, C0, generator=g) * 8.0
    dy = G.split_planes(dyv) if split else dyv.half()
    dy_val = (G.join_planes(dy) if split else dy.float()).double()
    dy_p = dy.clone()
    for b, n in enumerate(LENS):
        poisoned[b, n:] = NAN
        dy_p[..., b, (n - 10) // 5 + 1:, :] = NAN
    st = saved(dev, split, poisoned, LENS, C0, P0)
    dz = gn0_launch(dev, split, poisoned, LENS, C0, P0, dy_p, st)
    got = (G.join_planes(dz) if split else dz.float()).double()
    for b, n in enumerate(LENS):
        Tb = (n - 10) // 5 + 1
        assert bool((dz[..., b, Tb:, :].view(torch.int16) == 0).all()), (b, "rows past the clip's frames are not zero in every plane")
        with torch.enable_grad():
            fr = R.frontend(wave[b:b + 1, :n].double(), n, w0, 0, True, gamma, beta, None)
            z0 = fr["z0"].detach().requires_grad_(True)
            out = R.frontend_tail(z0, 0, gamma, beta, None)[0]
            (ref,) = torch.autograd.grad(out, z0, dy_val[b:b + 1, :Tb])
        ref = ref[0]
        assert torch.isfinite(got[b, :Tb]).all(), (b, "a sample or row past the length was read")
        # the scale of the error is the terms of dn - mean(dn) - nhat mean(dn nhat), not their difference: a one-frame clip has
        # dz0 = 0 exactly in the reference and fp32 leftovers of the cancellation in the kernel
        d, mb = (got[b, :Tb] - ref).abs(), torch.maximum(ref.abs().max(), dy_val[b, :Tb].abs().max())
        e = (d.max() / mb).item()
        print(f"gn0 bwd ragged [{'split' if split else 'f16'}] C0 {C0} clip {b} ({n} samples, {Tb} frames): max err {e:.3e} of max(|ref|, |dy|)")
        if split:
            assert d.max() <= TOL_NORM * mb, (b, n, e)
        else:
            assert (d / (2.0 ** -11 * ref.abs() + 2.0 ** -25 + TOL_NORM * mb)).max() <= 1.0, (b, n, e)
    full = (L,) * B
    st_sib = saved(dev, split, wave, None, C0, P0)
    st_full = saved(dev, split, wave, full, C0, P0)
    assert all(torch.equal(a, b) for a, b in zip(st_sib, st_full))
    a, b_ = gn0_launch(dev, split, wave, full, C0, P0, dy, st_full), gn0_launch(dev, split, wave, None, C0, P0, dy, st_sib)
    assert torch.equal(a.view(torch.int16), b_.view(torch.int16)), "full lengths are not the sibling bit for bit"


# ------------------------------------------------------------------------------------------------ the waveform end
def wave_bwd_launch(dev, wave, lens, gq, stats, P0, n_in, normalize=1):
    lib = _lib.lib()
    B, T0 = wave.shape[0], (L - 10) // 5 + 1
    wd, gd = wave.to(dev), gq.to(dev)
    dxh = torch.full((B, L), NAN, device=dev)
    part = torch.full((B, -(-L // 2048), 2), NAN, device=dev)
    dx = torch.full((B + 1, n_in), NAN, device=dev)
    ld = None if lens is None else i32(lens, dev)
    args = (gd.data_ptr(), wd.data_ptr(), wd.stride(0), n_in, B, L, stats.data_ptr(), dxh.data_ptr(), part.data_ptr(), normalize, 0.25,
            dx.data_ptr(), n_in, T0, P0)
    if lens is None:
        rc = lib.advh_wave_bwd(*args, stream())
    else:
        rc = lib.advh_wave_bwd_ragged(*args, ld.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == 0
    out = dx.cpu()
    assert torch.isnan(out[B]).all()                    # the guard row
    return out[:B]


def test_wave_bwd_ragged(gpu_device):
    _lib.init()
    dev = gpu_device
    wave = clips()
    B, T0, P0 = len(LENS), (L - 10) // 5 + 1, (L - 10) // 5 + 1 + 3
    g = torch.Generator().manual_seed(9)
    gq = torch.randn(B, P0, 16, generator=g) * 64.0
    gq[:, :, 10:] = 0.0                                  # the GEMM's padded columns
    gq[:, T0:] = 0.0                                     # rows [T0, P0) are zero in the chain
    poisoned, gq_p = wave.clone(), gq.clone()
    for b, n in enumerate(LENS):
        poisoned[b, n:] = NAN
        gq_p[b, (n - 10) // 5 + 1:] = NAN
    stats = saved(dev, False, poisoned, LENS, 32, P0)[0]
    dx = wave_bwd_launch(dev, poisoned, LENS, gq_p, stats, P0, L).double()
    for b, n in enumerate(LENS):
        Tb = (n - 10) // 5 + 1
        assert bool((dx[b, n:] == 0).all()), (b, "dx past the clip's length is not exactly zero")
        with torch.enable_grad():
            x = wave[b:b + 1, :n].double().requires_grad_(True)
            xhat = R.normalise(x)[0]
            win = xhat[0].unfold(0, 10, 5)               # [Tb, 10]: frame t reads samples 5 t .. 5 t + 9
            (ref,) = torch.autograd.grad((win * gq[b, :Tb, :10].double()).sum(), x)
        ref = ref[0] * 0.25
        assert torch.isfinite(dx[b, :n]).all(), (b, "a sample or row past the length was read")
        e = ((dx[b, :n] - ref).abs().max() / ref.abs().max()).item()
        print(f"wave bwd ragged clip {b} ({n} samples): max err {e:.3e} of max|ref|")
        assert e <= TOL_NORM, (b, n, e)
    full = (L,) * B
    st_sib = saved(dev, False, wave, None, 32, P0)[0]
    for n_in in (L, L + 100):                            # n_in > L: the sibling writes zeros behind L, so does the ragged form
        w = torch.cat([wave, torch.ones(B, n_in - L)], 1) if n_in > L else wave
        a = wave_bwd_launch(dev, w, full, gq, st_sib, P0, n_in)
        b_ = wave_bwd_launch(dev, w, None, gq, st_sib, P0, n_in)
        assert torch.equal(a, b_), "full lengths are not the sibling bit for bit"
