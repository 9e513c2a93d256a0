"""Kernel-level suite of the ragged row kernels: the waveform front end with per-clip lengths (csrc/frontend.hip), the
tail zeroing and the pool + logistic head over each clip's valid frames (csrc/rowops.hip), against the float64
``tests/embedder_ops_ref.py`` evaluated on each clip CROPPED to its length.  Samples / rows past a clip's length are NaN, so a
kernel that reads one for its value fails.  Bars: those of the sibling kernels' suites (tests/test_gpu_frontend.py check_rows and
check_saved's statistics terms, tests/test_gpu_rowops.py test_pool_logreg), 5e-6 of the clip's largest value for fp32 and
split outputs and the elementwise fp16 bound for fp16 ones.  With full lengths every kernel is bit-identical to its sibling."""
import pytest
import torch

import embedder_ops_ref as R
from addvisor_hip import _lib, gemm as G

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_KERNEL = 5e-6
SENTINEL = 777.0
NAN = float("nan")
L = 4000
LENS = (4000, 3999, 2500, 330, 325, 14, 10)          # T0 = 799, 798, 499, 65, 64 (the 64-frame tile of conv0), 1, 1


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def weights(C0):
    g = torch.Generator().manual_seed(C0)
    return (torch.randn(C0, 10, generator=g) * 0.45, torch.rand(C0, generator=g) + 0.5, torch.randn(C0, generator=g) * 0.5,
            torch.randn(C0, generator=g) * 0.1)          # w0, gamma, beta, bias


def clips():
    g = torch.Generator().manual_seed(L)
    w = torch.randn(len(LENS), L, generator=g)
    w[2] = w[2] * 0.5 + 2.0                               # a clip with a DC offset
    return w


def run_frontend(dev, split, wave, lens, C0, mode, has_bias, normalize, P0):
    """lens None: the sibling.  -> (out, stats, norm, mr) on the CPU."""
    lib = _lib.lib()
    w0, gamma, beta, bias = (t.to(dev) for t in weights(C0))
    B, T0 = wave.shape[0], (L - 10) // 5 + 1
    out = torch.full(((2,) if split else ()) + (B, P0, C0), SENTINEL, dtype=torch.float16, device=dev)
    stats = torch.full((B, 2), SENTINEL, device=dev)
    norm, mr = torch.full((B, C0, 2), SENTINEL, device=dev), torch.full((B, C0, 2), SENTINEL, device=dev)
    wd = wave.to(dev)
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    head = (wd.data_ptr(), wd.stride(0), L, B, L, w0.data_ptr(), bias.data_ptr() if has_bias else None, gamma.data_ptr(),
            beta.data_ptr(), mode, normalize, stats.data_ptr(), norm.data_ptr(), mr.data_ptr(), out.data_ptr())
    tail = (T0, P0, C0) + (() if lens is None else (ld.data_ptr(),)) + (stream(),)
    name = "advh_w2v2_frontend" + ("_split" if split else "") + ("" if lens is None else "_ragged")
    rc = getattr(lib, name)(*head, *((out.stride(0),) if split else ()), *tail)
    torch.cuda.synchronize()
    _lib.check(rc, name)
    return out.cpu(), stats.cpu(), norm.cpu(), mr.cpu()


@pytest.mark.parametrize("C0", [32, 512])
@pytest.mark.parametrize("mode,has_bias", [(0, False), (1, True)])
@pytest.mark.parametrize("split", [False, True])
def test_frontend_ragged(gpu_device, split, mode, has_bias, C0):
    _lib.init()
    w0, gamma, beta, bias = weights(C0)
    wave = clips()
    T0, P0 = (L - 10) // 5 + 1, (L - 10) // 5 + 1 + 3
    poisoned = wave.clone()
    for b, n in enumerate(LENS):
        poisoned[b, n:] = NAN
    for normalize in (1, 0):
        out, stats, norm, mr = run_frontend(gpu_device, split, poisoned, LENS, C0, mode, has_bias, normalize, P0)
        refs = [R.frontend(wave[b:b + 1, :n], n, w0, mode, bool(normalize), gamma, beta, bias if has_bias else None) for b, n in enumerate(LENS)]
        top = max(r["out"].abs().max() for r in refs)
        got = (G.join_planes(out) if split else out.float()).double()
        for b, n in enumerate(LENS):
            Tb = (n - 10) // 5 + 1
            assert (out[..., b, Tb:, :] == 0).all(), (b, "rows past the clip's frames are not zero")      # every plane
            ref = refs[b]["out"][0]
            assert ref.shape[0] == Tb
            d, mb = (got[b, :Tb] - ref).abs(), ref.abs().max()
            assert torch.isfinite(got[b, :Tb]).all(), (b, "a sample past the length was read")
            if split:
                assert d.max() <= torch.minimum(TOL_KERNEL * top, TOL_KERNEL * mb + 2.0 ** -25), (b, n, normalize, d.max().item())
            else:
                assert (d / (2.0 ** -11 * ref.abs() + 2.0 ** -25 + TOL_KERNEL * mb)).max() <= 1.0, (b, n, normalize)
            s, rs = stats[b].double(), refs[b]["stats"][0]
            assert (s[0] - rs[0]).abs() * rs[1] <= TOL_KERNEL and (s[1] - rs[1]).abs() / rs[1] <= TOL_KERNEL, (b, n, normalize)
            if mode == 0:
                m, rm = mr[b].double(), refs[b]["mr"][0]
                if Tb > 1:                                                                          # one frame: variance 0, rstd = 1 / sqrt(eps)
                    unit = (rm[:, 0].abs() * rm[:, 1]).max().clamp_min(1.0)
                    assert ((m[:, 0] - rm[:, 0]).abs() * rm[:, 1] / unit).max() <= TOL_KERNEL, (b, n)
                    assert ((m[:, 1] - rm[:, 1]).abs() / rm[:, 1]).max() <= TOL_KERNEL, (b, n)
        # garbage past the length changes nothing, bit for bit
        out2, stats2, norm2, mr2 = run_frontend(gpu_device, split, wave, LENS, C0, mode, has_bias, normalize, P0)
        assert torch.equal(out2.view(torch.int16), out.view(torch.int16)) and torch.equal(stats2, stats)
        if mode == 0:
            assert torch.equal(norm2, norm) and torch.equal(mr2, mr)
        # full lengths: the sibling, bit for bit
        full = run_frontend(gpu_device, split, wave, (L,) * len(LENS), C0, mode, has_bias, normalize, P0)
        sib = run_frontend(gpu_device, split, wave, None, C0, mode, has_bias, normalize, P0)
        assert torch.equal(full[0].view(torch.int16), sib[0].view(torch.int16)) and torch.equal(full[1], sib[1])
        if mode == 0:
            assert torch.equal(full[2], sib[2]) and torch.equal(full[3], sib[3])
    assert _lib.lib().advh_split_overflow(1) == 0


@pytest.mark.parametrize("H", [64, 1920, 30])                           # 30: H % 4 != 0, the scalar stores
@pytest.mark.parametrize("offset", [0, 1])                              # 1: a base that is not 16-byte aligned
def test_zero_tail_rows(gpu_device, H, offset):
    _lib.init()
    lib, B, T, GUARD = _lib.lib(), 4, 7, 2
    g = torch.Generator().manual_seed(H + offset)
    for frames in ((T, 1, 3, 0), (T, T, T, T)):
        src = torch.randn(offset + (B * T + GUARD) * H, generator=g)
        src[offset + 2 * T * H + 4 * H] = NAN                            # a NaN in a row that is cleared
        buf = src.to(gpu_device)
        x = buf[offset:]
        assert x.data_ptr() % 16 == (4 * offset) % 16
        fr = torch.tensor(frames, dtype=torch.int32, device=gpu_device)
        _lib.check(lib.advh_zero_tail_rows(x.data_ptr(), fr.data_ptr(), B, T, H, stream()), "advh_zero_tail_rows")
        torch.cuda.synchronize()
        expect = src.clone()
        body = expect[offset:offset + B * T * H].view(B, T, H)
        for b, f in enumerate(frames):
            body[b, f:] = 0.0
        got = buf.cpu()
        assert torch.equal(got.view(torch.int32), expect.view(torch.int32)), (H, offset, frames)       # exact, guard rows and the NaN-free rest included


POOL_T = [1, 2, 4, 5, 8, 9, 12, 13, 199]            # the row kernels take frames t and t + 4 and step by 8


@pytest.mark.parametrize("H", [4, 768, 1024, 1920, 2048, 30])           # 30: the any-H fallback
def test_pool_logreg_ragged(gpu_device, H):
    _lib.init()
    lib = _lib.lib()
    g = torch.Generator().manual_seed(H)
    coef = torch.randn(H, generator=g) / H ** 0.5
    cd, icpt = coef.to(gpu_device), 0.5
    T = 200
    frames = POOL_T + [T]
    B = len(frames)
    h = torch.randn(B, T, H, generator=g) + 0.3
    poisoned = h.clone()
    for b, f in enumerate(frames):
        poisoned[b, f:] = NAN

    def run(hh, fr):
        logit = torch.full((B,), SENTINEL, device=gpu_device)
        prob = torch.full((B,), SENTINEL, device=gpu_device)
        pooled = torch.full((B, H), SENTINEL, device=gpu_device)
        hd = hh.to(gpu_device)
        if fr is None:
            rc = lib.advh_pool_logreg(hd.data_ptr(), cd.data_ptr(), icpt, logit.data_ptr(), prob.data_ptr(), pooled.data_ptr(), B, T, H, stream())
        else:
            fd = torch.tensor(fr, dtype=torch.int32, device=gpu_device)
            rc = lib.advh_pool_logreg_ragged(hd.data_ptr(), cd.data_ptr(), icpt, logit.data_ptr(), prob.data_ptr(), pooled.data_ptr(),
                                             fd.data_ptr(), B, T, H, stream())
        torch.cuda.synchronize()
        _lib.check(rc, "pool_logreg")
        return logit.cpu(), prob.cpu(), pooled.cpu()
    logit, prob, pooled = run(poisoned, frames)
    rel = lambda out, ref: ((out.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()
    for b, f in enumerate(frames):
        rl, rp, rpool = R.pool_logreg(h[b:b + 1, :f], coef, icpt)
        e = max(rel(logit[b:b + 1], rl), rel(prob[b:b + 1], rp), rel(pooled[b:b + 1], rpool))
        assert e <= TOL_KERNEL, (H, f, e)
    # a batch of clips with the same count is the sibling on the cropped rows, bit for bit (same order of addition) ...
    for f in (5, 13):
        a = run(h, [f] * B)
        hc = h[:, :f].contiguous()
        logit_c = torch.full((B,), SENTINEL, device=gpu_device)
        prob_c = torch.full((B,), SENTINEL, device=gpu_device)
        hd = hc.to(gpu_device)
        _lib.check(lib.advh_pool_logreg(hd.data_ptr(), cd.data_ptr(), icpt, logit_c.data_ptr(), prob_c.data_ptr(), None, B, f, H, stream()), "pool")
        assert torch.equal(a[0], logit_c.cpu()) and torch.equal(a[1], prob_c.cpu())
    # ... and full lengths are the sibling
    full, sib = run(h, [T] * B), run(h, None)
    assert all(torch.equal(x, y) for x, y in zip(full, sib))
