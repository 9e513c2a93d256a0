"""GPU: the tail kernels of csrc/unet_ragged.hip on sentinel-filled maps, and ``HipUNet.forward(widths=)`` on the shared length
table of tests/ragged_explain_ref.py: against ``unet_ref`` on each clip's own crop at the mask bars of tests/test_gpu_pipeline.py,
exact zeros past every clip's width, NaN past the width without effect, bit for bit against the engine on the cropped clip alone
in the fp32-class mode, and the order of ragged and padded calls on one engine without effect."""
import pytest
import torch

import ragged_explain_ref as E
from addvisor_hip import _lib
from addvisor_hip.unet import HipUNet

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

B, W = len(E.LENGTHS), 24
WIDTHS = [w for _, _, w, _ in E.TABLE]


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------- the tail kernels
@pytest.mark.parametrize("split", [False, True], ids=["f16", "split"])
@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("widths", [[24, 24, 24], [20, 20, 20], [4, 4, 4], [24, 20, 4], [8, 4, 16]], ids=str)
def test_fmap_clip_tail(gpu_device, split, shift, widths):
    _lib.init()
    nb, H, C, PH, PW, Wm = 3, 5, 16, 1, 2, W >> shift
    g = torch.Generator().manual_seed(5 + shift)
    shape = ((2,) if split else ()) + (nb, H + 2 * PH, Wm + 2 * PW, C)
    x0 = torch.randn(shape, generator=g).half().to(gpu_device)                   # the sentinel: every cell its own bits
    wd = torch.tensor(widths, dtype=torch.int32, device=gpu_device)
    lo = x0.stride(0) if split else 0
    for ind in (-1, 9):
        x = x0.clone()
        rc = _lib.lib().advh_fmap_clip_tail(x.data_ptr(), lo, wd.data_ptr(), shift, nb, H, Wm, C, PH, PW, ind, stream())
        _lib.check(rc, "advh_fmap_clip_tail")
        want = x0.clone()
        for plane, p in enumerate((want[0], want[1]) if split else (want,)):
            inner = p[:, PH:PH + H, PW:PW + Wm, :]
            for b, w in enumerate(widths):
                inner[b, :, w >> shift:, :] = 0
                if ind >= 0:
                    inner[b, :, :w >> shift, ind] = 1.0 if plane == 0 else 0.0
        assert torch.equal(bits(x), bits(want)), (split, shift, widths, ind)      # halo cells and kept columns: their own bits
        if ind >= 0:
            hi = (x[0] if split else x)[:, PH:PH + H, PW:PW + Wm, ind]
            for b, w in enumerate(widths):
                assert (hi[b, :, :w >> shift] == 1).all() and (hi[b, :, w >> shift:] == 0).all()
                if split:
                    assert (bits(x[1][b, PH:PH + H, PW:PW + Wm, ind]) == 0).all()


@pytest.mark.parametrize("widths", [[24, 24, 24], [20, 20, 20], [4, 4, 4], [24, 20, 4]], ids=str)
def test_zero_tail_cols_f32(gpu_device, widths):
    _lib.init()
    nb, H = 3, 19
    x0 = torch.randn(nb, H, W, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    x0[:, :, ::5] = float("nan")                                                 # stores, not products: NaN goes too
    x = x0.clone()
    wd = torch.tensor(widths, dtype=torch.int32, device=gpu_device)
    _lib.check(_lib.lib().advh_zero_tail_cols_f32(x.data_ptr(), wd.data_ptr(), nb, H, W, stream()), "advh_zero_tail_cols_f32")
    want = x0.clone()
    for b, w in enumerate(widths):
        want[b, :, w:] = 0
    assert torch.equal(bits(x), bits(want))


# ----------------------------------------------------------------------------------------------------------------- the network
@pytest.fixture(scope="module")
def engines(gpu_device):
    cache = {}

    def get(precision):
        if precision not in cache:
            cache[precision] = HipUNet(E.models()[2], gpu_device, precision=precision)
        return cache[precision]
    return get


@pytest.fixture(scope="module")
def mag(gpu_device):
    """The oracle's own |X| of the table's clips, each alone, zeros past its frames: the U-Net is judged on its own."""
    return E.table_reference()["mag"].to(gpu_device)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_forward_widths_vs_oracle(gpu_device, engines, mag, precision):
    unet = engines(precision)
    ref = E.table_reference()["mask"]
    mask, logits = unet.forward(mag, widths=WIDTHS, want_logits=True)
    err = (mask.cpu() - ref).abs().max().item()
    print(f"ragged U-Net [{precision}]: max |mask - oracle alone| = {err:.3e} (bar {E.TOL[precision]['mask']:.1e})")
    assert mask.shape == (B, 512, W) and err <= E.TOL[precision]["mask"]
    for b, w in enumerate(WIDTHS):
        assert (bits(mask[b, :, w:]) == 0).all() and (bits(logits[b, :, w:]) == 0).all(), (precision, b)
    if precision == "f32":
        assert torch.equal(mask.cpu() > 0.5, ref > 0.5)
    # NaN past every clip's width (the spectrogram's last frame included) changes no bit, and the caller's tensor is not written
    junk = mag.clone()
    for b, w in enumerate(WIDTHS):
        junk[b, :, w:] = float("nan")
    keep = junk.clone()
    mask2, logits2 = unet.forward(junk, widths=torch.tensor(WIDTHS), want_logits=True)
    assert torch.equal(mask2, mask) and torch.equal(logits2, logits)
    assert torch.equal(bits(junk), bits(keep))
    crop = mag[:, :512, :W].contiguous()                                         # the crop as the whole tensor: still not written
    keep = crop.clone()
    assert torch.equal(unet.forward(crop, widths=WIDTHS), mask) and torch.equal(crop, keep)


def test_forward_widths_equals_the_clip_alone_bit_for_bit(gpu_device, engines, mag):
    """fp32-class mode: the ragged batch's columns are those of ``HipUNet.forward`` on the cropped clip alone."""
    unet = engines("f32")
    mask = unet.forward(mag, widths=WIDTHS)
    for b, w in enumerate(WIDTHS):
        alone = unet.forward(mag[b:b + 1, :, :w].contiguous())
        same = torch.equal(alone, mask[b:b + 1, :, :w])
        print(f"clip {b} ({w} columns): alone vs ragged batch, max |diff| {(alone - mask[b:b + 1, :, :w]).abs().max().item():.3e}")
        assert same, (b, w)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_order_of_calls_has_no_effect(gpu_device, mag, precision):
    unet = HipUNet(E.models()[2], gpu_device, precision=precision)               # a fresh engine: its first ragged call is a short one
    short, long = [4] * B, [24] * B
    s1 = unet.forward(mag, widths=short)
    l1 = unet.forward(mag, widths=long)
    s2 = unet.forward(mag, widths=short)
    assert torch.equal(s1, s2)
    fresh = HipUNet(E.models()[2], gpu_device, precision=precision)
    p0 = fresh.forward(mag)                                                      # the padded call on an engine that never ran ragged
    assert torch.equal(l1, p0)                                                   # every width the buffer's: the padded result, after a short call
    p1 = unet.forward(mag)
    r = unet.forward(mag, widths=WIDTHS)
    p2 = unet.forward(mag)
    assert torch.equal(p1, p2) and torch.equal(p1, p0)
    assert torch.equal(r, fresh.forward(mag, widths=WIDTHS))
    assert any(len(k) == 4 for k in unet._ws) and (B, 512, W) in unet._ws       # ragged calls keep workspaces of their own


def test_widths_refusals_happen_on_the_host(gpu_device, engines, mag):
    unet = engines("f32")
    for bad in ([24] * 8, [24] * 8 + [0], [24] * 8 + [28], [24] * 8 + [10], [24.0] * 9):
        with pytest.raises(ValueError):
            unet.forward(mag, widths=bad)
