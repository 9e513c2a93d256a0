"""GPU: the fp32-class 2-D line tile (csrc/conv_taps2d_x3.hip) is bit-identical to the x3 implicit GEMM it replaces -- layer by layer
on split-format maps of the U-Net's geometries (ragged edges included), and through the whole fp32-class U-Net."""
import pytest
import torch

from addvisor_hip import _lib, gemm as G, synthetic as syn
from addvisor_hip.unet import HipUNet

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def split_map(B, H, W, Cn, PH, PW, dev, x=None):
    f = G.FMap(B, H, W, Cn, PH, PW, split=True).alloc(dev)
    if x is not None:
        f.t[:, :, PH:PH + H, PW:PW + W] = G.split_planes(x).to(dev)
    return f


# (C, B, H, W, PH, PW): the production layers at B = 2 (e1 / d2 / e2 / d1 .block.3 of the 512 x 196 U-Net), then ragged tiles
CASES = [(32, 2, 256, 196, 2, 1), (64, 2, 256, 196, 1, 1), (64, 2, 128, 196, 1, 1), (32, 2, 512, 196, 1, 1),
         (32, 2, 37, 50, 2, 1), (64, 3, 16, 16, 1, 1), (64, 1, 70, 33, 1, 2), (32, 1, 17, 15, 1, 1), (64, 2, 31, 1, 1, 1)]


@pytest.mark.parametrize("Cn,B,H,W,PH,PW", CASES)
def test_taps2d_split_matches_implicit_gemm(gpu_device, Cn, B, H, W, PH, PW):
    _lib.init()
    g = torch.Generator().manual_seed(Cn * 7 + H + W)
    x = torch.randn(B, H, W, Cn, generator=g, dtype=torch.float64)
    w = torch.randn(Cn, Cn, 3, 3, generator=g, dtype=torch.float64) / (3 * Cn ** 0.5)
    b = torch.randn(Cn, generator=g, dtype=torch.float64) * 0.1
    src = split_map(B, H, W, Cn, PH, PW, gpu_device, x)
    ref, out = split_map(B, H, W, Cn, PH, PW, gpu_device), split_map(B, H, W, Cn, PH, PW, gpu_device)
    out.t[:, :, PH:PH + H, PW:PW + W] = float("nan")                       # every interior position must be written
    assert G.taps2d_split_supported([src], out, w)
    G.plan_conv2d([src], ref, w, b, slope=0.2, device=gpu_device).run(src.t, out_h=ref.t)
    G.Taps2dSplitPlan(src, out, w, b, slope=0.2, device=gpu_device).run(src.t, out_h=out.t)
    torch.cuda.synchronize()
    assert not torch.isnan(out.t).any()
    assert torch.equal(out.t, ref.t)                                        # both planes, halo included (zero in both)
    halo = out.t.clone()
    halo[:, :, PH:PH + H, PW:PW + W] = 0
    assert (halo == 0).all()


def test_split_unet_line_tile_bit_identical(gpu_device):
    """The whole fp32-class U-Net at the benchmark's shape (B = 64, 512 x 196): line tiles on == implicit GEMM only, mask and
    logits bit for bit."""
    sd = syn.unet_weights()
    g = torch.Generator().manual_seed(5)
    mag = (torch.rand(64, 513, 199, generator=g) * 3).to(gpu_device)
    on = HipUNet(sd, gpu_device, precision="f32", line_tile=True)
    m_on, l_on = on.forward(mag, want_logits=True)
    kinds = [type(p).__name__ for p, _, _ in on._workspace(64, 512, 196)["steps"]]
    assert kinds.count("Taps2dSplitPlan") == 4, kinds
    del on
    torch.cuda.empty_cache()
    off = HipUNet(sd, gpu_device, precision="f32", line_tile=False)
    m_off, l_off = off.forward(mag, want_logits=True)
    assert not any(type(p).__name__ == "Taps2dSplitPlan" for p, _, _ in off._workspace(64, 512, 196)["steps"])
    assert torch.equal(l_on, l_off)
    assert torch.equal(m_on, m_off)
