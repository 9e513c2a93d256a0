"""GPU: the U-Net's implicit GEMMs enumerate the interior of their destination only (``gemm.plan_conv2d(interior_only=True)``).
Layer by layer -- the nine GEMM-planned convolutions of the fp32-class inference network at the production geometry (B = 2) and at
ragged sizes -- the interior-only launch on a zero-haloed destination gives the padded launch's map bit for bit, both planes, halo
included (so the halo is seen to have stayed zero); the whole ``HipUNet`` gives the mask and logits of a copy whose plans were built
in the padded form, and a second forward through the same workspace gives the same bits (nothing dirtied a halo)."""
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


# name: (source channels, Cout, destination pitch, kernel, stride, padding, dilation, source halo, destination halo, (H, W) of the
# source at the production size 512 x 196)
LAYERS = {
    "e2.block.0": ([32], 64, 64, (5, 3), (2, 1), (2, 1), (1, 1), (2, 1), (1, 1), (256, 196)),
    "e3.block.0": ([64], 128, 128, (3, 3), (2, 2), (1, 1), (1, 1), (1, 1), (1, 1), (128, 196)),
    "e3.block.3": ([128], 128, 128, (3, 3), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (64, 98)),
    "e4.block.0": ([128], 256, 256, (3, 3), (2, 2), (1, 1), (1, 1), (1, 1), (1, 1), (64, 98)),
    "e4.block.3": ([256], 256, 256, (3, 3), (1, 1), (1, 1), (1, 1), (1, 1), (2, 2), (32, 49)),
    "bottleneck.0": ([256], 512, 512, (3, 3), (1, 1), (2, 2), (2, 2), (2, 2), (4, 4), (32, 49)),
    "bottleneck.3": ([512], 512, 576, (3, 3), (1, 1), (4, 4), (4, 4), (4, 4), (1, 1), (32, 49)),
    "d4.block.3": ([256], 256, 320, (3, 3), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (64, 98)),
    "d3.block.3": ([128], 128, 192, (3, 3), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1), (128, 196)),
}
# ragged sizes: (B, H, W) of the source; even H and W so that the strided layers keep their "same"-style output size
RAGGED = [(1, 2, 2), (3, 10, 14), (1, 38, 6), (2, 6, 50)]


def run_both(dev, name, B, H, W):
    Cins, Cout, Cd, k, stride, pad, dil, halo_in, halo_out, _ = LAYERS[name]
    g = torch.Generator().manual_seed(1000 * B + 10 * H + W)
    srcs = [split_map(B, H, W, c, *halo_in, dev, torch.randn(B, H, W, c, generator=g, dtype=torch.float64)) for c in Cins]
    w = torch.randn(Cout, sum(Cins), *k, generator=g, dtype=torch.float64) / (k[0] * k[1] * sum(Cins)) ** 0.5
    b = torch.randn(Cout, generator=g, dtype=torch.float64) * 0.1
    Ho = (H + 2 * pad[0] - dil[0] * (k[0] - 1) - 1) // stride[0] + 1
    Wo = (W + 2 * pad[1] - dil[1] * (k[1] - 1) - 1) // stride[1] + 1
    ref, out = (split_map(B, Ho, Wo, Cd, *halo_out, dev) for _ in range(2))
    PH, PW = halo_out
    out.t[:, :, PH:PH + Ho, PW:PW + Wo, :Cout] = float("nan")              # every interior element must be written
    kw = dict(stride=stride, padding=pad, dilation=dil, slope=0.2, device=dev)
    padded = G.plan_conv2d(srcs, ref, w, b, **kw)
    inner = G.plan_conv2d(srcs, out, w, b, interior_only=True, **kw)
    assert padded.desc.M == B * ref.Hp * ref.Wp and inner.desc.M == B * Ho * Wo and inner.tile == padded.tile
    a1 = srcs[1].t if len(srcs) > 1 else None
    padded.run(srcs[0].t, a1, out_h=ref.t)
    inner.run(srcs[0].t, a1, out_h=out.t)
    torch.cuda.synchronize()
    _lib.check_overflow(name)
    assert ref.t[0].abs().max() > 0.5                                       # the case is not degenerate
    assert torch.equal(out.t, ref.t), name                                  # both planes, halo and unused channels included
    halo = out.t.clone()
    halo[:, :, PH:PH + Ho, PW:PW + Wo] = 0
    assert (halo == 0).all()


@pytest.mark.parametrize("name", sorted(LAYERS))
def test_interior_only_layer_at_the_production_geometry(gpu_device, name):
    _lib.init()
    run_both(gpu_device, name, 2, *LAYERS[name][-1])


@pytest.mark.parametrize("B,H,W", RAGGED)
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_interior_only_layer_at_ragged_sizes(gpu_device, name, B, H, W):
    _lib.init()
    run_both(gpu_device, name, B, H, W)


def padded_form(monkeypatch):
    """Every plan_conv2d call made while this is in force builds the padded enumeration."""
    real = G.plan_conv2d
    monkeypatch.setattr(G, "plan_conv2d", lambda *a, **k: real(*a, **{**k, "interior_only": False}))


@pytest.mark.parametrize("line_tile,fuse_up", [(True, True), (False, True), (True, False)])
def test_unet_matches_its_padded_form(gpu_device, monkeypatch, line_tile, fuse_up):
    sd = syn.unet_weights()
    g = torch.Generator().manual_seed(5)
    mag = (torch.rand(2, 513, 199, generator=g) * 3).to(gpu_device)
    net = HipUNet(sd, gpu_device, precision="f32", line_tile=line_tile, fuse_up=fuse_up)
    m1, l1 = net.forward(mag, want_logits=True)
    gemms = [p for p, _, _ in net._workspace(2, 512, 196)["steps"] if isinstance(p, G.GemmPlan) and p.desc.Hg > 1]
    assert len(gemms) >= 8 and all(p.desc.halo_zero == 0 for p in gemms)    # every convolution on the GEMM enumerates an interior
    m2, l2 = net.forward(mag, want_logits=True)                             # the same workspace again: no halo was dirtied
    assert torch.equal(m2, m1) and torch.equal(l2, l1)
    other = (torch.rand(2, 513, 199, generator=g) * 3).to(gpu_device)
    net.forward(other)
    m3, l3 = net.forward(mag, want_logits=True)                             # and after another input went through it
    assert torch.equal(m3, m1) and torch.equal(l3, l1)
    with monkeypatch.context() as mp:
        padded_form(mp)
        ref = HipUNet(sd, gpu_device, precision="f32", line_tile=line_tile, fuse_up=fuse_up)
        mr, lr = ref.forward(mag, want_logits=True)
    convs = [p for p, _, _ in ref._workspace(2, 512, 196)["steps"] if isinstance(p, G.GemmPlan) and p.desc.halo_zero]
    assert len(convs) >= 8                                                  # the copy really runs the padded launches
    assert torch.equal(l1, lr)
    assert torch.equal(m1, mr)


def test_f16_unet_matches_its_padded_form(gpu_device, monkeypatch):
    """The fp16 mode's GEMM-planned layers take the same enumeration."""
    sd = syn.unet_weights()
    mag = torch.rand(1, 513, 199, generator=torch.Generator().manual_seed(6)).to(gpu_device)
    m1, l1 = HipUNet(sd, gpu_device, precision="f16").forward(mag, want_logits=True)
    with monkeypatch.context() as mp:
        padded_form(mp)
        mr, lr = HipUNet(sd, gpu_device, precision="f16").forward(mag, want_logits=True)
    assert torch.equal(l1, lr) and torch.equal(m1, mr)
