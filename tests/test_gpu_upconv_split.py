"""GPU, part 1: the fp32-class line tile of up1 + d1.block.0 (csrc/upconv_tile_x3.hip) is bit-identical to the x3 implicit GEMM of
``gemm.plan_upconv2d`` on the same split maps, at the production geometry and at ragged sizes.
Part 2: the U-Net's mask head in the epilogue of ``d1.block.3`` (csrc/conv_taps2d_head_x3.hip, the HEAD form of the kernel in
csrc/conv_taps2d_x3.h) is bit-identical to the two launches it replaces -- the 32-channel split line tile followed by
``advh_unet_head_split`` -- layer by layer (ragged tiles included) and through the whole fp32-class U-Net, and it keeps the split
format's range contract although the 32-channel map is no longer stored."""
import ctypes as C

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


def upconv_case(dev, B, Hc, W, pads=((1, 1), (1, 1), (1, 1))):
    """Maps and weights of an up1 + d1.block.0-shaped stage: coarse 64 channels, skip (x, indicator, 0 x6), 32 outputs.  The
    transposed convolution's bias is scaled x8 so that the indicator path matters."""
    g = torch.Generator().manual_seed(77 * B + Hc + W)
    (phc, pwc), (phs, pws), (pho, pwo) = pads
    xc = torch.randn(B, Hc, W, 64, generator=g, dtype=torch.float64)
    xs = torch.zeros(B, 2 * Hc, W, 8, dtype=torch.float64)
    xs[..., 0] = torch.rand(B, 2 * Hc, W, generator=g, dtype=torch.float64) * 3
    coarse = split_map(B, Hc, W, 64, phc, pwc, dev, xc)
    skip = G.add_indicator(split_map(B, 2 * Hc, W, 8, phs, pws, dev, xs), 1)
    wt = torch.randn(64, 32, 2, 1, generator=g, dtype=torch.float64) / 8
    bt = torch.randn(32, generator=g, dtype=torch.float64) * 0.1 * 8
    wc = torch.randn(32, 33, 3, 3, generator=g, dtype=torch.float64) / (3 * 33 ** 0.5)
    bc = torch.randn(32, generator=g, dtype=torch.float64) * 0.1
    mk = lambda: split_map(B, 2 * Hc, W, 32, pho, pwo, dev)
    return coarse, skip, mk, wt, bt, wc, bc


# (B, Hc, W, pads): the production stage at B = 2 (coarse 256 x 196 x 64 + xin -> 512 x 196 x 32), then ragged sizes: W = 1, 15, 33, 50,
# B = 1 and 3, the smallest coarse height the entry point accepts (1), heights that are not a multiple of the 16-row tile, other halos
P1 = ((1, 1), (1, 1), (1, 1))
UPCONV_CASES = [(2, 256, 196, P1), (1, 1, 1, P1), (3, 5, 15, P1), (1, 17, 33, ((2, 1), (1, 2), (1, 1))), (3, 16, 50, ((1, 2), (2, 1), (2, 3))),
                (1, 40, 15, P1), (1, 1, 50, P1)]


@pytest.mark.parametrize("B,Hc,W,pads", UPCONV_CASES)
def test_upconv_split_tile_matches_implicit_gemm(gpu_device, B, Hc, W, pads):
    _lib.init()
    coarse, skip, mk, wt, bt, wc, bc = upconv_case(gpu_device, B, Hc, W, pads)
    ref, out = mk(), mk()
    PH, PW = out.PH, out.PW
    out.t[:, :, PH:PH + 2 * Hc, PW:PW + W] = float("nan")                   # every interior element must be written
    assert G.upconv_tile_split_supported(coarse, skip, out, wt, wc, (2, 1), ("skip", 1))
    G.plan_upconv2d(coarse, skip, ref, wt, bt, wc, bc, stride=(2, 1), coarse_C=64, skip_C=1, indicator=("skip", 1), slope=0.2,
                    device=gpu_device).run(coarse.t, skip.t, out_h=ref.t)
    G.UpconvSplitTilePlan(coarse, skip, out, wt, bt, wc, bc, slope=0.2, device=gpu_device).run(coarse.t, skip.t, out_h=out.t)
    torch.cuda.synchronize()
    _lib.check_overflow("in-range stage")
    assert not torch.isnan(out.t).any()
    assert torch.equal(out.t, ref.t)                                        # both planes, halo included
    halo = out.t.clone()
    halo[:, :, PH:PH + 2 * Hc, PW:PW + W] = 0
    assert (halo == 0).all()
    # the indicator path matters: the same stage without the transposed convolution's bias gives another map
    nob = mk()
    G.plan_upconv2d(coarse, skip, nob, wt, bt * 0, wc, bc, stride=(2, 1), coarse_C=64, skip_C=1, indicator=("skip", 1), slope=0.2,
                    device=gpu_device).run(coarse.t, skip.t, out_h=nob.t)
    assert not torch.equal(nob.t, ref.t)


def test_upconv_split_tile_other_geometries(gpu_device):
    """What the kernel does not take: ``upconv_tile_split_supported`` is false and the entry point answers ADVH_EUNSUPPORTED."""
    _lib.init()
    coarse, skip, mk, wt, bt, wc, bc = upconv_case(gpu_device, 1, 4, 16)
    out = mk()
    assert G.upconv_tile_split_supported(coarse, skip, out, wt, wc, (2, 1), ("skip", 1))
    assert not G.upconv_tile_split_supported(coarse, skip, out, wt, wc, (2, 2), ("skip", 1))
    assert not G.upconv_tile_split_supported(coarse, skip, out, wt, wc, (2, 1), ("coarse", 64))
    c128 = G.FMap(1, 4, 16, 192, 1, 1, split=True)                          # up2 + d2.block.0: 128 coarse channels + indicator chunk
    assert not G.upconv_tile_split_supported(c128, G.FMap(1, 8, 16, 32, 1, 1, split=True), G.FMap(1, 8, 16, 64, 1, 1, split=True),
                                             torch.zeros(128, 64, 2, 1), torch.zeros(64, 96, 3, 3), (2, 1), ("coarse", 128))
    f16 = [G.FMap(f.B, f.H, f.W, f.C, f.PH, f.PW) for f in (coarse, skip, out)]
    assert not G.upconv_tile_split_supported(*f16, wt, wc, (2, 1), ("skip", 1))                  # fp16 maps: advh_upconv21_tile_f16
    plan = G.UpconvSplitTilePlan(coarse, skip, out, wt, bt, wc, bc, device=gpu_device)
    d = plan.desc
    d.Xc, d.Xs, d.W, d.bias, d.out_h = coarse.t.data_ptr(), skip.t.data_ptr(), plan.w.data_ptr(), plan.bias.data_ptr(), out.t.data_ptr()
    lo = (coarse.t.stride(0), skip.t.stride(0), plan.w.stride(0), out.t.stride(0))
    lib = _lib.lib()
    assert lib.advh_upconv21_tile_split(C.byref(d), 128, 64, *lo, None) == -4                    # ADVH_EUNSUPPORTED
    assert lib.advh_upconv21_tile_split(C.byref(d), 64, 64, *lo, None) == -4
    assert lib.advh_upconv21_tile_split(C.byref(d), 64, 32, 0, *lo[1:], None) == -1              # ADVH_EINVAL: no lo plane
    assert lib.advh_upconv21_tile_split(C.byref(d), 64, 32, lo[0] + 4, *lo[1:], None) == -1      # not a multiple of 8
    assert lib.advh_upconv21_tile_split(C.byref(d), 64, 32, *lo, None) == 0
    torch.cuda.synchronize()


def test_upconv_split_tile_keeps_the_range_contract(gpu_device):
    """An activation above 65 504 reaching the kernel's store raises SplitRangeError at ``_lib.check_overflow()``."""
    _lib.init()
    coarse, skip, mk, wt, bt, wc, bc = upconv_case(gpu_device, 1, 9, 20)
    out = mk()
    assert not flagged(lambda: G.UpconvSplitTilePlan(coarse, skip, out, wt, bt, wc, bc, device=gpu_device).run(coarse.t, skip.t, out_h=out.t))
    bc = bc.clone()
    bc[7] = 1.0e5
    plan = G.UpconvSplitTilePlan(coarse, skip, out, wt, bt, wc, bc, device=gpu_device)
    torch.cuda.synchronize()
    _lib.lib().advh_split_overflow(1)
    with pytest.raises(_lib.SplitRangeError):
        plan.run(coarse.t, skip.t, out_h=out.t)
        torch.cuda.synchronize()
        _lib.check_overflow("up1 + d1.block.0")
    torch.cuda.synchronize()
    assert _lib.lib().advh_split_overflow(1) == 0
    assert torch.isfinite(out.t).all()                                      # saturated, not inf


def head_case(dev, B, H, W, PH, PW, scale=1.0):
    """(source map, folded weight, bias, head weight, head bias) of a d1.block.3-shaped layer."""
    g = torch.Generator().manual_seed(1000 * B + H + W)
    x = torch.randn(B, H, W, 32, generator=g, dtype=torch.float64) * scale
    w = torch.randn(32, 32, 3, 3, generator=g, dtype=torch.float64) / (3 * 32 ** 0.5)
    b = torch.randn(32, generator=g, dtype=torch.float64) * 0.1
    hw = (torch.randn(32, generator=g) * 0.5).to(dev)
    return split_map(B, H, W, 32, PH, PW, dev, x), w, b, hw, 0.137


def two_launches(dev, src, w, b, hw, hb, tolerate_range=False):
    """The form the fused launch replaces: the layer into a stored map, then advh_unet_head_split on it."""
    B, H, W, PH, PW = src.B, src.H, src.W, src.PH, src.PW
    y = split_map(B, H, W, 32, PH, PW, dev)
    try:
        G.Taps2dSplitPlan(src, y, w, b, slope=0.2, device=dev).run(src.t, out_h=y.t)
    except _lib.SplitRangeError:                                            # raised after the launch: the map is written all the same
        if not tolerate_range:
            raise
    mask, logits = (torch.full((B, H, W), float("nan"), device=dev) for _ in range(2))
    rc = _lib.lib().advh_unet_head_split(y.t.data_ptr(), y.t.stride(0), B, H, W, PH, PW, hw.data_ptr(), hb, mask.data_ptr(),
                                         logits.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return mask, logits


def flagged(launch) -> bool:
    """Run ``launch`` with the sticky range flag cleared first; True iff it was raised (read after a synchronisation, or reported
    by the binding's own check)."""
    lib = _lib.lib()
    torch.cuda.synchronize()
    lib.advh_split_overflow(1)
    raised = False
    try:
        launch()
    except _lib.SplitRangeError:
        raised = True
    torch.cuda.synchronize()
    return bool(lib.advh_split_overflow(1)) or raised


# (B, H, W, PH, PW): the production layer at B = 2, then ragged tiles in both directions (and a one-column map)
HEAD_CASES = [(2, 512, 196, 1, 1), (1, 37, 50, 2, 1), (3, 17, 15, 1, 1), (1, 70, 33, 1, 2), (2, 31, 1, 1, 1)]


@pytest.mark.parametrize("B,H,W,PH,PW", HEAD_CASES)
def test_head_in_epilogue_matches_two_launches(gpu_device, B, H, W, PH, PW):
    _lib.init()
    src, w, b, hw, hb = head_case(gpu_device, B, H, W, PH, PW)
    m_ref, l_ref = two_launches(gpu_device, src, w, b, hw, hb)
    mask, logits = (torch.full((B, H, W), float("nan"), device=gpu_device) for _ in range(2))   # every position must be written
    dst = G.FMap(B, H, W, 32, PH, PW, split=True)                                                # geometry only: never stored
    plan = G.Taps2dSplitPlan(src, dst, w, b, slope=0.2, device=gpu_device).attach_head(hw, hb, mask, logits)
    plan.run(src.t)
    torch.cuda.synchronize()
    _lib.check_overflow("in-range layer")                                   # the unwritten lanes of ragged tiles raise nothing
    assert not torch.isnan(logits).any() and not torch.isnan(mask).any()
    assert l_ref.abs().max() > 0.5                                          # the case is not degenerate
    assert torch.equal(logits, l_ref)
    assert torch.equal(mask, m_ref)
    # logits are optional
    mask2 = torch.full((B, H, W), float("nan"), device=gpu_device)
    G.Taps2dSplitPlan(src, dst, w, b, slope=0.2, device=gpu_device).attach_head(hw, hb, mask2).run(src.t)
    torch.cuda.synchronize()
    assert torch.equal(mask2, m_ref)


def test_head_entry_point_takes_32_channels_only(gpu_device):
    _lib.init()
    src = split_map(1, 16, 16, 64, 1, 1, gpu_device)
    w = G.split_planes(torch.zeros(9, 64, 64, dtype=torch.float64)).contiguous().to(gpu_device)
    hw, mask = torch.zeros(64, device=gpu_device), torch.zeros(1, 16, 16, device=gpu_device)
    d = G.Taps2dDesc()
    d.X, d.W, d.B, d.H, d.W_, d.PH, d.PW, d.act, d.slope = src.t.data_ptr(), w.data_ptr(), 1, 16, 16, 1, 1, G.ACT["leaky"], 0.2
    rc = _lib.lib().advh_conv_taps2d_split_head(C.byref(d), 64, src.t.stride(0), w.stride(0), hw.data_ptr(), 0.0, mask.data_ptr(), None, None)
    assert rc == -4                                                         # ADVH_EUNSUPPORTED


def test_head_in_epilogue_keeps_the_range_contract(gpu_device):
    """An activation above 65 504 that reaches the (no longer performed) store of y1 still raises the sticky range flag --
    ``SplitRangeError`` at ``_lib.check_overflow()`` -- and the head sees the saturated planes: mask and logits equal the two-launch
    form's there too.  The same layer in range leaves the flag clear."""
    _lib.init()
    B, H, W = 1, 20, 21
    src, w, b, hw, hb = head_case(gpu_device, B, H, W, 1, 1)
    dst = G.FMap(B, H, W, 32, 1, 1, split=True)
    mask, logits = (torch.full((B, H, W), float("nan"), device=gpu_device) for _ in range(2))
    assert not flagged(lambda: G.Taps2dSplitPlan(src, dst, w, b, slope=0.2, device=gpu_device).attach_head(hw, hb, mask, logits).run(src.t))
    b = b.clone()
    b[5] = 1.0e5                                                            # channel 5 leaves the format's range at every position
    ref = []
    assert flagged(lambda: ref.extend(two_launches(gpu_device, src, w, b, hw, hb, tolerate_range=True)))
    plan = G.Taps2dSplitPlan(src, dst, w, b, slope=0.2, device=gpu_device).attach_head(hw, hb, mask, logits)
    torch.cuda.synchronize()
    _lib.lib().advh_split_overflow(1)
    with pytest.raises(_lib.SplitRangeError):
        plan.run(src.t)
        torch.cuda.synchronize()
        _lib.check_overflow("d1.block.3 with the head")
    torch.cuda.synchronize()
    assert _lib.lib().advh_split_overflow(1) == 0                           # reported once, then clear
    assert torch.isfinite(logits).all()
    assert torch.equal(mask, ref[0]) and torch.equal(logits, ref[1])


def test_split_unet_head_in_epilogue_bit_identical(gpu_device):
    """The whole fp32-class U-Net at the benchmark's shape (B = 64, 512 x 196): ``line_tile=True`` (d1.block.3 carries the head, y1
    has no storage) against ``line_tile=False`` (implicit GEMMs and advh_unet_head_split), mask and logits bit for bit."""
    sd = syn.unet_weights()
    g = torch.Generator().manual_seed(11)
    mag = (torch.rand(64, 513, 199, generator=g) * 3).to(gpu_device)
    on = HipUNet(sd, gpu_device, precision="f32", line_tile=True)
    m_on, l_on = on.forward(mag, want_logits=True)
    ws = on._workspace(64, 512, 196)
    plans = [p for p, _, _ in ws["steps"]]
    kinds = [type(p).__name__ for p in plans]
    assert kinds.count("Taps2dSplitPlan") == 4 and kinds.count("UpconvSplitTilePlan") == 1, kinds
    assert isinstance(plans[-2], G.UpconvSplitTilePlan)                     # up1 + d1.block.0
    assert plans[-1].head is not None and all(p.head is None for p in plans[:-1] if isinstance(p, G.Taps2dSplitPlan))
    assert ws["maps"]["y1"].t is None                                       # 822 MB at this shape that are no longer allocated
    m2, l2 = on.forward(mag, want_logits=True)                              # a second call through the cached workspace
    assert torch.equal(m2, m_on) and torch.equal(l2, l_on)
    del on, ws, plans
    torch.cuda.empty_cache()
    off = HipUNet(sd, gpu_device, precision="f32", line_tile=False)
    m_off, l_off = off.forward(mag, want_logits=True)
    ws = off._workspace(64, 512, 196)
    assert not any(isinstance(p, (G.Taps2dSplitPlan, G.UpconvSplitTilePlan)) for p, _, _ in ws["steps"]) and ws["maps"]["y1"].t is not None
    assert torch.equal(l_on, l_off)
    assert torch.equal(m_on, m_off)


def test_f16_unet_keeps_its_head_kernel(gpu_device):
    """The fp16 mode is untouched: its last plan carries no head and y1 is stored."""
    net = HipUNet(syn.unet_weights(), gpu_device, precision="f16", line_tile=True)
    mag = torch.rand(1, 513, 199, device=gpu_device)
    mask = net.forward(mag)
    ws = net._workspace(1, 512, 196)
    assert ws["maps"]["y1"].t is not None and getattr(ws["steps"][-1][0], "head", None) is None
    assert torch.isfinite(mask).all()
