"""GPU parity of the U-Net TRAINING step on the HIP kernels (addvisor.py:12-84 in train()
mode under train_addvisor.py:364-378).

Default precision = the fp32-class mode (split-format maps and gradients, three MFMAs per product: the reference trains in
fp32), where BOTH levels below are tight: per layer 2e-5 of max|ref|, end to end against fp32 autograd through the CPU oracle
cosine >= 0.9999 and relative L2 <= 1e-3 for EVERY parameter with the reference's LeakyReLU(0.2).  The fp16 mode
(precision="f16") keeps round 1's two-level statement:

Two levels, because LeakyReLU makes an end-to-end gradient comparison at fp16 inherently loose: a pre-activation that
the fp16 forward rounds across zero flips the local slope (1 vs 0.2) on a ~4e-4 fraction of the elements, a sparse
error of relative L2 size sqrt(fraction) ~ 2 % per layer that no kernel can avoid (torch AMP shows the same).
  (1) per-layer, tight: every weight gradient and every activation gradient the HIP path produces is compared with
      torch's conv2d_weight / conv_transpose2d / batch_norm autograd evaluated on the HIP path's OWN saved operands
      (|err| <= 4e-3 * max|ref|): this pins the transposes, the split-K GEMM indexing, the dgrad plans, the
      BatchNorm backward and the skip accumulation for all 22 layers.
  (2) end-to-end vs autograd through the CPU oracle (oracle/unet_ref.py, batch-statistics BatchNorm): mask
      |err| <= 1.5e-2; parameter gradients cosine >= 0.95 with the reference slope 0.2, and -- the kink-free control,
      LeakyReLU slope 1.0 on both sides, same kernels and data flow -- cosine >= 0.9999, relative L2 <= 1.5e-2
      (measured 0.999998); a descent step along the HIP gradient lowers the loss.

Both levels also run at the reference's full size, batch 2 on a 512 x 196 (4 s) or 512 x 248 (5 s) mask
(train_addvisor.py:363-378), with the magnitude fed uncropped as the STFT gives it and the references in fp64.  Only
there do the paths below turn on, which the small shapes never reach: split-K wgrad GEMMs with many K slices
(``_SplitKGemm`` with nz > 1), wgrad tile kernels with more tiles than workgroups (the NBUF=2 ring prefetching the next
tile), and the 1024-workgroup position reductions (BatchNorm, head, stem and skip wgrads) striding over many rows.  At
that size fp32 arithmetic of any kind flips a few LeakyReLU slopes against fp64, so the per-layer reference takes the
branch HIP took, and the fp32-class end-to-end bound with slope 0.2 is relative L2 <= 1e-2; the kink-free control there
keeps 1e-3 (test_train_step_against_oracle_autograd gives the error analysis)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn import grad as nngrad

from addvisor_hip import _lib, gemm as G, synthetic as syn
from addvisor_hip.unet_train import HipUNetTrain, BN_EPS, SLOPE
from oracle import unet_ref

pytestmark = pytest.mark.gpu


# the magnitude the STFT gives for the reference's 4 s / 5 s clips (n_fft 1024, hop 322, centred frames), which the U-Net
# crops to [512, 4 * (T // 4)]: the full-size cases feed it uncropped
STFT_SHAPE = {(512, 196): (513, 199), (512, 248): (513, 249)}


def setup(dev, B, H, W, seed, precision="f32", oracle_grads=True):
    """At the full size (STFT_SHAPE) the magnitude is [B, 513, T] and the oracle runs in fp64: its sums cover up to
    2 x 10^5 positions.  ``oracle_grads=False``: forward only (the upstream gradient), no oracle parameter gradients."""
    sd = syn.unet_weights(seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    Fq, Tq = STFT_SHAPE.get((H, W), (H, W))
    mag = torch.rand(B, Fq, Tq, generator=gen) * 3.0
    # a structured upstream gradient, as a real loss gives: d/dmask of mean((mask - target)^2) with a smooth target
    target = F.interpolate(torch.rand(B, 1, max(H // 8, 1), max(W // 4, 1), generator=gen), size=(H, W), mode="bilinear",
                           align_corners=False)[:, 0]
    names = [k for k in sd if k.endswith("weight") or k.endswith("bias")]
    dt = torch.float64 if (H, W) in STFT_SHAPE else torch.float32
    with torch.set_grad_enabled(oracle_grads):
        ref_sd = {k: v.clone().to(dt) if v.is_floating_point() else v.clone() for k, v in sd.items()}
        for k in names:
            ref_sd[k].requires_grad_(oracle_grads)
        ref_mask = unet_ref.unet_forward(mag[:, None, :H, :W].to(dt), ref_sd, bn_batch=True)[:, 0]
        dmask = (2.0 * (ref_mask.detach() - target) / ref_mask.numel()).float()
        ref_grads = None
        if oracle_grads:
            ref_grads = dict(zip(names, torch.autograd.grad((ref_mask * dmask.to(dt)).sum(), [ref_sd[k] for k in names], allow_unused=True)))

    params = {k: v.clone().float().to(dev) for k, v in sd.items()}
    net = HipUNetTrain(params, dev, precision=precision)
    assert net.precision == precision
    return net, params, mag, target, dmask, ref_mask.detach(), ref_grads


def interior(f, t=None):
    t = f.t if t is None else t
    t = G.join_planes(t) if f.split else t.float()            # fp32-class mode: [2, B, Hp, Wp, C] plane pair
    return t[:, f.PH:f.PH + f.H, f.PW:f.PW + f.W].cpu().permute(0, 3, 1, 2).contiguous()     # NCHW fp32


def close(a, b, tol, what):
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    assert err <= tol * scale + 1e-9, (what, err, scale)
    return err / (scale + 1e-30)


def wgrad2d_tiles(B, H, W, TR=16):
    """TR x 16-position tiles of one wgrad tile-kernel launch (csrc/conv_wgrad.hip): TR = 16 for ``advh_conv_wgrad2d_f16`` and the
    32 x 32 form of ``advh_conv_wgrad2d_split``, 8 for its other three forms"""
    return B * -(-H // TR) * -(-W // 16)


def split_tr(CI, CO):
    return 16 if CI == CO == 32 else 8


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("B,H,W,seed", [(2, 32, 8, 5), (3, 64, 24, 7), (2, 512, 196, 11), (2, 512, 248, 13)])
def test_every_layer_backward_is_exact_on_its_own_operands(gpu_device, B, H, W, seed, precision):
    """The references are fp64 sums over HIP's own operands.  Besides every tensor against its own maximum, each (output slice, input
    slice) block of a slice-pair wgrad, the magnitude column of d1.block.0 and the head's 33 sums are checked against their own maxima,
    so that a wrong slice or a dropped partial with small values cannot hide under a larger neighbour.  At the full size the magnitude
    comes uncropped ([B, 513, T]: the pack, stem and skip-wgrad kernels stride it by its own Fq / Tq) and the test asserts from the
    workspace that the paths only that size reaches did run: a split-K wgrad GEMM with nz > 1 K slices, and a wgrad tile kernel with
    more position tiles than workgroups."""
    full = (H, W) in STFT_SHAPE
    net, params, mag, target, dmask, _, _ = setup(gpu_device, B, H, W, seed, precision, oracle_grads=False)
    TOL = 2e-5 if precision == "f32" else 4e-3
    wq = (lambda w: w.double()) if precision == "f32" else (lambda w: w.half().double())     # the operand precision of the dgrad weights
    net.forward(mag.to(gpu_device), H=H)                                   # W = 4 * (T // 4), as the pipeline crops
    grads = net.backward(dmask.to(gpu_device))
    assert net._last[4:6] == (H, W)
    ws = net._workspace(B, H, W)
    m, z, g = ws["maps"], ws["z"], ws["g"]
    worst, flips, worst_band = 0.0, 0, 0.0
    # loss scale: recover it from the head (grads are unscaled, maps are scaled)
    gy1 = interior(g["y1"])
    dl = ws["dlogit"].cpu()
    hw = params["mask_head.0.weight"].cpu().reshape(32)
    S = (gy1[:, 0] / (dl * hw[0] + 1e-30)).median().item()
    assert abs(np.log2(S) - round(np.log2(S))) < 1e-3        # a power of two
    # mask head: dw[c] = sum dlogit * y1[c], db = sum dlogit over HIP's own dlogit and y1 (one kernel, one 33-sum output)
    y1, dl = interior(m["y1"]).double(), dl.double()
    ref33 = torch.cat([torch.einsum("bhw,bchw->c", dl, y1), dl.sum().reshape(1)])
    got33 = torch.cat([grads["mask_head.0.weight"].cpu().reshape(32), grads["mask_head.0.bias"].cpu().reshape(1)]).double()
    worst = max(worst, close(got33, ref33, TOL, "mask_head.0 weight / bias"))
    acc = {}
    for L in ws["layers"]:
        if L["kind"] == "up":
            name, (sh, sw) = L["name"], L["stride"]
            x, gy = interior(L["src"]).double(), interior(L["gdst"]).double()
            w = params[name + ".weight"].cpu()
            dw = torch.einsum("bchw,bdhiwj->cdij", x, gy.view(B, gy.shape[1], x.shape[2], sh, x.shape[3], sw))
            worst = max(worst, close(grads[name + ".weight"].cpu().double() * S, dw, TOL, name + ".weight"))
            worst = max(worst, close(grads[name + ".bias"].cpu().double() * S, gy.sum((0, 2, 3)), TOL, name + ".bias"))
            a = acc.setdefault(id(L["gsrc"]), [L["gsrc"], 0.0])
            a[1] = a[1] + F.conv2d(gy, wq(w), stride=(sh, sw))
            continue
        cname, bname, dst = L["cname"], L["bname"], L["dst"]
        (KH, KW), (sh, sw), pad, dil = L["k"], L["stride"], L["pad"], L["dil"]
        dzm = L["dz"]
        dz = interior(dzm)[:, :, ::sh, ::sw] if L["srcs"] != ["mag"] else interior(dzm)
        dz = dz[:, :, :m[dst].H, :m[dst].W].double()
        # BatchNorm + LeakyReLU backward on HIP's own z and incoming gradient.  LeakyReLU takes the branch HIP's forward took, the sign of
        # its own activation map: y = scale * z + shift from fp32 batch statistics can put an element that lies a rounding error from zero
        # on the other side of it than fp64 statistics do (fp32 autograd does the same), and a flipped slope moves that element's dz by 0.8
        # of its size.  At 2 x 10^5 positions a layer has ~10^7 elements and such a flip turns up (measured: one per f32 case at the full
        # size, |y| <= 1.2e-9 of its channel's maximum); every element whose branch differs must lie in that rounding band.
        zz = interior(z[dst]).double()
        gin = interior(g[dst]).double()
        pos = ~torch.signbit(interior(m[dst]))
        gamma, beta = params[bname + ".weight"].cpu().double(), params[bname + ".bias"].cpu().double()
        with torch.enable_grad():
            zr = zz.clone().requires_grad_(True)
            gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
            yb = F.batch_norm(zr, None, None, gr, br, True, 0.0, BN_EPS)
            y = yb * torch.where(pos, 1.0, SLOPE).double()
            dzr, dgr, dbr = torch.autograd.grad((y * gin).sum(), [zr, gr, br])
        yb = yb.detach()
        flip = (yb > 0) != pos
        if flip.any():
            band = (yb.abs() / yb.abs().amax((0, 2, 3), keepdim=True))[flip].max().item()
            flips, worst_band = flips + int(flip.sum()), max(worst_band, band)
            assert band <= 1e-5, (cname, int(flip.sum()), band)
        worst = max(worst, close(dz, dzr, TOL, cname + " dz"))
        worst = max(worst, close(grads[bname + ".weight"].cpu().double() * S, dgr, TOL, bname + ".weight"))
        worst = max(worst, close(grads[bname + ".bias"].cpu().double() * S, dbr, TOL, bname + ".bias"))
        # weight gradient on HIP's own input activations and dz
        w = params[cname + ".weight"].cpu()
        if L["srcs"] == ["mag"]:
            x = mag[:, None, :H, :W].double()
        else:
            x = torch.cat([interior(m[s]) for s in L["srcs"]], 1)[:, :w.shape[1]].double()
        dw = nngrad.conv2d_weight(x, w.shape, dz, stride=(sh, sw), padding=pad, dilation=dil)
        gw = grads[cname + ".weight"].cpu().double() * S
        worst = max(worst, close(gw, dw, TOL, cname + ".weight"))
        for _, d2, CI, CO, cx0, cz0, base in L.get("wg2d_pairs", []):          # every slice-pair launch against its own block
            blk = (slice(cz0, cz0 + CO), slice(base + cx0, base + cx0 + CI))
            worst = max(worst, close(gw[blk], dw[blk], TOL, f"{cname}.weight[{cz0}:{cz0 + CO}, {base + cx0}:{base + cx0 + CI}]"))
        if cname == "d1.block.0":                                              # the magnitude channel of the skip concat
            worst = max(worst, close(gw[:, 32], dw[:, 32], TOL, cname + ".weight[:, 32]"))
        assert grads[cname + ".bias"].abs().max().item() == 0.0
        if L["srcs"] == ["mag"]:
            continue
        # activation gradients: contributions of this layer to each source map
        dx = nngrad.conv2d_input(x.shape, wq(w), dz, stride=(sh, sw), padding=pad, dilation=dil)
        lo = 0
        for s in L["srcs"]:
            c = g[s].C
            a = acc.setdefault(id(g[s]), [g[s], 0.0])
            a[1] = a[1] + dx[:, lo:lo + c]
            lo += m[s].C
    for f, ref in acc.values():
        worst = max(worst, close(interior(f).double(), ref, TOL, "activation gradient"))
    if full:                                                 # the paths only the full size reaches did run
        nz = {L.get("cname", L.get("name")): L["wg"].desc.nz for L in ws["layers"] if "wg" in L}
        assert max(nz.values()) > 1, nz
        lib = _lib.lib()
        if precision == "f32":
            multi = sorted({(L["cname"], CI, CO) for L in ws["layers"] for _, d2, CI, CO, _, _, _ in L.get("wg2d_pairs", [])
                            if wgrad2d_tiles(d2.B, d2.H, d2.W_, split_tr(CI, CO)) > lib.advh_conv_wgrad2d_split_parts(CI, CO, d2.B, d2.H, d2.W_)})
        else:
            multi = [L["cname"] for L in ws["layers"] if "wg2d" in L
                     if wgrad2d_tiles(B, L["wg2d"].H, L["wg2d"].W_) > lib.advh_conv_wgrad2d_parts(z[L["dst"]].C, B, L["wg2d"].H, L["wg2d"].W_)]
        assert multi
        print(f"split-K slices {nz}; wgrad tile launches with more tiles than workgroups: {multi}")
    print(f"per-layer backward parity [{precision}] B={B} {H}x{W} (magnitude {tuple(mag.shape)}): worst max-rel err {worst:.2e}; "
          f"loss scale 2^{int(round(np.log2(S)))}; {flips} LeakyReLU branches differ from fp64 statistics, |y| <= {worst_band:.1e} of the channel max")


@pytest.mark.parametrize("B,H,W,seed,slope,precision", [(2, 32, 8, 5, 0.2, "f32"), (2, 32, 8, 5, 0.2, "f16"),
                                                         (3, 64, 24, 7, 0.2, "f32"), (3, 64, 24, 7, 0.2, "f16"),
                                                         (3, 64, 24, 7, 1.0, "f32"), (3, 64, 24, 7, 1.0, "f16"),
                                                         (2, 512, 196, 11, 0.2, "f32"), (2, 512, 248, 13, 0.2, "f32"),
                                                         (2, 512, 196, 11, 1.0, "f32"), (2, 512, 196, 11, 1.0, "f16")])
def test_train_step_against_oracle_autograd(gpu_device, monkeypatch, B, H, W, seed, slope, precision):
    """slope 0.2 = the reference network.  slope 1.0 = the kink-free control: the same kernels, launches and data
    flow with LeakyReLU turned into the identity on both sides, where end-to-end agreement must be (and is) tight.
    The full-size cases (the reference's batch 2 at 512 x 196 and 512 x 248, magnitude uncropped, oracle in fp64) keep the
    same bounds except one: fp32-class with slope 0.2 allows relative L2 <= 1e-2 per parameter (cosine >= 0.9999 stays).
    Error analysis: LeakyReLU(0.2)'s derivative jumps by 0.8 at zero.  fp32 arithmetic anywhere in the forward (batch
    statistics, convolution sums: the masks agree to ~2e-6) leaves a pre-activation that lies within a rounding error of
    zero on the other side of it than fp64 does; with ~10^7 elements per layer that happens a few times per step (the
    per-layer test sees one per case from the statistics alone).  A flipped slope changes one gradient element by 0.8 of
    its size; the BatchNorm backward spreads it over the channel (mean and
    projection terms) and every earlier layer inherits it, so parameter gradients move by a sparse error that grows with the
    element count.  No fp32 arithmetic avoids it: torch's own fp32 autograd of the same oracle differs from fp64 by relative
    L2 3.7e-3 (cosine 0.999993) at 512 x 196 and 3.6e-3 at 512 x 248, and by 1.7e-4 once the kink is removed (slope 1.0).
    Measured for the HIP path: worst relative L2 5.3e-3 (cosine 0.999986, up3.bias) at 512 x 196, 3.6e-3 (e4.block.4.bias)
    at 512 x 248.  The kink-free full-size control (f32, slope 1.0) keeps the tight 1e-3, measured 1.9e-5."""
    import addvisor_hip.unet_train as UT
    if slope != SLOPE:
        lrelu = F.leaky_relu
        monkeypatch.setattr(UT, "SLOPE", slope)
        monkeypatch.setattr(unet_ref.F, "leaky_relu", lambda x, s=0.2, **kw: lrelu(x, slope))
    net, params, mag, target, dmask, ref_mask, ref_grads = setup(gpu_device, B, H, W, seed, precision)
    f32 = precision == "f32"
    rel2_f32 = 1e-2 if ((H, W) in STFT_SHAPE and slope != 1.0) else 1e-3   # see the docstring's error analysis
    rm0 = params["e2.block.1.running_mean"].clone()
    mask = net.forward(mag.to(gpu_device), H=H, W=W)
    err = (mask.cpu() - ref_mask).abs().max().item()
    print(f"train-mode forward [{precision}] B={B} {H}x{W} slope {slope}: mask max err {err:.2e}")
    assert err <= (2e-5 if f32 else 1.5e-2)
    assert not torch.equal(params["e2.block.1.running_mean"], rm0)                   # running statistics were updated
    grads = net.backward(dmask.to(gpu_device))
    worst, worst_rel2 = (1.0, "", 0.0), (0.0, "")
    for k, r in ref_grads.items():
        gk = grads[k].cpu().reshape(r.shape)
        assert torch.isfinite(gk).all(), k
        if gk.abs().max().item() == 0.0:                                            # conv bias before a batch-stat BatchNorm
            assert r.abs().max().item() <= 1e-6 * max(1.0, dmask.abs().sum().item()), k
            continue
        cos = F.cosine_similarity(gk.flatten().double(), r.flatten().double(), dim=0).item()
        rel2 = ((gk - r).norm() / r.norm()).item()
        if cos < worst[0]:
            worst = (cos, k, rel2)
        worst_rel2 = max(worst_rel2, (rel2, k))
        if f32:                                                  # fp32-class mode: tight with the reference's LeakyReLU(0.2) too
            assert cos >= 0.9999 and rel2 <= rel2_f32, (k, cos, rel2)
        elif slope == 1.0:
            assert cos >= 0.9999 and rel2 <= 1.5e-2, (k, cos, rel2)
        else:
            assert cos >= 0.95, (k, cos, rel2)
    print(f"end-to-end parameter gradients [{precision}] (slope {slope}): worst cosine {worst[0]:.7f} (rel L2 {worst[2]:.2e}) at {worst[1]}; "
          f"worst rel L2 {worst_rel2[0]:.2e} at {worst_rel2[1]}")
    # a small step along the negative HIP gradient lowers the loss mean((mask - target)^2)
    loss0 = ((mask.cpu() - target) ** 2).mean().item()
    gn = max(v.abs().max().item() for v in grads.values())
    for k, v in grads.items():
        params[k].sub_(v.reshape(params[k].shape) * (2e-3 / gn))
    loss1 = ((net.forward(mag.to(gpu_device), H=H, W=W).cpu() - target) ** 2).mean().item()
    print(f"loss {loss0:.6f} -> {loss1:.6f}")
    assert loss1 < loss0


def test_backward_is_deterministic(gpu_device):
    net, params, mag, target, dmask, _, _ = setup(gpu_device, 2, 32, 8, 9)
    net.forward(mag.to(gpu_device), H=32, W=8); g1 = net.backward(dmask.to(gpu_device))
    net.forward(mag.to(gpu_device), H=32, W=8); g2 = net.backward(dmask.to(gpu_device))     # only the running buffers moved
    assert all(torch.equal(g1[k], g2[k]) for k in g1)


# more position tiles than workgroups, unequal tile counts per workgroup, so the persistent loop and the NBUF=2 ring (next tile's DMA under
# this tile's MFMAs) run: the layer geometries of the 4 s batch-2 step (d1.block.3, e2.block.3 / d3, the 32 x 64 slice of d2.block.0) and,
# per form, ragged cases with H % TR != 0 and W % 16 != 0 on sliced maps
WGRAD_SPLIT_MULTI = [(32, 32, 32, 0, 32, 0, 2, 512, 196), (64, 64, 64, 0, 64, 0, 2, 128, 196), (32, 64, 32, 0, 64, 0, 2, 256, 196),
                     (32, 32, 64, 32, 96, 64, 2, 200, 330), (64, 64, 192, 64, 128, 64, 2, 250, 170), (32, 64, 96, 64, 128, 0, 2, 150, 120),
                     (64, 32, 128, 0, 96, 64, 1, 333, 250)]


@pytest.mark.parametrize("CI,CO,Cx,cx0,Cz,cz0,B,H,W", [(32, 32, 32, 0, 32, 0, 2, 40, 24), (64, 64, 64, 0, 64, 0, 2, 24, 20), (64, 64, 192, 64, 128, 64, 3, 16, 12),
                                                       (32, 64, 96, 64, 128, 0, 2, 19, 33), (64, 32, 128, 0, 96, 64, 2, 9, 17), (32, 32, 64, 32, 96, 32, 1, 35, 50)]
                         + WGRAD_SPLIT_MULTI)
def test_wgrad2d_split_slice_pairs(gpu_device, CI, CO, Cx, cx0, Cz, cz0, B, H, W):
    """``advh_conv_wgrad2d_split`` (csrc/conv_wgrad.hip: transposing LDS reads, three fp16 MFMAs per fragment pair) on one (input slice,
    output slice) pair of wider split-format maps with different halos, ragged tile edges included, against the fp64 weight gradient of a
    3x3 "same" convolution (addvisor.py:20-24 under train_addvisor.py:376) on the joined values."""
    import ctypes as C
    from addvisor_hip.unet_train import Wgrad2dDesc
    _lib.init()
    lib = _lib.lib()
    parts = lib.advh_conv_wgrad2d_split_parts(CI, CO, B, H, W)
    ntiles = wgrad2d_tiles(B, H, W, split_tr(CI, CO))
    if (CI, CO, Cx, cx0, Cz, cz0, B, H, W) in WGRAD_SPLIT_MULTI:
        assert ntiles > parts and ntiles % parts and W % 16, (ntiles, parts)
    g = torch.Generator().manual_seed(CI + CO + H)
    x = G.FMap(B, H, W, Cx, 2, 1, split=True).alloc(gpu_device)
    z = G.FMap(B, H, W, Cz, 1, 3, split=True).alloc(gpu_device)
    xs, zs = G.split_planes(torch.randn(B, H, W, Cx, generator=g)), G.split_planes(torch.randn(B, H, W, Cz, generator=g) * 0.3)
    x.t[:, :, 2:2 + H, 1:1 + W] = xs.to(gpu_device)
    z.t[:, :, 1:1 + H, 3:3 + W] = zs.to(gpu_device)
    part = torch.empty(parts * 9 * CI * CO, dtype=torch.float32, device=gpu_device)
    dw = torch.full((9, CO, CI), float("nan"), dtype=torch.float32, device=gpu_device)
    d = Wgrad2dDesc(B=B, H=H, W_=W, PHx=2, PWx=1, PHz=1, PWz=3)
    d.X, d.DZ, d.partial = x.t.data_ptr(), z.t.data_ptr(), part.data_ptr()
    _lib.check(lib.advh_conv_wgrad2d_split(C.byref(d), CI, CO, Cx, cx0, Cz, cz0, x.t.stride(0), z.t.stride(0), dw.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "advh_conv_wgrad2d_split")
    torch.cuda.synchronize()
    xj = G.join_planes(xs).double()[..., cx0:cx0 + CI].permute(0, 3, 1, 2)          # [B, CI, H, W]
    zj = G.join_planes(zs).double()[..., cz0:cz0 + CO].permute(0, 3, 1, 2)
    ref = nngrad.conv2d_weight(xj, (CO, CI, 3, 3), zj, padding=1)                    # [CO, CI, 3, 3]
    got = dw.cpu().double().view(3, 3, CO, CI).permute(2, 3, 0, 1)
    assert torch.isfinite(got).all()
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"wgrad2d split {CI}x{CO} slice of {Cx}x{Cz} B={B} {H}x{W}: {ntiles} tiles on {parts} workgroups, rel err {err:.2e}")
    assert err < 2e-6


# one tile per workgroup; more tiles than workgroups: d1.block.3 / d2.block.3 of the 4 s batch-2 step, and ragged maps with 2-3 tiles per workgroup
WGRAD_F16_ONE = [(32, 2, 40, 24), (64, 1, 35, 50)]
WGRAD_F16_MULTI = [(32, 2, 512, 196), (64, 2, 256, 196), (32, 4, 250, 330), (64, 3, 190, 250)]


@pytest.mark.parametrize("C_,B,H,W", WGRAD_F16_ONE + WGRAD_F16_MULTI)
def test_wgrad2d_f16(gpu_device, C_, B, H, W):
    """``advh_conv_wgrad2d_f16`` (the fp16 mode's 3x3 stride-1 wgrad for square 32 / 64-channel layers: persistent workgroups streaming
    16 x 16-position tiles through a two-slot LDS ring) against the fp64 weight gradient on the same fp16 values.  The products of two
    fp16 values are exact in fp32, so the only error is fp32 accumulation: a workgroup sums at most 256 t products per output into one
    fp32 accumulator (t = the most tiles of one workgroup), whatever order the MFMAs use, the partials are added in fp64 and rounded
    once -- |err| <= (256 t + 1) u sum_p |x| |dz| with u = 2^-24 (Higham's gamma_n bound; measured <= 0.001 of it).  A tile read twice
    or lost moves outputs by sums of 256 products: a ring that prefetches the current tile again exceeds the bound 230-610 times."""
    import ctypes as C
    from addvisor_hip.unet_train import Wgrad2dDesc
    _lib.init()
    lib = _lib.lib()
    parts = lib.advh_conv_wgrad2d_parts(C_, B, H, W)
    ntiles = wgrad2d_tiles(B, H, W)
    if (C_, B, H, W) in WGRAD_F16_MULTI:
        assert ntiles > parts and ntiles % parts and W % 16, (ntiles, parts)
    else:
        assert ntiles <= parts
    t = -(-ntiles // parts)
    g = torch.Generator().manual_seed(C_ + H + W)
    x = G.FMap(B, H, W, C_, 1, 2).alloc(gpu_device)
    z = G.FMap(B, H, W, C_, 2, 1).alloc(gpu_device)
    xv, zv = torch.randn(B, H, W, C_, generator=g).half(), (torch.randn(B, H, W, C_, generator=g) * 0.3).half()
    x.t[:, 1:1 + H, 2:2 + W] = xv.to(gpu_device)
    z.t[:, 2:2 + H, 1:1 + W] = zv.to(gpu_device)
    part = torch.full((parts * 9 * C_ * C_,), float("nan"), dtype=torch.float32, device=gpu_device)
    dw = torch.full((9, C_, C_), float("nan"), dtype=torch.float32, device=gpu_device)
    d = Wgrad2dDesc(B=B, H=H, W_=W, PHx=1, PWx=2, PHz=2, PWz=1)
    d.X, d.DZ, d.partial = x.t.data_ptr(), z.t.data_ptr(), part.data_ptr()
    _lib.check(lib.advh_conv_wgrad2d_f16(C.byref(d), C_, dw.data_ptr(), torch.cuda.current_stream().cuda_stream), "advh_conv_wgrad2d_f16")
    torch.cuda.synchronize()
    xd, zd = xv.double().permute(0, 3, 1, 2), zv.double().permute(0, 3, 1, 2)
    ref = nngrad.conv2d_weight(xd, (C_, C_, 3, 3), zd, padding=1)                     # [CO, CI, 3, 3]
    mass = nngrad.conv2d_weight(xd.abs(), (C_, C_, 3, 3), zd.abs(), padding=1)        # sum_p |x| |dz| per output
    got = dw.cpu().double().view(3, 3, C_, C_).permute(2, 3, 0, 1)
    assert torch.isfinite(got).all()
    bound = (256 * t + 1) * 2.0 ** -24 * mass
    ratio = float(((got - ref).abs() / bound).max())
    print(f"wgrad2d f16 C={C_} B={B} {H}x{W}: {ntiles} tiles on {parts} workgroups (<= {t} each), max |err| / bound {ratio:.3f}, "
          f"rel err {float((got - ref).abs().max() / ref.abs().max()):.2e}")
    assert ratio <= 1.0
