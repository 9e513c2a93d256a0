"""The ADDvisor U-Net mask decoder (addvisor.py:12-84) on the HIP kernels.

Feature maps are zero-haloed NHWC fp16 (H = frequency bins, W = frames); every Conv2d /
ConvTranspose2d is one implicit-GEMM launch (``gemm.plan_conv2d`` / ``plan_convT2d``) with BatchNorm
(eval mode) folded into the weights, LeakyReLU(0.2) in the epilogue and the skip
concatenations done by pointer.  The 1-channel stem and the 1x1 mask head are direct kernels.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import torch

from . import _lib, gemm as G

SLOPE = 0.2
BN_EPS = 1e-5


def _fold_bn(sd, conv: str, bn: str, dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eval-mode BatchNorm folded into the convolution; ``dtype=torch.float64`` for the fp32-class mode (the folded
    weight is then split into two fp16 planes from its fp64 value)."""
    w, b = sd[conv + ".weight"].to(dtype), sd[conv + ".bias"].to(dtype)
    s = sd[bn + ".weight"].to(dtype) / torch.sqrt(sd[bn + ".running_var"].to(dtype) + BN_EPS)
    return w * s.view(-1, 1, 1, 1), (b - sd[bn + ".running_mean"].to(dtype)) * s + sd[bn + ".bias"].to(dtype)


def reference_flops(B: int, H: int, W: int) -> float:
    """2 x MACs of addvisor.py:31-60 on a ``B x 1 x H x W`` input (convolutions, transposed convolutions, 1x1 head)."""
    def conv(h, w, cin, cout, taps):
        return 2.0 * B * h * w * cin * cout * taps
    f = conv(H // 2, W, 1, 32, 15) + conv(H // 2, W, 32, 32, 9)
    f += conv(H // 4, W, 32, 64, 15) + conv(H // 4, W, 64, 64, 9)
    f += conv(H // 8, W // 2, 64, 128, 9) + conv(H // 8, W // 2, 128, 128, 9)
    f += conv(H // 16, W // 4, 128, 256, 9) + conv(H // 16, W // 4, 256, 256, 9)
    f += conv(H // 16, W // 4, 256, 512, 9) + conv(H // 16, W // 4, 512, 512, 9)
    f += conv(H // 16, W // 4, 512, 256, 4) + conv(H // 8, W // 2, 384, 256, 9) + conv(H // 8, W // 2, 256, 256, 9)
    f += conv(H // 8, W // 2, 256, 128, 4) + conv(H // 4, W, 192, 128, 9) + conv(H // 4, W, 128, 128, 9)
    f += conv(H // 4, W, 128, 64, 2) + conv(H // 2, W, 96, 64, 9) + conv(H // 2, W, 64, 64, 9)
    f += conv(H // 2, W, 64, 32, 2) + conv(H, W, 33, 32, 9) + conv(H, W, 32, 32, 9)
    return f + conv(H, W, 32, 1, 1)


class HipUNet:
    """``forward(mag [B, F>=H, T>=W] fp32) -> mask [B, H, W] fp32`` (H % 16 == 0, W % 4 == 0)."""

    def __init__(self, sd: Dict[str, torch.Tensor], device, line_tile: Optional[bool] = None, fuse_up: Optional[bool] = None,
                 precision: Optional[str] = None):
        """``line_tile``: run the layers that have an LDS line-tile kernel on it instead of the implicit GEMM; which layers those are
        is decided in one place, ``gemm.select_conv2d`` / ``gemm.select_upconv2d`` (the 3x3 32- / 64-channel same-geometry layers
        and, with ``fuse_up``, e2.block.0 and up1 + d1.block.0; fp16 and split-format kernels, the latter bit-identical to the
        implicit GEMM).  ``fuse_up``: fold every ConvTranspose2d into the convolution that follows it (``gemm.plan_upconv2d``) so
        the up-sampled maps are never written.
        ``precision``: "f16" | "f32" (default ``ADDVISOR_PRECISION``, i.e. f32): "f32" is the fp32-class mode -- every map a
        split-format plane pair, every convolution three MFMAs per product (``advh_gemm_desc.split``), weights folded in
        fp64 -- whose ``mask > 0.5`` index set reproduces the reference's fp32 CPU result (addvisor.py:57-60; asserted
        against tests/golden/unet.npz).  In that mode with ``line_tile`` the last layer, ``d1.block.3``, runs the 1x1 mask head in
        its epilogue (``advh_conv_taps2d_split_head``, bit-identical to ``advh_unet_head_split``): the map ``y1`` is then neither
        written nor allocated.

        Every convolution that stays on the implicit GEMM is planned ``interior_only`` (``gemm.plan_conv2d``): no launch
        computes or writes a halo pixel.  This rests on one invariant: every map comes from ``FMap.alloc`` (``torch.zeros``),
        has exactly one producer, and no producer stores outside the interior -- the GEMM plans (interior window, no halo
        zeroing), the line-tile kernels (their epilogues skip ``gy >= H || gx >= W`` and offset by the halo), the stem /
        pack kernels and ``add_indicator`` (an interior view) all keep to it, so the halos stay the zeros they were
        allocated as, forward after forward."""
        _lib.init()
        from .embedder import default_precision
        self.precision = precision or default_precision()
        if self.precision not in ("f16", "f32"):
            raise ValueError("precision must be 'f16' or 'f32'")
        self.split = self.precision == "f32"
        self.wdtype = torch.float64 if self.split else torch.float32
        if line_tile is None:                                  # both default on; the environment switches are for A/B measurements
            line_tile = os.environ.get("ADDVISOR_UNET_LINE_TILE", "1") != "0"
        if fuse_up is None:
            fuse_up = os.environ.get("ADDVISOR_UNET_FUSE_UP", "1") != "0"
        self.dev, self.line_tile, self.fuse_up = device, line_tile, fuse_up
        self.sd = {k.replace("module.", ""): v.detach() for k, v in sd.items()}     # LMAC_metrics.py:23-25
        w, b = _fold_bn(self.sd, "e1.block.0", "e1.block.1", self.wdtype)
        self.stem_w = w.reshape(32, 15).float().contiguous().to(device)
        self.stem_b = b.float().contiguous().to(device)
        self.head_w = self.sd["mask_head.0.weight"].float().reshape(32).contiguous().to(device)
        self.head_b = float(self.sd["mask_head.0.bias"].float().reshape(-1)[0])
        # ``gemm.select_conv2d``'s arguments next to ``line_tile``: e2.block.0 takes its line tile on the fused network only
        # (tools/bench_unet_layers.py --ab changes them before the first forward to build the earlier forms)
        self.conv_choice = dict(s21_tile=fuse_up)
        self._ws: Dict[Tuple[int, int, int], dict] = {}

    @property
    def _fused_head(self) -> bool:
        """fp32-class mode with line tiles: ``d1.block.3`` carries the mask head, ``y1`` has no storage."""
        return self.split and self.line_tile

    def _workspace(self, B: int, H: int, W: int, ragged: bool = False) -> dict:
        """Maps and launches of one input shape (``ragged``: the set of its own that calls with ``widths`` use, so that a padded
        call on the same engine finds its indicator channels as it left them).  With ``fuse_up`` the stages up4+d4 .. up1+d1 are fused launches and the up-sampled
        maps u4..u1 do not exist; the coarse maps b2 / y4 / y3 then carry one extra 8-channel chunk whose first channel is the
        in-image indicator (and unused channels up to the next multiple of 64, so every pixel starts on a 128-byte line), and for
        d1 the indicator rides in the 8-channel spectrogram map ``xin`` = (x, 1, 0, ...) that ``advh_unet_pack_x`` fills."""
        key = (B, H, W, "ragged") if ragged else (B, H, W)
        if key in self._ws:
            return self._ws[key]
        if H % 16 or W % 4:
            raise ValueError("U-Net input needs H % 16 == 0 and W % 4 == 0 (SURVEY.md D2)")
        dev, sd, fused = self.dev, self.sd, self.fuse_up
        F = lambda h, w, c, ph, pw: G.FMap(B, h, w, c, ph, pw, split=self.split).alloc(dev)
        coarse_map = lambda h, w, c: G.add_indicator(F(h, w, c + 64, 1, 1), c) if fused else F(h, w, c, 0, 0)
        up_map = lambda h, w, c: None if fused else F(h, w, c, 1, 1)
        m = dict(
            x1a=F(H // 2, W, 32, 2, 1), x1=F(H // 2, W, 32, 2, 1),
            x2a=F(H // 4, W, 64, 1, 1), x2=F(H // 4, W, 64, 1, 1),
            x3a=F(H // 8, W // 2, 128, 1, 1), x3=F(H // 8, W // 2, 128, 1, 1),
            x4a=F(H // 16, W // 4, 256, 1, 1), x4=F(H // 16, W // 4, 256, 2, 2),
            b1=F(H // 16, W // 4, 512, 4, 4), b2=coarse_map(H // 16, W // 4, 512),
            u4=up_map(H // 8, W // 2, 256), y4a=F(H // 8, W // 2, 256, 1, 1), y4=coarse_map(H // 8, W // 2, 256),
            u3=up_map(H // 4, W, 128), y3a=F(H // 4, W, 128, 1, 1), y3=coarse_map(H // 4, W, 128),
            u2=up_map(H // 2, W, 64), y2a=F(H // 2, W, 64, 1, 1), y2=F(H // 2, W, 64, 1, 1),
            u1=up_map(H, W, 40), xin=G.add_indicator(F(H, W, 8, 1, 1), 1) if fused else None,
            y1a=F(H, W, 32, 1, 1), y1=G.FMap(B, H, W, 32, 1, 1, split=self.split),
        )
        m = {k: f for k, f in m.items() if f is not None}
        if not self._fused_head:
            m["y1"].alloc(dev)
        steps = []

        def conv(srcs, dst, conv_name, bn_name, **kw):
            w, b = _fold_bn(sd, conv_name, bn_name, self.wdtype)
            cin = sum(m[s].C for s in srcs)
            if cin != w.shape[1]:                              # unfused d1: 33 real channels live in a 40-wide map
                w = torch.cat([w, w.new_zeros(w.shape[0], cin - w.shape[1], *w.shape[2:])], 1)
            plan = G.select_conv2d([m[s] for s in srcs], m[dst], w, b, line_tile=self.line_tile, slope=SLOPE, device=dev,
                                   **self.conv_choice, **kw)
            steps.append((plan, srcs, dst))

        def block(srcs, mid, dst, name, **first):              # ConvBlock, addvisor.py:12-25
            conv(srcs, mid, f"{name}.block.0", f"{name}.block.1", **first)
            conv([mid], dst, f"{name}.block.3", f"{name}.block.4")

        def stage(coarse, u, skip, mid, dst, up_name, name, stride, coarse_C, skip_C, indicator):
            """One decoder stage: ConvTranspose2d ``up_name`` into ``u``, then ConvBlock ``name`` on cat(u, skip) -- or, fused, the
            transposed convolution and ``name.block.0`` as one launch on (coarse, skip)."""
            wt, bt = sd[up_name + ".weight"].to(self.wdtype), sd[up_name + ".bias"].to(self.wdtype)
            if not fused:
                steps.append((G.plan_convT2d(m[coarse], m[u], wt, bt, stride=stride, device=dev), [coarse], u))
                return block([u, skip] if skip in m else [u], mid, dst, name)    # without ``xin`` the spectrogram is packed into u1
            wc, bc = _fold_bn(sd, f"{name}.block.0", f"{name}.block.1", self.wdtype)
            plan = G.select_upconv2d(m[coarse], m[skip], m[mid], wt, bt, wc, bc, line_tile=self.line_tile, stride=stride,
                                     coarse_C=coarse_C, skip_C=skip_C, indicator=indicator, slope=SLOPE, device=dev)
            steps.append((plan, [coarse, skip], mid))
            conv([mid], dst, f"{name}.block.3", f"{name}.block.4")

        conv(["x1a"], "x1", "e1.block.3", "e1.block.4")        # e1.block.0 is the direct stem kernel
        block(["x1"], "x2a", "x2", "e2", stride=(2, 1), padding=(2, 1))
        block(["x2"], "x3a", "x3", "e3", stride=(2, 2))
        block(["x3"], "x4a", "x4", "e4", stride=(2, 2))
        conv(["x4"], "b1", "bottleneck.0", "bottleneck.1", padding=(2, 2), dilation=(2, 2))
        conv(["b1"], "b2", "bottleneck.3", "bottleneck.4", padding=(4, 4), dilation=(4, 4))
        stage("b2", "u4", "x3", "y4a", "y4", "up4", "d4", (2, 2), 512, 128, ("coarse", 512))
        stage("y4", "u3", "x2", "y3a", "y3", "up3", "d3", (2, 2), 256, 64, ("coarse", 256))
        stage("y3", "u2", "x1", "y2a", "y2", "up2", "d2", (2, 1), 128, 32, ("coarse", 128))
        stage("y2", "u1", "xin", "y1a", "y1", "up1", "d1", (2, 1), 64, 1, ("skip", 1))
        ws = dict(maps=m, steps=steps, mask=torch.empty(B, H, W, dtype=torch.float32, device=dev),
                  logits=torch.empty(B, H, W, dtype=torch.float32, device=dev))
        ws["flops"] = reference_flops(B, H, W)                # the reference formulation's count, not the fused launches'
        if self._fused_head:
            last = steps[-1][0]
            assert isinstance(last, G.Taps2dSplitPlan), "d1.block.3 is a 3x3 32-channel same-geometry layer"
            last.attach_head(self.head_w, self.head_b, ws["mask"], ws["logits"])
        self._ws[key] = ws
        return ws

    def flops(self, B: int, H: int, W: int) -> float:
        return self._workspace(B, H, W)["flops"]

    @staticmethod
    def _check_widths(widths, B: int, W: int):
        """``widths`` of a ragged call as a list of ints: one per clip, each a multiple of 4 in ``[4, W]``.  Host only."""
        import numpy as np
        if torch.is_tensor(widths):
            if widths.dim() != 1 or widths.dtype.is_floating_point or widths.dtype.is_complex or widths.dtype == torch.bool:
                raise ValueError("widths must be a sequence or a 1-D integer tensor with one entry per clip")
            widths = widths.tolist()
        elif isinstance(widths, np.ndarray):
            if widths.ndim != 1 or not np.issubdtype(widths.dtype, np.integer):
                raise ValueError("widths must be a sequence or a 1-D integer tensor with one entry per clip")
            widths = widths.tolist()
        try:
            widths = list(widths)
        except TypeError:
            raise ValueError("widths must be a sequence or a 1-D integer tensor with one entry per clip") from None
        if len(widths) != B:
            raise ValueError(f"widths has {len(widths)} entries for a batch of {B} clips")
        out = []
        for b, w in enumerate(widths):
            if isinstance(w, bool) or not isinstance(w, (int, np.integer)):
                raise ValueError(f"widths[{b}] = {w!r} is not an integer column count")
            w = int(w)
            if w < 4 or w > W or w % 4:
                raise ValueError(f"widths[{b}] = {w}: a clip's mask width is a multiple of 4 in [4, {W}]")
            out.append(w)
        return out

    def tail_maps(self, ws: dict, W: int) -> dict:
        """The feature maps a ragged forward clears past each clip's width, in launch order: ``name -> (map, shift, indicator
        channel or -1)``.  The stem's output, the packed spectrogram and every step's output that has storage (``y1`` has none when
        ``d1.block.3`` carries the head); ``shift`` = 0 / 1 / 2 for the full-, half- and quarter-width maps; the indicator is the
        in-image channel of the maps the fused up-convolutions read (``_workspace``), rewritten on every ragged call."""
        m = ws["maps"]
        shift = {W: 0, W // 2: 1, W // 4: 2}                   # W >= 4: the three widths are distinct
        ind = {"b2": 512, "y4": 256, "y3": 128, "xin": 1} if self.fuse_up else {}
        names = ["x1a", "xin" if self.fuse_up else "u1"] + [dst for _, _, dst in ws["steps"]]
        return {n: (m[n], shift[m[n].W], ind.get(n, -1)) for n in names if m[n].t is not None}

    def _clip_tail(self, f: "G.FMap", shift: int, ind: int, widths_p: int, st: int) -> None:
        lo = f.t.stride(0) if self.split else 0
        _lib.check(_lib.lib().advh_fmap_clip_tail(f.t.data_ptr(), lo, widths_p, shift, f.B, f.H, f.W, f.C, f.PH, f.PW, ind, st),
                   "advh_fmap_clip_tail")

    def forward(self, mag: torch.Tensor, H: int = 512, W: Optional[int] = None, want_logits: bool = False, widths=None):
        """``mag``: fp32 CUDA ``[B, Fq, Tq]`` (t fastest); the ``H x W`` crop is read in place.

        ``widths`` (one multiple of 4 in ``[4, W]`` per clip): a ragged batch.  Clip ``b``'s mask columns ``< widths[b]`` are what
        the network gives on its ``H x widths[b]`` crop alone; columns behind are exactly 0 in mask and logits.  The existing
        kernels and plans run over the full ``W``; after the stem, the spectrogram pack and every layer, ``advh_fmap_clip_tail``
        clears the columns past each clip's width (``widths >> 0 / 1 / 2`` on the full-, half- and quarter-width maps), so a
        clip's last columns read the zeros its own padding would give, and rewrites the in-image indicator of the fused
        up-convolutions so the transposed convolution's bias stops at the clip's edge.  ``mag`` is never written and its columns
        ``>= widths[b]`` are never read for their value: the call works on a private ``H x W`` copy whose tail is zeroed first."""
        if mag.dim() != 3 or mag.dtype != torch.float32 or not mag.is_cuda:
            raise ValueError("mag must be a CUDA fp32 tensor [B, F, T]")
        B, Fq, Tq = mag.shape
        W = (Tq // 4) * 4 if W is None else W
        if H > Fq or W > Tq:
            raise ValueError("crop exceeds the spectrogram")
        if widths is not None:
            return self._forward_ragged(mag, H, W, want_logits, self._check_widths(widths, B, W))
        mag = mag.contiguous()
        return self._forward(mag, H, W, want_logits, self._workspace(B, H, W), None)

    def _forward_ragged(self, mag: torch.Tensor, H: int, W: int, want_logits: bool, widths, wd: Optional[torch.Tensor] = None):
        """``widths``: the checked list; ``wd``: the same as int32 on the device where the caller has uploaded it already."""
        B = mag.shape[0]
        ws = self._workspace(B, H, W, ragged=True)
        if wd is None:
            wd = torch.tensor(widths, dtype=torch.int32).to(mag.device)
        st = torch.cuda.current_stream().cuda_stream
        priv = mag[:, :H, :W].contiguous()                     # a copy even when the crop is the whole tensor
        if priv.data_ptr() == mag.data_ptr():
            priv = priv.clone()
        _lib.check(_lib.lib().advh_zero_tail_cols_f32(priv.data_ptr(), wd.data_ptr(), B, H, W, st), "advh_zero_tail_cols_f32")
        return self._forward(priv, H, W, want_logits, ws, wd)

    def _forward(self, mag: torch.Tensor, H: int, W: int, want_logits: bool, ws: dict, wd: Optional[torch.Tensor]):
        """The launches of one forward; ``wd``: the int32 device widths of a ragged call (``mag`` is then its private copy)."""
        B, Fq, Tq = mag.shape
        m, lib = ws["maps"], _lib.lib()
        st = torch.cuda.current_stream().cuda_stream
        x1a = m["x1a"]
        xcat, xc0 = (m["xin"], 0) if self.fuse_up else (m["u1"], 32)
        tails = self.tail_maps(ws, W) if wd is not None else {}
        if self.split:
            _lib.check(lib.advh_unet_stem_split(mag.data_ptr(), Fq, Tq, B, H, W, self.stem_w.data_ptr(), self.stem_b.data_ptr(),
                                                x1a.t.data_ptr(), x1a.t.stride(0), x1a.PH, x1a.PW, SLOPE, st), "advh_unet_stem_split")
            _lib.check(lib.advh_unet_pack_x_split(mag.data_ptr(), Fq, Tq, B, H, W, xcat.t.data_ptr(), xcat.t.stride(0), xcat.C, xc0,
                                                  xcat.PH, xcat.PW, st), "advh_unet_pack_x_split")
        else:
            _lib.check(lib.advh_unet_stem(mag.data_ptr(), Fq, Tq, B, H, W, self.stem_w.data_ptr(), self.stem_b.data_ptr(),
                                          x1a.t.data_ptr(), x1a.PH, x1a.PW, SLOPE, st), "advh_unet_stem")
            _lib.check(lib.advh_unet_pack_x(mag.data_ptr(), Fq, Tq, B, H, W, xcat.t.data_ptr(), xcat.C, xc0, xcat.PH, xcat.PW, st),
                       "advh_unet_pack_x")
        if wd is not None:
            self._clip_tail(*tails["x1a"], wd.data_ptr(), st)
            self._clip_tail(*tails["xin" if self.fuse_up else "u1"], wd.data_ptr(), st)
        for plan, srcs, dst in ws["steps"]:
            a0 = m[srcs[0]].t
            a1 = m[srcs[1]].t if len(srcs) > 1 else None
            plan.run(a0, a1, out_h=m[dst].t)
            if dst in tails:
                self._clip_tail(*tails[dst], wd.data_ptr(), st)
        y1 = m["y1"]
        if self._fused_head:
            pass                                               # mask and logits came out of d1.block.3's epilogue
        elif self.split:
            _lib.check(lib.advh_unet_head_split(y1.t.data_ptr(), y1.t.stride(0), B, H, W, y1.PH, y1.PW, self.head_w.data_ptr(),
                                                self.head_b, ws["mask"].data_ptr(), ws["logits"].data_ptr(), st), "advh_unet_head_split")
        else:
            _lib.check(lib.advh_unet_head(y1.t.data_ptr(), B, H, W, y1.PH, y1.PW, self.head_w.data_ptr(), self.head_b,
                                          ws["mask"].data_ptr(), ws["logits"].data_ptr(), st), "advh_unet_head")
        if wd is not None:
            for plane in (ws["mask"], ws["logits"]):
                _lib.check(lib.advh_zero_tail_cols_f32(plane.data_ptr(), wd.data_ptr(), B, H, W, st), "advh_zero_tail_cols_f32")
        mask = ws["mask"].clone()
        return (mask, ws["logits"].clone()) if want_logits else mask
