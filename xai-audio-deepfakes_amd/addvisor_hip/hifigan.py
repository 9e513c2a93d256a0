"""HiFi-GAN V1 generator on the HIP kernels (reference handle: hifigan.py:106-110, 180).

``decode_batch(mel [B, 80, T]) -> wav [B, 1, T*256]``.  Every Conv1d / ConvTranspose1d is an
implicit-GEMM launch on zero-haloed channels-last fp16 maps (``gemm.plan_conv1d_same`` /
``plan_convT1d``); LeakyReLU is applied by the producer (each GEMM writes the raw map for the residual
path and, through ``out_h2``, the pre-activated copy the next conv reads), the MRF average and the
1-channel conv_post + tanh are small direct kernels.  Weight-norm is assumed folded (inference form).

Fidelity options.  The reference reaches the generator through SpeechBrain's wrapper, whose source is not available
offline; two of its choices change the numbers and are therefore options here, mirrored by ``oracle/hifigan_ref.py``:
``padding_mode`` of the "same" Conv1d layers ("zeros" = the published Kong et al. model, the default; "reflect" = the
default of SpeechBrain's ``Conv1d``) and ``inference_padding`` (mel frames replicated on both sides before the
generator, output length ``(T + 2 p) * 256``; 0 = off, the default; SpeechBrain / Coqui generators ship with 5).
"reflect" fills the map halos with the mirrored interior after every producing launch (``advh_halo_fill_f16``); the
fused line-tile kernels keep their intermediate in LDS with zero padding, so that mode runs the implicit GEMM only.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, Optional, Tuple

import torch

from . import _lib, gemm as G
from .embedder import default_precision
from .synthetic import HifiganConfig

HALO = 32          # >= the largest "same" padding: (11 - 1) * 5 / 2 = 25


# One entry of the decode loop.  ``plan`` / ``src`` by ``kind``: "gemm" the plan and its input map, "halo" the fill mode (1 = the mirrored
# interior, 0 = zeros) and the map, "mix" the LeakyReLU slope and the maps averaged into ``dst``.
Step = namedtuple("Step", "kind plan src resid dst dst2", defaults=(None, None, None))


def _launch(plan, src, dst, resid=None, dst2=None):
    return Step("gemm", plan, src, resid, dst, dst2)


def _halo(m, mode=1):
    return Step("halo", mode, m)


def _mix(slope, outs, dst):
    return Step("mix", slope, outs, dst=dst)


class HipHifigan:
    def __init__(self, cfg: HifiganConfig, sd: Dict[str, torch.Tensor], device, line_tile: bool = True, fuse: bool = True,
                 padding_mode: str = "zeros", inference_padding: int = 0, precision: Optional[str] = None):
        """``precision``: None = ``ADDVISOR_PRECISION`` (default "f32": the fp32-class mode of the explanation path -- split-format
        maps, three MFMAs per product; the reference runs the vocoder in fp32, hifigan.py:180) or "f16" (fp16 operands; stated
        tolerance 2e-2 on waveforms).  ``padding_mode`` / ``inference_padding``: see the module docstring.
        "f16": ``line_tile`` runs the 32- / 64-channel ResBlock convolutions on the weights-in-LDS kernel (``advh_conv_taps_f16``) instead
        of the implicit GEMM; ``fuse`` (needs ``line_tile``) whole ResBlock steps where both weights fit in LDS (``advh_resblock_pair_f16``).
        "f32": ``line_tile`` is ignored; ``fuse`` gates both the fused step of the 32-channel stage (``advh_resblock_pair_x3``) and the
        64-channel line tile with streamed weights (``advh_conv_taps_split``); the other layers run the x3 implicit GEMM.
        "reflect" forces the implicit GEMM everywhere: the tile kernels zero-pad their LDS intermediate."""
        _lib.init()
        precision = precision or default_precision()
        self._ctor = dict(line_tile=line_tile, fuse=fuse, padding_mode=padding_mode, inference_padding=inference_padding)
        if precision not in ("f16", "f32"):
            raise ValueError("precision must be 'f16' or 'f32'")
        self.precision, self.split = precision, precision == "f32"
        if padding_mode not in ("zeros", "reflect"):
            raise ValueError("padding_mode must be 'zeros' or 'reflect'")
        if inference_padding < 0:
            raise ValueError("inference_padding must be >= 0")
        self.padding_mode, self.inference_padding = padding_mode, int(inference_padding)
        tiles = padding_mode == "zeros"
        self.lds_tile = tiles and not self.split and line_tile          # fp16 weights-in-LDS convolutions
        self.lds_fuse = self.lds_tile and fuse                           # fp16 fused ResBlock steps
        self.split_tile = tiles and self.split and fuse                  # split fused 32-channel steps + 64-channel line tile
        self.cfg, self.dev = cfg, device
        self.sd = {k: v.detach().float() for k, v in sd.items()}
        ch = cfg.upsample_initial_channel
        for _ in cfg.upsample_rates:
            ch //= 2
        if ch % 8:
            raise ValueError("every HiFi-GAN stage needs a channel count that is a multiple of 8")
        if cfg.in_channels % 8:
            raise ValueError("mel channels must be a multiple of 8")
        self.post_w = self.sd["conv_post.weight"][0].t().contiguous().to(device)       # [k][C]
        self.post_b = float(self.sd["conv_post.bias"][0])
        self._ws: Dict[Tuple[int, int], dict] = {}

    def with_precision(self, precision: str) -> "HipHifigan":
        """This generator at ``precision`` (itself if it already is): ``ExplainPipeline`` runs its vocoder at the path's
        precision, so that the explanation has ONE arithmetic class."""
        if precision == self.precision:
            return self
        return type(self)(self.cfg, self.sd, self.dev, precision=precision, **self._ctor)

    def _stage_policy(self, co: int) -> Tuple[bool, bool]:
        """``(in_lds, fused)`` of the stage with ``co`` channels.  ``in_lds``: its ResBlock kernels apply LeakyReLU to the raw map inside
        their line buffer, so the stage keeps no pre-activated copies (no ``lx`` / ``la`` / ``lb`` maps): an fp16 stage whose every kernel
        size fits the line tile, a split stage whose EVERY step has the fused kernel.  ``fused``: it uses ``select_resblock_step``."""
        ks, ds = self.cfg.resblock_kernel_sizes, self.cfg.resblock_dilations
        if self.split:
            fused = (self.split_tile and all(G.resblock_pair_x3_lds_bytes(co, k, d) > 0 for k in ks for d in ds)
                     and HALO >= (max(ks) - 1) * max(ds) // 2)
            return fused, fused
        in_lds = self.lds_tile and co in (32, 64) and all(G.taps_tile(co, k, (k - 1) * max(ds)) > 0 for k in ks)
        return in_lds, in_lds and self.lds_fuse

    def _resblock_step(self, steps, p: str, d: int, policy, cx, clx, tmp, ox, ol):
        """Append step ``d`` of ResBlock ``p``, ``ox = cx + conv2(lrelu(conv1(lrelu(cx))))``: one fused launch where the stage fuses and the kernel
        takes the step, else conv1 (``clx`` = lrelu(cx), or ``cx`` if ``in_lds``) -> ``tmp`` and conv2 -> ``ox`` (+ lrelu(ox) -> ``ol``) with their halo fills."""
        (in_lds, fused), sd = policy, self.sd
        dil, slope = self.cfg.resblock_dilations[d], self.cfg.leaky_slope
        w1, b1, w2, b2 = (sd[f"{p}convs{c}.{d}.{n}"] for c in (1, 2) for n in ("weight", "bias"))
        plan = G.select_resblock_step(cx, ox, w1, b1, w2, b2, dilation=dil, slope=slope, fused=fused, device=self.dev)
        if plan is not None:
            steps.append(_launch(plan, cx, ox))
            return
        pick = dict(line_tile=self.lds_tile, split_tile=self.split_tile, device=self.dev)
        reflect, c1_src = self.padding_mode == "reflect", cx if in_lds else clx
        steps.append(_launch(G.select_conv1d(c1_src, tmp, w1, b1, role="conv1", dilation=dil, act="leaky", slope=slope,
                                             pre_slope=slope if in_lds else None, **pick), c1_src, tmp))
        if reflect:
            steps.append(_halo(tmp))
        steps.append(_launch(G.select_conv1d(tmp, ox, w2, b2, role="conv2", slope2=slope, **pick), tmp, ox, resid=cx, dst2=ol))
        if reflect and ol is not None:             # the next conv1 reads lrelu(x) reflect-padded (the raw ox only feeds residuals)
            steps.append(_halo(ol))

    def _workspace(self, B: int, T: int) -> dict:
        if (B, T) in self._ws:
            return self._ws[B, T]
        cfg, sd, dev = self.cfg, self.sd, self.dev
        M = lambda t, c: G.Map1D(B, t, c, HALO, split=self.split).alloc(dev)
        ch, reflect = cfg.upsample_initial_channel, self.padding_mode == "reflect"
        mel, cur = M(T, cfg.in_channels), M(T, ch)           # cur: lrelu(conv_pre(mel))
        steps = [_halo(mel)] if reflect else []
        steps.append(_launch(G.plan_conv1d_same(mel, cur, sd["conv_pre.weight"], sd["conv_pre.bias"], act="leaky",
                                                slope=cfg.leaky_slope, device=dev), mel, cur))
        t, nk, nd, nstage = T, len(cfg.resblock_kernel_sizes), len(cfg.resblock_dilations), len(cfg.upsample_rates)
        for i, r in enumerate(cfg.upsample_rates):
            co, t2 = ch // 2, t * r
            policy = in_lds, _ = self._stage_policy(co)
            x, lx = M(t2, co), None if in_lds else M(t2, co)
            steps.append(_launch(G.plan_convT1d(cur, x, sd[f"ups.{i}.weight"], sd[f"ups.{i}.bias"], stride=r,
                                                slope2=cfg.leaky_slope, device=dev), cur, x, dst2=lx))
            if reflect:                                    # the ResBlock convolutions read x / lrelu(x) reflect-padded
                steps += [_halo(x), _halo(lx)]
            tmp, pa, pb = M(t2, co), M(t2, co), M(t2, co)
            la, lb = (None, None) if in_lds else (M(t2, co), M(t2, co))
            outs = [M(t2, co) for _ in range(nk)]
            for j in range(nk):
                cx, clx = x, lx
                for d in range(nd):
                    last = d == nd - 1
                    ox = outs[j] if last else (pa if d % 2 == 0 else pb)
                    ol = None if (last or in_lds) else (la if d % 2 == 0 else lb)
                    self._resblock_step(steps, f"resblocks.{i * nk + j}.", d, policy, cx, clx, tmp, ox, ol)
                    cx, clx = ox, ol
            nxt = M(t2, co)
            steps.append(_mix(cfg.leaky_slope if i < nstage - 1 else 0.01, outs, nxt))       # F.leaky_relu's default before conv_post
            if reflect:
                # the mix runs over whole padded maps; the transposed convolution that follows needs a ZERO halo (it is not a
                # "same" conv), conv_post a reflected one
                steps.append(_halo(nxt, 1 if i == nstage - 1 else 0))
            cur, ch, t = nxt, co, t2
        self._ws[B, T] = ws = dict(mel=mel, steps=steps, last=cur, T_out=t, wav=torch.empty(B, 1, t, dtype=torch.float32, device=dev))
        ws["flops"] = sum(s.plan.flops for s in steps if s.kind == "gemm") + 2.0 * B * t * ch * cfg.post_kernel
        return ws

    def flops(self, B: int, T: int) -> float:
        return self._workspace(B, T)["flops"]

    def decode_batch(self, mel: torch.Tensor) -> torch.Tensor:
        """``mel [B, n_mels, T]`` (fp32, on the GPU) -> ``wav [B, 1, T * hop]`` fp32."""
        if mel.dim() == 2:
            mel = mel[None]
        if mel.dim() != 3 or mel.shape[1] != self.cfg.in_channels:
            raise ValueError(f"mel must be [B, {self.cfg.in_channels}, T]")
        mel = mel.to(self.dev, torch.float32).contiguous()
        B, C, T0 = mel.shape
        pad = self.inference_padding
        T = T0 + 2 * pad
        ws = self._workspace(B, T)
        lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        sp = self.split
        if sp:
            _lib.check(lib.advh_hifigan_pack_mel_split(mel.data_ptr(), ws["mel"].t.data_ptr(), ws["mel"].t.stride(0), B, C, T0, pad, HALO, st),
                       "advh_hifigan_pack_mel_split")
        elif pad:
            _lib.check(lib.advh_hifigan_pack_mel_pad(mel.data_ptr(), ws["mel"].t.data_ptr(), B, C, T0, pad, HALO, st), "advh_hifigan_pack_mel_pad")
        else:
            _lib.check(lib.advh_hifigan_pack_mel(mel.data_ptr(), ws["mel"].t.data_ptr(), B, C, T, HALO, st), "advh_hifigan_pack_mel")
        for kind, plan, src, resid, dst, dst2 in ws["steps"]:
            if kind == "gemm":
                plan.run(src.t, out_h=dst.t, resid=None if resid is None else resid.t, out_h2=None if dst2 is None else dst2.t)
            elif kind == "halo":                       # split maps: both planes are [B][P][C] images of the same geometry
                _lib.check(lib.advh_halo_fill_f16(src.t.data_ptr(), src.B * (2 if sp else 1), src.T, src.C, src.halo, plan, st), "advh_halo_fill_f16")
            elif sp:
                _lib.check(lib.advh_hifigan_mrf_mix_split(*(m.t.data_ptr() for m in src), dst.t.data_ptr(), plan, dst.t.stride(0), dst.t.stride(0), st),
                           "advh_hifigan_mrf_mix_split")
            else:
                _lib.check(lib.advh_hifigan_mrf_mix(*(m.t.data_ptr() for m in src), dst.t.data_ptr(), plan, dst.t.numel(), st), "advh_hifigan_mrf_mix")
        last = ws["last"]
        if sp:
            _lib.check(lib.advh_hifigan_conv_post_split(last.t.data_ptr(), last.t.stride(0), self.post_w.data_ptr(), self.post_b,
                                                        ws["wav"].data_ptr(), B, last.C, last.T, HALO, self.cfg.post_kernel, st),
                       "advh_hifigan_conv_post_split")
        else:
            _lib.check(lib.advh_hifigan_conv_post(last.t.data_ptr(), self.post_w.data_ptr(), self.post_b, ws["wav"].data_ptr(), B,
                                                  last.C, last.T, HALO, self.cfg.post_kernel, st), "advh_hifigan_conv_post")
        return ws["wav"].clone()
