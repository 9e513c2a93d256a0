"""Input gradient of the frozen classifier  F(x) = logreg(mean_t(hidden_states[k](wav2vec2(norm(x)))))
on the HIP kernels: the quantity Captum's Saliency / InputXGradient / IntegratedGradients differentiate
(captum_saliency.py:84-100, 116-135).

The weights are frozen, so the backward pass is dgrad-only: every dense product is the forward's implicit GEMM
with the transposed weight (``gemm.plan_linear(W.T)``, ``plan_conv1d_dgrad``), with the activation derivative
(``dact_src``) fused in its epilogue; LayerNorm, attention and the waveform front end have dedicated backward
kernels (csrc/backward.hip, frontend_bwd.hip).  The forward of this class is the same arithmetic as
``HipEmbedder.forward`` but writes every tensor the backward needs (pre-activations, LayerNorm inputs, QKV)
to its own buffer instead of updating in place.

Precision follows the embedder (``precision=None``): with an fp32-class embedder ("f32", the reference's arithmetic class --
captum_saliency.py:116-135 and loss_function.py:46-53 differentiate with fp32 autograd) every saved activation and every
gradient between GEMMs is a split-format plane pair (hi + lo * 2^-11, ~22 bits; csrc/device_math.h), the dgrad GEMMs run
three fp16 MFMAs per product on transposed split weights, LayerNorm / front-end backward read and write plane pairs and the
attention backward runs on the fp32-input matrix instruction (csrc/attention_bwd_f32.hip).  ``precision="f16"`` keeps the
fp16-operand chain (fp16 gradients between GEMMs).  In both modes the gradients are multiplied by ``loss_scale`` (a power of
two: exact, the chain is linear in the gradient) so that small values stay in the fp16 exponent range of the planes, and
the residual-stream gradient is fp32.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, gemm as G
from .embedder import FE_SLACK_ROWS, HipEmbedder, plan_posconv


def plan_conv1d_dgrad(B: int, P_out: int, weight: torch.Tensor, stride: int, device=None, cache=None, split: bool = False) -> G.GemmPlan:
    """Input gradient of the channels-last Conv1d of ``gemm.plan_conv1d_cl`` (no padding): position
    ``u = s*q + phase`` of the input receives ``sum_{i} dZ[q - (nt-1) + i] . W[:, :, phase + s*(nt-1-i)]``
    (nt = ceil(k/s) taps), so the layer is a GEMM over rows q with K = nt*Cout (nt adjacent dZ rows = one
    contiguous slab) and N = s*Cin, whose row q of the output is input rows s*q .. s*q+s-1.
    ``A0`` must point ``nt-1`` rows BEFORE dZ[0] (a zero guard row), and every clip needs >= 1 zero filler row."""
    Cout, Cin, k = weight.shape
    s = stride
    nt = -(-k // s)
    assert Cout % 8 == 0 and Cin % 4 == 0
    def w2():
        m = torch.zeros(s * Cin, nt * Cout)
        for phase in range(s):
            for i in range(nt):
                j = phase + s * (nt - 1 - i)
                if j < k:
                    m[phase * Cin:(phase + 1) * Cin, i * Cout:(i + 1) * Cout] = weight[:, :, j].t()
        return m[None]
    cc = Cout // 8
    return G.GemmPlan(M=B * P_out, N=s * Cin, w2=w2, ktab=np.arange(nt * cc, dtype=np.int64),
                      sources=[G.Source(P_out * cc, 0, cc, 0)], Hg=1, Wg=P_out, window=(0, 1, 0, P_out), halo_zero=False,
                      out=(P_out * s * Cin, 0, s * Cin, 0), device=device, cache=cache, split=split), nt


def check_layer(layer, nl: int) -> int:
    """A layer of the ``captum.attr.Layer*`` methods: an integer index into ``hidden_states``, ``0 <= layer <= nl``
    (``nl = HipEmbedder.nl``; the layers above it do not reach the logit).  Raises ValueError."""
    if isinstance(layer, bool) or not isinstance(layer, (int, np.integer)) or not 0 <= layer <= nl:
        raise ValueError(f"layer must be an integer index into hidden_states, 0 <= layer <= {nl}; got {layer!r} "
                         "(layers above layer_index do not reach the logit)")
    return int(layer)


def check_box(box, T: int, H: int) -> Tuple[int, int, int, int, int, int]:
    """A selection box ``(t0, t1, tstep, h0, h1, hstep)`` over the ``[T, H]`` frame of a layer (the normalised neuron selector
    of the ``captum.attr.Neuron*`` methods, ``attribution.check_neuron_selector``): six ints, half-open ranges inside the frame,
    non-empty, steps > 0.  Raises ValueError."""
    ok = isinstance(box, (tuple, list)) and len(box) == 6 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in box)
    if ok:
        t0, t1, ts, h0, h1, hs = (int(v) for v in box)
        ok = 0 <= t0 < t1 <= T and ts > 0 and 0 <= h0 < h1 <= H and hs > 0
    if not ok:
        raise ValueError(f"a selection box is (t0, t1, tstep, h0, h1, hstep) inside [0, {T}) x [0, {H}), non-empty, steps > 0; got {box!r}")
    return t0, t1, ts, h0, h1, hs


GELU_RULES = ("gradient", "identity")
F16_WIDE_HEAD_MAX_T = 208       # advh_attention_bwd_f16: frames it holds for head dims above 64 (include/addvisor_hip.h)


@dataclass(frozen=True)
class LrpRules:
    """The conservative-propagation rules of ``EmbedderGrad.backward(rules=...)`` (Ali et al. 2022; csrc/lrp.hip): ``ln`` -- a
    LayerNorm's ``1/sigma`` is a constant of the backward pass; ``attention`` -- the attention probabilities are; ``gelu`` --
    ``"gradient"`` leaves the FFN's GELU backward as it is, ``"identity"`` (AttnLRP) makes ``Phi(x) = GELU(x)/x`` a constant."""
    ln: bool = True
    attention: bool = True
    gelu: str = "gradient"

    def __post_init__(self):
        if not isinstance(self.ln, bool) or not isinstance(self.attention, bool):
            raise ValueError(f"the ln and attention rules are bools; got {self.ln!r}, {self.attention!r}")
        if not isinstance(self.gelu, str) or self.gelu not in GELU_RULES:
            raise ValueError(f"the gelu rule must be one of {GELU_RULES}, not {self.gelu!r}")


def check_chain_frames(emb: HipEmbedder, L: int, long_clips: bool = False) -> None:
    """The default gradient chain keeps the whole-clip attention kernels, forward and backward: ``AdvhError`` for a batch of ``L``
    samples with more frames than they hold, unless the chain was built with ``long_clips=True`` (the streamed kernels of
    csrc/attention_long.hip and csrc/attention_bwd_long.hip above that length).  Host only."""
    T = emb._lengths(int(L))[-1]
    if T > emb.WHOLE_CLIP_MAX_FRAMES and not long_clips:
        raise _lib.AdvhError(f"EmbedderGrad.forward: ADVH_EUNSUPPORTED: the gradient chain is held for T <= {emb.WHOLE_CLIP_MAX_FRAMES} frames "
                             f"({emb.whole_clip_max_samples()} samples) and this clip has T = {T} ({int(L)} samples); the forward-only "
                             "methods (HipEmbedder.forward, classify, explain, the perturbation attributions) take longer clips, and so "
                             "does a chain built with long_clips=True (EmbedderGrad, HipAttribution; ADDVISOR_LONG_CLIPS=1 for the "
                             "runtime singleton)")


class EmbedderGrad:
    long_clips = False          # the default chain refuses clips above 256 frames (check_chain_frames)
    long_maps = False           # and attention_maps= / attention_probs / rules= above 256 frames or after a ragged pass

    def __init__(self, emb: HipEmbedder, precision: Optional[str] = None, long_clips: bool = False, long_maps: bool = False):
        """``precision``: None = the embedder's own ("f32": split-format chain; "f16": fp16 chain), or "f16" to run the fp16
        chain next to an fp32-class embedder (``HipEmbedder.f16_twin``).
        ``long_clips=True``: clips above 256 frames (82 319 samples) are taken -- there the attention runs on the streamed kernels,
        forward (advh_attention_long_*) and backward (advh_attention_bwd_long_*, both precisions on the fp32-input matrix
        instruction); ``seed``, ``to_layer``, ``from_layer``, ``forward_from`` and ``lengths=`` work as below that length, while
        ``attention_maps=``, ``attention_probs`` and ``rules=`` keep the 256-frame limit of their ``T x T`` kernels unless
        ``long_maps`` is set.  At 256 frames and below every launch is the default chain's.
        ``long_maps=True`` (needs ``long_clips=True``): above 256 frames, and after a ragged pass (``forward(lengths=...)``) at
        any length, ``attention_probs``, ``attention_maps=`` and ``rules=`` run the streamed kernels of
        csrc/attention_maps_long.hip (advh_attention_maps_long, advh_attention_bwd_value_long); a clip of a ragged pass gets its
        own map in the top-left ``T_b x T_b`` block and exact zeros elsewhere.  At 256 frames and below after a non-ragged pass
        every launch is still the whole-clip one."""
        if precision not in (None, "f16", "f32"):
            raise ValueError("precision must be None, 'f16' or 'f32'")
        if not isinstance(long_clips, bool):
            raise ValueError(f"long_clips must be a bool, not {long_clips!r}")
        if not isinstance(long_maps, bool):
            raise ValueError(f"long_maps must be a bool, not {long_maps!r}")
        if long_maps and not long_clips:
            raise ValueError("long_maps=True needs long_clips=True: the maps of a long clip come from the long gradient chain's saves")
        self.long_clips = long_clips
        self.long_maps = long_maps
        if precision == "f16":
            emb = emb.f16_twin()
        elif precision == "f32" and not emb.split:
            raise ValueError("an fp32-class gradient chain needs an fp32-class embedder (HipEmbedder(precision='f32'))")
        self.emb = emb
        self.split = emb.split
        self.precision = emb.precision
        self.cfg, self.dev, self.sd = emb.cfg, emb.dev, emb.sd
        self.layer_mode = emb.layer_mode                       # "layer" feature extractor (wav2vec2-large / xls-r)
        self.stable = self.cfg.do_stable_layer_norm            # pre-LN encoder
        self._ws: Dict[Tuple[int, int], dict] = {}
        self._wcache: dict = {}
        self._stop: Optional[int] = None                       # forward(to_layer=l): the layer the last pass stopped at
        self._rag: Optional[torch.Tensor] = None               # forward(lengths=...): int32 [2, B] on the device, samples | frames

    # ------------------------------------------------------------------ buffers and plans
    def _workspace(self, B: int, L: int) -> dict:
        key = (B, L)
        if key in self._ws:
            return self._ws[key]
        emb, cfg, dev, sd, sp = self.emb, self.cfg, self.dev, self.sd, self.split
        f = emb._workspace(B, L)                      # forward plans / shapes are shared
        Ls, P, T, M = f["Ls"], f["P"], f["T"], f["M"]
        for i in range(len(Ls)):
            if P[i] <= Ls[i]:
                raise ValueError("backward needs one zero filler row per clip (P > L)")
        H, I, C = cfg.hidden_size, cfg.intermediate_size, cfg.conv_dim
        nfe, nl = len(Ls), emb.nl
        h16, f32 = torch.float16, torch.float32
        pl = (2,) if sp else ()                       # fp32-class chain: every fp16 tensor is a [2, ...] plane pair
        z = lambda *s, dt=h16: torch.zeros(*((pl + tuple(s)) if dt == h16 else s), dtype=dt, device=dev)
        w = dict(f=f)
        # Feature-encoder level i (i < nfe - 1): y_i (post-GELU), z_i (pre-activation) and dZ_i all live in buffers of ONE
        # shape -- a zero guard row, the [B][P_i][C_i] rows, then the readable slack rows the affine-row loader of the next
        # layer's plan may touch (gemm.plan_conv1d_cl(slack_rows=...)) -- so that in the fp32-class mode the fp16-side operands
        # of one GEMM epilogue (out_h, out_pre, dact_src) share one plane pitch (advh_gemm_desc.o_lo).
        lvl = lambda i: z((1 + B * P[i] + FE_SLACK_ROWS) * C[i])
        self._body = lambda t, i: t[..., C[i]:]                                   # rows from the first data row on (guard skipped)
        # forward saves ------------------------------------------------------------------
        w["y"] = [lvl(i) for i in range(nfe - 1)]                                  # post-GELU outputs of layers 0..nfe-2
        w["z"] = [lvl(0) if self.layer_mode else None]                             # pre-norm / pre-GELU outputs of the convs
        w["z"] += [lvl(i) for i in range(1, nfe - 1)] + [z(M, C[-1])]
        w["dyb"] = lvl(0) if self.layer_mode else None
        w["dfeat"] = z(M, C[-1]) if self.layer_mode else None
        w["t16"] = z(M, H)
        w["xf"] = z(M, H, dt=f32)
        w["feat"] = z(M, C[-1])
        w["pc"] = z(M, H)                                                        # pre-GELU positional conv
        w["h1"] = z(M, H, dt=f32)                                                # input of encoder.layer_norm
        w["x"] = [z(M, H, dt=f32) for _ in range(nl + 1)]                        # layer inputs / final output
        w["qkv"] = [z(M, 3 * H) for _ in range(nl)]
        w["s1"] = [z(M, H, dt=f32) for _ in range(nl)]
        w["m"] = [z(M, H, dt=f32) for _ in range(nl)]
        w["g1"] = [z(M, I) for _ in range(nl)]
        w["s2"] = [z(M, H, dt=f32) for _ in range(nl)]
        # backward scratch ---------------------------------------------------------------
        w["dlogit"] = z(B, dt=f32)
        w["da"] = z(M, H, dt=f32)
        w["db"] = z(M, H, dt=f32)
        w["d16"] = z(M, H)
        w["dI"] = z(M, I)
        w["dctx"] = z(M, H)
        w["dqkv"] = z(M, 3 * H)
        w["dfeatn"] = z(M, C[-1])
        # dZ_i: per-clip padded layout [B][P_i][C_i] with one zero guard row in front
        w["dz"] = [lvl(i) for i in range(nfe - 1)] + [z((B * P[-1] + 1) * C[-1])]
        w["g"] = z(B * P[0], 16, dt=f32)
        ntile = -(-P[0] // 64)
        w["part"] = z(B, ntile, C[0], 2, dt=f32)
        w["sums"] = z(B, C[0], 2, dt=f32)
        w["dxh"] = z(B, L, dt=f32)
        w["wpart"] = z(B, -(-L // 2048), 2, dt=f32)
        if T > emb.WHOLE_CLIP_MAX_FRAMES:             # long_clips: the streamed attention backward's (m, 1/l, delta), shared by the layers
            nb = _lib.lib().advh_attention_bwd_long_ws_bytes(B, T, cfg.num_attention_heads)
            w["att_stats"] = torch.empty(nb // 4, dtype=f32, device=dev)
        # backward plans -----------------------------------------------------------------
        wc = self._wcache
        lin = lambda wt, key: G.plan_linear(M, wt, None, device=dev, cache=(wc, key), split=sp)
        layers = []
        for l in range(nl):
            p = f"encoder.layers.{l}."
            if ("qkv", l) in wc:
                wqkv = torch.empty(3 * H, H, device="meta")
            else:
                wqkv = torch.cat([sd[p + f"attention.{n}_proj.weight"] for n in ("q", "k", "v")], 0)
            layers.append(dict(ff2=lin(sd[p + "feed_forward.output_dense.weight"].t(), ("ff2", l)),
                               ff1=lin(sd[p + "feed_forward.intermediate_dense.weight"].t(), ("ff1", l)),
                               out=lin(sd[p + "attention.out_proj.weight"].t(), ("out", l)), qkv=lin(wqkv.t(), ("qkv", l))))
        w["layers"] = layers
        w["proj"] = lin(sd["feature_projection.projection.weight"].t(), "proj")
        K, Gp = cfg.num_conv_pos_embeddings, cfg.num_conv_pos_embedding_groups
        g0 = sd["encoder.pos_conv_embed.conv.parametrizations.weight.original0"]
        v0 = sd["encoder.pos_conv_embed.conv.parametrizations.weight.original1"]
        wconv = lambda: g0 * v0 / v0.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()
        w["pos"] = plan_posconv(B, T, H, Gp, K, wconv, flip=True, device=dev, cache=(wc, "pos"), split=sp)   # [g][ci][(k', co)], taps flipped
        fe = []
        for i in range(1, nfe):
            plan, nt = plan_conv1d_dgrad(B, P[i], sd[f"feature_extractor.conv_layers.{i}.conv.weight"], cfg.conv_stride[i], dev,
                                         cache=(wc, ("fe", i)), split=sp)
            fe.append((plan, nt))
        w["fe"] = fe
        w0t = torch.zeros(16, C[0])
        w0t[:10] = sd["feature_extractor.conv_layers.0.conv.weight"].reshape(C[0], 10).t()
        w["g_plan"] = G.plan_linear(B * P[0], w0t, None, device=dev, cache=(wc, "w0t"), split=sp)
        self._ws[key] = w
        return w

    # ------------------------------------------------------------------ forward with saves
    def forward(self, wave: torch.Tensor, length: Optional[int] = None, to_layer: Optional[int] = None, lengths=None):
        """The classifier with the backward's saves: ``(logits [B,1], probs [B,1])``.  ``to_layer=l`` (the neuron methods,
        ``captum.attr.Neuron*``): the pass stops at ``hidden_states[l]`` -- the front end and layers ``0 .. l-1`` run with their
        saves, and for ``l == nl`` of a full-depth pre-LN model the final LayerNorm, whose output ``hidden_states[nl]`` is; no
        layer ``>= l``, no pooling and no logreg is launched -- and returns it, ``[B, T, H]`` fp32.  After such a pass only
        ``hidden(l' <= l)`` and ``backward(from_layer <= l, ...)`` are defined.
        ``lengths`` (a sequence or 1-D integer tensor of ``B`` sample counts; ``HipEmbedder.forward``): a ragged batch.  Clip
        ``b`` is ``wave[b, :lengths[b]]``, what lies behind is padding of any content, and everything this pass and the
        ``backward`` after it return for the clip is what they return for that clip run alone, unpadded: logits pooled over its
        own ``T_b = frame_lengths(lengths)[b]`` frames, ``to_layer`` hidden states with rows ``t >= T_b`` zero, ``dx[b, lengths[b]:]``
        and layer gradients on rows ``t >= T_b`` exactly 0.  Workspace and plans are those of the padded ``(B, L)`` call.
        After a ragged pass ``forward_from`` raises, and ``attention_probs``, ``backward(attention_maps=...)`` and
        ``backward(rules=...)`` raise unless the chain has ``long_maps=True``."""
        lens = None
        if lengths is not None:                            # host checks, before any allocation, plan or launch
            if length is not None:
                raise ValueError("give length= (one length for the batch) or lengths= (one per clip), not both")
            if wave.dim() != 2:
                raise ValueError("wave must be a tensor [B, n]")
            lens = self.emb._check_lengths(lengths, wave.shape[0], wave.shape[1])
        stop = None if to_layer is None else check_layer(to_layer, self.emb.nl)
        check_chain_frames(self.emb, wave.shape[-1] if length is None else int(length), self.long_clips)     # before any allocation, plan or launch
        emb, cfg, lib, sp = self.emb, self.cfg, _lib.lib(), self.split
        wave = wave.contiguous()
        B, n_in = wave.shape
        L = n_in if length is None else int(length)
        w = self._workspace(B, L)
        rag = None
        if lens is not None:                               # sample and frame counts in one small copy: rag[0] = lens, rag[1] = frames
            rag = torch.tensor([lens, emb.frame_lengths(lens)], dtype=torch.int32).to(self.dev, non_blocking=False)
        f = w["f"]
        st = torch.cuda.current_stream().cuda_stream
        Ls, P, T, M, H = f["Ls"], f["P"], f["T"], f["M"], cfg.hidden_size
        eps, C, nfe, nl = cfg.layer_norm_eps, cfg.conv_dim, len(f["Ls"]), emb.nl
        ln0 = emb.fe_ln[0]
        lm = self.layer_mode
        body = self._body
        y = [body(t, i) for i, t in enumerate(w["y"])]
        zb = [None if t is None else (body(t, i) if i < nfe - 1 else t) for i, t in enumerate(w["z"])]
        out0 = zb[0] if lm else y[0]
        if rag is not None and sp:
            _lib.check(lib.advh_w2v2_frontend_split_ragged(
                wave.data_ptr(), wave.stride(0), n_in, B, L, emb.w0.data_ptr(), None if emb.b0 is None else emb.b0.data_ptr(),
                ln0.g.data_ptr(), ln0.b.data_ptr(), 1 if lm else 0, 1, f["stats"].data_ptr(), f["norm"].data_ptr(), f["mr"].data_ptr(),
                out0.data_ptr(), out0.stride(0), Ls[0], P[0], C[0], rag[0].data_ptr(), st), "advh_w2v2_frontend_split_ragged")
        elif rag is not None:
            _lib.check(lib.advh_w2v2_frontend_ragged(
                wave.data_ptr(), wave.stride(0), n_in, B, L, emb.w0.data_ptr(), None if emb.b0 is None else emb.b0.data_ptr(),
                ln0.g.data_ptr(), ln0.b.data_ptr(), 1 if lm else 0, 1, f["stats"].data_ptr(), f["norm"].data_ptr(), f["mr"].data_ptr(),
                out0.data_ptr(), Ls[0], P[0], C[0], rag[0].data_ptr(), st), "advh_w2v2_frontend_ragged")
        elif sp:
            _lib.check(lib.advh_w2v2_frontend_split(
                wave.data_ptr(), wave.stride(0), n_in, B, L, emb.w0.data_ptr(), None if emb.b0 is None else emb.b0.data_ptr(),
                ln0.g.data_ptr(), ln0.b.data_ptr(), 1 if lm else 0, 1, f["stats"].data_ptr(), f["norm"].data_ptr(), f["mr"].data_ptr(),
                out0.data_ptr(), out0.stride(0), Ls[0], P[0], C[0], st), "advh_w2v2_frontend_split")
        else:
            _lib.check(lib.advh_w2v2_frontend(
                wave.data_ptr(), wave.stride(0), n_in, B, L, emb.w0.data_ptr(), None if emb.b0 is None else emb.b0.data_ptr(),
                ln0.g.data_ptr(), ln0.b.data_ptr(), 1 if lm else 0, 1, f["stats"].data_ptr(), f["norm"].data_ptr(), f["mr"].data_ptr(),
                out0.data_ptr(), Ls[0], P[0], C[0], st), "advh_w2v2_frontend")
        if lm:
            ln0(zb[0], B * P[0], 1e-5, out_h=y[0], gelu=True, split=sp)
        for i in range(1, nfe):
            last = i == nfe - 1
            dst = w["feat"] if last else y[i]
            if lm:                                         # conv (+bias) -> z_i ; LayerNorm + GELU -> y_i
                f["fe_plans"][i - 1].run(y[i - 1], out_h=zb[i])
                emb.fe_ln[i](zb[i], M if last else B * P[i], 1e-5, out_h=dst, gelu=True, split=sp)
            else:
                f["fe_plans"][i - 1].run(y[i - 1], out_h=dst, out_pre=zb[i])
        emb.fp_ln(w["feat"], M, eps, out_h=f["featn"], split=sp)
        h = f["h"]
        f["proj"].run(f["featn"], out_f=h)
        if rag is not None:                                # hidden_states[~mask] = 0: the positional conv's zero padding
            _lib.check(lib.advh_zero_tail_rows(h.data_ptr(), rag[1].data_ptr(), B, T, H, st), "advh_zero_tail_rows")
        K, Gp = cfg.num_conv_pos_embeddings, cfg.num_conv_pos_embedding_groups
        if sp:
            _lib.check(lib.advh_posconv_gather_split(h.data_ptr(), f["xg"].data_ptr(), f["xg"].stride(0), B, T, H, Gp, K, K // 2, st),
                       "advh_posconv_gather_split")
        else:
            _lib.check(lib.advh_posconv_gather(h.data_ptr(), f["xg"].data_ptr(), B, T, H, Gp, K, K // 2, None, st), "advh_posconv_gather")
        h16 = f["h16"]
        if self.stable:
            f["pos"].run(f["xg"], out_f=w["x"][0], resid=h, out_pre=w["pc"])
        else:
            f["pos"].run(f["xg"], out_f=w["h1"], resid=h, out_pre=w["pc"])
            emb.enc_ln(w["h1"], M, eps, out_f=w["x"][0], out_h=h16, split=sp)
        self._start = None
        self._stop = stop
        self._rag = rag
        self._encoder_tail(w, 0, B, stop)
        self._last = (wave, B, n_in, L)
        if stop is not None:
            hid = self._hidden_buf(w, stop).view(B, T, H).clone()
            if rag is not None:
                _lib.check(lib.advh_zero_tail_rows(hid.data_ptr(), rag[1].data_ptr(), B, T, H, st), "advh_zero_tail_rows")
            return hid
        return f["logit"].clone().view(B, 1), f["prob"].clone().view(B, 1)

    def _encoder_tail(self, w: dict, start: int, B: int, stop: Optional[int] = None) -> None:
        """Layers ``start .. nl-1`` on the rows of ``w["x"][start]`` (post-LN: and their operand copy in ``h16``), the final
        LayerNorm where the model has one, and the pooling + logreg, with the saves of the backward.  ``stop=l``: layers
        ``start .. l-1`` alone, and the final LayerNorm only when ``l == nl`` (it produces ``hidden_states[nl]``); no pooling."""
        emb, cfg, lib, sp = self.emb, self.cfg, _lib.lib(), self.split
        f = w["f"]
        st = torch.cuda.current_stream().cuda_stream
        T, M, H = f["T"], f["M"], cfg.hidden_size
        eps, nl = cfg.layer_norm_eps, emb.nl
        h16 = f["h16"]
        rag = self._rag                                    # the [2, B] lengths of a ragged pass (forward(lengths=...)), else None
        for l in range(start, nl if stop is None else stop):
            lay = f["layers"][l]
            if self.stable:
                emb.ln1[l](w["x"][l], M, eps, out_h=h16, split=sp)
            lay["qkv"].run(h16, out_h=w["qkv"][l])
            if T > emb.WHOLE_CLIP_MAX_FRAMES:              # long_clips (forward refused otherwise): the streamed kernel, frames or NULL
                fp = None if rag is None else rag[1].data_ptr()
                if sp:
                    _lib.check(lib.advh_attention_long_split(w["qkv"][l].data_ptr(), w["qkv"][l].stride(0), f["ctx"].data_ptr(),
                                                             f["ctx"].stride(0), fp, B, T, H, cfg.num_attention_heads, st),
                               "advh_attention_long_split")
                else:
                    _lib.check(lib.advh_attention_long_f16(w["qkv"][l].data_ptr(), f["ctx"].data_ptr(), fp, B, T, H,
                                                           cfg.num_attention_heads, st), "advh_attention_long_f16")
            elif rag is not None and sp:
                _lib.check(lib.advh_attention_split_ragged(w["qkv"][l].data_ptr(), w["qkv"][l].stride(0), f["ctx"].data_ptr(),
                                                           f["ctx"].stride(0), rag[1].data_ptr(), B, T, H, cfg.num_attention_heads, st),
                           "advh_attention_split_ragged")
            elif rag is not None:
                _lib.check(lib.advh_attention_f16_ragged(w["qkv"][l].data_ptr(), f["ctx"].data_ptr(), rag[1].data_ptr(), B, T, H,
                                                         cfg.num_attention_heads, st), "advh_attention_f16_ragged")
            elif sp:
                _lib.check(lib.advh_attention_split(w["qkv"][l].data_ptr(), w["qkv"][l].stride(0), f["ctx"].data_ptr(), f["ctx"].stride(0),
                                                    B, T, H, cfg.num_attention_heads, st), "advh_attention_split")
            else:
                _lib.check(lib.advh_attention_f16(w["qkv"][l].data_ptr(), f["ctx"].data_ptr(), B, T, H, cfg.num_attention_heads, st),
                           "advh_attention_f16")
            if self.stable:                                # x_{l+1} = m + ffn(LN2(m)),  m = x_l + attn(LN1(x_l))
                lay["out"].run(f["ctx"], out_f=w["m"][l], resid=w["x"][l])
                emb.ln2[l](w["m"][l], M, eps, out_h=h16, split=sp)
                lay["ff1"].run(h16, out_h=f["ffn"], out_pre=w["g1"][l])
                lay["ff2"].run(f["ffn"], out_f=w["x"][l + 1], resid=w["m"][l])
            else:                                          # x_{l+1} = LN2(m + ffn(m)),  m = LN1(x_l + attn(x_l))
                lay["out"].run(f["ctx"], out_f=w["s1"][l], resid=w["x"][l])
                emb.ln1[l](w["s1"][l], M, eps, out_f=w["m"][l], out_h=h16, split=sp)
                lay["ff1"].run(h16, out_h=f["ffn"], out_pre=w["g1"][l])
                lay["ff2"].run(f["ffn"], out_f=w["s2"][l], resid=w["m"][l])
                emb.ln2[l](w["s2"][l], M, eps, out_f=w["x"][l + 1], out_h=h16, split=sp)
        final = w["x"][nl]
        self._final_ln = self.stable and nl == cfg.num_hidden_layers
        if stop is not None and stop < nl:
            return
        if self._final_ln:
            emb.enc_ln(w["x"][nl], M, eps, out_f=w["xf"], split=sp)
            final = w["xf"]
        if stop is not None:
            return
        if rag is not None:
            _lib.check(lib.advh_pool_logreg_ragged(final.data_ptr(), emb.coef.data_ptr(), emb.intercept, f["logit"].data_ptr(),
                                                   f["prob"].data_ptr(), None, rag[1].data_ptr(), B, T, H, st), "advh_pool_logreg_ragged")
            return
        _lib.check(lib.advh_pool_logreg(final.data_ptr(), emb.coef.data_ptr(), emb.intercept, f["logit"].data_ptr(),
                                        f["prob"].data_ptr(), None, B, T, H, st), "advh_pool_logreg")

    # ------------------------------------------------------------------ the chain from / to a layer (captum.attr.Layer*)
    def _hidden_buf(self, w: dict, l: int) -> torch.Tensor:
        # hidden_states[nl] of a full-depth pre-LN model is the output of the final LayerNorm: it lives in w["xf"]
        return w["xf"] if (l == self.emb.nl and self._final_ln) else w["x"][l]

    def hidden(self, layer: int) -> torch.Tensor:
        """``hidden_states[layer]`` of the last ``forward`` / ``forward_from`` as a fresh ``[B, T, H]`` fp32 tensor."""
        l = check_layer(layer, self.emb.nl)
        if getattr(self, "_last", None) is None:
            raise RuntimeError("hidden() needs a forward pass first")
        if self._start is not None and l < self._start:
            raise ValueError(f"the last pass started at layer {self._start}: hidden_states[{l}] was not computed")
        if self._stop is not None and l > self._stop:
            raise ValueError(f"the last pass stopped at layer {self._stop}: hidden_states[{l}] was not computed")
        _, B, _, L = self._last
        w = self._workspace(B, L)
        hid = self._hidden_buf(w, l).view(B, w["f"]["T"], self.cfg.hidden_size).clone()
        if self._rag is not None:                          # a ragged pass: rows past a clip's frames are zero
            _lib.check(_lib.lib().advh_zero_tail_rows(hid.data_ptr(), self._rag[1].data_ptr(), B, w["f"]["T"], self.cfg.hidden_size,
                                                      torch.cuda.current_stream().cuda_stream), "advh_zero_tail_rows")
        return hid

    def forward_from(self, layer: int, hidden: torch.Tensor):
        """The classifier from ``hidden_states[layer]`` on: ``hidden [R, T, H]`` fp32 rows take the place of the layer's input,
        layers ``layer .. nl-1`` run with the saves of ``forward`` (so that ``backward(to_layer >= layer)`` works afterwards),
        then the final LayerNorm of a full-depth pre-LN model -- it produces ``hidden_states[nl]``, so a chain started AT ``nl``
        is the pooling + logreg alone -- and the pooling + logreg.  Nothing below the layer is launched.  ``T`` must be the
        frame count of the last ``forward`` (its clip length picks the workspace).  Returns ``(logits [R,1], probs [R,1])``."""
        l = check_layer(layer, self.emb.nl)
        if getattr(self, "_last", None) is None:
            raise RuntimeError("forward_from() needs one forward pass first (it fixes the clip length of the workspace)")
        if self._rag is not None:
            raise RuntimeError("the last pass was ragged (forward(lengths=...)): forward_from takes no per-clip lengths")
        L = self._last[3]
        H, nl = self.cfg.hidden_size, self.emb.nl
        if not torch.is_tensor(hidden) or hidden.dim() != 3 or hidden.dtype != torch.float32 or not hidden.is_cuda:
            raise ValueError("hidden must be a CUDA fp32 tensor [R, T, H]")
        R = hidden.shape[0]
        w = self._workspace(R, L)
        f = w["f"]
        T, M = f["T"], f["M"]
        if tuple(hidden.shape[1:]) != (T, H):
            raise ValueError(f"hidden must be [R, {T}, {H}] (the frames of the last forward), not {list(hidden.shape)}")
        hidden = hidden.contiguous()
        self._final_ln = self.stable and nl == self.cfg.num_hidden_layers
        # post-LN: layer l reads its GEMM operand from h16, which the previous LayerNorm wrote -- written here from the same values
        op = f["h16"] if (l < nl and not self.stable) else None
        _lib.check(_lib.lib().advh_layer_inject(
            hidden.data_ptr(), M, H, self._hidden_buf(w, l).data_ptr(), None if op is None else op.data_ptr(), int(self.split),
            op.stride(0) if (op is not None and self.split) else 0, torch.cuda.current_stream().cuda_stream), "advh_layer_inject")
        self._start = l
        self._stop = None
        st = torch.cuda.current_stream().cuda_stream
        if l == nl:
            _lib.check(_lib.lib().advh_pool_logreg(self._hidden_buf(w, l).data_ptr(), self.emb.coef.data_ptr(), self.emb.intercept,
                                                   f["logit"].data_ptr(), f["prob"].data_ptr(), None, R, T, H, st), "advh_pool_logreg")
        else:
            self._encoder_tail(w, l, R)
        self._last = (None, R, None, L)
        return f["logit"].clone().view(R, 1), f["prob"].clone().view(R, 1)

    def layer_tap(self, g: torch.Tensor, inv_scale: float = 1.0, act: Optional[torch.Tensor] = None, want_out: bool = True,
                  row_sum: Optional[torch.Tensor] = None):
        """advh_layer_tap on contiguous fp32 rows ``g [rows, ...]``: ``g * inv_scale (* act)`` as a fresh tensor of g's shape
        (None with ``want_out=False``), and the per-row sums into ``row_sum [rows]`` if given."""
        rows = g.shape[0]
        out = torch.empty_like(g) if want_out else None
        _lib.check(_lib.lib().advh_layer_tap(g.data_ptr(), None if act is None else act.data_ptr(), inv_scale, rows, g.numel() // rows,
                                             None if out is None else out.data_ptr(), None if row_sum is None else row_sum.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "advh_layer_tap")
        return out

    # ------------------------------------------------------------------ backward
    def _ln_bwd(self, ln, x, dy, M, out_f=None, out_h=None, add=None, dact=None, remap=(0, 0), gelu=False, eps=None):
        eps = self.cfg.layer_norm_eps if eps is None else eps
        st = torch.cuda.current_stream().cuda_stream
        x32, dy32 = int(x.dtype == torch.float32), int(dy.dtype == torch.float32)
        p = lambda t: None if t is None else t.data_ptr()
        if self.split:                                     # fp16-side tensors are plane pairs: pass each one's plane pitch
            lo = lambda t, is32=0: 0 if (t is None or is32) else t.stride(0)
            _lib.check(_lib.lib().advh_layernorm_bwd_split(
                x.data_ptr(), x32, lo(x, x32), dy.data_ptr(), dy32, lo(dy, dy32), ln.g.data_ptr(), ln.b.data_ptr(), int(gelu), p(add),
                p(dact), lo(dact), p(out_f), p(out_h), lo(out_h), M, ln.C, eps, remap[0], remap[1], st), "advh_layernorm_bwd_split")
            return
        _lib.check(_lib.lib().advh_layernorm_bwd(
            x.data_ptr(), x32, dy.data_ptr(), dy32, ln.g.data_ptr(), ln.b.data_ptr(), int(gelu), p(add), p(dact), p(out_f), p(out_h), M,
            ln.C, eps, remap[0], remap[1], st), "advh_layernorm_bwd")

    def _att_bwd(self, qkv, dctx, dqkv, B, T, H, heads, st):
        lib = _lib.lib()
        if self.split:
            _lib.check(lib.advh_attention_bwd_split(qkv.data_ptr(), qkv.stride(0), dctx.data_ptr(), dctx.stride(0), dqkv.data_ptr(),
                                                    dqkv.stride(0), B, T, H, heads, st), "advh_attention_bwd_split")
        else:
            if H // heads > 64 and T > F16_WIDE_HEAD_MAX_T:
                raise _lib.AdvhError(f"advh_attention_bwd_f16: ADVH_EUNSUPPORTED: head dim {H // heads} > 64 is held for T <= {F16_WIDE_HEAD_MAX_T} frames only "
                                     f"(T = {T}: its whole-clip tiles exceed the 160 KiB of LDS); shorten the clip or use precision='f32'")
            _lib.check(lib.advh_attention_bwd_f16(qkv.data_ptr(), dctx.data_ptr(), dqkv.data_ptr(), B, T, H, heads, st),
                       "advh_attention_bwd_f16")

    def _att_bwd_ragged(self, qkv, dctx, dqkv, frames, B, T, H, heads, st):
        """``_att_bwd`` of a ragged pass (advh_attention_bwd_*_ragged): same refusals, ``frames`` int32 [B] on the device."""
        lib = _lib.lib()
        if self.split:
            _lib.check(lib.advh_attention_bwd_split_ragged(qkv.data_ptr(), qkv.stride(0), dctx.data_ptr(), dctx.stride(0), dqkv.data_ptr(),
                                                           dqkv.stride(0), frames.data_ptr(), B, T, H, heads, st),
                       "advh_attention_bwd_split_ragged")
        else:
            if H // heads > 64 and T > F16_WIDE_HEAD_MAX_T:
                raise _lib.AdvhError(f"advh_attention_bwd_f16_ragged: ADVH_EUNSUPPORTED: head dim {H // heads} > 64 is held for T <= {F16_WIDE_HEAD_MAX_T} "
                                     f"frames only (T = {T}: its whole-clip tiles exceed the 160 KiB of LDS); shorten the clip or use precision='f32'")
            _lib.check(lib.advh_attention_bwd_f16_ragged(qkv.data_ptr(), dctx.data_ptr(), dqkv.data_ptr(), frames.data_ptr(), B, T, H,
                                                         heads, st), "advh_attention_bwd_f16_ragged")

    def _att_bwd_long(self, qkv, dctx, dqkv, stats, frames, B, T, H, heads, st):
        """advh_attention_bwd_long_*: the streamed backward of a ``long_clips`` chain above 256 frames; ``frames`` int32 [B] on
        the device (a ragged pass) or None."""
        lib = _lib.lib()
        fp = None if frames is None else frames.data_ptr()
        if self.split:
            _lib.check(lib.advh_attention_bwd_long_split(qkv.data_ptr(), qkv.stride(0), dctx.data_ptr(), dctx.stride(0), dqkv.data_ptr(),
                                                         dqkv.stride(0), stats.data_ptr(), fp, B, T, H, heads, st),
                       "advh_attention_bwd_long_split")
        else:
            _lib.check(lib.advh_attention_bwd_long_f16(qkv.data_ptr(), dctx.data_ptr(), dqkv.data_ptr(), stats.data_ptr(), fp, B, T, H,
                                                       heads, st), "advh_attention_bwd_long_f16")

    def _refuse_maps_above_limit(self, what: str) -> None:
        """``attention_maps=``, ``attention_probs`` and ``rules=`` run ``T x T`` kernels (csrc/attention_maps.hip, lrp.hip) that hold
        a whole clip: ``AdvhError`` when the last pass had more frames, before any launch or allocation, unless the chain was
        built with ``long_maps=True`` (the streamed kernels of csrc/attention_maps_long.hip).  Host only."""
        if self.long_maps:
            return
        L = self._last[3]
        T = self.emb._lengths(int(L))[-1]
        if T > self.emb.WHOLE_CLIP_MAX_FRAMES:
            raise _lib.AdvhError(f"{what}: ADVH_EUNSUPPORTED: the T x T attention kernels behind it are held for T <= "
                                 f"{self.emb.WHOLE_CLIP_MAX_FRAMES} frames ({self.emb.whole_clip_max_samples()} samples) and the last pass "
                                 f"had T = {T} ({int(L)} samples); long_clips lifts the limit of the gradient alone, and a chain built "
                                 "with long_maps=True (EmbedderGrad, HipAttribution; ADDVISOR_LONG_MAPS=1 for the runtime singleton) "
                                 "lifts this one")

    def _streamed_maps(self, T: int) -> bool:
        """Whether ``attention_probs`` / ``attention_maps=`` / the AH-rule of the last pass run the streamed kernels: a
        ``long_maps`` chain above 256 frames or after a ragged pass."""
        return self.long_maps and (T > self.emb.WHOLE_CLIP_MAX_FRAMES or self._rag is not None)

    def _att_stats(self, w: dict, B: int, T: int) -> torch.Tensor:
        """The streamed kernels' ``(m, 1/l)`` workspace: ``w["att_stats"]`` of the long chain, allocated here for a ragged pass
        at 256 frames and below."""
        if "att_stats" not in w:
            nb = _lib.lib().advh_attention_bwd_long_ws_bytes(B, T, self.cfg.num_attention_heads)
            w["att_stats"] = torch.empty(nb // 4, dtype=torch.float32, device=self.dev)
        return w["att_stats"]

    def _zero_tail(self, g32, g16, rag, B, T, H, st):
        """Rows ``t >= T_b`` of a residual-stream gradient = 0: the fp32 buffer and its fp16 / plane-pair copy."""
        lib = _lib.lib()
        _lib.check(lib.advh_zero_tail_rows(g32.data_ptr(), rag[1].data_ptr(), B, T, H, st), "advh_zero_tail_rows")
        _lib.check(lib.advh_zero_tail_rows_h(g16.data_ptr(), g16.stride(0) if self.split else 0, rag[1].data_ptr(), B, T, H, st),
                   "advh_zero_tail_rows_h")

    def _ln_bwd_frozen(self, ln, x, dy, M, out_f=None, out_h=None, add=None):
        """advh_layernorm_bwd_frozen(_split): ``_ln_bwd`` with ``1/sigma`` a constant (the LN-rule)."""
        st = torch.cuda.current_stream().cuda_stream
        x32, dy32 = int(x.dtype == torch.float32), int(dy.dtype == torch.float32)
        p = lambda t: None if t is None else t.data_ptr()
        if self.split:
            lo = lambda t, is32=0: 0 if (t is None or is32) else t.stride(0)
            _lib.check(_lib.lib().advh_layernorm_bwd_frozen_split(
                x.data_ptr(), x32, lo(x, x32), dy.data_ptr(), dy32, lo(dy, dy32), ln.g.data_ptr(), p(add), p(out_f), p(out_h), lo(out_h),
                M, ln.C, self.cfg.layer_norm_eps, st), "advh_layernorm_bwd_frozen_split")
            return
        _lib.check(_lib.lib().advh_layernorm_bwd_frozen(
            x.data_ptr(), x32, dy.data_ptr(), dy32, ln.g.data_ptr(), p(add), p(out_f), p(out_h), M, ln.C, self.cfg.layer_norm_eps, st),
            "advh_layernorm_bwd_frozen")

    def _att_bwd_value(self, qkv, dctx, dqkv, B, T, H, heads, st):
        """advh_attention_bwd_value: ``_att_bwd`` with the probabilities a constant (the AH-rule): dV alone, dQ = dK = 0."""
        lo = lambda t: t.stride(0) if self.split else 0
        _lib.check(_lib.lib().advh_attention_bwd_value(qkv.data_ptr(), lo(qkv), dctx.data_ptr(), lo(dctx), dqkv.data_ptr(), lo(dqkv),
                                                       B, T, H, heads, st), "advh_attention_bwd_value")

    def _gelu_identity_bwd(self, d, g1, st):
        """advh_gelu_identity_bwd in place: ``d <- d * Phi(g1)`` (the GELU identity rule)."""
        lo = lambda t: t.stride(0) if self.split else 0
        n = d.numel() // (2 if self.split else 1)
        _lib.check(_lib.lib().advh_gelu_identity_bwd(d.data_ptr(), lo(d), g1.data_ptr(), lo(g1), d.data_ptr(), lo(d), n, st),
                   "advh_gelu_identity_bwd")

    def _att_maps(self, qkv, dctx, out, fuse, dscale, B, T, H, heads, st):
        """advh_attention_maps on one layer's saved ``qkv`` (``dctx=None``: the probabilities) into the fp32 view ``out``."""
        lo = lambda t: t.stride(0) if (self.split and t is not None) else 0
        _lib.check(_lib.lib().advh_attention_maps(qkv.data_ptr(), lo(qkv), None if dctx is None else dctx.data_ptr(), lo(dctx), dscale,
                                                  fuse, out.data_ptr(), B, T, H, heads, st), "advh_attention_maps")

    def _att_maps_long(self, qkv, dctx, out, fuse, dscale, stats, frames, B, T, H, heads, st):
        """advh_attention_maps_long: ``_att_maps`` for any ``T`` and per-clip ``frames`` (int32 [B] on the device, or None)."""
        lo = lambda t: t.stride(0) if (self.split and t is not None) else 0
        _lib.check(_lib.lib().advh_attention_maps_long(qkv.data_ptr(), lo(qkv), None if dctx is None else dctx.data_ptr(), lo(dctx), dscale,
                                                       fuse, out.data_ptr(), stats.data_ptr(), None if frames is None else frames.data_ptr(),
                                                       B, T, H, heads, st), "advh_attention_maps_long")

    def _att_bwd_value_long(self, qkv, dctx, dqkv, stats, frames, B, T, H, heads, st):
        """advh_attention_bwd_value_long: ``_att_bwd_value`` for any ``T`` and per-clip ``frames``."""
        lo = lambda t: t.stride(0) if self.split else 0
        _lib.check(_lib.lib().advh_attention_bwd_value_long(qkv.data_ptr(), lo(qkv), dctx.data_ptr(), lo(dctx), dqkv.data_ptr(), lo(dqkv),
                                                            stats.data_ptr(), None if frames is None else frames.data_ptr(), B, T, H, heads,
                                                            st), "advh_attention_bwd_value_long")

    def attention_probs(self, layer: int, fuse: int = 0) -> torch.Tensor:
        """The attention probabilities ``softmax(Q K^T / sqrt(d))`` of encoder layer ``layer`` (``0 <= layer < nl``) at the clips
        of the last pass, recomputed from its saved ``qkv`` (read-only: no state of the chain changes): ``[B, heads, T, T]``
        fp32 (``fuse=0``) or fused over heads, ``[B, T, T]`` (``fuse`` 1 mean, 2 max, 3 min), rows = queries.  On a ``long_maps``
        chain after a ragged pass clip ``b``'s map is that of the clip alone in the top-left ``T_b x T_b`` block, 0 elsewhere."""
        l = check_layer(layer, self.emb.nl - 1)
        if fuse not in (0, 1, 2, 3):
            raise ValueError("fuse must be 0 (none), 1 (mean), 2 (max) or 3 (min)")
        if getattr(self, "_last", None) is None:
            raise RuntimeError("attention_probs() needs a forward pass first")
        self._refuse_maps_above_limit("EmbedderGrad.attention_probs")
        if self._rag is not None and not self.long_maps:
            raise ValueError("the last pass was ragged (forward(lengths=...)): attention maps take no per-clip lengths "
                             "(a chain built with long_maps=True takes them)")
        if self._start is not None and l < self._start:
            raise ValueError(f"the last pass started at layer {self._start}: layer {l}'s attention did not run")
        if self._stop is not None and l >= self._stop:
            raise ValueError(f"the last pass stopped at layer {self._stop}: layer {l}'s attention did not run")
        _, B, _, L = self._last
        w = self._workspace(B, L)
        T, H, heads = w["f"]["T"], self.cfg.hidden_size, self.cfg.num_attention_heads
        out = torch.empty((B, T, T) if fuse else (B, heads, T, T), dtype=torch.float32, device=self.dev)
        st = torch.cuda.current_stream().cuda_stream
        if self._streamed_maps(T):
            self._att_maps_long(w["qkv"][l], None, out, fuse, 1.0, self._att_stats(w, B, T), None if self._rag is None else self._rag[1],
                                B, T, H, heads, st)
        else:
            self._att_maps(w["qkv"][l], None, out, fuse, 1.0, B, T, H, heads, st)
        return out

    def neuron_values(self, v: torch.Tensor, box) -> torch.Tensor:
        """advh_neuron_values: ``out[r]`` = the sum over the selection box of the contiguous fp32 rows ``v [R, T, H]``."""
        R, T, H = v.shape
        b = (ctypes.c_int * 6)(*check_box(box, T, H))
        out = torch.empty(R, dtype=torch.float32, device=v.device)
        _lib.check(_lib.lib().advh_neuron_values(v.data_ptr(), R, T, H, b, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "advh_neuron_values")
        return out

    def _seed_args(self, B, T, H, seed, to_layer, from_layer, neuron, layer_seed, row_scale):
        """The arguments of ``backward(from_layer=l, ...)``, before any launch: ``(l, box | None)``."""
        if from_layer is None:
            if neuron is not None or layer_seed is not None or row_scale is not None:
                raise ValueError("neuron, layer_seed and row_scale belong to backward(from_layer=l, ...)")
            return None, None
        l = check_layer(from_layer, self.emb.nl)
        if seed is not None or to_layer is not None:
            raise ValueError("backward(from_layer=l, ...) runs the chain below the layer: it takes neither seed nor to_layer")
        if (neuron is None) == (layer_seed is None):
            raise ValueError("backward(from_layer=l, ...) needs exactly one of neuron (a selection box) and layer_seed ([R, T, H])")
        if self._start is not None:
            raise RuntimeError(f"the last pass started at layer {self._start} (forward_from): the lower chain has no saves of it")
        if self._stop is not None and l > self._stop:
            raise ValueError(f"the last pass stopped at layer {self._stop}: a backward from layer {l} needs a pass up to there")
        dev_f32 = lambda t: torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32
        if neuron is None:
            if row_scale is not None:
                raise ValueError("row_scale scales a neuron's seed; fold it into layer_seed")
            if not dev_f32(layer_seed) or tuple(layer_seed.shape) != (B, T, H):
                raise ValueError(f"layer_seed must be a CUDA fp32 tensor [{B}, {T}, {H}] (the rows of the last forward)")
            return l, None
        if row_scale is not None and (not dev_f32(row_scale) or tuple(row_scale.shape) != (B,)):
            raise ValueError(f"row_scale must be a CUDA fp32 tensor [{B}]")
        return l, check_box(neuron, T, H)

    def backward(self, loss_scale: float = 4096.0, seed: Optional[torch.Tensor] = None, to_layer: Optional[int] = None,
                 from_layer: Optional[int] = None, neuron=None, layer_seed: Optional[torch.Tensor] = None,
                 row_scale: Optional[torch.Tensor] = None, attention_maps=None, rules: Optional[LrpRules] = None) -> torch.Tensor:
        """d logit / d wave for the clips of the last ``forward`` call: ``[B, n_in]`` fp32.  With ``seed [B]``
        (dL/d logit per clip) the result is dL/d wave instead (vector-Jacobian product: LMACLoss backward).
        ``to_layer=l``: the chain stops once ``d logit / d hidden_states[l]`` is in the residual-stream buffer and returns it,
        ``[B, T, H]`` fp32 (divided by ``loss_scale``, advh_layer_tap); the layers below, the positional convolution, the feature
        encoder and the waveform kernels are not launched.  It works after ``forward`` and after ``forward_from(l', .)`` with
        ``l' <= l``; ``hidden_states[nl]`` of a full-depth pre-LN model is the final LayerNorm's output, so ``to_layer=nl`` is the
        pooling's backward alone there.
        ``from_layer=l`` (the neuron methods, ``captum.attr.Neuron*``): the chain starts at ``hidden_states[l]`` from a seed
        gradient instead of the logit -- ``neuron=box``: ``loss_scale (* row_scale[r])`` inside the selection box
        (``check_box``) of every clip row and 0 elsewhere; ``layer_seed [B, T, H]``: ``loss_scale * layer_seed``
        (advh_layer_seed) -- and runs layers ``l-1 .. 0`` and the lower chain: ``[B, n_in]`` fp32, the vector-Jacobian product
        ``seed . d hidden_states[l] / d wave`` (divided by ``loss_scale``).  Nothing above the layer is launched.  It works after
        ``forward(...)`` with ``to_layer`` None or ``>= l``, also after a ``backward(to_layer=...)`` of the same pass (the saves
        are read-only); at ``l == nl`` of a full-depth pre-LN model the seed passes through the final LayerNorm's backward.
        ``attention_maps=(out, fuse)``: every layer ``l`` the chain passes also writes its gradient-weighted attention map
        ``(dF/dA_l * A_l)^+`` (advh_attention_maps on the layer's saved ``qkv`` and the gradient at its attention context, divided
        by ``loss_scale``) into ``out[l - to_layer]``: ``out`` is a contiguous CUDA fp32 tensor ``[layers, B, T, T]`` (``fuse`` 1
        mean, 2 max, 3 min over heads) or ``[layers, B, heads, T, T]`` (``fuse=0``); ``layers`` is at most the number of layers the
        chain runs, and the lowest ``layers`` of them write.  The maps only read the chain's buffers: the gradient is the same with and without them.
        ``rules`` (an ``LrpRules``; None: the plain gradient, every launch as without the argument): the encoder layers the chain
        runs, and the final LayerNorm of a full-depth pre-LN model, propagate conservatively (Ali et al. 2022; csrc/lrp.hip) --
        ``ln``: the LayerNorm backwards hold ``1/sigma`` constant; ``attention``: the attention backward holds the probabilities
        constant (``dV = P^T dO``, ``dQ = dK = 0``); ``gelu="identity"``: the FFN's GELU backward multiplies by ``Phi(g1)``
        instead of ``GELU'(g1)``.  The chain below the encoder has no rules: ``to_layer`` is required, and ``rules`` does not
        combine with ``from_layer`` (ValueError before any launch).  It combines with ``attention_maps``, which only reads.
        Both stop at 256 frames and refuse a ragged pass unless the chain has ``long_maps=True``: then, above 256 frames or after
        ``forward(lengths=...)``, the maps come from advh_attention_maps_long (clip ``b``'s in the top-left ``T_b x T_b`` block, 0
        elsewhere) and the attention rule runs advh_attention_bwd_value_long (csrc/attention_maps_long.hip)."""
        if rules is not None:
            if not isinstance(rules, LrpRules):
                raise ValueError(f"rules must be an LrpRules or None, not {rules!r}")
            if from_layer is not None:
                raise ValueError("rules does not combine with from_layer: the chain below a layer's seed has no propagation rules")
            if to_layer is None:
                raise ValueError("backward(rules=...) needs to_layer: the positional convolution, the feature encoder and the "
                                 "waveform kernels have no propagation rules")
            check_layer(to_layer, self.emb.nl)
        if getattr(self, "_last", None) is None:
            raise RuntimeError("backward() needs a forward pass first")
        if attention_maps is not None or rules is not None:    # before any launch or allocation
            self._refuse_maps_above_limit("EmbedderGrad.backward(attention_maps=...)" if rules is None else "EmbedderGrad.backward(rules=...)")
        rag = self._rag
        if rag is not None and (attention_maps is not None or rules is not None) and not self.long_maps:
            raise ValueError("the last pass was ragged (forward(lengths=...)): backward takes neither attention_maps nor rules "
                             "after it (they have no per-clip lengths; a chain built with long_maps=True takes both)")
        _w = self._workspace(self._last[1], self._last[3])["f"]
        top, box = self._seed_args(self._last[1], _w["T"], self.cfg.hidden_size, seed, to_layer, from_layer, neuron, layer_seed, row_scale)
        if from_layer is None and self._stop is not None:
            raise RuntimeError(f"the last pass stopped at layer {self._stop} (forward(to_layer=...)): only backward(from_layer <= "
                               f"{self._stop}, ...) is defined")
        stop = 0 if to_layer is None else check_layer(to_layer, self.emb.nl)
        if to_layer is None and self._start is not None:
            raise RuntimeError(f"the last pass started at layer {self._start} (forward_from): only backward(to_layer >= "
                               f"{self._start}) is defined")
        if to_layer is not None and self._start is not None and stop < self._start:
            raise ValueError(f"the last pass started at layer {self._start}: the gradient at layer {stop} needs a pass from there")
        emb, cfg, lib, sp = self.emb, self.cfg, _lib.lib(), self.split
        wave, B, n_in, L = self._last
        w = self._workspace(B, L)
        f = w["f"]
        st = torch.cuda.current_stream().cuda_stream
        Ls, P, T, M, H = f["Ls"], f["P"], f["T"], f["M"], cfg.hidden_size
        C, nfe, nl = cfg.conv_dim, len(f["Ls"]), emb.nl
        da, db, d16, t16 = w["da"], w["db"], w["d16"], w["t16"]
        heads = cfg.num_attention_heads
        maps = None
        if attention_maps is not None:                     # checked before the first launch
            maps, fuse = attention_maps
            n_run = (nl if top is None else top) - stop
            shape = (B, T, T) if fuse else (B, heads, T, T)
            if fuse not in (0, 1, 2, 3) or not torch.is_tensor(maps) or not maps.is_cuda or maps.dtype != torch.float32 \
                    or not maps.is_contiguous() or tuple(maps.shape[1:]) != shape or not 1 <= maps.shape[0] <= n_run:
                raise ValueError(f"attention_maps must be (out, fuse): fuse in 0..3 and out a contiguous CUDA fp32 tensor "
                                 f"[1..{n_run}] + {list(shape)}")
        if top is not None:                                # da / d16 = the seed at hidden_states[top]: every element written
            p = lambda t: None if t is None else t.data_ptr()
            src = None if layer_seed is None else layer_seed.contiguous()
            rs = None if row_scale is None else row_scale.contiguous()
            _lib.check(lib.advh_layer_seed(
                p(src), p(rs), loss_scale, B, T, H,
                None if box is None else (ctypes.c_int * 6)(*box), da.data_ptr(), d16.data_ptr(), int(sp), d16.stride(0) if sp else 0, st),
                "advh_layer_seed")
            if rag is not None:                            # a seed or box reaching past a clip's frames is ignored
                self._zero_tail(da, d16, rag, B, T, H, st)
        else:
            top = nl
            if seed is None:
                w["dlogit"].fill_(loss_scale)
            else:
                w["dlogit"].copy_(seed.reshape(-1).to(w["dlogit"].dtype) * loss_scale)
            if rag is not None and sp:
                _lib.check(lib.advh_pool_logreg_bwd_split_ragged(emb.coef.data_ptr(), w["dlogit"].data_ptr(), da.data_ptr(), d16.data_ptr(),
                                                                 d16.stride(0), rag[1].data_ptr(), B, T, H, st),
                           "advh_pool_logreg_bwd_split_ragged")
            elif rag is not None:
                _lib.check(lib.advh_pool_logreg_bwd_ragged(emb.coef.data_ptr(), w["dlogit"].data_ptr(), da.data_ptr(), d16.data_ptr(),
                                                           rag[1].data_ptr(), B, T, H, st), "advh_pool_logreg_bwd_ragged")
            elif sp:
                _lib.check(lib.advh_pool_logreg_bwd_split(emb.coef.data_ptr(), w["dlogit"].data_ptr(), da.data_ptr(), d16.data_ptr(),
                                                          d16.stride(0), B, T, H, st), "advh_pool_logreg_bwd_split")
            else:
                _lib.check(lib.advh_pool_logreg_bwd(emb.coef.data_ptr(), w["dlogit"].data_ptr(), da.data_ptr(), d16.data_ptr(), B, T, H, st),
                           "advh_pool_logreg_bwd")
        # the rules swap a launch for its conservative form (csrc/lrp.hip); rules=None is the plain chain, launch for launch
        ln_bwd = self._ln_bwd_frozen if (rules is not None and rules.ln) else self._ln_bwd
        att_bwd = self._att_bwd_value if (rules is not None and rules.attention) else self._att_bwd
        att_maps = self._att_maps
        frames = None if rag is None else rag[1]
        streamed = self._streamed_maps(T)                  # long_maps: above 256 frames or after a ragged pass
        if streamed and maps is not None:
            att_maps = lambda qkv, dctx, out, fuse_, ds, B_, T_, H_, heads_, st_: self._att_maps_long(
                qkv, dctx, out, fuse_, ds, self._att_stats(w, B, T), frames, B_, T_, H_, heads_, st_)
        if streamed and rules is not None and rules.attention:                 # the AH-rule, streamed
            att_bwd = lambda qkv, dctx, dqkv, B_, T_, H_, heads_, st_: self._att_bwd_value_long(
                qkv, dctx, dqkv, self._att_stats(w, B, T), frames, B_, T_, H_, heads_, st_)
        elif T > emb.WHOLE_CLIP_MAX_FRAMES:                # long_clips; without long_maps rules were refused above
            att_bwd = lambda qkv, dctx, dqkv, B_, T_, H_, heads_, st_: self._att_bwd_long(
                qkv, dctx, dqkv, w["att_stats"], frames, B_, T_, H_, heads_, st_)
        elif rag is not None:                              # rows past a clip's frames: never read, written as zeros
            att_bwd = lambda qkv, dctx, dqkv, B_, T_, H_, heads_, st_: self._att_bwd_ragged(qkv, dctx, dqkv, rag[1], B_, T_, H_, heads_, st_)
        gelu_id = rules is not None and rules.gelu == "identity"

        def ff2_bwd(bl, l):                                                                   # d16 -> w["dI"] = d(pre-GELU)
            if gelu_id:
                bl["ff2"].run(d16, out_h=w["dI"], dact_src=None)
                self._gelu_identity_bwd(w["dI"], w["g1"][l], st)
            else:
                bl["ff2"].run(d16, out_h=w["dI"], dact_src=w["g1"][l])
        if self._final_ln and stop < nl and top == nl:
            ln_bwd(emb.enc_ln, w["x"][nl], da, M, out_f=db, out_h=d16)
            da, db = db, da
        for l in range(top - 1, stop - 1, -1):
            bl = w["layers"][l]
            if self.stable:                                # da = d x_{l+1} (fp32), d16 its fp16 copy
                ff2_bwd(bl, l)
                bl["ff1"].run(w["dI"], out_h=t16)                                             # d LN2(m)
                ln_bwd(emb.ln2[l], w["m"][l], t16, M, out_f=db, out_h=d16, add=da)            # db = d m
                bl["out"].run(d16, out_h=w["dctx"])
                if maps is not None and l - stop < maps.shape[0]:
                    att_maps(w["qkv"][l], w["dctx"], maps[l - stop], fuse, 1.0 / loss_scale, B, T, H, heads, st)
                att_bwd(w["qkv"][l], w["dctx"], w["dqkv"], B, T, H, heads, st)
                bl["qkv"].run(w["dqkv"], out_h=t16)                                           # d LN1(x_l)
                ln_bwd(emb.ln1[l], w["x"][l], t16, M, out_f=da, out_h=d16, add=db)            # da = d x_l
            else:
                ln_bwd(emb.ln2[l], w["s2"][l], da, M, out_f=db, out_h=d16)                    # db = d s2
                ff2_bwd(bl, l)                                                                # d(pre-GELU)
                bl["ff1"].run(w["dI"], out_f=da, resid=db)                                    # da = d m
                ln_bwd(emb.ln1[l], w["s1"][l], da, M, out_f=db, out_h=d16)                    # db = d s1
                bl["out"].run(d16, out_h=w["dctx"])
                if maps is not None and l - stop < maps.shape[0]:
                    att_maps(w["qkv"][l], w["dctx"], maps[l - stop], fuse, 1.0 / loss_scale, B, T, H, heads, st)
                att_bwd(w["qkv"][l], w["dctx"], w["dqkv"], B, T, H, heads, st)
                bl["qkv"].run(w["dqkv"], out_f=da, resid=db)                                  # da = d x_l
        if to_layer is not None:                                                              # da = d hidden_states[stop]
            return self.layer_tap(da.view(B, T, H), 1.0 / loss_scale)
        if not self.stable:
            self._ln_bwd(emb.enc_ln, w["h1"], da, M, out_f=db)                                # d h1
            da, db = db, da
        K, Gp = cfg.num_conv_pos_embeddings, cfg.num_conv_pos_embedding_groups
        if sp:
            _lib.check(lib.advh_posconv_gather_bwd_split(da.data_ptr(), f["xg"].data_ptr(), f["xg"].stride(0), B, T, H, Gp, K, K // 2 - 1,
                                                         w["pc"].data_ptr(), w["pc"].stride(0), st), "advh_posconv_gather_bwd_split")
        else:
            _lib.check(lib.advh_posconv_gather(da.data_ptr(), f["xg"].data_ptr(), B, T, H, Gp, K, K // 2 - 1, w["pc"].data_ptr(), st),
                       "advh_posconv_gather")
        w["pos"].run(f["xg"], out_f=db, out_h=d16, resid=da)                                  # d h0
        if rag is not None:        # the backward of the forward's zeroing of h: the convolution spread the last frames' gradient into padded rows
            self._zero_tail(db, d16, rag, B, T, H, st)
        w["proj"].run(d16, out_h=w["dfeatn"])
        dz = w["dz"]
        last = nfe - 1
        body = lambda i: dz[i][..., C[i]:]                                                    # skip the guard row
        zb = lambda i: w["z"][i] if i == last else self._body(w["z"][i], i)
        if self.layer_mode:
            self._ln_bwd(emb.fp_ln, w["feat"], w["dfeatn"], M, out_h=w["dfeat"])
            self._ln_bwd(emb.fe_ln[last], zb(last), w["dfeat"], M, out_h=body(last), remap=(T, P[last]), gelu=True, eps=1e-5)
        else:
            self._ln_bwd(emb.fp_ln, w["feat"], w["dfeatn"], M, out_h=body(last), dact=zb(last), remap=(T, P[last]))
        for i in range(last, 0, -1):
            plan, nt = w["fe"][i - 1]
            a0 = dz[i] if nt == 2 else body(i)
            if self.layer_mode:
                dyb = self._body(w["dyb"], 0)                                                 # level-0 sized scratch: large enough for every level
                plan.run(a0, out_h=dyb)
                self._ln_bwd(emb.fe_ln[i - 1], zb(i - 1), dyb, B * P[i - 1], out_h=body(i - 1), gelu=True, eps=1e-5)
            else:
                plan.run(a0, out_h=body(i - 1), dact_src=zb(i - 1) if i > 1 else None)
        if not self.layer_mode:
            ln0 = emb.fe_ln[0]
            if rag is not None and sp:
                _lib.check(lib.advh_w2v2_frontend_bwd_group_split_ragged(
                    wave.data_ptr(), wave.stride(0), n_in, B, L, emb.w0.data_ptr(), ln0.g.data_ptr(), f["stats"].data_ptr(),
                    f["norm"].data_ptr(), f["mr"].data_ptr(), body(0).data_ptr(), dz[0].stride(0), w["part"].data_ptr(),
                    w["sums"].data_ptr(), body(0).data_ptr(), dz[0].stride(0), Ls[0], P[0], C[0], rag[0].data_ptr(), st),
                    "advh_w2v2_frontend_bwd_group_split_ragged")
            elif rag is not None:
                _lib.check(lib.advh_w2v2_frontend_bwd_group_ragged(
                    wave.data_ptr(), wave.stride(0), n_in, B, L, emb.w0.data_ptr(), ln0.g.data_ptr(), f["stats"].data_ptr(),
                    f["norm"].data_ptr(), f["mr"].data_ptr(), body(0).data_ptr(), w["part"].data_ptr(), w["sums"].data_ptr(),
                    body(0).data_ptr(), Ls[0], P[0], C[0], rag[0].data_ptr(), st), "advh_w2v2_frontend_bwd_group_ragged")
            elif sp:
                _lib.check(lib.advh_w2v2_frontend_bwd_group_split(
                    wave.data_ptr(), wave.stride(0), n_in, B, L, emb.w0.data_ptr(), ln0.g.data_ptr(), f["stats"].data_ptr(),
                    f["norm"].data_ptr(), f["mr"].data_ptr(), body(0).data_ptr(), dz[0].stride(0), w["part"].data_ptr(),
                    w["sums"].data_ptr(), body(0).data_ptr(), dz[0].stride(0), Ls[0], P[0], C[0], st), "advh_w2v2_frontend_bwd_group_split")
            else:
                _lib.check(lib.advh_w2v2_frontend_bwd_group(
                    wave.data_ptr(), wave.stride(0), n_in, B, L, emb.w0.data_ptr(), ln0.g.data_ptr(), f["stats"].data_ptr(),
                    f["norm"].data_ptr(), f["mr"].data_ptr(), body(0).data_ptr(), w["part"].data_ptr(), w["sums"].data_ptr(),
                    body(0).data_ptr(), Ls[0], P[0], C[0], st), "advh_w2v2_frontend_bwd_group")
        w["g_plan"].run(body(0), out_f=w["g"])
        dx = torch.empty((B, n_in), dtype=torch.float32, device=wave.device)
        if rag is not None:
            _lib.check(lib.advh_wave_bwd_ragged(w["g"].data_ptr(), wave.data_ptr(), wave.stride(0), n_in, B, L, f["stats"].data_ptr(),
                                                w["dxh"].data_ptr(), w["wpart"].data_ptr(), 1, 1.0 / loss_scale, dx.data_ptr(), n_in,
                                                Ls[0], P[0], rag[0].data_ptr(), st), "advh_wave_bwd_ragged")
            return dx
        _lib.check(lib.advh_wave_bwd(w["g"].data_ptr(), wave.data_ptr(), wave.stride(0), n_in, B, L, f["stats"].data_ptr(),
                                     w["dxh"].data_ptr(), w["wpart"].data_ptr(), 1, 1.0 / loss_scale, dx.data_ptr(), n_in,
                                     Ls[0], P[0], st), "advh_wave_bwd")
        return dx
