#!/usr/bin/env python3
"""Conservative LRP for the encoder next to the chain it rides on, in one process: wav2vec2-base shape, 16 clips x 4 s
(T = 199), both precisions.
  - ``transformer_lrp`` (default rules, and all three rules with the GELU identity rule) next to
    ``layer_gradient_x_activation(w, 0)`` over the same clips: the same forward and a backward to layer 0 whose LayerNorm and
    attention backwards (and, with the identity rule, the FFN's GELU derivative) are replaced by the kernels of csrc/lrp.hip.
  - the time per layer of each of the three new launches, timed alone, next to the launches they replace: the value-only
    attention backward against the full attention backward, the frozen-sigma LayerNorm backward against the plain one (two per
    layer each), and the GELU identity multiply.
By count the LRP chain does less work than its comparison (no dP / dS / dQ / dK products; one extra elementwise pass with the
identity rule), so the aim, reported and not gated, is ``ratio_to_chain <= 1.0``; two thirds of the qkv dgrad GEMM multiply the
zeros of dQ and dK (a V-slice plan would skip them).  The one condition (exit status 1 otherwise): LRP takes less than twice its
comparison in both precisions, and its relevance is finite.  The methods are alternated and each figure is the median of 3 timed
calls after one warm-up of each.  Times come from device events."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xai-audio-deepfakes_amd"))
import torch  # noqa: E402

from addvisor_hip import synthetic as syn  # noqa: E402
from addvisor_hip.attribution import HipAttribution  # noqa: E402
from addvisor_hip.embedder import HipEmbedder  # noqa: E402

torch.set_grad_enabled(False)
B, L, REPS = 16, 64000, 3
dev = torch.device("cuda:0")
cfg = syn.base_config()
sd = syn.embedder_weights(cfg)
coef, icpt = syn.logreg_weights(cfg.hidden_size)
w = syn.make_clips(B, L).to(dev)


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3


def run(precision):
    emb = HipEmbedder(cfg, sd, coef, icpt, dev, precision=precision)
    att = HipAttribution(emb)
    eg = att.eg
    nl, heads, H = emb.nl, cfg.num_attention_heads, cfg.hidden_size
    eg.forward(w)
    eg.backward(att.loss_scale, to_layer=0)                  # leaves gradients in the chain's buffers for the timed launches
    ws = eg._workspace(B, L)
    T, M = ws["f"]["T"], ws["f"]["M"]
    st = torch.cuda.current_stream().cuda_stream
    ln = emb.ln1[0]
    scratch = torch.empty_like(ws["dI"])

    def all_layers(fn):
        for l in range(nl):
            fn(l)

    def gelu_identity(l):
        scratch.copy_(ws["dI"])                              # the multiply runs in place: keep the chain's buffer as it is
        eg._gelu_identity_bwd(scratch, ws["g1"][l], st)

    methods = {"chain_to_layer_0": lambda: att.layer_gradient_x_activation(w, 0),
               "transformer_lrp": lambda: att.transformer_lrp(w),
               "transformer_lrp_identity": lambda: att.transformer_lrp(w, gelu_rule="identity"),
               "attention_bwd_value": lambda: all_layers(lambda l: eg._att_bwd_value(ws["qkv"][l], ws["dctx"], ws["dqkv"], B, T, H, heads, st)),
               "attention_bwd": lambda: all_layers(lambda l: eg._att_bwd(ws["qkv"][l], ws["dctx"], ws["dqkv"], B, T, H, heads, st)),
               "layernorm_bwd_frozen": lambda: all_layers(lambda l: eg._ln_bwd_frozen(ln, ws["x"][l], ws["t16"], M, out_f=ws["db"], out_h=ws["d16"],
                                                                                      add=ws["da"])),
               "layernorm_bwd": lambda: all_layers(lambda l: eg._ln_bwd(ln, ws["x"][l], ws["t16"], M, out_f=ws["db"], out_h=ws["d16"], add=ws["da"])),
               "gelu_identity_bwd_and_copy": lambda: all_layers(gelu_identity),
               "copy": lambda: all_layers(lambda l: scratch.copy_(ws["dI"]))}
    for fn in methods.values():
        once(fn)
    ts = {k: [] for k in methods}
    for _ in range(REPS):
        for k, fn in methods.items():
            ts[k].append(once(fn))
    med = {k: statistics.median(v) for k, v in ts.items()}
    out = {"T": T, "layers": nl}
    for k in ("chain_to_layer_0", "transformer_lrp", "transformer_lrp_identity"):
        out[k] = {"ms_per_call": round(1e3 * med[k], 3), "clips_per_s": round(B / med[k], 1), "spread": round((max(ts[k]) - min(ts[k])) / med[k], 4)}
    for k in ("transformer_lrp", "transformer_lrp_identity"):
        out[k]["ratio_to_chain"] = round(med[k] / med["chain_to_layer_0"], 4)
        out[k]["aim_met"] = med[k] <= med["chain_to_layer_0"]
    d = H // heads
    out["attention_bwd_value"] = {"ms_per_layer": round(1e3 * med["attention_bwd_value"] / nl, 4),
                                  "replaces_ms_per_layer": round(1e3 * med["attention_bwd"] / nl, 4),
                                  "tflops": round(3 * 2.0 * B * heads * T * T * d * nl / med["attention_bwd_value"] / 1e12, 2)}   # S twice, dV once
    out["layernorm_bwd_frozen"] = {"ms_per_launch": round(1e3 * med["layernorm_bwd_frozen"] / nl, 4),
                                   "replaces_ms_per_launch": round(1e3 * med["layernorm_bwd"] / nl, 4), "launches_per_layer": 2}
    out["gelu_identity_bwd"] = {"ms_per_layer": round(1e3 * max(med["gelu_identity_bwd_and_copy"] - med["copy"], 0.0) / nl, 4)}
    worst = max(med["transformer_lrp"], med["transformer_lrp_identity"])
    out["under_twice_the_chain"] = worst < 2.0 * med["chain_to_layer_0"]
    out["finite"] = bool(torch.isfinite(att.transformer_lrp(w, gelu_rule="identity")).all().item())
    return out


res = {"workload": f"wav2vec2-base shape, {B} clips x 4 s, transformer_lrp next to layer_gradient_x_activation(w, 0)", "aim_ratio_to_chain": 1.0}
for precision in ("f32", "f16"):
    res[precision] = run(precision)
print(json.dumps(res))
sys.exit(0 if all(res[p]["under_twice_the_chain"] and res[p]["finite"] for p in ("f32", "f16")) else 1)
