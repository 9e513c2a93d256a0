#!/usr/bin/env python3
"""Attention rollout and gradient-weighted rollout next to the chains they ride on, in one process: wav2vec2-base shape,
fp32-class chain, 16 clips x 4 s (T = 199).
  - ``attention_rollout`` next to ``EmbedderGrad.forward`` over the same clips: the forward plus, per layer, one launch of
    advh_attention_maps (probabilities, heads fused) and one advh_rollout_step;
  - ``attention_grad_rollout`` next to ``layer_gradient_x_activation(w, 0)``: the same forward plus a backward to layer 0 -- the
    chain without the maps -- against the chain that writes every layer's gradient-weighted map on its way, then rolls them out.
Also reported: the time per layer of the maps launch (probabilities and gradient-weighted, heads fused by the mean) and of the
rollout step, timed alone, with the rate the maps launch reaches on its two T x T x d products per head.  The one condition (exit
status 1 otherwise): the gradient rollout takes less than twice its chain.  The aim, reported and not gated: the gradient rollout
runs at >= 0.90 of the chain's rate; ``over_chain_ms`` and the per-launch figures say where the rest goes.  The methods are
alternated and each figure is the median of 3 timed calls after one warm-up of each.  Times come from device events."""
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
emb = HipEmbedder(cfg, sd, coef, icpt, dev, precision="f32")
att = HipAttribution(emb)
eg = att.eg
w = syn.make_clips(B, L).to(dev)
nl, heads, H = emb.nl, cfg.num_attention_heads, cfg.hidden_size


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3


eg.forward(w)
eg.backward(att.loss_scale, to_layer=0)                      # leaves a gradient at the attention context for the timed launch
ws = eg._workspace(B, L)
T = ws["f"]["T"]
st = torch.cuda.current_stream().cuda_stream
fused = torch.empty((B, T, T), dtype=torch.float32, device=dev)
X = torch.rand((B, T, T), dtype=torch.float32, device=dev) / T
Y = torch.empty_like(X)


def all_layers(fn):
    for l in range(nl):
        fn(l)


methods = {"forward": lambda: eg.forward(w),
           "attention_rollout": lambda: att.attention_rollout(w),
           "chain_to_layer_0": lambda: att.layer_gradient_x_activation(w, 0),
           "attention_grad_rollout": lambda: att.attention_grad_rollout(w),
           "maps_probabilities": lambda: all_layers(lambda l: eg._att_maps(ws["qkv"][l], None, fused, 1, 1.0, B, T, H, heads, st)),
           "maps_gradient": lambda: all_layers(lambda l: eg._att_maps(ws["qkv"][l], ws["dctx"], fused, 1, 1.0 / att.loss_scale, B, T, H,
                                                                      heads, st)),
           "rollout_step": lambda: all_layers(lambda l: att._rollout_step(fused, X, Y, 1.0, 1.0, 1.0, False))}
for fn in methods.values():
    once(fn)
ts = {k: [] for k in methods}
for _ in range(REPS):
    for k, fn in methods.items():
        ts[k].append(once(fn))
med = {k: statistics.median(v) for k, v in ts.items()}
d = H // heads
product_flop = 2.0 * B * heads * T * T * d                   # one T x T x d product over every head and clip
out = {"workload": f"wav2vec2-base shape, fp32-class chain, {B} clips x 4 s (T = {T}), {nl} layers"}
for k in ("forward", "attention_rollout", "chain_to_layer_0", "attention_grad_rollout"):
    out[k] = {"ms_per_call": round(1e3 * med[k], 3), "clips_per_s": round(B / med[k], 1),
              "spread": round((max(ts[k]) - min(ts[k])) / med[k], 4)}
for k, products in (("maps_probabilities", 1), ("maps_gradient", 2)):
    out[k] = {"ms_per_layer": round(1e3 * med[k] / nl, 4), "gflop_per_layer": round(products * product_flop / 1e9, 3),
              "tflops": round(products * product_flop * nl / med[k] / 1e12, 2)}
out["rollout_step"] = {"ms_per_layer": round(1e3 * med["rollout_step"] / nl, 4),
                       "tflops": round(2.0 * B * T ** 3 * nl / med["rollout_step"] / 1e12, 2)}
out["attention_rollout"]["rate_over_forward"] = round(med["forward"] / med["attention_rollout"], 4)
ratio = med["chain_to_layer_0"] / med["attention_grad_rollout"]
out["attention_grad_rollout"].update(rate_over_chain=round(ratio, 4), aim=0.90, aim_met=ratio >= 0.90,
                                     over_chain_ms=round(1e3 * (med["attention_grad_rollout"] - med["chain_to_layer_0"]), 3),
                                     maps_ms=round(1e3 * med["maps_gradient"], 3), rollout_steps_ms=round(1e3 * med["rollout_step"], 3))
out["under_twice_the_chain"] = med["attention_grad_rollout"] < 2.0 * med["chain_to_layer_0"]
out["finite"] = bool(torch.isfinite(att.attention_grad_rollout(w)).all().item() and torch.isfinite(att.attention_rollout(w)).all().item())
print(json.dumps(out))
sys.exit(0 if out["under_twice_the_chain"] and out["finite"] else 1)
