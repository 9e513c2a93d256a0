#!/usr/bin/env python3
"""NeuronIntegratedGradients' throughput next to the input-space IntegratedGradients over the same clips, in one process:
wav2vec2-base shape, fp32-class chain, 16 clips x 4 s, 50 Gauss-Legendre steps (800 path points, 128 per chunk), a noise
baseline for both methods (so that both run the baseline-aware path of csrc/attribution_paths.hip).
  - ``integrated_gradients``: every path point runs the whole chain, forward and backward;
  - ``neuron_integrated_gradients`` at l = nl, l = 6 and l = 0 (one unit, ``(7, 5)``): every path point runs the chain BELOW the
    layer only -- the waveform kernels, the feature encoder, the positional convolution and layers 0 .. l-1, forward and
    backward, plus one seed kernel; no layer >= l, no pooling, no logreg.
Reported per method: seconds per call, path points per second, the time per path point and the run-to-run spread
((max - min) / median of the timed calls); next to them the FLOP-proportional prediction,
``(HipEmbedder.flops - HipEmbedder.flops_from(l)) / HipEmbedder.flops`` from the plans' own FLOP counts -- the time per path
point the truncated chain would take if time followed the forward's algorithmic FLOPs -- and its distance to the measurement
(reported, not gated).  Two conditions (exit status 1 otherwise): a path point at l = nl takes no longer than a path point of
``integrated_gradients`` beyond the larger of the two spreads (it launches a subset of the same kernels plus one seed kernel),
and the time per path point falls as l falls.  The methods are alternated and each figure is the median of 3 timed calls after
one warm-up of each.  Times come from device events."""
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
B, L, STEPS, REPS, NEURON = 16, 64000, 50, 3, (7, 5)
if not torch.cuda.is_available():
    sys.exit("bench_neuron_attr.py measures on a GPU; none is available")
dev = torch.device("cuda:0")
cfg = syn.base_config()
sd = syn.embedder_weights(cfg)
coef, icpt = syn.logreg_weights(cfg.hidden_size)
emb = HipEmbedder(cfg, sd, coef, icpt, dev, precision="f32")
att = HipAttribution(emb)
nl = emb.nl
w = syn.make_clips(B, L).to(dev)
base = (0.05 * torch.randn(B, L, generator=torch.Generator().manual_seed(3))).to(dev)


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3


layers = (nl, 6, 0)
methods = {"integrated_gradients": lambda: att.integrated_gradients(w, n_steps=STEPS, baselines=base)}
for l in layers:
    methods[f"neuron_ig_l{l}"] = lambda l=l: att.neuron_integrated_gradients(w, l, NEURON, baselines=base, n_steps=STEPS)
for fn in methods.values():
    once(fn)
ts = {k: [] for k in methods}
for _ in range(REPS):
    for k, fn in methods.items():
        ts[k].append(once(fn))
points = B * STEPS
full = emb.flops(B, L)
out = {"workload": f"wav2vec2-base shape, fp32-class chain, {B} clips x 4 s, {STEPS} steps ({points} path points), nl = {nl}, "
                   f"neuron {NEURON}, neuron_loss_scale {att.neuron_loss_scale:g}",
       "forward_gflop_per_clip": round(full / B / 1e9, 2)}
med = {k: statistics.median(v) for k, v in ts.items()}
spread = {k: (max(v) - min(v)) / med[k] for k, v in ts.items()}
for k, v in ts.items():
    out[k] = {"s_per_call": round(med[k], 4), "path_points_per_s": round(points / med[k], 1),
              "ms_per_path_point": round(1e3 * med[k] / points, 4), "spread": round(spread[k], 4)}
for l in layers:
    k = f"neuron_ig_l{l}"
    share = (full - emb.flops_from(B, L, l)) / full
    pred = share * med["integrated_gradients"]
    out[k].update(layer=l, flop_share=round(share, 4), predicted_ms_per_path_point=round(1e3 * pred / points, 4),
                  measured_over_predicted=round(med[k] / pred, 3), speedup_over_full_ig=round(med["integrated_gradients"] / med[k], 3))
top = f"neuron_ig_l{nl}"
out["top_no_slower_than_ig"] = med[top] <= med["integrated_gradients"] * (1 + max(spread[top], spread["integrated_gradients"]))
out["falls_with_layer"] = med[top] > med["neuron_ig_l6"] > med["neuron_ig_l0"]
out["finite"] = bool(torch.isfinite(att.neuron_integrated_gradients(w, 6, NEURON, baselines=base, n_steps=4)).all().item())
print(json.dumps(out))
sys.exit(0 if out["top_no_slower_than_ig"] and out["falls_with_layer"] and out["finite"] else 1)
