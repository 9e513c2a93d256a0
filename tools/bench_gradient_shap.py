#!/usr/bin/env python3
"""Path points per second of the baseline-aware attributions next to zero-baseline IntegratedGradients, in one process:
wav2vec2-large, 16 clips x 4 s, internal batch 160, fp32-class chain; 800 path points per attribution (IG 50 steps,
GradientShap 50 samples).  Each figure is the median of 3 timed runs after a warm-up of the same call."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xai-audio-deepfakes_amd"))
import torch
from addvisor_hip import synthetic as syn
from addvisor_hip.attribution import HipAttribution
from addvisor_hip.embedder import HipEmbedder
torch.set_grad_enabled(False)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
chunk = int(sys.argv[2]) if len(sys.argv) > 2 else 160
which = sys.argv[3] if len(sys.argv) > 3 else "large"
dev = torch.device("cuda:0")
cfg = syn.large_config() if which == "large" else syn.base_config()
sd = syn.embedder_weights(cfg)
coef, icpt = syn.logreg_weights(cfg.hidden_size)
att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev))
w = syn.make_clips(B, 64000).to(dev)
g = torch.Generator().manual_seed(0)
noise_base = (0.05 * torch.randn(B, 64000, generator=g)).to(dev)
dist = (0.05 * torch.randn(8, 64000, generator=g)).to(dev)
variants = {
    "ig_zero_baseline": lambda: att.integrated_gradients(w, n_steps=50, internal_batch_size=chunk),
    "ig_noise_baseline": lambda: att.integrated_gradients(w, n_steps=50, internal_batch_size=chunk, baselines=noise_base),
    "gradient_shap_stdevs0": lambda: att.gradient_shap(w, dist, n_samples=50, stdevs=0.0, seed=1, internal_batch_size=chunk),
    "gradient_shap_stdevs0.1": lambda: att.gradient_shap(w, dist, n_samples=50, stdevs=0.1, seed=1, internal_batch_size=chunk),
}
res, finite = {}, True
for name, fn in variants.items():
    fn()                                                       # warm-up: the chunk-shaped workspace, code objects
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    finite &= bool(torch.isfinite(out).all().item())
    res[name] = round(50 * B / statistics.median(ts), 1)
ref = res["ig_zero_baseline"]
print(json.dumps({"workload": f"attribution path points/s, wav2vec2-{which}, {B} clips x 4 s, 800 points, internal batch {chunk}, f32",
                  "path_points_per_s": res, "ratio_to_zero_baseline_ig": {k: round(v / ref, 4) for k, v in res.items()},
                  "finite": finite}))
