#!/usr/bin/env python3
"""NoiseTunnel's throughput next to the wrapped method over the same expanded rows, in one process: wav2vec2-large (BASELINE
config 5's shape), fp32-class chain, 16 clips x 4 s.
  - NoiseTunnel(Saliency), nt_samples = 10: 160 noisy rows, against ``saliency`` over the 160 ``repeat_interleave``d clips;
  - NoiseTunnel(IntegratedGradients), nt_samples = 5, n_steps = 10, internal_batch_size = 160: 80 noisy clips x 10 steps,
    against IntegratedGradients over the 80 expanded clips with the same arguments.
The ratio (plain time / tunnel time) is what the noisy-row and fold / finalize kernels and the host loop cost.  Each timed run
repeats the call until it holds about 2 s of work; the two sides are alternated (plain, tunnel, ...) and each figure is the median
of 3 timed runs after one warm-up of each.  Times come from device events."""
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
B, L, REPS, RUN_S = 16, 64000, 3, 2.0
dev = torch.device("cuda:0")
cfg = syn.large_config()
sd = syn.embedder_weights(cfg)
coef, icpt = syn.logreg_weights(cfg.hidden_size)
att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision="f32"))
w = syn.make_clips(B, L).to(dev)


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3


def compare(plain, tunnel):
    """Warm-up of each, then calls per run for ~RUN_S s, then REPS alternated runs of each side."""
    once(plain), once(tunnel)
    n = max(1, round(RUN_S / once(plain)))
    ts = {"plain": [], "tunnel": []}
    for _ in range(REPS):
        for side, fn in (("plain", plain), ("tunnel", tunnel)):
            ts[side].append(once(lambda: [fn() for _ in range(n)]) / n)
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {"calls_per_run": n, "plain_s": round(med["plain"], 5), "tunnel_s": round(med["tunnel"], 5),
            "ratio": round(med["plain"] / med["tunnel"], 4),
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ts.items()}}


out = {"workload": f"wav2vec2-large shape, fp32-class chain, {B} clips x 4 s"}
S = 10
rows = w.repeat_interleave(S, 0)
r = compare(lambda: att.saliency(rows), lambda: att.noise_tunnel(w, att.saliency, "smoothgrad", S, None, 0.01, seed=1))
out["saliency"] = {"nt_samples": S, "rows": B * S, "rows_per_s": round(B * S / r["tunnel_s"], 1), **r}
S = 5
clips = w.repeat_interleave(S, 0)
kw = dict(n_steps=10, internal_batch_size=160)
r = compare(lambda: att.integrated_gradients(clips, **kw),
            lambda: att.noise_tunnel(w, att.integrated_gradients, "smoothgrad", S, None, 0.01, seed=1, **kw))
out["integrated_gradients"] = {"nt_samples": S, "n_steps": 10, "internal_batch_size": 160, "path_points": B * S * 10,
                               "path_points_per_s": round(B * S * 10 / r["tunnel_s"], 1), **r}
out["finite"] = bool(torch.isfinite(att.noise_tunnel(w, att.saliency, "vargrad", 2, None, 0.01, seed=2)).all().item())
print(json.dumps(out))
