#!/usr/bin/env python3
"""Captum's infidelity and sensitivity_max next to the work they wrap, in one process: wav2vec2-large (BASELINE config 5's shape),
fp32-class chain, 16 clips x 4 s, n_perturb_samples = 10 in one chunk.
  - infidelity with NoisyPerturbation (fused rows), internal_batch_size = 160: against the plain forward over the same rows --
    the 160 noisy rows and the 16 clips, as the metric runs them (the rows come from the same Philox noise);
  - sensitivity_max over Saliency (default uniform perturbation): against ``saliency`` over the same 176 rows, in the metric's
    two calls (the 16 clips, then the 160 perturbed rows).
The ratio (plain time / metric time) is what the new kernels and the host loop cost.  Each timed run repeats the call until it
holds about 2 s of work; the two sides are alternated (plain, metric, ...) and each figure is the median of 3 timed runs after
one warm-up of each.  Times come from device events."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xai-audio-deepfakes_amd"))
import torch  # noqa: E402

from addvisor_hip import attribution as AT, synthetic as syn  # noqa: E402
from addvisor_hip.attribution import HipAttribution, NoisyPerturbation  # noqa: E402
from addvisor_hip.embedder import HipEmbedder  # noqa: E402

torch.set_grad_enabled(False)
B, L, S, REPS, RUN_S = 16, 64000, 10, 3, 2.0
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


def compare(plain, metric):
    """Warm-up of each, then calls per run for ~RUN_S s, then REPS alternated runs of each side."""
    once(plain), once(metric)
    n = max(1, round(RUN_S / once(plain)))
    ts = {"plain": [], "metric": []}
    for _ in range(REPS):
        for side, fn in (("plain", plain), ("metric", metric)):
            ts[side].append(once(lambda: [fn() for _ in range(n)]) / n)
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {"calls_per_run": n, "plain_s": round(med["plain"], 5), "metric_s": round(med["metric"], 5),
            "ratio": round(med["plain"] / med["metric"], 4),
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ts.items()}}


out = {"workload": f"wav2vec2-large shape, fp32-class chain, {B} clips x 4 s, n_perturb_samples {S}"}
attr = att.saliency(w)
noisy = NoisyPerturbation(0.01)
rows = torch.empty(B * S, L, dtype=torch.float32, device=dev)
AT.metric_rows(AT.metric_desc(w, 1, S, 0, S, AT.MR_GAUSS, 0.01, attr), 0, B * S, rows, torch.empty(B * S, device=dev))
r = compare(lambda: (att.logits(rows), att.logits(w)),
            lambda: att.infidelity(w, noisy, attr, n_perturb_samples=S, seed=1, internal_batch_size=B * S))
out["infidelity"] = {"rows": B * S, "rows_per_s": round(B * S / r["metric_s"], 1), **r}
urows = AT.uniform_rows(w, 2, S, 0, S, 0.02)
r = compare(lambda: (att.saliency(w), att.saliency(urows)),
            lambda: att.sensitivity_max(att.saliency, w, n_perturb_samples=S, seed=2))
out["sensitivity_max"] = {"explained_rows": B * (S + 1), "rows_per_s": round(B * (S + 1) / r["metric_s"], 1), **r}
out["finite"] = bool(torch.isfinite(att.infidelity(w, noisy, attr, n_perturb_samples=2, normalize=True, seed=3)).all().item())
print(json.dumps(out))
