#!/usr/bin/env python3
"""Perturbed rows per second of Lime and FeaturePermutation next to the plain classifier forward over the same number of rows, in
one process: wav2vec2-base shape, fp32-class, 16 clips x 4 s, 40 segments of 1 600 samples, internal batch 128.  Lime with
n_samples = 50 (Captum's default) evaluates 50 * 16 = 800 rows (7 chunks), with n_samples = 256 4 096 rows (32 chunks, the
KernelShap figure of tools/bench_shapley.py), each with its device similarity weights and 16 host Lasso fits; FeaturePermutation
evaluates 40 * 16 = 640 rows (5 chunks) plus the forward of the clips.  The plain figure is ``emb.forward`` on the same number of
128-row chunks, so the ratio is what the row, similarity and accumulate kernels, the host draws and fits, and the logit copies
cost.  Times come from device events around each call (A-B-A: plain, method, plain again); each figure is the median of 3 timed
runs after one warm-up call."""
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
B, L, SEG, CHUNK, REPS = 16, 64000, 1600, 128, 3
K = L // SEG
dev = torch.device("cuda:0")
cfg = syn.base_config()
sd = syn.embedder_weights(cfg)
coef, icpt = syn.logreg_weights(cfg.hidden_size)
emb = HipEmbedder(cfg, sd, coef, icpt, dev, precision="f32")
att = HipAttribution(emb)
w = syn.make_clips(B, L).to(dev)
mask = (torch.arange(L, device=dev) // SEG)[None]
pts = syn.make_clips(CHUNK, L, seed=7).to(dev)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1) / 1e3)
    return statistics.median(ts), ts


def plain(nchunk):
    def run():
        for _ in range(nchunk):
            emb.forward(pts, want_hidden=False)
    return run


out = {"workload": f"wav2vec2-base shape, f32, {B} clips x 4 s, {K} segments of {SEG} samples, internal batch {CHUNK}"}
for name, rows, fn in (
        ("lime_n50", 50 * B, lambda: att.lime(w, feature_mask=mask, n_samples=50, seed=1, internal_batch_size=CHUNK)),
        ("lime_n256", 256 * B, lambda: att.lime(w, feature_mask=mask, n_samples=256, seed=1, internal_batch_size=CHUNK)),
        ("feature_permutation", K * B, lambda: att.feature_permutation(w, feature_mask=mask, seed=1, internal_batch_size=CHUNK))):
    nchunk = -(-rows // CHUNK)
    runs = {}
    for label, f in (("plain_forward", plain(nchunk)), (name, fn), ("plain_forward_again", plain(nchunk))):   # A-B-A
        med, ts = timed(f)
        runs[label] = {"s": round(med, 4), "rows_per_s": round(rows / med, 1), "spread": round((max(ts) - min(ts)) / med, 4)}
    plain_s = min(runs["plain_forward"]["s"], runs["plain_forward_again"]["s"])
    out[name] = {"rows": rows, "chunks": nchunk, "rows_per_s": runs[name]["rows_per_s"],
                 "ratio_to_plain_forward": round(plain_s / runs[name]["s"], 4), "runs": runs,
                 "finite": bool(torch.isfinite(fn()).all().item())}
print(json.dumps(out))
