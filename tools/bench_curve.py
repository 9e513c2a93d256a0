#!/usr/bin/env python3
"""Perturbation curves next to the plain classifier forward over the same number of chunks, in one process: wav2vec2-base
shape, fp32-class, 16 clips x 4 s, internal batch 128.
  (a) ``curve_summary`` over K = 40 segments of 100 ms, S = 20: a deletion and an insertion curve of 21 x 16 = 336 rows each
      (672 rows; 3 chunks per curve, the last one padded: 6 forwards of 128 rows);
  (b) ``perturbation_curve`` (deletion, MoRF) with every sample its own feature, K = 64 000, S = 20: 336 rows, 3 forwards;
  the score + rank launches of (b) on their own (the rank is a counting rank: K^2 = 4.1e9 key comparisons per clip).
The plain figure is ``emb.forward`` on the same number of 128-row chunks, so a ratio is what the score / rank / row / fold
kernels, the padding rows' share aside, and the logit copies cost.  Times come from device events around each call; each figure
is the median of 7 timed runs after two warm-up calls, plain forward before and after (A-B-A)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xai-audio-deepfakes_amd"))
import torch  # noqa: E402

from addvisor_hip import attribution as AT, synthetic as syn  # noqa: E402
from addvisor_hip.attribution import HipAttribution  # noqa: E402
from addvisor_hip.embedder import HipEmbedder  # noqa: E402

torch.set_grad_enabled(False)
B, L, SEG, S, CHUNK, REPS = 16, 64000, 1600, 20, 128, 7
dev = torch.device("cuda:0")
cfg = syn.base_config()
sd = syn.embedder_weights(cfg)
coef, icpt = syn.logreg_weights(cfg.hidden_size)
emb = HipEmbedder(cfg, sd, coef, icpt, dev, precision="f32")
att = HipAttribution(emb)
w = syn.make_clips(B, L).to(dev)
attr = torch.randn(B, L, generator=torch.Generator().manual_seed(3)).to(dev)
mask = (torch.arange(L) // SEG)[None]
K = L // SEG
rows = (S + 1) * B
nchunk = -(-rows // CHUNK)
pts = syn.make_clips(CHUNK, L, seed=7).to(dev)


def plain(n):
    def run():
        for _ in range(n):
            emb.forward(pts, want_hidden=False)
    return run


def summary():
    return att.curve_summary(w, attr, feature_mask=mask, steps=S, internal_batch_size=CHUNK)


def per_sample():
    return att.perturbation_curve(w, attr, steps=S, internal_batch_size=CHUNK)


def score_rank():
    return AT.feature_rank(AT.feature_scores(attr, None, L), True)


def timed(fn):
    for _ in range(2):
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


res = {}
for name, fn in (("plain_6_chunks", plain(2 * nchunk)), ("curve_summary_k40", summary), ("plain_6_chunks_again", plain(2 * nchunk)),
                 ("plain_3_chunks", plain(nchunk)), ("deletion_k64000", per_sample), ("plain_3_chunks_again", plain(nchunk)),
                 ("score_rank_k64000", score_rank)):
    med, ts = timed(fn)
    res[name] = {"s": round(med, 5), "spread": round((max(ts) - min(ts)) / med, 4)}
finite = all(bool(torch.isfinite(v).all().item()) for v in summary().values()) and bool(torch.isfinite(per_sample().curve).all().item())
plain6 = min(res["plain_6_chunks"]["s"], res["plain_6_chunks_again"]["s"])
plain3 = min(res["plain_3_chunks"]["s"], res["plain_3_chunks_again"]["s"])
print(json.dumps({"workload": f"perturbation curves, wav2vec2-base shape, f32, {B} clips x 4 s, S = {S}, internal batch {CHUNK}; "
                              f"(a) curve_summary, K = {K} segments, {2 * rows} rows in {2 * nchunk} chunks; (b) deletion, K = {L} samples, "
                              f"{rows} rows in {nchunk} chunks",
                  "a_rows_per_s": round(2 * rows / res["curve_summary_k40"]["s"], 1),
                  "a_ratio_to_plain_forward": round(plain6 / res["curve_summary_k40"]["s"], 4),
                  "b_ratio_to_plain_forward": round(plain3 / res["deletion_k64000"]["s"], 4),
                  "b_score_rank_share_of_call": round(res["score_rank_k64000"]["s"] / res["deletion_k64000"]["s"], 4),
                  "b_rank_key_comparisons": B * L * L, "runs": res, "finite": finite}))
