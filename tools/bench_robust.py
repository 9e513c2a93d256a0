#!/usr/bin/env python3
"""Captum's PGD and the FGSM epsilon ladder next to the work they wrap, in one process: wav2vec2-large (BASELINE config 5's shape),
fp32-class chain, 16 clips x 4 s.
  - PGD Linf, 10 steps (radius 2e-3, step 5e-4, default loss): against ``saliency`` over the same 160 rows (16 clips x 10) in one
    call -- the same forward + backward per row, so the ratio (plain time / attack time) is what the attack's own kernels, its
    loss seed and ten dependent passes of 16 rows in place of one pass of 160 cost -- and (``sequential``) against ten calls of
    ``saliency`` over the 16 clips, which separates the batch-size effect from the attack's own work;
  - ``fgsm_min_epsilon`` with a ladder of K = 16 epsilons, internal_batch_size = 256: against the plain forward over the same 256
    ladder rows; the attack adds one forward + backward over the 16 clips, the ladder kernel and the fold.
Each timed run repeats the call until it holds about 2 s of work; the two sides are alternated (plain, attack, ...) and each
figure is the median of 3 timed runs after one warm-up of each.  Times come from device events."""
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
from addvisor_hip.robust import HipRobust  # noqa: E402

torch.set_grad_enabled(False)
B, L, STEPS, K, REPS, RUN_S = 16, 64000, 10, 16, 3, 2.0
dev = torch.device("cuda:0")
cfg = syn.large_config()
sd = syn.embedder_weights(cfg)
coef, icpt = syn.logreg_weights(cfg.hidden_size)
att = HipAttribution(HipEmbedder(cfg, sd, coef, icpt, dev, precision="f32"))
rob = HipRobust(att)
w = syn.make_clips(B, L).to(dev)
tgt = torch.arange(B) % 2


def once(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3


def compare(plain, attack):
    """Warm-up of each, then calls per run for ~RUN_S s, then REPS alternated runs of each side."""
    once(plain), once(attack)
    n = max(1, round(RUN_S / once(plain)))
    ts = {"plain": [], "attack": []}
    for _ in range(REPS):
        for side, fn in (("plain", plain), ("attack", attack)):
            ts[side].append(once(lambda: [fn() for _ in range(n)]) / n)
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {"calls_per_run": n, "plain_s": round(med["plain"], 5), "attack_s": round(med["attack"], 5),
            "ratio": round(med["plain"] / med["attack"], 4),
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ts.items()}}


out = {"workload": f"wav2vec2-large shape, fp32-class chain, {B} clips x 4 s"}
rows = w.repeat(STEPS, 1)
r = compare(lambda: att.saliency(rows), lambda: rob.pgd(w, 2e-3, 5e-4, STEPS, tgt))
out["pgd_linf"] = {"steps": STEPS, "clip_steps_per_s": round(B * STEPS / r["attack_s"], 1), **r}
out["pgd_linf"]["sequential"] = compare(lambda: [att.saliency(w) for _ in range(STEPS)], lambda: rob.pgd(w, 2e-3, 5e-4, STEPS, tgt))
eps = [2.5e-4 * (k + 1) for k in range(K)]
ladder = w.repeat_interleave(K, 0)
r = compare(lambda: att.logits(ladder), lambda: rob.fgsm_min_epsilon(w, eps, tgt, internal_batch_size=B * K))
out["fgsm_min_epsilon"] = {"K": K, "ladder_rows_per_s": round(B * K / r["attack_s"], 1), **r}
adv = rob.pgd(w, 2e-3, 5e-4, 2, tgt, norm="L2", random_start=True, seed=1)
out["finite"] = bool(torch.isfinite(adv).all().item())
print(json.dumps(out))
