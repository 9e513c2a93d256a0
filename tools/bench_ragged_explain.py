"""Ragged explanations: what per-clip lengths cost against the padded ``explain``, and what they save against one call per clip.

    python tools/bench_ragged_explain.py [--model base] [--precision f32] [--clips 64] [--length 64000] [--rounds 10] [--warmup 2]

Workload: ``--clips`` clips in a buffer of ``--length`` samples (4 s), the seeded lengths of tools/bench_ragged.py (eight values
between a quarter of the buffer and the buffer, mean 2.6 s at the defaults), wav2vec2-base shape, the default synthetic U-Net.
Three things are timed; the first two alternate round by round so that clock and host drift hit both alike, the third has a
window of its own:

  padded      ``explain(waves)``: every clip explained together with its padding (what the library offered before);
  ragged      ``explain(waves, lengths=...)``: every clip as it is alone;
  per_clip    one warmed-up batch-1 ``explain`` per clip on a pipeline of the clip's own length, sharing the embedder and the
              U-Net (the only correct way before): workspaces and plans per distinct length are built before the timed window.

``tail`` is the summed device time of one ragged call's tail launches (advh_fmap_clip_tail after every producer, the three
advh_zero_tail_cols_f32), replayed alone between two events: what the ragged U-Net pays over the padded one.

Each figure is the median over the rounds of a host clock around work that ends in a device synchronise; min and max are printed
with it.  One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("base", "tiny"), default="base")
    ap.add_argument("--precision", choices=("f32", "f16"), default="f32")
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--length", type=int, default=64000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xai-audio-deepfakes_amd"))
    import numpy as np
    import torch
    from addvisor_hip import _lib, pipeline as P, synthetic as syn
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged_explain needs a GPU: a time from anything else says nothing")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    cfg = syn.base_config() if args.model == "base" else syn.tiny_config(False)
    coef, icpt = syn.logreg_weights(cfg.hidden_size)
    B, L = args.clips, args.length
    pipe = P.ExplainPipeline(cfg, syn.embedder_weights(cfg), coef, icpt, syn.unet_weights(), dev, audio_length=L, sampling_rate=1,
                             precision=args.precision)
    values = [int(v) for v in np.linspace(L // 4, L, 8)]
    lengths = np.random.Generator(np.random.PCG64(args.seed)).choice(values, size=B).tolist()
    waves = syn.make_clips(B, L).to(dev)
    singles = [waves[b:b + 1, :n].contiguous() for b, n in enumerate(lengths)]
    alone = {n: P.ExplainPipeline(None, None, None, None, None, dev, audio_length=n, sampling_rate=1, precision=args.precision,
                                  embedder=pipe.embedder, unet=pipe.unet) for n in set(lengths)}

    def padded():
        pipe.explain(waves)

    def ragged():
        pipe.explain(waves, lengths=lengths)

    def per_clip():
        for w, n in zip(singles, lengths):
            alone[n].explain(w)

    windows = [{"padded": padded, "ragged": ragged}, {"per_clip": per_clip}]
    times = {}
    for runs in windows:
        for fn in runs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times.update({k: [] for k in runs})
        for _ in range(args.rounds):
            for k, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)

    # the tail launches of one ragged call, alone (they only store, so a replay leaves the maps as the call left them)
    unet = pipe.unet
    T = 1 + L // pipe.hop
    W = 4 * (T // 4)
    _, widths = pipe.frame_counts(lengths)
    ws = unet._workspace(B, 512, W, ragged=True)
    wd = torch.tensor(widths, dtype=torch.int32).to(dev)
    tail_maps = unet.tail_maps(ws, W)                      # the maps the forward itself clears, in its launch order
    plane = torch.empty(B, 512, W, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def tails():
        lib = _lib.lib()
        for p in (plane, ws["mask"], ws["logits"]):            # the private copy of |X|, then the two output planes
            lib.advh_zero_tail_cols_f32(p.data_ptr(), wd.data_ptr(), B, 512, W, st)
        for f, shift, ind in tail_maps.values():
            unet._clip_tail(f, shift, ind, wd.data_ptr(), st)
        return 3 + len(tail_maps)

    tail_ms, launches = [], 0
    for i in range(args.warmup + args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launches = tails()
        e1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            tail_ms.append(e0.elapsed_time(e1))
    times["tail"] = tail_ms

    out = {"model": args.model, "precision": args.precision, "clips": B, "length": L, "rounds": args.rounds,
           "mean_length": sum(lengths) / B, "distinct_lengths": len(set(lengths)), "tail_launches": launches}
    for k, v in times.items():
        out[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        print(f"{k:9s} median {statistics.median(v):9.3f} ms   min {min(v):9.3f}   max {max(v):9.3f}", flush=True)
    out["ragged_over_padded"] = round(out["ragged_ms"]["median"] / out["padded_ms"]["median"], 4)
    out["per_clip_over_ragged"] = round(out["per_clip_ms"]["median"] / out["ragged_ms"]["median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
