"""Clips longer than 256 frames: what the streamed attention (csrc/attention_long.hip) costs next to the whole-clip kernels.

    python tools/bench_long_clips.py [--precision f32,f16] [--rounds 15] [--warmup 3] [--parts a,b,c]

One MI355X, wav2vec2-base shape.  Every figure is the median over alternating rounds of a host clock around work that ends in a
device synchronise, printed with its min and max (the spread to hold a difference against).  Operands are random, not zeros.

  (a) kernel alone   advh_attention_long_* at T = 499 (10 s), B = 16, 12 heads of 64, next to the existing advh_attention_* at
                     T = 256, same B, same build; each round times --launches back-to-back launches of one, then of the other.
                     Both as (query, key) pairs per second; the yardstick for the ratio long / whole is 1 minus the whole-clip
                     kernel's own (max - min) / median in this run.
  (b) forward        16 clips x 10 s against 40 clips x 4 s (the same number of samples; the 4 s call is the existing path).
                     Predicted 10 s time = the 4 s time + layers x (pairs_long - pairs_short) / the whole-clip kernel's pair rate
                     of (a); reported: measured / predicted, next to the 4 s forward's spread.
  (c) ragged         32 clips in a 12 s buffer, lengths seeded in 2 .. 12 s: forward(wave, lengths=...) against the padded
                     forward(wave) and against one warmed-up batch-1 call per clip, as tools/bench_ragged.py does.
One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import time


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def alternate(runs, rounds, warmup, sync):
    """{name: [ms per round]} of the callables in ``runs``, alternating round by round after ``warmup`` calls of each."""
    for fn in runs.values():
        for _ in range(warmup):
            fn()
    sync()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            sync()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f32,f16")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xai-audio-deepfakes_amd"))
    import numpy as np
    import torch
    from addvisor_hip import _lib, gemm as G, synthetic as syn
    from addvisor_hip.embedder import HipEmbedder
    if not torch.cuda.is_available():
        raise SystemExit("bench_long_clips needs a GPU: a time from anything else says nothing")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    parts = set(args.parts.split(","))
    _lib.init()
    lib = _lib.lib()
    cfg = syn.base_config()
    heads, H, nl = cfg.num_attention_heads, cfg.hidden_size, min(cfg.layer_index, cfg.num_hidden_layers)
    out = {"model": "base", "rounds": args.rounds}

    for precision in args.precision.split(","):
        res = out[precision] = {}
        sp = precision == "f32"
        rate_whole = None
        if "a" in parts or "b" in parts:
            B, T_long, T_whole = 16, 499, 256
            g = torch.Generator().manual_seed(args.seed)

            def operands(T):
                rows = torch.randn(B * T, 3 * H, generator=g) * 1.5
                qkv = (G.split_planes(rows.double()) if sp else rows.half()).to(dev)
                ctx = torch.empty(((2,) if sp else ()) + (B * T, H), dtype=torch.float16, device=dev)
                return qkv, ctx
            (ql, cl), (qw, cw) = operands(T_long), operands(T_whole)
            st = torch.cuda.current_stream().cuda_stream

            def long_():
                for _ in range(args.launches):
                    rc = (lib.advh_attention_long_split(ql.data_ptr(), ql.stride(0), cl.data_ptr(), cl.stride(0), None, B, T_long, H, heads, st)
                          if sp else lib.advh_attention_long_f16(ql.data_ptr(), cl.data_ptr(), None, B, T_long, H, heads, st))
                assert rc == 0

            def whole():
                for _ in range(args.launches):
                    rc = (lib.advh_attention_split(qw.data_ptr(), qw.stride(0), cw.data_ptr(), cw.stride(0), B, T_whole, H, heads, st)
                          if sp else lib.advh_attention_f16(qw.data_ptr(), cw.data_ptr(), B, T_whole, H, heads, st))
                assert rc == 0
            t = alternate({"long": long_, "whole": whole}, args.rounds, args.warmup, sync)
            _lib.check_overflow("bench_long_clips (a)")
            pairs = {"long": B * heads * T_long ** 2, "whole": B * heads * T_whole ** 2}
            a = {k: {"us_per_launch": stat([x * 1e3 / args.launches for x in v]),
                     "gpairs_per_s": round(pairs[k] * args.launches / (statistics.median(v) * 1e-3) / 1e9, 2)} for k, v in t.items()}
            w = a["whole"]["us_per_launch"]
            a["ratio_long_over_whole"] = round(a["long"]["gpairs_per_s"] / a["whole"]["gpairs_per_s"], 4)
            a["aim"] = round(1.0 - (w["max"] - w["min"]) / w["median"], 4)
            rate_whole = pairs["whole"] * args.launches / (statistics.median(t["whole"]) * 1e-3)
            res["kernel"] = a
            print(precision, "(a)", json.dumps(a), flush=True)

        coef, icpt = syn.logreg_weights(cfg.hidden_size)
        emb = HipEmbedder(cfg, syn.embedder_weights(cfg), coef, icpt, dev, precision=precision)
        if "b" in parts:
            w_long, w_short = syn.make_clips(16, 160000).to(dev), syn.make_clips(40, 64000).to(dev)
            t = alternate({"long": lambda: emb.forward(w_long, want_hidden=False), "short": lambda: emb.forward(w_short, want_hidden=False)},
                          args.rounds, args.warmup, sync)
            T_l, T_s = emb._workspace(16, 160000)["T"], emb._workspace(40, 64000)["T"]
            extra = nl * (16 * heads * T_l ** 2 - 40 * heads * T_s ** 2)
            b = {k + "_ms": stat(v) for k, v in t.items()}
            b["frames"] = [T_l, T_s]
            b["predicted_long_ms"] = round(b["short_ms"]["median"] + extra / rate_whole * 1e3, 4)
            b["measured_over_predicted"] = round(b["long_ms"]["median"] / b["predicted_long_ms"], 4)
            b["short_spread"] = round((b["short_ms"]["max"] - b["short_ms"]["min"]) / b["short_ms"]["median"], 4)
            res["forward"] = b
            print(precision, "(b)", json.dumps(b), flush=True)
            del w_long, w_short
        if "c" in parts:
            B, L = 32, 192000
            lengths = np.random.Generator(np.random.PCG64(args.seed)).integers(32000, L + 1, size=B).tolist()
            wave = syn.make_clips(B, L).to(dev)
            singles = [wave[i:i + 1, :n].contiguous() for i, n in enumerate(lengths)]

            def per_clip():
                for s in singles:
                    emb.forward(s, want_hidden=False)
            t = alternate({"padded": lambda: emb.forward(wave, want_hidden=False),
                           "ragged": lambda: emb.forward(wave, lengths=lengths, want_hidden=False)}, args.rounds, args.warmup, sync)
            t.update(alternate({"per_clip": per_clip}, max(3, args.rounds // 3), 1, sync))       # a window of its own, as bench_ragged
            c = {k + "_ms": stat(v) for k, v in t.items()}
            c["mean_length"] = sum(lengths) / B
            c["ragged_over_padded"] = round(c["ragged_ms"]["median"] / c["padded_ms"]["median"], 4)
            c["per_clip_over_ragged"] = round(c["per_clip_ms"]["median"] / c["ragged_ms"]["median"], 4)
            res["ragged"] = c
            print(precision, "(c)", json.dumps(c), flush=True)
            del wave, singles
        del emb
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
