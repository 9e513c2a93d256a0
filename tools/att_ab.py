"""A/B of two builds of the library on the forward attention (csrc/attention.hip): are the outputs the same words, and is one slower?

    python tools/att_ab.py --old LIB --new LIB [--mode bits|time|both] [--rounds 5]

bits: every case of tests/attention_kernel_cases.ATT_CASES on the tests' seeded inputs, once per library; the outputs are compared as
      int16 words (both planes for the split entry).
time: four shapes, 20 launches each after 3 warm-ups, old and new alternating over --rounds rounds; median and range per library and
      shape, and the largest |old - new| of a round.  Run it with the same library on both sides first: that gives the spread of
      the machine at that hour, which is what a difference between two builds has to exceed.

The exit status is 1 if bits mode found a differing word and 0 otherwise; time mode only prints, it passes no judgement.

Every measurement runs in a child process of its own (the library is chosen at import through ADDVISOR_HIP_LIB), one at a time,
each under a timeout; the first child that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "xai-audio-deepfakes_amd"), os.path.join(ROOT, "tests")]

# (entry, B, T, heads, dm): the pipeline's shape (wav2vec2-base, 192 clips of 4 s) and the reference's own embedder (XLS-R-2B:
# head dim 120, which the split entry streams in key blocks)
TIME_SHAPES = [("split", 192, 199, 12, 64), ("f16", 192, 199, 12, 64), ("split", 64, 199, 16, 120), ("f16", 64, 199, 16, 120)]
WARMUP, LAUNCHES = 3, 20
CHILD_TIMEOUT = {"bits": 300, "time": 180}       # seconds


# ------------------------------------------------------------------------------------------------------------------ children
def operands(vals, entry, dev):
    """(qkv, ctx) on the device for float64 rows [B*T, 3H]: fp16, or the two planes of the split format."""
    import torch
    from addvisor_hip import gemm as G
    qkv = (vals.half() if entry == "f16" else G.split_planes(vals)).to(dev)
    return qkv, torch.zeros(qkv.shape[:-1] + (vals.shape[1] // 3,), dtype=torch.float16, device=dev)


def launch(entry, qkv, ctx, B, T, H, heads):
    import torch
    from addvisor_hip import _lib
    st = torch.cuda.current_stream().cuda_stream
    if entry == "f16":
        rc = _lib.lib().advh_attention_f16(qkv.data_ptr(), ctx.data_ptr(), B, T, H, heads, st)
    else:
        rc = _lib.lib().advh_attention_split(qkv.data_ptr(), qkv.stride(0), ctx.data_ptr(), ctx.stride(0), B, T, H, heads, st)
    _lib.check(rc, f"attention {entry}")


def child_bits(out_path):
    import torch
    import attention_kernel_cases as K
    from addvisor_hip import _lib
    _lib.init()
    dev, outs = torch.device("cuda:0"), {}
    for c in K.ATT_CASES:
        entry, T, heads, dm, B = c
        qkv, ctx = operands(K.inputs("random", entry, T, heads, dm, B), entry, dev)
        launch(entry, qkv, ctx, B, T, heads * dm, heads)
        torch.cuda.synchronize()
        outs[K.att_id(c)] = ctx.cpu().view(torch.int16)
    torch.save(outs, out_path)


def child_time(out_path):
    import torch
    from addvisor_hip import _lib
    _lib.init()
    dev, us = torch.device("cuda:0"), []
    for entry, B, T, heads, dm in TIME_SHAPES:
        H = heads * dm
        g = torch.Generator().manual_seed(B * T + dm)
        qkv, ctx = operands(torch.randn(B * T, 3 * H, generator=g), entry, dev)
        for _ in range(WARMUP):
            launch(entry, qkv, ctx, B, T, H, heads)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            launch(entry, qkv, ctx, B, T, H, heads)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
        del qkv, ctx
    with open(out_path, "w") as f:
        json.dump(us, f)


# -------------------------------------------------------------------------------------------------------------------- parent
def run_child(mode, lib, out_path):
    """One child with the GPU open; anything but a clean exit ends the whole run, and nothing is started after it."""
    env = dict(os.environ, ADDVISOR_HIP_LIB=os.path.abspath(lib))
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--out", out_path], env=env,
                            timeout=CHILD_TIMEOUT[mode]).returncode
    except subprocess.TimeoutExpired:
        sys.exit(f"att_ab: the {mode} child on {lib} did not finish within {CHILD_TIMEOUT[mode]} s; stopping")
    if rc != 0:
        sys.exit(f"att_ab: the {mode} child on {lib} exited with {rc}; stopping")


def bits(old, new, tmp):
    import torch
    paths = [os.path.join(tmp, f"bits_{i}.pt") for i in range(2)]
    for lib, path in zip((old, new), paths):
        run_child("bits", lib, path)
    a, b = (torch.load(p) for p in paths)
    assert set(a) == set(b)
    differing = {k: int((a[k] != b[k]).sum()) for k in a if not torch.equal(a[k], b[k])}
    for k, n in differing.items():
        print(f"bits: {k}: {n} of {a[k].numel()} words differ")
    print(f"bits: {len(a) - len(differing)} of {len(a)} cases identical word for word")
    return not differing


def timing(old, new, rounds, tmp):
    us = {"old": [], "new": []}                                            # per library: [round][shape]
    for r in range(rounds):
        for tag, lib in (("old", old), ("new", new)):
            path = os.path.join(tmp, f"time_{tag}_{r}.json")
            run_child("time", lib, path)
            with open(path) as f:
                us[tag].append(json.load(f))
    for i, (entry, B, T, heads, dm) in enumerate(TIME_SHAPES):
        print(f"time: {entry:5s} {B} x {T} x {heads} x {dm}  ({LAUNCHES} launches, {rounds} rounds, us per launch)")
        for tag in ("old", "new"):
            v = [rnd[i] for rnd in us[tag]]
            print(f"time:   {tag}  median {statistics.median(v):8.1f}   range {min(v):8.1f} .. {max(v):8.1f}")
        med = statistics.median(rnd[i] for rnd in us["new"]) - statistics.median(rnd[i] for rnd in us["old"])
        worst = max(abs(n[i] - o[i]) for o, n in zip(us["old"], us["new"]))
        print(f"time:   new - old: medians {med:+8.1f}   largest |difference| of a round {worst:8.1f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", help="library of the build to compare against")
    ap.add_argument("--new", help="library of the build under test")
    ap.add_argument("--mode", choices=("bits", "time", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of old and new in timing mode (at least 5)")
    ap.add_argument("--child", choices=("bits", "time"), help=argparse.SUPPRESS)
    ap.add_argument("--out", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return {"bits": child_bits, "time": child_time}[a.child](a.out)
    if not a.old or not a.new:
        ap.error("--old and --new are required")
    for lib in (a.old, a.new):
        if not os.path.exists(lib):
            ap.error(f"{lib} does not exist")
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    same = True
    with tempfile.TemporaryDirectory() as tmp:
        if a.mode in ("bits", "both"):
            same = bits(a.old, a.new, tmp)
        if a.mode in ("time", "both"):
            timing(a.old, a.new, a.rounds, tmp)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
