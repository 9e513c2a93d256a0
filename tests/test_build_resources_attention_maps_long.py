"""CPU-only: the instances compiled from csrc/attention_maps_long.hip are exactly those the dispatch mirror of
tests/attention_maps_long_cases.py selects for the cases of tests/test_gpu_attention_maps_long.py (three statistics, six maps
and three value kernels, and the two rollout kernels), none uses scratch, the LDS formulas of DESIGN 4.35 stay within 160 KiB, the
row-sum bar's numpy-fp32 figure is what the cases file records, the maps cases are within reach of fp32 arithmetic, and the HIP
files that existed before csrc/attention_maps_long.hip, all 42 that remain, still compile to the recorded device assembly
(tests/golden/device_asm_sha256.json)."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import attention_bwd_long_cases as C
import attention_maps_long_cases as M
from test_build_resources import CSRC, ROOT
from test_build_resources_backward import instances, resources

SRC = "attention_maps_long.hip"
INSTANCES = ({(M.STATS_KERNEL, D) for D in (32, 64, 128)} | {(M.VALUE_KERNEL, D) for D in (32, 64, 128)}
             | {(M.MAPS_KERNEL, D, g) for D in (32, 64, 128) for g in (False, True)})
LDS = {(M.STATS_KERNEL, 32): 18432, (M.STATS_KERNEL, 64): 34816, (M.STATS_KERNEL, 128): 67584,
       (M.MAPS_KERNEL, 32, False): 18432, (M.MAPS_KERNEL, 64, False): 34816, (M.MAPS_KERNEL, 128, False): 67584,
       (M.MAPS_KERNEL, 32, True): 36864, (M.MAPS_KERNEL, 64, True): 69632, (M.MAPS_KERNEL, 128, True): 135168,
       (M.VALUE_KERNEL, 32): 37888, (M.VALUE_KERNEL, 64): 70656, (M.VALUE_KERNEL, 128): 136192}      # the instance table of DESIGN 4.35


def test_compiled_instances_are_the_twelve_and_each_has_its_cases():
    compiled = instances(SRC, M.STATS_KERNEL) | instances(SRC, M.MAPS_KERNEL) | instances(SRC, M.VALUE_KERNEL)
    assert compiled == INSTANCES, sorted(map(str, compiled ^ INSTANCES))
    sel = {}
    for c in M.MAPS_CASES:
        for inst in M.instances_of(c[1], c[3]):
            sel.setdefault(inst, []).append(c)
    assert set(sel) == compiled
    for inst, cases in sel.items():
        blocks = {M.blocks(c[1]) for c in cases}
        assert {1, 2, 3} <= blocks and max(blocks) >= 5, (inst, sorted(blocks))          # blocks of the streaming loop / tiles per side
        assert {c[0] for c in cases} == set(M.ENTRIES), inst                             # both operand formats
        assert any(c[3] < inst[1] for c in cases) and all(c[2] == 3 for c in cases), inst   # a padded head dim; an odd head count
        assert {c[1] for c in cases} >= set(M.T_ALL), inst
    assert set(M.T_ALL) == {1, 16, 17, 128, 129, 256, 257, 273, 385, 513}
    assert {d for c in M.MAPS_CASES for d in [c[3]]} == set(M.HEAD_DIMS) and len(M.HEAD_DIMS) == 7
    assert {M.padded(d) for d in M.INSTANCE_DIMS} == {32, 64, 128} and set(M.INSTANCE_DIMS) == {24, 64, 120}
    for shapes in (M.KIND_SHAPES, [c[1:] for c in M.FRAME_CASES]):
        assert {i for s in shapes for i in M.instances_of(s[0], s[2])} == INSTANCES
    assert M.FRAMES == ((513, 1, 257), (513, 256, 273), (513, 17, 129)) and all(c[1] == 513 for c in M.FRAME_CASES)
    assert set(M.ROLLOUT_T) == {1, 17, 64, 65, 257, 513} and M.ROLLOUT_PARAMS == ((1.0, 1.0, 0.0, 1), (1.0, 1.0, 1.0, 0))
    assert all(len(M.ROLLOUT_FRAMES[T]) == 3 and max(M.ROLLOUT_FRAMES[T]) <= T and min(M.ROLLOUT_FRAMES[T]) >= 1 for T in M.ROLLOUT_T)


def test_block_sizes_fit_the_lds_budget():
    for inst, want in LDS.items():
        got = M.lds_stats(inst[1]) if inst[0] == M.STATS_KERNEL else (M.lds_value(inst[1]) if inst[0] == M.VALUE_KERNEL else M.lds_maps(*inst[1:]))
        assert got == want <= 160 * 1024, (inst, got)
    assert M.BLOCK == 128 and M.BLOCK % 16 == 0                                           # eight wavefronts, one 16-row tile each


def test_new_kernels_do_not_spill():
    res = {k: v for k, v in resources(SRC).items() if "_kernel" in k}
    assert len(res) == 14, sorted(res)                                                   # twelve instances and the two rollout kernels
    for k, v in res.items():
        print(k, v)
        assert v["scratch"] == 0, (k, v)
        assert v["occupancy"] >= 2, (k, v)
        assert v["vgprs"] <= 256, (k, v)


def test_the_file_has_no_atomics():
    text = open(os.path.join(CSRC, SRC)).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "atomic" not in code.lower()


@pytest.mark.parametrize("s", [("random", e, T, M.HEADS, dm, M.B) for e in M.ENTRIES for T, dm in ((273, 24), (513, 64), (513, 120))]
                         + [(k, e) + sh for k in ("uniform", "peaked", "ordered") for sh in M.KIND_SHAPES for e in M.ENTRIES], ids=str)
def test_bars_are_within_reach_of_fp32(s):
    """A plain numpy fp32 restatement of the streamed recurrences stays within half the maps bar on these inputs -- P and the
    gradient form -- and its rows of P sum to 1 within the recorded figure, from which the GPU suite takes its row-sum bar."""
    kind, entry, T, heads, dm, B = s
    qkv, dctx = M.maps_inputs(kind, entry, T, heads, dm, B)
    ref = M.maps_reference(kind, entry, T, heads, dm, B)
    _, _, P = M.stats_np32(qkv, B, T, heads, dm)
    rel = lambda got, r: (np.abs(got.astype(np.float64) - r.numpy()).max() / r.abs().max().item())
    eP, eG = rel(P, ref["P"]), rel(M.ga_np32(qkv, dctx, B, T, heads, dm), M.maps_ref(ref, True, 1.0, 0))
    dev = M.rowsum_deviation(P)
    print(f"{s}: numpy fp32 P {eP:.2e}, P * dP {eG:.2e} (bar {M.TOL_MAPS:.0e}); rows sum to 1 within {dev:.2e}")
    assert eP <= 0.5 * M.TOL_MAPS and eG <= 0.5 * M.TOL_MAPS
    assert dev <= M.ROWSUM_NP32_WORST and M.rowsum_bar(qkv, B, T, heads, dm) <= 4 * M.ROWSUM_NP32_WORST
    # blocks of 128 or one block: the same statistics to a few ulp (the recurrence is what the row sums test)
    m1, inv1, _ = M.stats_np32(qkv, B, T, heads, dm, block=1 << 20)
    m, inv, _ = M.stats_np32(qkv, B, T, heads, dm)
    assert np.array_equal(m, m1) and np.abs(inv / inv1 - 1).max() < 1e-6


@pytest.mark.parametrize("entry", M.ENTRIES)
def test_the_peaked_makers_own_dctx_is_beyond_fp32_for_the_gradient_form(entry):
    """attention_maps_long_cases.maps_inputs: with the peaked maker's own dO (orthogonal to v_i, scaled by 2^12) plain fp32 misses
    5e-6 of max|P * dP| by orders of magnitude, whatever the kernel -- the reason the gradient form of that input takes the random
    maker's dctx.  The probabilities of the same input are within reach."""
    T, heads, dm, B = M.KIND_SHAPES[0]
    qkv, dctx = C.inputs("peaked", entry, T, heads, dm, B)
    ref = M.reference("peaked", entry, T, heads, dm, B)
    got = M.ga_np32(qkv, dctx, B, T, heads, dm).astype(np.float64)
    want = M.maps_ref(ref, True, 1.0, 0)
    e = np.abs(got - want.numpy()).max() / want.abs().max().item()
    print(f"peaked [{entry}] with its own dctx: numpy fp32 P * dP rel err {e:.2e}")
    assert e > 4 * M.TOL_MAPS


def device_asm_digest(src):
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function",
                        "-I../../include", "-I.", "--cuda-device-only", "-S", src, "-o", "-"], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kept = [l for l in r.stdout.splitlines(keepends=True) if not re.match(r"\s*\.(file|ident)", l)]
    return hashlib.sha256("".join(kept).encode()).hexdigest()


def compiler_version():
    return subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()[1].strip()


def test_existing_files_compile_to_the_recorded_device_assembly():
    """Every HIP file that existed before csrc/attention_maps_long.hip compiles to the device assembly of the commit before it
    (sha-256 without the .file and .ident lines), all 42 of them: the four files of ragged kernel copies have since been folded
    into their siblings, whose six entries were recorded anew with the ragged instances in them (tools/asm_ab.py holds the batch
    instances of such a file against the commit before).  The digests belong to one compiler: with another one the
    fixture is recorded anew from the unchanged sources (``python tests/test_build_resources_attention_maps_long.py``), as it is
    for a file whose kernels a later change edits on purpose."""
    from concurrent.futures import ThreadPoolExecutor
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "device_asm_sha256.json")))
    have = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert set(gold["sha256"]) <= set(have) and SRC in have and SRC not in gold["sha256"] and len(gold["sha256"]) == 42
    assert gold["compiler"] == compiler_version(), "another compiler than the one the digests were recorded with: record them anew"
    files = sorted(gold["sha256"])
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        got = dict(zip(files, pool.map(device_asm_digest, files)))
    moved = [f for f in files if got[f] != gold["sha256"][f]]
    assert not moved, f"the device assembly changed: {moved}"


if __name__ == "__main__":                                   # records the fixture from the sources as they stand
    path = os.path.join(ROOT, "tests", "golden", "device_asm_sha256.json")
    gold = json.load(open(path))
    gold["compiler"] = compiler_version()
    gold["sha256"] = {f: device_asm_digest(f) for f in sorted(gold["sha256"])}
    json.dump(gold, open(path, "w"), indent=1, sort_keys=True)
