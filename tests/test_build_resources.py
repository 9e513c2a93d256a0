"""CPU-only: the matrix-core kernels of the hot path must compile WITHOUT scratch (register spills).  A spill in
`gemm_x3_kernel` is a 2.5x slowdown of the whole fp32-class mode that no parity test sees (it happened in round 3 when a branch
was added to `split_f32`): hipcc's kernel-resource remarks are parsed for every GEMM instantiation."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xai-audio-deepfakes_amd", "csrc")


def resources(src):
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function",
                        f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, src), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def test_gemm_kernels_do_not_spill():
    res = resources("gemm.hip")
    x3 = {k: v for k, v in res.items() if "gemm_x3_kernel" in k}
    f16 = {k: v for k, v in res.items() if "gemm_f16_kernel" in k}
    assert len(x3) == 6 and len(f16) >= 4, sorted(res)
    for k, v in {**x3, **f16}.items():
        assert v["scratch"] == 0, (k, v)
    for k, v in x3.items():
        assert v["occupancy"] >= 2, (k, v)                     # two co-resident workgroups hide each other's DMA
    main = [v for k, v in f16.items() if "ILi128ELi128ELi2ELi2ELi4E" in k]
    assert main and all(v["occupancy"] >= 4 for v in main), main      # 4 workgroups per CU on the fp16 128x128 tile


def test_attention_and_resblock_kernels_do_not_spill():
    """The fp32-class attention kernels (forward, both head-dim classes, and the fp32 backward) and the fused x3 ResBlock pair:
    the D = 128 streaming kernel spilled 216 B per lane until round 3 (the staging loop of four planes was unrolled)."""
    for src, names in (("attention.hip", ("attention_x3_kernel", "attention_x3_stream_kernel")),
                       ("attention_bwd_f32.hip", ("attention_bwd_f32_kernel",)),
                       ("resblock_pair_x3.hip", ("resblock_pair_x3_kernel",))):
        res = resources(src)
        hit = {k: v for k, v in res.items() if any(n in k for n in names)}
        assert hit, (src, sorted(res))
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
    # the split-arithmetic attention backward: no scratch, except the 13-tile / head-dim-64 instance (T = 199: the production
    # shape), which keeps <= 96 bytes per lane for values that live across its two passes -- outside the product loops; with the
    # whole register file (four wavefronts) it measured 392 us against 293 us (profiles/r03_attention_bwd_x3.txt)
    res = resources("attention_bwd_x3.hip")
    hit = {k: v for k, v in res.items() if "attention_bwd_x3_kernel" in k}
    assert len(hit) == 16, sorted(res)                     # eight instances, each for a batch and for a ragged batch (RAGGED)
    for k, v in hit.items():
        assert v["scratch"] <= (96 if "ILi13ELi64ELi8E" in k else 0), (k, v)
