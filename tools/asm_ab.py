#!/usr/bin/env python3
"""Device assembly of the same HIP files from two source trees, kernel by kernel.  CPU-only.

    python tools/asm_ab.py --old TREE --new TREE FILE...

TREE is a checkout of this repository, FILE the name of a file in its csrc (backward.hip).  Each file is compiled from both trees
with the flags of tests/test_build_resources_attention_maps_long.py::device_asm_digest, the output is cut into one piece per
kernel (from the kernel's label to the end of its "Kernel info" comment block, so the kernel descriptor and the register
figures are part of it), and in each piece the kernel's own mangled name, the section named after it and the function number in
local labels (.LBB<n>_<m>, .Lfunc_end<n>) are replaced by placeholders.  Kernels are paired by name and template arguments; a
kernel of the new tree that has no partner under its own arguments is looked up without its last argument when that is `false`
(a kernel that gained a trailing compile-time switch).  Per pair the tool prints `identical`, or the differing lines and both
instruction counts.  It exits 1 if any pair differs in a line other than .amdhsa_kernarg_size, and judges nothing else: kernels
without a partner are listed, not compared."""
import argparse
import difflib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("xai-audio-deepfakes_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-I../../include", "-I.", "--cuda-device-only", "-S"]


def device_asm(tree, src):
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [src, "-o", "-"], cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{tree}: {src} does not compile\n{r.stderr[-2000:]}")
    return r.stdout


def key_of(sym):
    """(name, (arg, ...)) of an Itanium-mangled kernel: the innermost identifier and its integer / bool template arguments."""
    rest, name = re.sub(r"^_ZN?", "", sym), sym
    while re.match(r"\d", rest):                                    # <length><identifier> per namespace, the kernel's last
        n = re.match(r"\d+", rest).group(0)
        name, rest = rest[len(n):len(n) + int(n)], rest[len(n) + int(n):]
    targs = re.match(r"I((?:L[a-z]n?\d+E)+)E", rest)
    args = re.findall(r"L([a-z])(n?\d+)E", targs.group(1)) if targs else []
    return name, tuple(("true" if v == "1" else "false") if t == "b" else v for t, v in args)


def kernels(text):
    """{key: normalised lines} of every kernel (a symbol with an .amdhsa_kernel descriptor) in one file's assembly."""
    lines = text.splitlines()
    syms = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur, sym, info = {}, None, None, False
    for l in lines:
        m = re.match(r"(\S+):", l)
        if cur is None and m and m.group(1) in syms:
            cur, sym, info = [], m.group(1), False
        if cur is None:
            continue
        if info and re.match(r"\s*\.(text|section)\b", l):         # the next function begins
            out[key_of(sym)] = cur
            cur = None
            continue
        info = info or ".AMDGPU.csdata" in l
        l = re.sub(r"^\s*\.section\s+\.text\.\S*", "\t.text", l)    # a template instance lives in a section named after it
        l = l.replace(sym, "KERNEL").replace(sym[2:], "KERNEL")     # sym[2:]: inside the names of its static __shared__ arrays
        l = re.sub(r"(\.L|\b)(BB|func_begin|func_end|tmp)\d+", r"\1\2", l)     # BB<n>_<m> without .L: the loop comments
        cur.append(("\t" if l[:1] in " \t" else "") + " ".join(l.split()))      # the label's width moves the comment column
    if cur is not None:
        out[key_of(sym)] = cur
    return out


def instructions(lines):
    return sum(1 for l in lines if l.startswith("\t") and not l.lstrip().startswith((".", ";")))


def show(key):
    return key[0] + ("<" + ", ".join(key[1]) + ">" if key[1] else "")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--old", required=True)
    ap.add_argument("--new", required=True)
    ap.add_argument("files", nargs="+")
    a = ap.parse_args()
    jobs = [(t, f) for f in a.files for t in (a.old, a.new)]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        asm = dict(zip(jobs, pool.map(lambda j: kernels(device_asm(*j)), jobs)))
    bad = 0
    for f in a.files:
        old, new = asm[(a.old, f)], asm[(a.new, f)]
        pairs, alone = [], []
        for k in sorted(new):
            short = (k[0], k[1][:-1]) if k[1] and k[1][-1] == "false" else None
            ko = k if k in old else (short if short in old else None)
            (pairs if ko else alone).append((ko, k))
        print(f"== {f}: {len(pairs)} paired kernels")
        for ko, k in pairs:
            diff = [l for l in difflib.unified_diff(old[ko], new[k], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
            other = [l for l in diff if ".amdhsa_kernarg_size" not in l]
            n_old, n_new = instructions(old[ko]), instructions(new[k])
            if not diff:
                print(f"{show(k)}: identical ({n_new} instructions)")
            elif not other and n_old == n_new:
                print(f"{show(k)}: identical apart from {' -> '.join(l[1:].strip() for l in diff)} ({n_new} instructions)")
            else:
                bad += 1
                print(f"{show(k)}: DIFFERS, {n_old} -> {n_new} instructions")
                print("\n".join("    " + l for l in diff[:40]) + (f"\n    ... {len(diff) - 40} more lines" if len(diff) > 40 else ""))
        paired_old = {ko for ko, _ in pairs}
        for _, k in alone:
            print(f"{show(k)}: only in --new, not compared")
        for k in sorted(set(old) - paired_old):
            print(f"{show(k)}: only in --old, not compared")
    print(f"{bad} paired kernels differ" if bad else "every paired kernel is identical apart from .amdhsa_kernarg_size")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
