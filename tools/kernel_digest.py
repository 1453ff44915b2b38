#!/usr/bin/env python3
"""One digest per gfx950 kernel of the given HIP sources: has a change altered a kernel's device code?

    python tools/kernel_digest.py [--flags "..."] pbs_plus_amd/csrc/kernels.hip ... > after.txt

Each source is compiled to device assembly with the Makefile's flags (CXXFLAGS and KFLAGS; --flags replaces them).
For every symbol of namespace pbsk the text from its label to the end of the function, and its kernel descriptor,
are normalised (basic-block and temporary label numbers, which count through the whole file, and trailing comments
are dropped) and hashed. Output: "<digest> <kind> <file> <symbol>" per line, sorted by symbol; kind = code, desc
(the descriptor) or data. Two runs (before / after a change, or one file against the files it was split into)
compare with diff, without the file column where the files differ: awk '{print $1, $2, $4}'.
Text only: nothing here knows what an instruction means.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

FLAGS = "-O3 -std=c++17 -fPIC -Wall -Wno-unused-result -mllvm -amdgpu-sched-strategy=max-ilp"
LABEL = re.compile(r"^(_ZN4pbsk\w+):")


def normalise(lines):
    out = []
    for ln in lines:
        ln = re.sub(r"BB\d+_", "BB_", ln.split(";", 1)[0])
        out.append(re.sub(r"\.Ltmp\d+", ".Ltmp", ln).rstrip())
    return hashlib.sha256("\n".join(out).encode()).hexdigest()[:16]


def digests(asm):
    """[(symbol, kind, digest)]: kind = code (label .. .Lfunc_end), desc (.amdhsa_kernel block) or data (label .. .size)."""
    lines = asm.splitlines()
    found = []
    for i, ln in enumerate(lines):
        m = LABEL.match(ln)
        if m:
            for j in range(i + 1, len(lines)):
                if lines[j].startswith(".Lfunc_end"):
                    found.append((m.group(1), "code", normalise(lines[i:j])))
                    break
                if lines[j].lstrip().startswith(".size") or LABEL.match(lines[j]):
                    found.append((m.group(1), "data", normalise(lines[i:j])))
                    break
        elif ln.lstrip().startswith(".amdhsa_kernel _ZN4pbsk"):
            j = next(k for k in range(i, len(lines)) if lines[k].lstrip().startswith(".end_amdhsa_kernel"))
            found.append((ln.split()[1], "desc", normalise(lines[i:j + 1])))
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--flags", default=FLAGS)
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--arch", default="gfx950")
    a = ap.parse_args()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for src in a.sources:
            out = src  # (a .s file: device assembly kept from an earlier run)
            if not src.endswith(".s"):
                out = os.path.join(tmp, "dev.s")
                subprocess.run([a.hipcc, f"--offload-arch={a.arch}", *a.flags.split(), "--offload-device-only", "-S", src,
                                "-o", out], check=True)
            with open(out) as f:
                rows += [(sym, kind, os.path.basename(src), d) for sym, kind, d in digests(f.read())]
    for sym, kind, src, d in sorted(rows):
        print(f"{d} {kind} {src} {sym}")
    kernels = [r[0] for r in rows if r[1] == "desc"]
    print(f"# {len(set(kernels))} kernels, {len(kernels) - len(set(kernels))} defined more than once", file=sys.stderr)


if __name__ == "__main__":
    main()
