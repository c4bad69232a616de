"""Static instruction count of the plane kernel's outbox flush
(plane_flush_outbox alone, scripts/microbench/flush_count.hip, same flags as
the product build) without and with the completion test of
SDK_PLANE_ROOTFULL: every instruction between the kernel's label and its
s_endpgm, all paths (the edge-dword branches included), minus the stub's own
outbox fill.

    python scripts/isa_flush_count.py   -> profiles/isa_plane_flush.json
"""
import collections
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = os.path.join(ROOT, "scripts", "microbench", "flush_count.hip")
BUDGET = 350  # extra VALU per flush the change was given


def count(extra, define):
    asm = os.path.join(tempfile.mkdtemp(), "k.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *extra,
                           "-D" + define, "--cuda-device-only", "-S", "-o", asm, MICRO], stderr=subprocess.DEVNULL)
    lines = open(asm).read().split("\n")
    st = next(i for i, l in enumerate(lines) if l.startswith("_Z10flush_only"))
    en = next(i for i in range(st, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    ops = [l.strip().split()[0] for l in lines[st:en]
           if l.strip() and not l.strip().startswith((";", ".")) and not l.rstrip().endswith(":")]
    c = collections.Counter(ops)
    return {"instructions": len(ops), "valu": sum(v for k, v in c.items() if k.startswith("v_")),
            "salu": sum(v for k, v in c.items() if k.startswith("s_")), "top": c.most_common(8)}


def main():
    sys.path.insert(0, ROOT)
    from sudoku_solver_distributed_amd import build as B  # same flags as the product build
    extra = dict(B.SRCS)["plane_kernels.hip"]
    before, after = count(extra, "SDK_PLANE_ROOTFULL=0"), count(extra, "SDK_PLANE_ROOTFULL=1")
    out = {"kernel": "flush_only (plane_flush_outbox alone, scripts/microbench/flush_count.hip, hipcc -O3 gfx950 %s)"
                     % " ".join(extra),
           "rootfull_0": before, "rootfull_1": after, "extra_valu_per_flush": after["valu"] - before["valu"],
           "budget_valu": BUDGET}
    with open(os.path.join(ROOT, "profiles", "isa_plane_flush.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
