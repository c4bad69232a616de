"""Static VALU count of the plane kernels outside the pass, against a parent
revision: what a change to the search step (plane::search_step_impl) costs.

    python scripts/isa_step_count.py [--parent HEAD] [-DNAME=V ...]   -> profiles/isa_plane_step.json

Per kernel (plane_kernel, plane_kernel_multi), for the parent revision and
the working tree, built with the product's flags: the VALU instructions of
the largest basic block (the pass, inlined: its opcode histogram must not
move, a reordered pass alone once cost 3.4 %) and of every other block
together (refill, search step, stores, tail).  The difference of the second
figure is what the change added to the step.
"""
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"plane_kernel": "_Z12plane_kernel", "plane_kernel_multi": "_Z18plane_kernel_multi"}


def blocks_of(lines, symbol):
    st = next(i for i, l in enumerate(lines) if l.startswith(symbol))
    en = next(i for i in range(st, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    blocks, cur = [], []
    for l in lines[st:en]:
        if re.match(r"^\S+:", l):
            blocks.append(cur)
            cur = []
        else:
            t = l.strip()
            if t and not t.startswith((";", ".")):
                cur.append(t.split()[0])
    blocks.append(cur)
    return blocks


def count(tree, extra, defines):
    asm = os.path.join(tempfile.mkdtemp(), "k.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *extra,
                           *defines, "--cuda-device-only", "-S", "-o", asm,
                           os.path.join(tree, "sudoku_solver_distributed_amd", "csrc", "plane_kernels.hip")],
                          stderr=subprocess.DEVNULL)
    lines = open(asm).read().split("\n")
    out = {}
    for name, sym in KERNELS.items():
        blocks = blocks_of(lines, sym)
        body = max(blocks, key=len)
        valu = lambda ops: sum(1 for o in ops if o.startswith("v_"))
        out[name] = {"pass_block_valu": valu(body), "pass_block_opcodes": dict(sorted(collections.Counter(body).items())),
                     "other_blocks_valu": sum(valu(b) for b in blocks) - valu(body),
                     "other_blocks_bcnt": sum(b.count("v_bcnt_u32_b32") for b in blocks if b is not body)}
    return out


def main():
    args = sys.argv[1:]
    parent = args[args.index("--parent") + 1] if "--parent" in args else "HEAD"
    defines = [a for a in args if a.startswith("-D")]
    sys.path.insert(0, ROOT)
    from sudoku_solver_distributed_amd import build as B
    extra = dict(B.SRCS)["plane_kernels.hip"]
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", parent, "sudoku_solver_distributed_amd", "include"],
                               stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", tmp], stdin=tar.stdout)
        tar.wait()
        before = count(tmp, extra, [])
    after = count(ROOT, extra, defines)
    res = {"what": "VALU of the plane kernels' largest basic block (the pass) and of all their other blocks, "
                   "parent against the working tree (scripts/isa_step_count.py, hipcc -O3 gfx950 %s)" % " ".join(extra),
           "parent": subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", parent]).decode().strip(),
           "defines": defines, "kernels": {}}
    for k in KERNELS:
        b, a = before[k], after[k]
        res["kernels"][k] = {
            "pass_block_valu": [b["pass_block_valu"], a["pass_block_valu"]],
            "pass_block_opcodes_unchanged": b["pass_block_opcodes"] == a["pass_block_opcodes"],
            "other_blocks_valu": [b["other_blocks_valu"], a["other_blocks_valu"]],
            "step_valu_added": a["other_blocks_valu"] - b["other_blocks_valu"],
            "other_blocks_v_bcnt": [b["other_blocks_bcnt"], a["other_blocks_bcnt"]]}
    if not defines:
        with open(os.path.join(ROOT, "profiles", "isa_plane_step.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
