"""Build libsudoku_hip.so in-tree for gfx950 with hipcc (no JIT, no torch ext).

    python -m sudoku_solver_distributed_amd.build
"""
from __future__ import annotations

import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
# translation units and their extra flags (plane_kernels.hip: see its header;
# count_kernels.hip, the completion count, is a unit of its own so that the
# solve kernels' code generation and scheduler flags stay exactly as they are;
# iterative-minreg keeps its board loader from spilling: 116 VGPRs and no
# scratch, where LLVM's default scheduler spills 34 registers, DESIGN.md §12;
# canon_kernels.hip, the canonical form, and rate_kernels.hip, the puzzle
# rating, likewise units of their own, LLVM's defaults; cand_kernels.hip, the
# exact candidates, min_kernels.hip, the minimisation, and sample_kernels.hip,
# the random completion, and uniq_kernels.hip, the unique candidates, units of
# their own with the count's scheduler, DESIGN.md §15, §16, §17 and §18;
# exact_kernels.hip, the exact count shared over the grid, and enum_kernels.hip,
# the completion list on the same rounds, likewise, §20 and §21;
# backdoor_kernels.hip, the backdoor search on the rating's closures, a unit of
# its own like rate_kernels.hip, LLVM's defaults, §23; ua_kernels.hip, the
# unavoidable sets of a grid, likewise, §24; hit_kernels.hip, the hitting
# sets of a family of cell sets, likewise, §25; logic_kernels.hip, the named
# techniques on the rating's closures, likewise, §26; path_kernels.hip, the
# solving path on logic.h's matrices, likewise, §27)
# SDK_PLANE_SCHED: machine-scheduler strategy of the plane kernel's unit
# (iterative-ilp measured +1.4 % over LLVM's default on one MI355X, same
# registers; "default" = LLVM's own, for A/B builds)
_SCHED = os.environ.get("SDK_PLANE_SCHED", "iterative-ilp")


# SDK_PLANE_LLVM: more LLVM options for the plane unit (space-separated, each
# passed through -mllvm; A/B builds of the code generator only)
_LLVM_EXTRA = os.environ.get("SDK_PLANE_LLVM", "").split()


def sources(sched: str = _SCHED):
    """Translation units and their flags for one plane-unit scheduler."""
    extra = [f for o in _LLVM_EXTRA for f in ("-mllvm", o)]
    return (("sudoku_kernels.hip", []),
            ("plane_kernels.hip", ([] if sched == "default" else ["-mllvm", f"-amdgpu-sched-strategy={sched}"]) + extra),
            ("count_kernels.hip", ["-mllvm", "-amdgpu-sched-strategy=iterative-minreg"]),
            ("canon_kernels.hip", []),
            ("rate_kernels.hip", []),
            ("cand_kernels.hip", ["-mllvm", "-amdgpu-sched-strategy=iterative-minreg"]),
            ("min_kernels.hip", ["-mllvm", "-amdgpu-sched-strategy=iterative-minreg"]),
            ("sample_kernels.hip", ["-mllvm", "-amdgpu-sched-strategy=iterative-minreg"]),
            ("uniq_kernels.hip", ["-mllvm", "-amdgpu-sched-strategy=iterative-minreg"]),
            ("exact_kernels.hip", ["-mllvm", "-amdgpu-sched-strategy=iterative-minreg"]),
            ("enum_kernels.hip", ["-mllvm", "-amdgpu-sched-strategy=iterative-minreg"]),
            ("backdoor_kernels.hip", []),
            ("ua_kernels.hip", []),
            ("hit_kernels.hip", []),
            ("logic_kernels.hip", []),
            ("path_kernels.hip", []))


SRCS = sources()
# Every build this module is used for (product, diagnostic and A/B tuning
# builds): name -> (-D set, plane-unit scheduler).  scripts/store_hazard_check.py
# scans each of them for the wide-store data hazard; build() scans any other
# -D set before linking it.
VARIANTS = {
    "default": ((), _SCHED),
    "stamps": (("SDK_PLANE_STAMPS=1",), _SCHED),
    "waves5": (("SDK_PLANE_WAVES_PER_EU=5",), _SCHED),
    "waves6": (("SDK_PLANE_WAVES_PER_EU=6",), _SCHED),
    "nopinacc": (("SDK_PLANE_PIN_ACC=0",), _SCHED),
    # rule D's box -> row form computed per word, one-wave workgroups (the kernel before the LDS table)
    "locktbl-off": (("SDK_PLANE_LOCKTBL=0",), _SCHED),
    # rule C's box terms computed per word (the kernel before the column table)
    "coltbl-off": (("SDK_PLANE_COLTBL=0",), _SCHED),
    "sched-default": ((), "default"),
    "sched-minreg": ((), "iterative-minreg"),
    "sched-maxocc": ((), "iterative-maxocc"),
    "sched-max-ilp": ((), "max-ilp"),
}
OUT = os.path.join(_HERE, "libsudoku_hip.so")
ARCH = os.environ.get("SDK_OFFLOAD_ARCH", "gfx950")


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return "hipcc"


def build(force: bool = False, verbose: bool = False, defines=(), out: str = OUT) -> str:
    """Compile every translation unit for gfx950 and link the C-ABI library.
    `defines` / `out`: A/B builds of tuning macros into another in-tree .so
    (loaded with SDK_LIB=...)."""
    csrc = os.path.join(_HERE, "csrc")
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc) if not f.endswith(".o")] + [os.path.join(ROOT, "include", "sudoku_hip.h")]
    if (not force and os.path.exists(out)
            and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)):
        return out
    if tuple(defines) and tuple(defines) not in {v[0] for v in VARIANTS.values()}:
        # an A/B build nobody has scanned yet: the wide-store hazard check first
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        import store_hazard_check
        if store_hazard_check.check_build(SRCS, defines, "+".join(defines)):
            raise RuntimeError(f"wide-store data hazard in the build with {defines} (scripts/store_hazard_check.py)")
    objs = []
    for name, extra in SRCS:
        obj = out + "." + name + ".o"
        cmd = [hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall", *extra,
               *[f"-D{d}" for d in defines],
               "-c", "-o", obj, os.path.join(csrc, name)]
        if verbose:
            cmd.append("-Rpass-analysis=kernel-resource-usage")
        subprocess.check_call(cmd)
        objs.append(obj)
    subprocess.check_call([hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", out + ".tmp", *objs])
    for obj in objs:
        os.remove(obj)
    os.replace(out + ".tmp", out)
    return out


if __name__ == "__main__":
    # python -m sudoku_solver_distributed_amd.build [--force] [-v] [--tag T -DNAME=V ...]
    args = sys.argv[1:]
    defs = [a[2:] for a in args if a.startswith("-D")]
    tag = args[args.index("--tag") + 1] if "--tag" in args else None
    dst = os.path.join(_HERE, f"libsudoku_hip_{tag}.so") if tag else OUT
    print(build(force="--force" in args or bool(tag), verbose="-v" in args, defines=defs, out=dst))
