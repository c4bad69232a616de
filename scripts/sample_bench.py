"""Rate of the random full grids (BatchSolver.random_grids) on one MI355X
against the path they replace in the puzzle generator, recorded, not gated;
bench.py is not involved.

    python scripts/sample_bench.py                 # -> profiles/sample_rate.json
    python scripts/sample_bench.py --host-model    # passes per grid on the CPU, no GPU

What is timed is what a caller pays: wall time around the call, the device
synchronised before the clock starts and before it stops.  Four records:

  random_grids     solver.random_grids(n, seed) at 2^16 and 2^20 grids
  generate_batch   gen.generate_batch(n, 0, seed) at 2^16, host loop included:
                   the parent path of the generator's full grids.  A run takes
                   seconds, so 3 runs after one warm-up.
  unique_batch     gen.unique_batch(n, seed=seed, fused=True) end to end with
                   grids="walk" (2^16, 3 runs) against grids="random" (2^16, and
                   2^20 with 3 runs: the turn orders are drawn on the host)
  host_model       (--host-model, on the CPU) the host build of plane_sample.h
                   (tests/native/sample_host.cpp) on the empty board under seed
                   1, keys 0..4607: passes per grid (mean, max), the deepest
                   stack level and the draws per grid

Method: --warmup warm-up calls of every shape first (at least 3; one for the
shapes that take seconds), then --runs timed runs (at least 8; 3 for those);
median, min and max of the runs' milliseconds.  The claim checked is the
direction only: random_grids(65536) beats generate_batch(65536, 0) on the same
machine; the ratio of the medians is recorded as
generate_batch_over_random_grids.  Without a GPU the measurement fails; nothing
is written.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SLOW_RUNS = 3  # the shapes with generate_batch's host loop in them


def host_model(keys=4608, seed=1):
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "libsample_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", out,
                           os.path.join(ROOT, "tests", "native", "sample_host.cpp")])
    f = ctypes.CDLL(out).sample_host_batch
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    f.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int, u64, u64, ctypes.c_uint32, vp, vp, vp]
    grids, status = np.zeros((keys, 81), np.uint8), np.zeros(keys, np.int32)
    passes, deepest, draws = np.zeros(keys, np.uint64), np.zeros(keys, np.uint32), np.zeros(keys, np.uint32)
    f(None, grids.ctypes.data, status.ctypes.data, 1, keys, seed, 0, 81, passes.ctypes.data, deepest.ctypes.data,
      draws.ctypes.data)
    assert (status == 1).all() and len({g.tobytes() for g in grids}) == keys
    return {"board": "empty", "seed": seed, "keys": keys, "passes_per_grid_mean": float(passes.mean()),
            "passes_per_grid_max": int(passes.max()), "passes_per_grid_p99": float(np.percentile(passes, 99)),
            "deepest_stack_level": int(deepest.max()), "draws_per_grid_mean": float(draws.mean()),
            "draws_per_grid_max": int(draws.max())}


def stats(ms, n):
    med = statistics.median(ms)
    return {"items": n, "runs": len(ms), "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
            "items_per_s_median": n / (med * 1e-3)}


def timed(f, runs, warmup):
    import torch
    for _ in range(warmup):
        f()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def measure(sizes, runs, warmup, seed):
    import torch
    from sudoku_solver_distributed_amd.gen import generate_batch, random_grids, unique_batch
    from sudoku_solver_distributed_amd.solver import get_solver
    solver = get_solver("cuda:0")
    dev = solver.device
    small = sizes[0]
    g = solver.random_grids(small, seed)
    assert bool(solver.check(g).all()) and torch.unique(g, dim=0).shape[0] == small
    res = {"runs": runs, "warmup": warmup, "seed": seed, "device": torch.cuda.get_device_name(dev),
           "random_grids": {}, "generate_batch": {}, "unique_batch_fused": {"walk": {}, "random": {}}}
    for n in sizes:
        res["random_grids"][str(n)] = stats(timed(lambda: random_grids(n, seed, device=dev), runs, warmup), n)
        few = n > small  # unique_batch draws its turn orders on the host: seconds at 2^20
        res["unique_batch_fused"]["random"][str(n)] = stats(
            timed(lambda: unique_batch(n, seed=seed, device=dev, fused=True, grids="random"),
                  SLOW_RUNS if few else runs, 1 if few else warmup), n)
    res["generate_batch"][str(small)] = stats(timed(lambda: generate_batch(small, 0, seed, device=dev), SLOW_RUNS, 1), small)
    res["unique_batch_fused"]["walk"][str(small)] = stats(
        timed(lambda: unique_batch(small, seed=seed, device=dev, fused=True, grids="walk"), SLOW_RUNS, 1), small)
    res["generate_batch_over_random_grids"] = (res["generate_batch"][str(small)]["ms_median"] /
                                               res["random_grids"][str(small)]["ms_median"])
    res["unique_batch_walk_over_random"] = (res["unique_batch_fused"]["walk"][str(small)]["ms_median"] /
                                            res["unique_batch_fused"]["random"][str(small)]["ms_median"])
    res["random_grids_beats_generate_batch"] = res["generate_batch_over_random_grids"] > 1.0
    solver.verify()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_rate.json"))
    ap.add_argument("--host-model", action="store_true")
    a = ap.parse_args()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    if a.host_model:
        res = host_model()
        doc["host_model"] = res
    else:
        if a.runs < 8 or a.warmup < 3:
            ap.error("at least 8 timed runs and 3 warm-up rounds")
        res = measure(a.items, a.runs, a.warmup, a.seed)
        doc = dict(res, **{k: v for k, v in doc.items() if k == "host_model"})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
