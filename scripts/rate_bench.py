"""Rate of the puzzle rating (BatchSolver.rate) on one MI355X, recorded, not
gated; bench.py is not involved.

    python scripts/rate_bench.py                  # -> profiles/rate_rate.json

Inputs, 2^16 boards each: hard17_batch boards (17 clues) and symmetry images
of the hard_search_seeds.  Each at max_level 3 (rate_kernel alone) and 4
(rate_kernel, then rate_trial_kernel for the boards level 3 leaves open);
rating and open counts are asked for, the marks are not.

Method: warm-up launches of every shape first, then --launches timed launches
of each, the shapes alternating, every launch between two device events on
the stream, one final synchronise before the events are read.  Reported:
median, min and max of the launches' boards per second; the share of the
boards the trial kernel takes and, from the two levels' medians, of the time.

CPU baseline: the host build of csrc/rate.h (tests/native/rate_host.cpp, g++
-O2 -fopenmp) with 16 threads on the first 256 boards of each set, wall time
of the call; the GPU's answers for those boards are checked against it.
Without a GPU the measurement fails; nothing is written.
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
N = 1 << 16
LEVELS = (3, 4)
CPU_SAMPLE = 256
CPU_THREADS = 16


def host_build(tmp):
    so = os.path.join(tmp, "librate_host.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-fopenmp", "-o", so,
                    os.path.join(ROOT, "tests", "native", "rate_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.rate_host_batch.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int]
    lib.rate_host_batch.restype = None
    return lib


def host_rate(lib, boards, max_level):
    """(seconds, rating, open) of the host build on `boards` (numpy)."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8)
    r = np.zeros(len(boards), dtype=np.int32)
    o = np.zeros((len(boards), 4), dtype=np.int32)
    t0 = time.perf_counter()
    lib.rate_host_batch(boards.ctypes.data, r.ctypes.data, o.ctypes.data, None, len(boards), max_level)
    return time.perf_counter() - t0, r, o


def measure(launches, warmup):
    import torch
    from sudoku_solver_distributed_amd import gen
    from sudoku_solver_distributed_amd.solver import get_solver
    solver = get_solver("cuda:0")
    dev = solver.device
    kinds = {"hard17": gen.hard17_batch(N, seed=1).to(dev), "hard_search": gen.hard_search_batch(N, seed=1).to(dev)}
    shapes = {f"{kind}_level{m}": (boards, m) for kind, boards in kinds.items() for m in LEVELS}
    run = lambda b, m: solver.rate(b, max_level=m, return_open=True)
    for _ in range(warmup):
        for b, m in shapes.values():
            run(b, m)
    torch.cuda.synchronize()
    events = {k: [] for k in shapes}
    for _ in range(launches):
        for k, (b, m) in shapes.items():  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(b, m)
            e1.record()
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    res = {"launches": launches, "warmup": warmup, "boards": N, "device": torch.cuda.get_device_name(dev),
           "outputs": "rating + open"}
    for k, evs in events.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        rate = sorted(N / (t * 1e-3) for t in ms)
        res[k] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                  "boards_per_s_median": statistics.median(rate), "boards_per_s_min": rate[0],
                  "boards_per_s_max": rate[-1]}
    for kind, boards in kinds.items():
        rating = run(boards, 4)[0].cpu().numpy()
        at3 = run(boards, 3)[0].cpu().numpy()
        t3, t4 = res[f"{kind}_level3"]["ms_median"], res[f"{kind}_level4"]["ms_median"]
        res[f"{kind}_ratings"] = {str(k): int(v) for k, v in zip(*np.unique(rating, return_counts=True))}
        res[f"{kind}_trial_kernel"] = {"share_of_boards": float((at3 == 4).mean()), "share_of_time": (t4 - t3) / t4}
    res["cpu_host_build"] = {"threads": CPU_THREADS, "boards": CPU_SAMPLE}
    os.environ["OMP_NUM_THREADS"] = str(CPU_THREADS)
    with tempfile.TemporaryDirectory() as tmp:
        lib = host_build(tmp)
        for kind, boards in kinds.items():
            sample = boards[:CPU_SAMPLE]
            for m in LEVELS:
                host_rate(lib, sample.cpu().numpy(), m)  # the threads are started
                secs, r, o = host_rate(lib, sample.cpu().numpy(), m)
                gr, go = run(sample, m)
                if not (np.array_equal(gr.cpu().numpy(), r) and np.array_equal(go.cpu().numpy(), o)):
                    raise SystemExit(f"{kind} at max_level {m}: the GPU's answers differ from the host build's")
                cpu_rate = CPU_SAMPLE / secs
                res["cpu_host_build"][f"{kind}_level{m}"] = {
                    "seconds": secs, "boards_per_s": cpu_rate,
                    "gpu_over_cpu": res[f"{kind}_level{m}"]["boards_per_s_median"] / cpu_rate}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_rate.json"))
    a = ap.parse_args()
    if a.launches < 10:
        ap.error("at least 10 timed launches")
    res = measure(a.launches, a.warmup)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
