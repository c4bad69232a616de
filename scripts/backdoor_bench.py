"""Rate of the backdoor search (BatchSolver.backdoors) on one MI355X, recorded,
not gated; bench.py is not involved.

    python scripts/backdoor_bench.py          # -> profiles/backdoor_rate.json

Inputs: hard17_batch boards (17 clues) with their completions (count_solutions,
not timed): 2^12 boards at (level 2, max_size 2) and at (level 1, max_size 3),
and 64 boards at (level 1, max_size 4).  Size, count, first and cover are all
asked for.

Method: warm-up launches of every shape first, then --launches timed launches
of each, the shapes alternating, every launch between two device events on
the stream, one final synchronise before the events are read.  Reported:
median, min and max of the launches' boards per second and trials per second.
A trial is one subset closed: a board with n open cells after the level's
closure and the answer s runs C(n, 1) + ... + C(n, min(s, max_size)) of them
(none when s is 0), counted here from rate()'s open counts and the sizes.

CPU baseline: the host build of csrc/backdoor.h (tests/native/backdoor_host.cpp,
g++ -O2 -fopenmp) with 16 threads on the first boards of each shape, wall time
of the call; the GPU's answers for those boards, all four outputs, are checked
against it.  Without a GPU the measurement fails; nothing is written.
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
from math import comb

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# name -> (boards, level, max_size, boards of the CPU sample)
SHAPES = {"level2_max2": (1 << 12, 2, 2, 256), "level1_max3": (1 << 12, 1, 3, 64), "level1_max4": (64, 1, 4, 16)}
CPU_THREADS = 16


def host_build(tmp):
    so = os.path.join(tmp, "libbackdoor_host.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-fopenmp", "-o", so,
                    os.path.join(ROOT, "tests", "native", "backdoor_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.backdoor_host_batch.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    lib.backdoor_host_batch.restype = None
    return lib


def host_run(lib, boards, grids, level, max_size):
    """(seconds, size, count, first, cover) of the host build (numpy in and out)."""
    boards, grids = np.ascontiguousarray(boards, dtype=np.uint8), np.ascontiguousarray(grids, dtype=np.uint8)
    n = len(boards)
    s, c = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    f, v = np.zeros((n, 4), dtype=np.uint8), np.zeros((n, 81), dtype=np.uint8)
    t0 = time.perf_counter()
    lib.backdoor_host_batch(boards.ctypes.data, grids.ctypes.data, s.ctypes.data, c.ctypes.data, f.ctypes.data,
                            v.ctypes.data, n, level, max_size)
    return time.perf_counter() - t0, s, c, f, v


def trials(opens, sizes, max_size):
    """Subsets closed for boards with `opens` open cells and answers `sizes`."""
    return sum(sum(comb(int(n), k) for k in range(1, min(int(s), max_size) + 1)) for n, s in zip(opens, sizes) if s > 0)


def measure(launches, warmup):
    import torch
    from sudoku_solver_distributed_amd import gen
    from sudoku_solver_distributed_amd.solver import get_solver
    solver = get_solver("cuda:0")
    dev = solver.device
    boards = gen.hard17_batch(1 << 12, seed=1).to(dev)
    counts, grids = solver.count_solutions(boards, limit=2, return_first=True)
    assert bool((counts == 1).all())
    run = lambda name: solver.backdoors(boards[:SHAPES[name][0]], level=SHAPES[name][1], max_size=SHAPES[name][2],
                                        solutions=grids[:SHAPES[name][0]], return_count=True, return_first=True,
                                        return_cover=True)
    for _ in range(warmup):
        for name in SHAPES:
            run(name)
    torch.cuda.synchronize()
    events = {k: [] for k in SHAPES}
    for _ in range(launches):
        for name in SHAPES:  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name)
            e1.record()
            events[name].append((e0, e1))
    torch.cuda.synchronize()
    res = {"launches": launches, "warmup": warmup, "device": torch.cuda.get_device_name(dev),
           "outputs": "size + count + first + cover", "input": "hard17_batch(4096, seed=1) and its completions"}
    answers = {}
    for name, (n, level, max_size, _) in SHAPES.items():
        answers[name] = [t.cpu().numpy() for t in run(name)]
        opens = solver.rate(boards[:n], max_level=level, return_open=True)[1][:, level - 1].cpu().numpy()
        work = trials(opens, answers[name][0], max_size)
        ms = [a.elapsed_time(b) for a, b in events[name]]
        per_s = lambda x: {"median": statistics.median(x / (t * 1e-3) for t in ms), "min": x / (max(ms) * 1e-3),
                           "max": x / (min(ms) * 1e-3)}
        res[name] = {"boards": n, "level": level, "max_size": max_size, "trials": work,
                     "sizes": {str(k): int(v) for k, v in zip(*np.unique(answers[name][0], return_counts=True))},
                     "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                     "boards_per_s": per_s(n), "trials_per_s": per_s(work)}
    res["cpu_host_build"] = {"threads": CPU_THREADS}
    os.environ["OMP_NUM_THREADS"] = str(CPU_THREADS)
    with tempfile.TemporaryDirectory() as tmp:
        lib = host_build(tmp)
        b, g = boards.cpu().numpy(), grids.cpu().numpy()
        host_run(lib, b[:CPU_THREADS], g[:CPU_THREADS], 2, 1)  # the threads are started
        for name, (n, level, max_size, sample) in SHAPES.items():
            secs, *host = host_run(lib, b[:sample], g[:sample], level, max_size)
            for what, h, d in zip(("size", "count", "first", "cover"), host, answers[name]):
                if not np.array_equal(h, d[:sample]):
                    raise SystemExit(f"{name}: the GPU's {what} differs from the host build's")
            opens = solver.rate(boards[:sample], max_level=level, return_open=True)[1][:, level - 1].cpu().numpy()
            work = trials(opens, host[0], max_size)
            res["cpu_host_build"][name] = {
                "boards": sample, "trials": work, "seconds": secs, "boards_per_s": sample / secs,
                "trials_per_s": work / secs, "gpu_over_cpu_trials": res[name]["trials_per_s"]["median"] / (work / secs),
                "answers_equal": True}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backdoor_rate.json"))
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
