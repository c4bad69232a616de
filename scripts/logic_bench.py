"""Rate of the named techniques (BatchSolver.logic) on one MI355X, recorded,
not gated; bench.py is not involved.

    python scripts/logic_bench.py                 # -> profiles/logic_rate.json

Inputs, 2^16 boards each: hard17_batch boards (17 clues) and symmetry images
of the hard_search_seeds.  Each at the default ladder (logic_kernel, then
logic_wave_kernel for the boards the first three steps leave open) and at
[N, N|H, N|H|L] (logic_kernel alone); step, open and left are asked for, the
marks are not.  BatchSolver.rate at max_level 3 runs on the same tensors in
the same process: the yardstick for the cost of the shared first phase.

Method: warm-up launches of every shape first, then --launches timed launches
of each, the shapes alternating, every launch between two device events on
the stream, one final synchronise before the events are read.  Reported:
median, min and max of the launches' boards per second; the share of the
boards that reach the wave kernel and the tally of steps.

CPU baseline: the host build of csrc/logic.h (tests/native/logic_host.cpp, g++
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
CPU_SAMPLE = 256
CPU_THREADS = 16


def host_build(tmp):
    so = os.path.join(tmp, "liblogic_host.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-fopenmp", "-o", so,
                    os.path.join(ROOT, "tests", "native", "logic_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.logic_host_batch.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int64]
    lib.logic_host_batch.restype = ctypes.c_int
    return lib


def host_logic(lib, boards, ladder):
    """(seconds, step, open, left) of the host build on `boards` (numpy)."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8)
    lad = np.array(ladder, dtype=np.uint32)
    s = np.zeros(len(boards), dtype=np.int32)
    o = np.zeros((len(boards), 8), dtype=np.int32)
    le = np.zeros((len(boards), 8), dtype=np.int32)
    t0 = time.perf_counter()
    rc = lib.logic_host_batch(boards.ctypes.data, None, lad.ctypes.data, len(lad), s.ctypes.data, o.ctypes.data,
                              le.ctypes.data, None, len(boards))
    assert rc == 0
    return time.perf_counter() - t0, s, o, le


def measure(launches, warmup):
    import torch
    from sudoku_solver_distributed_amd import gen
    from sudoku_solver_distributed_amd.solver import DEFAULT_LADDER, get_solver
    solver = get_solver("cuda:0")
    dev = solver.device
    ladders = {"default": list(DEFAULT_LADDER), "nhl": list(DEFAULT_LADDER[:3])}
    kinds = {"hard17": gen.hard17_batch(N, seed=1).to(dev), "hard_search": gen.hard_search_batch(N, seed=1).to(dev)}
    shapes = {f"{kind}_{name}": (boards, lad) for kind, boards in kinds.items() for name, lad in ladders.items()}
    shapes.update({f"{kind}_rate_level3": (boards, None) for kind, boards in kinds.items()})

    def run(b, lad):
        if lad is None:
            return solver.rate(b, max_level=3, return_open=True)
        return solver.logic(b, lad, return_open=True, return_left=True)

    for _ in range(warmup):
        for b, lad in shapes.values():
            run(b, lad)
    torch.cuda.synchronize()
    events = {k: [] for k in shapes}
    for _ in range(launches):
        for k, (b, lad) in shapes.items():  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(b, lad)
            e1.record()
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    res = {"launches": launches, "warmup": warmup, "boards": N, "device": torch.cuda.get_device_name(dev),
           "outputs": "step + open + left (rate: rating + open)", "ladders": ladders}
    for k, evs in events.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        rate = sorted(N / (t * 1e-3) for t in ms)
        res[k] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                  "boards_per_s_median": statistics.median(rate), "boards_per_s_min": rate[0],
                  "boards_per_s_max": rate[-1]}
    for kind, boards in kinds.items():
        step, opens, _ = run(boards, ladders["default"])
        res[f"{kind}_steps"] = {str(k): int(v) for k, v in zip(*np.unique(step.cpu().numpy(), return_counts=True))}
        res[f"{kind}_wave_kernel"] = {"share_of_boards": float((opens[:, 2] > 0).float().mean())}
    res["cpu_host_build"] = {"threads": CPU_THREADS, "boards": CPU_SAMPLE}
    os.environ["OMP_NUM_THREADS"] = str(CPU_THREADS)
    with tempfile.TemporaryDirectory() as tmp:
        lib = host_build(tmp)
        for kind, boards in kinds.items():
            sample = boards[:CPU_SAMPLE]
            for name, lad in ladders.items():
                host_logic(lib, sample.cpu().numpy(), lad)  # the threads are started
                secs, s, o, le = host_logic(lib, sample.cpu().numpy(), lad)
                gs, go, gl = run(sample, lad)
                if not (np.array_equal(gs.cpu().numpy(), s) and np.array_equal(go.cpu().numpy(), o)
                        and np.array_equal(gl.cpu().numpy(), le)):
                    raise SystemExit(f"{kind} at the ladder {name}: the GPU's answers differ from the host build's")
                cpu_rate = CPU_SAMPLE / secs
                res["cpu_host_build"][f"{kind}_{name}"] = {
                    "seconds": secs, "boards_per_s": cpu_rate,
                    "gpu_over_cpu": res[f"{kind}_{name}"]["boards_per_s_median"] / cpu_rate}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logic_rate.json"))
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
