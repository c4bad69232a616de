"""Rate of the canonical form (BatchSolver.canonical) on one MI355X, recorded,
not gated; bench.py is not involved.

    python scripts/canon_bench.py                 # -> profiles/canon_rate.json

Inputs, each at n = 1, 4096 and 2^17 boards per launch: hard17_batch boards
(17 clues), minimal puzzles (symmetry images of 4096 unique_batch puzzles) and
full grids (symmetry images of 4096 generate_batch grids).  canon, sym and
autos are all asked for; slices = 0 (the library's own choice).

Method: warm-up launches of every shape first, then --launches timed launches
of each, the shapes alternating, every launch between two device events on
the stream, one final synchronise before the events are read.  Reported:
median, min and max of the launches' boards per second.

CPU baseline: scripts/hard17/hard17_search.c --canon (the only other
implementation) with 16 OpenMP threads on the first 256 boards of each kind,
wall time of the whole process; the GPU's canon of those boards is checked
against its output (the tool prints distinct classes only, so the check is on
the set).  Without a GPU the measurement fails; nothing is written.
"""
import argparse
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
SIZES = (1, 4096, 1 << 17)
CPU_SAMPLE = 256
CPU_THREADS = 16


def inputs(dev):
    import torch
    from sudoku_solver_distributed_amd import gen
    n = max(SIZES)
    minimal = gen.unique_batch(4096, 81, seed=1, device=dev).cpu().numpy()
    grids = gen.generate_batch(4096, 0, seed=1, device=dev).cpu().numpy()
    kinds = {"hard17": gen.hard17_batch(n, seed=1).numpy(),
             "minimal": gen._symmetry_images(minimal, n, seed=2),
             "full_grid": gen._symmetry_images(grids, n, seed=3)}
    clues = {k: float((v[:4096] > 0).sum(1).mean()) for k, v in kinds.items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in kinds.items()}, clues


def cpu_baseline(boards):
    """(seconds, distinct canon lines) of the C tool on `boards` (numpy)."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "hard17_search")
        subprocess.run(["gcc", "-O3", "-fopenmp", "-o", exe, os.path.join(ROOT, "scripts", "hard17", "hard17_search.c")],
                       check=True)
        text = "".join("".join(map(str, b)) + "\n" for b in boards.tolist())
        t0 = time.perf_counter()
        out = subprocess.run([exe, "--canon"], input=text, check=True, capture_output=True, text=True,
                             env=dict(os.environ, OMP_NUM_THREADS=str(CPU_THREADS))).stdout.split()
        return time.perf_counter() - t0, set(out)


def measure(launches, warmup):
    import torch
    from sudoku_solver_distributed_amd.solver import get_solver
    solver = get_solver("cuda:0")
    dev = solver.device
    kinds, clues = inputs(dev)
    shapes = {}
    for kind, boards in kinds.items():
        for n in SIZES:
            shapes[f"{kind}_n{n}"] = (n, boards[:n].contiguous())
    run = lambda b: solver.canonical(b, return_sym=True, return_autos=True)
    for _ in range(warmup):
        for _, b in shapes.values():
            run(b)
    torch.cuda.synchronize()
    events = {k: [] for k in shapes}
    for _ in range(launches):
        for k, (_, b) in shapes.items():  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(b)
            e1.record()
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    res = {"launches": launches, "warmup": warmup, "slices": 0, "device": torch.cuda.get_device_name(dev),
           "mean_clues": clues, "outputs": "canon + sym + autos"}
    for k, evs in events.items():
        n = shapes[k][0]
        ms = [a.elapsed_time(b) for a, b in evs]
        rate = sorted(n / (t * 1e-3) for t in ms)
        res[k] = {"boards": n, "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                  "boards_per_s_median": statistics.median(rate), "boards_per_s_min": rate[0],
                  "boards_per_s_max": rate[-1]}
    res["cpu_tool"] = {"threads": CPU_THREADS, "boards": CPU_SAMPLE}
    for kind, boards in kinds.items():
        sample = boards[:CPU_SAMPLE]
        secs, lines = cpu_baseline(sample.cpu().numpy())
        got = {"".join(map(str, row)) for row in solver.canonical(sample).cpu().numpy().tolist()}
        if got != lines:
            raise SystemExit(f"{kind}: the GPU's classes differ from the CPU tool's")
        cpu_rate = CPU_SAMPLE / secs
        res["cpu_tool"][kind] = {"seconds": secs, "boards_per_s": cpu_rate, "classes": len(lines),
                                 "gpu_over_cpu_at_n%d" % max(SIZES):
                                     res[f"{kind}_n{max(SIZES)}"]["boards_per_s_median"] / cpu_rate}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "canon_rate.json"))
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
