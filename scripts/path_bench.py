"""Rate of the solving path (sdk_path_batch, BatchSolver.path's kernel) on one
MI355X, recorded, not gated; bench.py is not involved.

    python scripts/path_bench.py                  # -> profiles/path_rate.json

Inputs, 2^16 boards each: hard17_batch boards (17 clues) and symmetry images
of the hard_search_seeds.  Shapes, per input: rules = ALL listing every event
(the capacity from a counting call), rules = ALL counting only (capacity 0, no
list) and max_rounds = 1 (hints, listed); counts, rounds, status and hist are
asked for, the marks are not.  The C ABI entry is called itself, on
preallocated buffers: BatchSolver.path's sort and CSR offsets are torch's and
are not in the figures.  BatchSolver.logic with ladder=[ALL] -- the same
fixpoint without the list -- runs on the same tensors in the same process.

Method: warm-up launches of every shape first, then --launches timed launches
of each, the shapes alternating, every launch between two device events on
the stream, one final synchronise before the events are read.  Reported:
median, min and max of the launches' boards per second, the ratio to logic,
events per board, the tally of statuses and of events per class.

CPU baseline: the host build of csrc/path.h (tests/native/path_host.cpp, g++
-O2 -fopenmp) with 16 threads on the first 256 boards of each set, wall time
of the call; the GPU's events for those boards are checked against it.
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
ALL = 0x1FF


def host_build(tmp):
    so = os.path.join(tmp, "libpath_host.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-fopenmp", "-o", so,
                    os.path.join(ROOT, "tests", "native", "path_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.path_host_batch.argtypes = [vp, vp, ctypes.c_uint32, ctypes.c_int, i64, vp, i64, vp, vp, vp, vp, vp, vp]
    lib.path_host_batch.restype = ctypes.c_int
    return lib


def host_path(lib, boards, max_rounds, capacity):
    """(seconds, sorted rows) of the host build on `boards` (numpy)."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8)
    n = len(boards)
    rows = np.zeros((max(capacity, 1), 4), dtype=np.uint32)
    c, r, s = (np.zeros(n, dtype=np.int32) for _ in range(3))
    info = np.zeros(2, dtype=np.int64)
    t0 = time.perf_counter()
    rc = lib.path_host_batch(boards.ctypes.data, None, ALL, max_rounds, n, rows.ctypes.data, capacity, c.ctypes.data,
                             r.ctypes.data, s.ctypes.data, None, None, info.ctypes.data)
    secs = time.perf_counter() - t0
    assert rc == 0 and info[0] == info[1] == capacity
    return secs, sort_rows(rows[:capacity])


def sort_rows(rows):
    return rows[np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))]


class Call:
    """sdk_path_batch on buffers of its own."""

    def __init__(self, solver, boards, max_rounds, capacity):
        import torch
        self.solver, self.boards, self.max_rounds, self.capacity = solver, boards, max_rounds, capacity
        n, dev = boards.shape[0], solver.device
        self.n = n
        self.rows = torch.empty((capacity, 4), dtype=torch.int32, device=dev) if capacity else None
        self.count, self.rounds, self.status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
        self.hist = torch.empty((n, 9), dtype=torch.int32, device=dev)
        self.info = torch.zeros(2, dtype=torch.int64, device=dev)
        self.scratch = torch.empty(int(solver.lib.sdk_path_scratch_bytes(n, 0)), dtype=torch.uint8, device=dev)
        self.stream = int(torch.cuda.current_stream(dev).cuda_stream)

    def __call__(self):
        rc = self.solver.lib.sdk_path_batch(self.boards.data_ptr(), None, ALL, self.max_rounds, self.n,
                                            self.rows.data_ptr() if self.capacity else None, self.capacity, self.count.data_ptr(),
                                            self.rounds.data_ptr(), self.status.data_ptr(), self.hist.data_ptr(), None,
                                            self.info.data_ptr(), self.scratch.data_ptr(), self.scratch.numel(), 0, self.stream)
        assert rc == 0


def measure(launches, warmup):
    import torch
    from sudoku_solver_distributed_amd import gen
    from sudoku_solver_distributed_amd.solver import get_solver
    solver = get_solver("cuda:0")
    dev = solver.device
    kinds = {"hard17": gen.hard17_batch(N, seed=1).to(dev), "hard_search": gen.hard_search_batch(N, seed=1).to(dev)}
    shapes, totals = {}, {}
    with torch.cuda.device(dev):
        for kind, boards in kinds.items():
            for name, mr in (("all", 0), ("hint", 1)):
                count = Call(solver, boards, mr, 0)
                count()
                torch.cuda.synchronize()
                totals[kind, name] = int(count.info[0].item())
                shapes[f"{kind}_{name}_listed"] = Call(solver, boards, mr, totals[kind, name])
            shapes[f"{kind}_all_count_only"] = Call(solver, boards, 0, 0)
            shapes[f"{kind}_logic_all"] = (lambda b=boards: solver.logic(b, [ALL], return_left=True))
        for _ in range(warmup):
            for call in shapes.values():
                call()
        torch.cuda.synchronize()
        events = {k: [] for k in shapes}
        for _ in range(launches):
            for k, call in shapes.items():  # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                events[k].append((e0, e1))
        torch.cuda.synchronize()
    prop = torch.cuda.get_device_properties(dev)
    res = {"launches": launches, "warmup": warmup, "boards": N, "device": torch.cuda.get_device_name(dev),
           "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count, "rules": ALL,
           "outputs": "rows + count + rounds + status + hist (logic: step + left)"}
    for k, evs in events.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        rate = sorted(N / (t * 1e-3) for t in ms)
        res[k] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                  "boards_per_s_median": statistics.median(rate), "boards_per_s_min": rate[0], "boards_per_s_max": rate[-1]}
    for kind in kinds:
        for shape in ("all_listed", "all_count_only", "hint_listed"):
            res[f"{kind}_{shape}"]["logic_over_path"] = (res[f"{kind}_logic_all"]["boards_per_s_median"]
                                                         / res[f"{kind}_{shape}"]["boards_per_s_median"])
        full = shapes[f"{kind}_all_listed"]
        assert full.info.tolist() == [totals[kind, "all"]] * 2
        res[f"{kind}_events_per_board"] = totals[kind, "all"] / N
        res[f"{kind}_hint_events_per_board"] = totals[kind, "hint"] / N
        res[f"{kind}_rounds_mean"] = float(full.rounds.float().mean())
        res[f"{kind}_status"] = {str(k): int(v) for k, v in zip(*np.unique(full.status.cpu().numpy(), return_counts=True))}
        res[f"{kind}_events_by_class"] = full.hist.sum(0).tolist()
    res["cpu_host_build"] = {"threads": CPU_THREADS, "boards": CPU_SAMPLE}
    os.environ["OMP_NUM_THREADS"] = str(CPU_THREADS)
    with tempfile.TemporaryDirectory() as tmp, torch.cuda.device(dev):
        lib = host_build(tmp)
        for kind, boards in kinds.items():
            sample = boards[:CPU_SAMPLE].contiguous()
            for name, mr in (("all", 0), ("hint", 1)):
                count = Call(solver, sample, mr, 0)
                count()
                torch.cuda.synchronize()
                call = Call(solver, sample, mr, int(count.info[0].item()))
                call()
                torch.cuda.synchronize()
                host_path(lib, sample.cpu().numpy(), mr, call.capacity)  # the threads are started
                secs, rows = host_path(lib, sample.cpu().numpy(), mr, call.capacity)
                if not np.array_equal(sort_rows(call.rows.cpu().numpy().view(np.uint32)), rows):
                    raise SystemExit(f"{kind} ({name}): the GPU's events differ from the host build's")
                cpu_rate = CPU_SAMPLE / secs
                res["cpu_host_build"][f"{kind}_{name}"] = {
                    "seconds": secs, "boards_per_s": cpu_rate, "events": call.capacity,
                    "gpu_over_cpu": res[f"{kind}_{name}_listed"]["boards_per_s_median"] / cpu_rate}
    res["not_measured"] = ["pencil-mark inputs (d_start)", "rule masks other than ALL", "d_marks", "lists past 4 GiB",
                           "BatchSolver.path's sort and CSR offsets (torch)"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_rate.json"))
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
