"""Rate of the unavoidable-set search (sdk_unavoidable_batch, what
BatchSolver.unavoidable runs first) on one MI355X, recorded, not gated;
bench.py is not involved.

    python scripts/ua_bench.py          # -> profiles/ua_rate.json

Inputs: random_grids(4096, seed=1).  Shapes: all 4096 at max_size 10 and 12,
the first 64 at 14, the first one and the first 64 at 16.  The list's capacity
is the shape's row total, known from a first untimed call with capacity 0, so
every row is written.

Method: warm-up launches of every shape first, then --launches timed launches
of each, the shapes alternating, every launch between two device events on
the stream, one final synchronise before the events are read.  Reported:
median, min and max of the launches' grids per second and search nodes per
second.  A node is one digit placed by the walk of csrc/ua.h; the nodes of a
grid depend on the grid and max_size alone and are counted by the host build.
Also recorded, once per shape and by the host's clock: BatchSolver.unavoidable
as a whole (search, sort, duplicates, minimal filter).

CPU baseline: the host build of csrc/ua.h (tests/native/ua_host.cpp, g++ -O2
-fopenmp) with 16 threads on the first grids of each shape, wall time of the
call; the GPU's rows of those grids are checked against it as multisets, the
counts as they are.  Without a GPU the measurement fails; nothing is written.
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
# name -> (grids, max_size, grids of the CPU sample)
SHAPES = {"m10_4096": (1 << 12, 10, 512), "m12_4096": (1 << 12, 12, 256), "m14_64": (64, 14, 32), "m16_1": (1, 16, 1),
          "m16_64": (64, 16, 16)}
CPU_THREADS = 16


def host_build(tmp):
    so = os.path.join(tmp, "libua_host.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-fopenmp", "-o", so,
                    os.path.join(ROOT, "tests", "native", "ua_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.ua_host_batch.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4
    lib.ua_host_batch.restype = ctypes.c_int
    return lib


def host_run(lib, grids, max_size, capacity):
    """(seconds, rows, count, nodes) of the host build (numpy in and out)."""
    grids = np.ascontiguousarray(grids, dtype=np.uint8)
    n = len(grids)
    rows = np.zeros((max(capacity, 1), 4), dtype=np.uint32)
    count, status = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    info, nodes = np.zeros(2, dtype=np.int64), np.zeros(n, dtype=np.uint64)
    t0 = time.perf_counter()
    rc = lib.ua_host_batch(grids.ctypes.data, n, max_size, rows.ctypes.data, capacity, count.ctypes.data, status.ctypes.data,
                           info.ctypes.data, nodes.ctypes.data)
    secs = time.perf_counter() - t0
    assert rc == 0 and (status == 1).all()
    return secs, rows[:info[1]], count, nodes


def sorted_rows(rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 4)
    return rows[np.lexsort((rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]))]


def measure(launches, warmup):
    import torch
    from sudoku_solver_distributed_amd.solver import get_solver
    solver = get_solver("cuda:0")
    dev, L = solver.device, solver.lib
    grids = solver.random_grids(1 << 12, seed=1)
    torch.cuda.synchronize()
    stream = int(torch.cuda.current_stream(dev).cuda_stream)
    buf = {}
    for name, (n, m, _) in SHAPES.items():
        need = int(L.sdk_unavoidable_scratch_bytes(n, 0))
        b = {"count": torch.empty(n, dtype=torch.int32, device=dev), "status": torch.empty(n, dtype=torch.int32, device=dev),
             "info": torch.zeros(2, dtype=torch.int64, device=dev), "sc": torch.empty(need, dtype=torch.uint8, device=dev)}
        assert L.sdk_unavoidable_batch(grids.data_ptr(), n, m, None, 0, b["count"].data_ptr(), b["status"].data_ptr(),
                                       b["info"].data_ptr(), b["sc"].data_ptr(), need, 0, stream) == 0
        b["total"] = int(b["info"].tolist()[0])
        b["rows"] = torch.empty((b["total"], 4), dtype=torch.int32, device=dev)
        buf[name] = b

    def run(name):
        n, m, _ = SHAPES[name]
        b = buf[name]
        assert L.sdk_unavoidable_batch(grids.data_ptr(), n, m, b["rows"].data_ptr(), b["total"], b["count"].data_ptr(),
                                       b["status"].data_ptr(), b["info"].data_ptr(), b["sc"].data_ptr(), b["sc"].numel(), 0,
                                       stream) == 0
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
           "timed": "sdk_unavoidable_batch, every row listed", "input": "random_grids(4096, seed=1)"}
    os.environ["OMP_NUM_THREADS"] = str(CPU_THREADS)
    g = grids.cpu().numpy()
    with tempfile.TemporaryDirectory() as tmp:
        lib = host_build(tmp)
        host_run(lib, g[:CPU_THREADS], 8, 1 << 12)  # the threads are started
        for name, (n, m, sample) in SHAPES.items():
            b = buf[name]
            assert b["info"].tolist() == [b["total"], b["total"]] and bool((b["status"] == 1).all())
            count = b["count"].cpu().numpy()
            secs, hrows, hcount, hnodes = host_run(lib, g[:sample], m, b["total"])
            rows = b["rows"].cpu().numpy().view(np.uint32)
            if not np.array_equal(hcount, count[:sample]) or not np.array_equal(sorted_rows(hrows),
                                                                                  sorted_rows(rows[rows[:, 3] < sample])):
                raise SystemExit(f"{name}: the GPU's rows differ from the host build's")
            nodes = int(hnodes.sum())
            if n > sample:  # the rest of the grids, for their nodes only (not timed)
                _, _, rcount, rnodes = host_run(lib, g[sample:n], m, 0)
                if not np.array_equal(rcount, count[sample:]):
                    raise SystemExit(f"{name}: the GPU's counts differ from the host build's")
                nodes += int(rnodes.sum())
            ms = [a.elapsed_time(z) for a, z in events[name]]
            per_s = lambda x: {"median": statistics.median(x / (t * 1e-3) for t in ms), "min": x / (max(ms) * 1e-3),
                               "max": x / (min(ms) * 1e-3)}
            t0 = time.perf_counter()
            sets, offsets = solver.unavoidable(grids[:n], max_size=m, capacity=b["total"])
            torch.cuda.synchronize()
            whole = time.perf_counter() - t0
            res[name] = {"grids": n, "max_size": m, "rows": b["total"], "nodes": nodes, "minimal_sets": int(sets.shape[0]),
                         "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                         "grids_per_s": per_s(n), "nodes_per_s": per_s(nodes), "unavoidable_call_seconds": whole,
                         "cpu_host_build": {"threads": CPU_THREADS, "grids": sample, "nodes": int(hnodes.sum()), "seconds": secs,
                                            "grids_per_s": sample / secs, "nodes_per_s": int(hnodes.sum()) / secs,
                                            "answers_equal": True}}
            res[name]["gpu_over_cpu_nodes"] = res[name]["nodes_per_s"]["median"] / res[name]["cpu_host_build"]["nodes_per_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ua_rate.json"))
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
