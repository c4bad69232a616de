"""Rate of the batched completion count (BatchSolver.count_solutions, limit 2)
on one MI355X, recorded, not gated; bench.py is not involved.

    python scripts/count_bench.py                 # -> profiles/count_rate.json
    python scripts/count_bench.py --host-model    # passes per board on the CPU, no GPU

Inputs: 2^20 hard17_batch boards (17 clues, one completion: the count must
exhaust each search) and 2^20 boards erased to 50 empties (the hard17 boards'
full grids, 50 random cells of each erased on the device: mostly a few
completions, the count stops at the second).  For context BatchSolver.solve
runs on the same hard17 boards in the same process, the three launches
alternating; the solve path is the parent commit's.

Method: warm-up launches of every shape first, then --launches timed launches
of each, every one between two device events on the stream, one final
synchronise before the events are read.  Reported: median, min and max of
the launches' boards per second, and the count / solve ratio of the medians.
Without a GPU the measurement fails; nothing is written.

--host-model: the same searches' passes per board from the host builds of the
headers (tests/native/count_host.cpp, ahead_host.cpp) on 4096 hard17 boards:
what the count costs next to the solve in passes, before any drain effect.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_model(n=4096, seed=1):
    from sudoku_solver_distributed_amd.gen import hard17_batch
    boards = np.ascontiguousarray(hard17_batch(n, seed=seed).numpy())
    tmp = tempfile.mkdtemp()
    libs = {}
    for name in ("count_host", "ahead_host"):
        out = os.path.join(tmp, f"lib{name}.so")
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", out,
                               os.path.join(ROOT, "tests", "native", name + ".cpp")])
        libs[name] = ctypes.CDLL(out)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    cnt = np.zeros(n, dtype=np.int32)
    p, d = ctypes.c_uint64(), u32()
    f = libs["count_host"].count_host_batch
    f.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int32, u32, vp, vp]
    f(boards.ctypes.data, cnt.ctypes.data, None, n, 2, 81, ctypes.byref(p), ctypes.byref(d))
    assert (cnt == 1).all()
    g = libs["ahead_host"].ahead_solve_batch
    g.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int, u32, u32, ctypes.c_int, vp, vp]
    out, st = np.zeros_like(boards), np.zeros(n, dtype=np.int32)
    gs, ps = ctypes.c_uint64(), ctypes.c_uint64()
    g(boards.ctypes.data, out.ctypes.data, st.ctypes.data, n, 0, 32, 128, 1, ctypes.byref(gs), ctypes.byref(ps))
    res = {"boards": n, "seed": seed, "count_limit2_passes_per_board": p.value / n,
           "solve_passes_per_board": ps.value / n, "count_deepest_stack_level": d.value}
    res["passes_ratio_count_over_solve"] = res["count_limit2_passes_per_board"] / res["solve_passes_per_board"]
    return res


def measure(n, launches, warmup):
    import torch
    from sudoku_solver_distributed_amd.gen import hard17_batch
    from sudoku_solver_distributed_amd.solver import get_solver
    solver = get_solver("cuda:0")
    dev = solver.device
    hard = hard17_batch(n, seed=1, device=dev)
    full, st = solver.solve(hard)
    assert bool((st == 1).all().item())
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    cells = torch.argsort(torch.rand((n, 81), device=dev, generator=gen), dim=1)[:, :50]
    e50 = full.scatter(1, cells, 0)
    out, status = torch.empty_like(hard), torch.empty(n, dtype=torch.int32, device=dev)
    shapes = {
        "count_hard17": lambda: solver.count_solutions(hard, limit=2),
        "solve_hard17": lambda: solver.solve(hard, out=out, status=status),
        "count_erased50": lambda: solver.count_solutions(e50, limit=2),
    }
    c_hard = shapes["count_hard17"]()
    c_e50 = shapes["count_erased50"]()
    assert bool((c_hard == 1).all().item())  # and the first launches are warm-up
    for _ in range(warmup):
        for f in shapes.values():
            f()
    torch.cuda.synchronize()
    events = {k: [] for k in shapes}
    for _ in range(launches):
        for k, f in shapes.items():  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    res = {"boards_per_launch": n, "launches": launches, "warmup": warmup, "limit": 2,
           "device": torch.cuda.get_device_name(dev),
           "erased50_counts": {"0": int((c_e50 == 0).sum()), "1": int((c_e50 == 1).sum()), "2": int((c_e50 == 2).sum())}}
    for k, evs in events.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        rate = sorted(n / (t * 1e-3) for t in ms)
        res[k] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                  "boards_per_s_median": statistics.median(rate), "boards_per_s_min": rate[0],
                  "boards_per_s_max": rate[-1]}
    res["count_over_solve_hard17"] = res["count_hard17"]["boards_per_s_median"] / res["solve_hard17"]["boards_per_s_median"]
    solver.verify()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_rate.json"))
    ap.add_argument("--host-model", action="store_true")
    a = ap.parse_args()
    if a.host_model:
        print(json.dumps(host_model()))
        return
    if a.launches < 10:
        ap.error("at least 10 timed launches")
    res = measure(a.boards, a.launches, a.warmup)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
