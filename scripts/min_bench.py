"""Rate of the batched minimisation (BatchSolver.minimize) on one MI355X
against the loop it replaces, recorded, not gated; bench.py is not involved.

    python scripts/min_bench.py                 # -> profiles/min_rate.json
    python scripts/min_bench.py --host-model    # passes per board on the CPU, no GPU
    python scripts/min_bench.py --boards 262144 --trial boards_262144
                                                # another batch size into the file's "trials"

Inputs: full grids made once with generate_batch(n, 0, seed), 2^16 of them,
and each board's random turn order as gen.unique_batch draws it.  Two shapes,
the same grids and orders for both:

  rounds81  gen.unique_batch's 81-round loop (a scatter / gather / where over
            the batch and one count_solutions(limit=2) launch per round),
            restated below line for line: unique_batch draws its own grids
            inside the call, so the loop alone cannot be timed through it.
            The yardstick, not the code under test.
  fused     one minimize(full, order, max_empty=81) call.

Both give the same puzzles (asserted).  Also minimize(probe=True) on
hard17_batch boards, where every one of the 17 tests has to find a second
completion by search, as boards per second.

Method (DESIGN.md §12's): three warm-up rounds of every shape first, then
--runs timed runs of each (at least 8), the shapes alternating in one process,
every run between two device events on the stream, one final synchronise
before the events are read.  Reported: median, min and max of the runs'
milliseconds.  accept: fused's median is not above rounds81's by more than
rounds81's own max - min.  Without a GPU the measurement fails; nothing is
written.

--host-model: passes per board of the host build of plane_min.h
(tests/native/min_host.cpp) on the fixture's 32 full grids with their orders,
against 81 rounds of the count's host model (tests/native/count_host.cpp) at
limit 2 on the same grids and orders: what the refutation claim rests on.
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


def host_model():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import min_cases as M
    fx = M.load_fixture()
    tmp = tempfile.mkdtemp()
    libs = {}
    for name in ("min_host", "count_host"):
        out = os.path.join(tmp, f"lib{name}.so")
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", out,
                               os.path.join(ROOT, "tests", "native", name + ".cpp")])
        libs[name] = ctypes.CDLL(out)
    vp, i64, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32
    fmin, fcount = libs["min_host"].min_host_batch, libs["count_host"].count_host_batch
    fmin.argtypes = [vp, vp, vp, vp, vp, i64, ctypes.c_int, ctypes.c_int, u32, vp]
    fcount.argtypes = [vp, vp, vp, i64, ctypes.c_int32, u32, vp, vp]
    sel = [k for k, n in enumerate(fx["names"]) if n.startswith("g_") and n[2:].isdigit()]
    grids, order = np.ascontiguousarray(fx["boards"][sel]), np.ascontiguousarray(fx["order"][sel])
    n = len(sel)
    out, status, removed = np.zeros((n, 81), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
    st = (ctypes.c_uint64 * 3)()
    fmin(grids.ctypes.data, order.ctypes.data, out.ctypes.data, status.ctypes.data, removed.ctypes.data, n, 0, 81, 81, st)
    puzzle, rounds = grids.copy(), 0
    for t in range(81):
        trial = puzzle.copy()
        trial[np.arange(n), order[:, t]] = 0
        cnt = np.zeros(n, dtype=np.int32)
        passes, deepest = ctypes.c_uint64(0), ctypes.c_uint32(0)
        fcount(trial.ctypes.data, cnt.ctypes.data, None, n, 2, 81, ctypes.byref(passes), ctypes.byref(deepest))
        rounds += passes.value
        puzzle = np.where((cnt == 1)[:, None], trial, puzzle)
    assert np.array_equal(puzzle, out) and (status == 1).all()
    return {"boards": n, "clues_left_min": int((out != 0).sum(1).min()), "clues_left_max": int((out != 0).sum(1).max()),
            "fused_passes_per_board": st[0] / n, "fused_tests_per_board": st[1] / n, "deepest_stack_level": int(st[2]),
            "rounds81_passes_per_board": rounds / n, "rounds81_over_fused": rounds / st[0]}


def rounds81(solver, full, order, empty_boxes):
    """gen.unique_batch's step 3 on given grids and orders."""
    import torch
    n = full.shape[0]
    puzzle = full.clone()
    empties = torch.zeros(n, dtype=torch.int64, device=full.device)
    zero = torch.zeros((), dtype=torch.uint8, device=full.device)
    for t in range(81 if n and empty_boxes > 0 else 0):
        cell = order[:, t:t + 1]
        live = (empties < empty_boxes).unsqueeze(1)
        trial = puzzle.scatter(1, cell, torch.where(live, zero, puzzle.gather(1, cell)))
        keep = live & (solver.count_solutions(trial, limit=2) == 1).unsqueeze(1)
        puzzle = torch.where(keep, trial, puzzle)
        empties += keep.squeeze(1)
    return puzzle


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def measure(n, runs, warmup, seed):
    import torch
    from sudoku_solver_distributed_amd.gen import generate_batch, hard17_batch
    from sudoku_solver_distributed_amd.solver import get_solver
    solver = get_solver("cuda:0")
    dev = solver.device
    full = generate_batch(n, 0, seed, device=dev)
    order_np = np.argsort(np.random.default_rng(seed).random((n, 81)), axis=1)
    order64 = torch.as_tensor(order_np, dtype=torch.int64, device=dev)
    order8 = torch.as_tensor(order_np.astype(np.uint8), device=dev)
    hard = hard17_batch(n, seed=seed, device=dev)
    shapes = {
        "rounds81": lambda: rounds81(solver, full, order64, 81),
        "fused": lambda: solver.minimize(full, order8, return_removed=True),
        "probe_hard17": lambda: solver.minimize(hard, probe=True, return_removed=True),
    }
    want = shapes["rounds81"]()  # (and the first launches are warm-up)
    got, status, removed = shapes["fused"]()
    assert torch.equal(got, want) and bool((status == 1).all().item())
    _, hs, hr = shapes["probe_hard17"]()
    assert bool((hs == 1).all().item()) and not bool(hr.any().item())  # 17-clue puzzles are minimal
    for _ in range(warmup):
        for f in shapes.values():
            f()
    torch.cuda.synchronize()
    events = {k: [] for k in shapes}
    for _ in range(runs):
        for k, f in shapes.items():  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    clues = (got != 0).sum(1)
    res = {"boards": n, "runs": runs, "warmup": warmup, "seed": seed, "device": torch.cuda.get_device_name(dev),
           "clues_left": {"min": int(clues.min()), "mean": float(clues.float().mean()), "max": int(clues.max())}}
    for k, evs in events.items():
        res[k] = stats([a.elapsed_time(b) for a, b in evs])
        res[k]["boards_per_s_median"] = n / (res[k]["ms_median"] * 1e-3)
    a, b = res["rounds81"], res["fused"]
    res["rounds81_over_fused_ms"] = a["ms_median"] / b["ms_median"]
    res["accept"] = b["ms_median"] <= a["ms_median"] + (a["ms_max"] - a["ms_min"])
    solver.verify()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=1 << 16)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "min_rate.json"))
    ap.add_argument("--trial", default=None, help="store the result under trials[NAME] of the file instead of replacing it")
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
        res = measure(a.boards, a.runs, a.warmup, a.seed)
        if a.trial:
            doc.setdefault("trials", {})[a.trial] = res
        else:
            doc = dict(res, **{k: v for k, v in doc.items() if k in ("trials", "host_model")})
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
