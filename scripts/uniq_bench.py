"""Rate of the batched unique candidates (BatchSolver.unique_candidates) on
one MI355X against the composition it replaces; bench.py is not involved.

    python scripts/uniq_bench.py                 # -> profiles/uniq_rate.json
    python scripts/uniq_bench.py --host-model    # passes per board on the CPU, no GPU

The yardstick is the composition from calls that were there before
(tests/uniq_cases.py composed(): candidates, then count_solutions(limit=2) over
every candidate placement of an empty cell); both must give identical arrays
(asserted before anything is timed).

Shape 1, 2^14 boards: hard17_batch boards' full grids with 50 random cells
erased on the device (a few to a few dozen completions: the sweep alone answers
them).  Acceptance: the new call's median is not above the yardstick's median
by more than the yardstick's own max - min.  Shape 2, 2^14 boards: hard17_batch
boards with one random clue removed (16 clues, the exchange's own shape):
recorded, no threshold.  Also recorded: gen.exchange on the 80 hard17_classes
puzzles (neighbours, classes among them, milliseconds).

Method (count_bench.py's): warm-up rounds of every shape first, then
--launches (>= 8) timed launches of each, the shapes alternating in one
process, every launch between two device events on the stream, one final
synchronise before the events are read.  Reported: median, min and max of the
launches' milliseconds.  Without a GPU the measurement fails; nothing is
written.

--host-model: passes per board from the host build of plane_uniq.h
(tests/native/uniq_host.cpp) on hard17 boards, on the two shapes' kinds of
boards (1024, 1024 and 256 of them, made on the host) and on the test fixture,
at SDK_UNIQ_SWEEP 2, 16, 64, 256 and 1024: all passes, those of the sweep,
targeted searches, and the slowest board.  The default sweep was chosen from
this table.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
SWEEPS = (2, 16, 64, 256, 1024)


def host_model(seed=1):
    from sudoku_solver_distributed_amd.gen import hard17_batch
    import uniq_cases as U
    out = os.path.join(tempfile.mkdtemp(), "libuniq_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", out,
                           os.path.join(ROOT, "tests", "native", "uniq_host.cpp")])
    f = ctypes.CDLL(out).uniq_host_batch
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    f.argtypes = [vp, vp, vp, vp, ctypes.c_int64, u32, u32, vp, vp]

    def run(boards, sweep):
        boards = np.ascontiguousarray(boards)
        n = len(boards)
        once, marks = np.zeros((n, 81), dtype=np.uint16), np.zeros((n, 81), dtype=np.uint16)
        count = np.zeros(n, dtype=np.int32)
        st = (ctypes.c_uint64 * 5)()
        f(boards.ctypes.data, once.ctypes.data, marks.ctypes.data, count.ctypes.data, n, 81, sweep, st, None)
        return once, marks, count, {"passes_per_board": st[0] / n, "sweep_passes_per_board": st[1] / n,
                                    "targeted_passes_per_board": (st[0] - st[1]) / n, "searches_per_board": st[2] / n,
                                    "deepest_stack_level": int(st[3]), "slowest_board_passes": int(st[4])}

    rng = np.random.default_rng(seed)
    hard = hard17_batch(1024, seed=seed).numpy()
    once, marks, count, _ = run(hard, 2)
    assert (count == 1).all() and np.array_equal(once, marks)
    full = (np.log2(marks.astype(np.float64)) + 1).astype(np.uint8)  # single bits: the completion
    e50 = full.copy()
    for g in e50:
        g[rng.choice(81, 50, replace=False)] = 0
    minus1 = hard[:256].copy()
    for g in minus1:
        g[rng.choice(np.nonzero(g)[0])] = 0
    fixture = U.load_fixture()[1]
    res = {"seed": seed}
    for name, boards in (("hard17", hard), ("erased50", e50), ("minus1", minus1), ("fixture", fixture)):
        res[name] = {"boards": len(boards)}
        ref = None
        for sweep in SWEEPS:
            o, m, c, st = run(boards, sweep)
            ref = ref or (o, m, c)
            assert all(np.array_equal(a, b) for a, b in zip(ref, (o, m, c)))  # results never depend on the sweep
            res[name][f"sweep{sweep}"] = st
    return res


def measure(n, launches, warmup):
    import torch
    import uniq_cases as U
    from sudoku_solver_distributed_amd import gen
    from sudoku_solver_distributed_amd.solver import get_solver
    solver = get_solver("cuda:0")
    dev = solver.device
    hard = gen.hard17_batch(n, seed=1, device=dev)
    full, st = solver.solve(hard)
    assert bool((st == 1).all().item())
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    cells = torch.argsort(torch.rand((n, 81), device=dev, generator=g), dim=1)[:, :50]
    e50 = full.scatter(1, cells, 0)
    clue = torch.argmax(torch.rand((n, 81), device=dev, generator=g) * (hard != 0), dim=1, keepdim=True)
    minus1 = hard.scatter(1, clue, 0)
    assert bool(((minus1 != 0).sum(1) == 16).all().item())
    shapes = {
        "uniq_erased50": lambda: solver.unique_candidates(e50, return_marks=True, return_count=True),
        "composed_erased50": lambda: U.composed(solver, e50)[:3],
        "uniq_minus1": lambda: solver.unique_candidates(minus1, return_marks=True, return_count=True),
        "composed_minus1": lambda: U.composed(solver, minus1)[:3],
    }
    info = {}
    for kind, boards in (("erased50", e50), ("minus1", minus1)):  # identical arrays (and the first launches are warm-up)
        a, b = shapes[f"uniq_{kind}"](), shapes[f"composed_{kind}"]()
        assert all(torch.equal(x, y) for x, y in zip(a, b)), kind
        pop = lambda t: int(sum(((t.to(torch.int32) >> d) & 1).sum() for d in range(9)))
        empty = boards == 0
        info[kind] = {"once_bits_of_empty_cells_per_board": pop(a[0] * empty) / n,
                      "marks_bits_of_empty_cells_per_board": pop(a[1] * empty) / n,
                      "counts": {str(k): int((a[2] == k).sum()) for k in (0, 1, 2)}}
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
    res = {"boards_per_launch": n, "launches": launches, "warmup": warmup, "device": torch.cuda.get_device_name(dev),
           "boards": info}
    for k, evs in events.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        res[k] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms_spread": max(ms) - min(ms),
                  "boards_per_s_median": n / (statistics.median(ms) * 1e-3)}
    for kind in ("erased50", "minus1"):
        res[f"uniq_over_composed_{kind}_ms"] = res[f"uniq_{kind}"]["ms_median"] / res[f"composed_{kind}"]["ms_median"]
    y = res["composed_erased50"]
    res["acceptance_erased50"] = {"rule": "uniq median <= composed median + (composed max - composed min)",
                                  "bound_ms": y["ms_median"] + y["ms_spread"],
                                  "met": res["uniq_erased50"]["ms_median"] <= y["ms_median"] + y["ms_spread"]}
    # exchange on the corpus: neighbours found, classes among them
    classes = torch.from_numpy(np.array([[int(c) for c in s] for s in gen.hard17_classes()], dtype=np.uint8)).to(dev)
    gen.exchange(classes)  # warm-up (and the scratch's size)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nb = gen.exchange(classes)[0]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    canon = solver.canonical(nb)
    both = torch.unique(torch.cat([solver.canonical(classes), canon]), dim=0).shape[0]
    res["exchange_hard17_classes"] = {"puzzles": int(classes.shape[0]), "neighbours": int(nb.shape[0]),
                                      "classes_among_neighbours": int(torch.unique(canon, dim=0).shape[0]),
                                      "classes_not_in_the_corpus": both - int(classes.shape[0]), "ms": ms}
    solver.verify()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=1 << 14)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uniq_rate.json"))
    ap.add_argument("--host-model", action="store_true")
    a = ap.parse_args()
    if a.host_model:
        print(json.dumps(host_model(), indent=1))
        return
    if a.launches < 8:
        ap.error("at least 8 timed launches")
    res = measure(a.boards, a.launches, a.warmup)
    doc = res
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = dict(res, **{k: v for k, v in json.load(f).items() if k == "host_model"})
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
