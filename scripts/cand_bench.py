"""Rate of the batched exact candidates (BatchSolver.candidates) on one
MI355X, recorded, not gated; bench.py is not involved.

    python scripts/cand_bench.py                 # -> profiles/cand_rate.json
    python scripts/cand_bench.py --host-model    # passes and searches per board on the CPU, no GPU
    SDK_LIB=.../libsudoku_hip_sweep8.so python scripts/cand_bench.py --trial sweep8
                                                 # an A/B build's figures into the file's "trials"

Inputs, 2^16 boards a launch: hard17_batch boards (17 clues, one completion:
the sweep is the whole answer, the very search count_solutions(limit=2) runs --
timed beside it on the same boards, and the ratio reported); their full grids
with 50 random cells erased on the device (mostly a few completions); and the
boards with one random clue removed (16 clues, very many completions: the
targeted searches do the work).

Method (count_bench.py's): warm-up rounds of every shape first, then
--launches timed launches of each, the shapes alternating in one process,
every launch between two device events on the stream, one final synchronise
before the events are read.  Reported: median, min and max of the launches'
milliseconds and boards per second.  Without a GPU the measurement fails;
nothing is written.

--host-model: passes and targeted searches per board from the host build of
plane_cand.h (tests/native/cand_host.cpp) on the same three kinds of boards
(1024, 1024 and 256 of them, made on the host), at SDK_CAND_SWEEP 2, 8 and 64:
what the device time can be set against.
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
SWEEPS = (2, 8, 64)


def host_model(seed=1):
    from sudoku_solver_distributed_amd.gen import hard17_batch
    out = os.path.join(tempfile.mkdtemp(), "libcand_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", out,
                           os.path.join(ROOT, "tests", "native", "cand_host.cpp")])
    f = ctypes.CDLL(out).cand_host_batch
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    f.argtypes = [vp, vp, vp, ctypes.c_int64, u32, u32, vp]

    def run(boards, sweep):
        boards = np.ascontiguousarray(boards)
        marks = np.zeros((len(boards), 81), dtype=np.uint16)
        count = np.zeros(len(boards), dtype=np.int32)
        st = (ctypes.c_uint64 * 3)()
        f(boards.ctypes.data, marks.ctypes.data, count.ctypes.data, len(boards), 81, sweep, st)
        return marks, count, {"passes_per_board": st[0] / len(boards), "searches_per_board": st[1] / len(boards),
                              "deepest_stack_level": int(st[2])}

    rng = np.random.default_rng(seed)
    hard = hard17_batch(1024, seed=seed).numpy()
    marks, count, _ = run(hard, 2)
    assert (count == 1).all()
    full = (np.log2(marks.astype(np.float64)) + 1).astype(np.uint8)  # single bits: the completion
    e50 = full.copy()
    for g in e50:
        g[rng.choice(81, 50, replace=False)] = 0
    minus1 = hard[:256].copy()
    for g in minus1:
        g[rng.choice(np.nonzero(g)[0])] = 0
    res = {"seed": seed}
    for name, boards in (("hard17", hard), ("erased50", e50), ("minus1", minus1)):
        res[name] = {"boards": len(boards)}
        for sweep in SWEEPS:
            res[name][f"sweep{sweep}"] = run(boards, sweep)[2]
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
    clue = torch.argmax(torch.rand((n, 81), device=dev, generator=gen) * (hard != 0), dim=1, keepdim=True)
    minus1 = hard.scatter(1, clue, 0)
    assert bool(((minus1 != 0).sum(1) == 16).all().item())
    shapes = {
        "cand_hard17": lambda: solver.candidates(hard, return_count=True),
        "count_hard17": lambda: solver.count_solutions(hard, limit=2),
        "cand_erased50": lambda: solver.candidates(e50, return_count=True),
        "cand_minus1": lambda: solver.candidates(minus1, return_count=True),
    }
    m, c = shapes["cand_hard17"]()  # (and the first launches are warm-up)
    assert bool((c == 1).all().item()) and torch.equal(m.to(torch.int64), torch.ones_like(m, dtype=torch.int64) << (full.to(torch.int64) - 1))
    _, c_e50 = shapes["cand_erased50"]()
    assert torch.equal(c_e50, solver.count_solutions(e50, limit=2))
    m1, c_m1 = shapes["cand_minus1"]()
    assert bool((c_m1 == 2).all().item())
    width = lambda marks: float(((marks.to(torch.int32).unsqueeze(2) >> torch.arange(9, device=dev)) & 1).sum(2).float().mean())
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
           "erased50_counts": {"0": int((c_e50 == 0).sum()), "1": int((c_e50 == 1).sum()), "2": int((c_e50 == 2).sum())},
           "candidates_per_cell": {"erased50": width(solver.candidates(e50)), "minus1": width(m1)}}
    for k, evs in events.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        rate = sorted(n / (t * 1e-3) for t in ms)
        res[k] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                  "boards_per_s_median": statistics.median(rate), "boards_per_s_min": rate[0],
                  "boards_per_s_max": rate[-1]}
    res["cand_over_count_hard17_ms"] = res["cand_hard17"]["ms_median"] / res["count_hard17"]["ms_median"]
    solver.verify()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=1 << 16)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cand_rate.json"))
    ap.add_argument("--trial", default=None, help="store the result under trials[NAME] of the file instead of replacing it")
    ap.add_argument("--host-model", action="store_true")
    a = ap.parse_args()
    if a.host_model:
        print(json.dumps(host_model()))
        return
    if a.launches < 10:
        ap.error("at least 10 timed launches")
    res = measure(a.boards, a.launches, a.warmup)
    doc = res
    if a.trial:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc.setdefault("trials", {})[a.trial] = res
    elif os.path.exists(a.out):
        with open(a.out) as f:
            doc = dict(res, **{k: v for k, v in json.load(f).items() if k in ("trials", "host_model")})
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
