"""Time of the exact completion count (BatchSolver.count_exact) on one MI355X,
recorded, not gated; bench.py is not involved.

    python scripts/exact_bench.py                 # -> profiles/exact_rate.json

1. h2_alone: the heavy fixture board H2 (7 299 350 completions,
   tests/golden/exact_cases.json) alone, at the default knobs on the full grid,
   against the SAME build with the sharing confined to one wave (max_waves=1:
   64 lanes, the default slice).  That second figure is an A/B of the feature's
   own knob, not an outside yardstick; the outside figure is the oracle's time
   for the same board on a CPU, and the correctness yardstick is the fixture
   value, asserted on every launch.  Sharing switched off altogether (one lane,
   a slice above any pass count) is one launch of minutes: not run, see
   DESIGN.md §20.  H1 (885 469) is timed the same way.
2. batch_d: 2^16 full grids with 50 cells erased (every count far below 1024):
   count_exact against count_solutions(limit=1024), the capped kernel; both
   must give the same numbers.
3. sweep: slice x max_tasks (whose ring caps the fill target below two lines a
   lane) on H2 and on the batch, and the empty board's wall time at the default
   round budget (PARTIAL by construction).

Method: warm-up launches of every shape first, then --launches timed launches
of each, alternating in one process, every one between two device events on
the stream (count_exact is synchronous, so the events span its rounds and the
host's read-backs between them).  Reported: median, min and max in ms.
Without a GPU the measurement fails; nothing is written.
"""
import argparse
import json
import os
import statistics
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "exact_cases.json")


def _timed(torch, shapes, launches, warmup):
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
    out = {}
    for k, evs in events.items():
        ms = [a.elapsed_time(b) for a, b in evs]
        out[k] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "launches": len(ms)}
    return out


def measure(launches, warmup, batch_boards):
    import torch
    from sudoku_solver_distributed_amd.solver import EXACT_MAX_ROUNDS, EXACT_SLICE, get_solver
    solver = get_solver("cuda:0")
    dev = solver.device
    with open(FIXTURE) as f:
        fx = json.load(f)
    heavy = {k: (torch.tensor([[int(c) for c in fx[k]["board"]]], dtype=torch.uint8, device=dev), int(fx[k]["count"]))
             for k in ("h1", "h2")}
    full = solver.random_grids(batch_boards, seed=7)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    cells = torch.argsort(torch.rand((batch_boards, 81), device=dev, generator=gen), dim=1)[:, :50]
    batch = full.scatter(1, cells, 0)
    capped = solver.count_solutions(batch, limit=1024)
    over = capped >= 1024  # (a board at the cap has no exact number to compare with: an empty copy of a light one)
    batch[over] = batch[~over][:1]
    capped = solver.count_solutions(batch, limit=1024).to(torch.int64)
    assert int(capped.max()) < 1024 and int(capped.min()) >= 1
    stats = {}

    def exact(boards, want, key, **kw):
        def run():
            c, st = solver.count_exact(boards, return_stats=True, **kw)
            assert want(c), key
            stats[key] = st
        return run

    def is_count(v):
        return lambda c: int(c[0]) == v

    same_as_capped = lambda c: bool((c == capped).all())  # noqa: E731
    res = {"device": torch.cuda.get_device_name(dev), "defaults": {"slice": EXACT_SLICE, "max_rounds": EXACT_MAX_ROUNDS},
           "grid_waves": int(solver.lib.sdk_device_cu_count()) * 16, "warmup": warmup}
    # 1. the heavy boards alone, full grid against one wave (few launches of the slow shape)
    shapes = {f"{k}_default": exact(b, is_count(v), f"{k}_default") for k, (b, v) in heavy.items()}
    res["heavy_alone"] = _timed(torch, shapes, launches, warmup)
    one = {f"{k}_one_wave": exact(b, is_count(v), f"{k}_one_wave", max_waves=1, max_rounds=1 << 24)
           for k, (b, v) in heavy.items()}
    res["heavy_alone"].update(_timed(torch, one, 3, 1))
    # 2. the light batch against the capped kernel
    shapes = {"exact": exact(batch, same_as_capped, "batch_exact"),
              "capped_limit1024": lambda: solver.count_solutions(batch, limit=1024)}
    res["batch_d"] = dict(_timed(torch, shapes, launches, warmup), boards=batch_boards,
                          replaced_at_cap=int(over.sum()), count_max=int(capped.max()),
                          count_mean=float(capped.float().mean()))
    # 3. the sweep
    lanes = res["grid_waves"] * 64
    sweep = {}
    for s in (32, 128, 256, 1024, 4096):
        for tasks in (lanes // 4, 0):
            tag = f"slice{s}_tasks{tasks}"
            sweep.update(_timed(torch, {f"h2_{tag}": exact(heavy["h2"][0], is_count(heavy["h2"][1]), f"h2_{tag}", slice=s,
                                                          max_tasks=tasks, max_rounds=1 << 20),
                                        f"batch_{tag}": exact(batch, same_as_capped, f"batch_{tag}", slice=s,
                                                              max_tasks=tasks, max_rounds=1 << 20)}, 3, 1))
    res["sweep"] = sweep
    empty = torch.zeros((1, 81), dtype=torch.uint8, device=dev)
    res["empty_board"] = {}
    for rounds in (64, EXACT_MAX_ROUNDS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        c, status, st = solver.count_exact(empty, max_rounds=rounds, return_status=True, return_stats=True)
        wall = time.perf_counter() - t
        assert int(status[0]) == 2 and st["rounds"] == rounds
        res["empty_board"][f"rounds{rounds}"] = {"wall_s": wall, "lower_bound": int(c[0]), "stats": st}
    res["stats"] = stats
    for k, v in res["heavy_alone"].items():
        v["ms_per_round"] = v["ms_median"] / stats[k]["rounds"]
    solver.verify()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1 << 16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_rate.json"))
    a = ap.parse_args()
    if a.launches < 10:
        ap.error("at least 10 timed launches")
    res = measure(a.launches, a.warmup, a.batch)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
