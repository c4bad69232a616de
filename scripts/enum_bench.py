"""Time of the completion list (BatchSolver.completions, sdk_enumerate_batch) on
one MI355X, recorded, not gated; bench.py is not involved.

    python scripts/enum_bench.py                 # -> profiles/enum_rate.json

1. heavy_alone: the fixture boards H2 (7 299 350 completions) and H1 (885 469)
   alone on the full grid, listed (the raw entry: no sort, no grouping) against
   count_exact at the same knobs.  The ratio is the cost of emission.
2. batch_d: 2^16 full grids with 50 cells erased (DESIGN.md §20's batch), listed
   with limit 0 and limit 64, against count_exact and count_solutions(limit=1024)
   on the same boards.
3. sort: completions(sort=True) against sort=False on H2: the cost of the sort.

Every launch is asserted against the known counts.  Method: warm-up launches of
every shape first, then --launches timed launches of each, alternating in one
process, every one between two device events on the stream (the calls are
synchronous, so the events span their rounds and the host's read-backs).
Reported: median, min and max in ms.  Without a GPU the measurement fails;
nothing is written.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

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
    dev, lib = solver.device, solver.lib
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
    over = capped >= 1024
    batch[over] = batch[~over][:1]
    capped = solver.count_solutions(batch, limit=1024).to(torch.int64)
    assert int(capped.max()) < 1024 and int(capped.min()) >= 1
    batch_total = int(capped.sum())
    infos = {}

    def raw(boards, capacity, limit, want_count, want_total, key):
        """The entry itself on preallocated buffers: what emission costs, without torch's share."""
        n = boards.shape[0]
        grids = torch.empty((capacity, 81), dtype=torch.uint8, device=dev)
        owner = torch.empty(capacity, dtype=torch.int32, device=dev)
        count = torch.empty(n, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        need = int(lib.sdk_enumerate_scratch_bytes(n, 0, 0))
        sc = torch.empty(need, dtype=torch.uint8, device=dev)
        st = (ctypes.c_int64 * 6)()

        def run():
            rc = lib.sdk_enumerate_batch(boards.data_ptr(), n, grids.data_ptr(), owner.data_ptr(), capacity, limit,
                                         count.data_ptr(), status.data_ptr(), EXACT_SLICE, EXACT_MAX_ROUNDS, 0,
                                         sc.data_ptr(), need, 0, int(torch.cuda.current_stream(dev).cuda_stream), st)
            assert rc == 0 and st[4] == want_total and st[5] == want_total, (key, list(st))
            assert bool((count == want_count).all()), key
            infos[key] = dict(zip(("rounds", "donated", "parks", "max_passes", "total", "listed"), (int(v) for v in st)))
        return run

    def exact(boards, want_count, key):
        def run():
            c = solver.count_exact(boards)
            assert bool((c == want_count).all()), key
        return run

    res = {"device": torch.cuda.get_device_name(dev), "defaults": {"slice": EXACT_SLICE, "max_rounds": EXACT_MAX_ROUNDS},
           "grid_waves": int(lib.sdk_device_cu_count()) * 16, "warmup": warmup}
    # 1. the heavy boards alone
    shapes = {}
    for k, (b, v) in heavy.items():
        want = torch.tensor([v], dtype=torch.int64, device=dev)
        shapes[f"{k}_enumerate"] = raw(b, v, 0, want, v, f"{k}_enumerate")
        shapes[f"{k}_count_exact"] = exact(b, want, f"{k}_count_exact")
    res["heavy_alone"] = _timed(torch, shapes, launches, warmup)
    for k in heavy:
        res["heavy_alone"][f"{k}_emission_ratio"] = (res["heavy_alone"][f"{k}_enumerate"]["ms_median"] /
                                                     res["heavy_alone"][f"{k}_count_exact"]["ms_median"])
    # 2. the light batch
    lim = torch.clamp(capped, max=64)
    shapes = {"enumerate_limit0": raw(batch, batch_total, 0, capped, batch_total, "batch_limit0"),
              "enumerate_limit64": raw(batch, int(lim.sum()), 64, lim, int(lim.sum()), "batch_limit64"),
              "count_exact": exact(batch, capped, "batch_exact"),
              "capped_limit1024": lambda: solver.count_solutions(batch, limit=1024)}
    res["batch_d"] = dict(_timed(torch, shapes, launches, warmup), boards=batch_boards, replaced_at_cap=int(over.sum()),
                          rows_limit0=batch_total, rows_limit64=int(lim.sum()))
    # 3. the sort, on H2
    h2, v2 = heavy["h2"]

    def listed(sort):
        def run():
            g, off = solver.completions(h2, capacity=v2, sort=sort)
            assert g.shape[0] == v2 and int(off[1]) == v2
        return run

    res["sort_h2"] = _timed(torch, {"sort_true": listed(True), "sort_false": listed(False)}, launches, warmup)
    res["info"] = infos
    solver.verify()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1 << 16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enum_rate.json"))
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
