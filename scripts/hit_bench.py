"""Rate of the hitting-set search (sdk_hitting_sets_batch, what
BatchSolver.hitting_sets and sub_puzzles run) on one MI355X, recorded, not
gated; bench.py is not involved.

    python scripts/hit_bench.py          # -> profiles/hit_rate.json

Shapes (sets: the grids' minimal unavoidable sets at 12 cells):
  a  random_grids(N, seed=1), A all 81 cells, R empty, count only, at k = 12
     and 13: below the grids' hitting numbers (15 or 16), so every launch
     walks each family to the end and counts 0.  At tau - 1 and tau themselves
     one grid is 3 x 10^7 and 3 x 10^8 nodes and more, minutes for the host
     comparison: not run.  N is 4096 unless a probe launch of 8 grids says
     that 4096 would run longer than --budget seconds; then the largest power
     of two that fits.
  b  the unique_batch(4096, seed=5) puzzles P with the most common number of
     clues, A = P plus 5 of the grid's digits, k = |P|, every row listed: the
     kernel alone, and BatchSolver.sub_puzzles end to end by the host's clock.
  c  one hard17 puzzle: gen.neighbourhood at d = 1, 2 and 3 by the host's clock
     (unavoidable, hitting sets, boards, count_solutions, sort).
  d  one hard17 grid, A all cells, R empty, count only, k rising from tau
     while a launch stays under --budget seconds: one launch a k, with the
     counts; then gen.min_hitting_clues of that grid by the host's clock.

Method for a and b: --warmup launches of every shape first, then --launches
timed launches of each, the shapes alternating, every launch between two
device events on the stream, one final synchronise before the events are read.
Reported: median, min and max of the launches' nodes per second and rows per
second.  A node is one start() or step() call of csrc/hit.h -- one iteration
of a lane; the nodes of a family depend on the family, k and the task cut
alone and are counted by the host build.

CPU baseline: the host build of csrc/hit.h (tests/native/hit_host.cpp, g++ -O2
-fopenmp) with 16 threads on the first families of each shape, wall time of
the call; the GPU's counts of those families are checked against it, and for
b the rows as sets.  The file is written after every section.  Without a GPU
the measurement fails.
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
CPU_THREADS = 16


def host_build(tmp):
    so = os.path.join(tmp, "libhit_host.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-fopenmp", "-o", so,
                    os.path.join(ROOT, "tests", "native", "hit_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.hit_host_batch.argtypes = [vp, vp, vp, vp, i64, i, i64, vp, i64, vp, vp, vp, vp, i]
    lib.hit_host_batch.restype = i
    return lib


def host_run(lib, fam, lo, hi, k, capacity, mode, limit=0):
    """(seconds, rows, count, nodes) of the host build on families lo..hi of
    fam = (sets (S, 4) uint32, offsets, allowed (n, 4), required (n, 4))."""
    sets, offsets, A, R = fam
    off = np.ascontiguousarray(offsets[lo:hi + 1] - offsets[lo])
    s = np.ascontiguousarray(sets[offsets[lo]:offsets[hi]])
    a, r = np.ascontiguousarray(A[lo:hi]), np.ascontiguousarray(R[lo:hi])
    n = hi - lo
    rows = np.zeros((max(capacity, 1), 4), dtype=np.uint32)
    count, status = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    info, nodes = np.zeros(2, dtype=np.int64), np.zeros(n, dtype=np.uint64)
    t0 = time.perf_counter()
    rc = lib.hit_host_batch(s.ctypes.data, off.ctypes.data, a.ctypes.data, r.ctypes.data, n, k, limit, rows.ctypes.data,
                            capacity, count.ctypes.data, status.ctypes.data, info.ctypes.data, nodes.ctypes.data, mode)
    secs = time.perf_counter() - t0
    assert rc == 0 and (status >= 1).all()
    return secs, rows[:info[1]], count, nodes


def host_tau(lib, fam, lo, hi, start):
    """The hitting number of families lo..hi by the host build: limit 1 from
    `start` upward (fine tasks, nothing listed)."""
    tau = np.full(hi - lo, -1, dtype=np.int64)
    k = start
    while (tau < 0).any():
        _, _, count, _ = host_run(lib, fam, lo, hi, k, 0, 1, limit=1)
        tau[(tau < 0) & (count > 0)] = k
        k += 1
    return tau


def sorted_rows(rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 4)
    return rows[np.lexsort((rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]))]


class Shape:
    """One call's device arguments: families (sets, offsets, A, R as (., 4)
    int32 / int64 tensors), k and whether rows are listed.  The constructor
    runs the count once (probe_seconds, by the host's clock)."""

    def __init__(self, solver, sets, offsets, A, R, k, listed):
        import torch
        self.L, dev = solver.lib, solver.device
        self.sets, self.offsets, self.A, self.R, self.k = sets, offsets, A, R, k
        self.n = n = offsets.shape[0] - 1
        self.count = torch.empty(n, dtype=torch.int64, device=dev)
        self.status = torch.empty(n, dtype=torch.int32, device=dev)
        self.info = torch.zeros(2, dtype=torch.int64, device=dev)
        self.sc = torch.empty(int(self.L.sdk_hitting_sets_scratch_bytes(n, 0)), dtype=torch.uint8, device=dev)
        self.stream = int(torch.cuda.current_stream(dev).cuda_stream)
        self.rows, self.capacity = None, 0
        t0 = time.perf_counter()
        self.run()
        torch.cuda.synchronize()
        self.probe_seconds = time.perf_counter() - t0
        self.total = int(self.info.tolist()[0])
        if listed:
            self.capacity = self.total
            self.rows = torch.empty((max(self.total, 1), 4), dtype=torch.int32, device=dev)

    def run(self):
        rc = self.L.sdk_hitting_sets_batch(self.sets.data_ptr(), self.offsets.data_ptr(), self.A.data_ptr(), self.R.data_ptr(),
                                           self.n, self.k, 0, self.rows.data_ptr() if self.capacity else None, self.capacity,
                                           self.count.data_ptr(), self.status.data_ptr(), self.info.data_ptr(),
                                           self.sc.data_ptr(), self.sc.numel(), 0, self.stream)
        assert rc == 0

    def host_arrays(self):
        return (self.sets.cpu().numpy().view(np.uint32), self.offsets.cpu().numpy(), self.A.cpu().numpy().view(np.uint32),
                self.R.cpu().numpy().view(np.uint32))


def families(solver, grids, allowed=None):
    import torch
    sets, offsets = solver.unavoidable(grids, max_size=12, packed=True)
    n = grids.shape[0]
    s = torch.zeros((sets.shape[0], 4), dtype=torch.int32, device=solver.device)
    s[:, :3] = sets
    return s, offsets, solver._cell_masks(allowed, n, "allowed", (1 << 81) - 1), solver._cell_masks(None, n, "required", 0)


def to_host(fam):
    return (fam[0].cpu().numpy().view(np.uint32), fam[1].cpu().numpy(), fam[2].cpu().numpy().view(np.uint32),
            fam[3].cpu().numpy().view(np.uint32))


def say(*a):
    print(*a, flush=True)


def measure(launches, warmup, budget, save):
    import torch
    from sudoku_solver_distributed_amd import gen
    from sudoku_solver_distributed_amd.solver import get_solver
    solver = get_solver("cuda:0")
    dev = solver.device
    os.environ["OMP_NUM_THREADS"] = str(CPU_THREADS)
    tmp = tempfile.TemporaryDirectory()
    lib = host_build(tmp.name)
    res = {"launches": launches, "warmup": warmup, "budget_seconds": budget, "device": torch.cuda.get_device_name(dev),
           "timed": "sdk_hitting_sets_batch between device events", "node": "one start() or step() call of csrc/hit.h",
           "sets": "minimal unavoidable sets of at most 12 cells"}
    shapes = {}
    # ---- a
    grids = solver.random_grids(1 << 12, seed=1)
    fam = families(solver, grids)
    hfam = to_host(fam)
    ks = (12, 13)
    for k in ks:
        probe = Shape(solver, fam[0][:fam[1][8]], fam[1][:9], fam[2][:8], fam[3][:8], k, False)
        n = 1 << 12
        while n > 1 and probe.probe_seconds * n / 8 > budget:
            n >>= 1
        shapes[f"a_k{k}"] = (Shape(solver, fam[0][:fam[1][n]], fam[1][:n + 1], fam[2][:n], fam[3][:n], k, False), min(n, 16),
                             {"input": f"random_grids({n}, seed=1), A all cells, count only",
                              "probe_8_grids_seconds": probe.probe_seconds})
        say(f"a_k{k}: probe {probe.probe_seconds:.3f} s, {n} grids")
    save(res)
    # ---- b
    puzzles, full = gen.unique_batch(1 << 12, seed=5, return_solutions=True)
    clues = (puzzles != 0).sum(dim=1)
    kb = int(statistics.mode(clues.tolist()))
    idx = torch.nonzero(clues == kb)[:, 0]
    rng = np.random.default_rng(5)
    q = puzzles[idx].clone()
    noise = torch.from_numpy(rng.random((idx.shape[0], 81))).to(dev)
    noise[q != 0] = 2.0
    add = torch.argsort(noise, dim=1)[:, :5]
    q.scatter_(1, add, torch.gather(full[idx], 1, add))
    allowed = (q != 0).to(torch.uint8)
    famb = families(solver, full[idx], allowed)
    shapes["b_kernel"] = (Shape(solver, *famb, kb, True), min(int(idx.shape[0]), 256),
                          {"input": f"the {int(idx.shape[0])} puzzles of unique_batch(4096, seed=5) with {kb} clues, A = P plus 5 "
                                    f"digits, every row listed"})
    # ---- timed launches of a and b, alternating
    for _ in range(warmup):
        for s, _, _ in shapes.values():
            s.run()
    torch.cuda.synchronize()
    events = {k: [] for k in shapes}
    for _ in range(launches):
        for name, (s, _, _) in shapes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s.run()
            e1.record()
            events[name].append((e0, e1))
    torch.cuda.synchronize()
    def compare(name):
        s, sample, note = shapes[name]
        assert s.info.tolist() == [s.total, s.capacity] and bool((s.status == 1).all())
        arrays = s.host_arrays()
        mode = (1 if s.n <= 4096 else 0) | (0 if s.capacity else 2)
        host_run(lib, arrays, 0, min(CPU_THREADS, s.n), 0, 0, 2)  # the threads are started
        secs, hrows, hcount, hnodes = host_run(lib, arrays, 0, sample, s.k, s.capacity, mode)
        count = s.count.cpu().numpy()
        if not np.array_equal(hcount, count[:sample]):
            raise SystemExit(f"{name}: the GPU's counts differ from the host build's")
        if s.capacity:
            rows = s.rows.cpu().numpy().view(np.uint32)[:s.total]
            if not np.array_equal(sorted_rows(hrows), sorted_rows(rows[rows[:, 3] < sample])):
                raise SystemExit(f"{name}: the GPU's rows differ from the host build's")
        nodes, exact = int(hnodes.sum()), True
        if s.n > sample:
            if secs * (s.n - sample) / sample < 60:  # the rest of the families, for their nodes only (not timed)
                _, _, rcount, rnodes = host_run(lib, arrays, sample, s.n, s.k, 0, mode)
                if not np.array_equal(rcount, count[sample:]):
                    raise SystemExit(f"{name}: the GPU's counts differ from the host build's")
                nodes += int(rnodes.sum())
            else:
                nodes, exact = int(nodes * s.n / sample), False
        ms = [a.elapsed_time(z) for a, z in events[name]]
        per_s = lambda x: {"median": statistics.median(x / (t * 1e-3) for t in ms), "min": x / (max(ms) * 1e-3),
                           "max": x / (min(ms) * 1e-3)}
        res[name] = dict(note, families=s.n, k=s.k, rows=s.total, nodes=nodes, nodes_counted_on_every_family=exact,
                         ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), nodes_per_s=per_s(nodes),
                         rows_per_s=per_s(s.total),
                         cpu_host_build={"threads": CPU_THREADS, "families": sample, "nodes": int(hnodes.sum()),
                                         "seconds": secs, "nodes_per_s": int(hnodes.sum()) / secs, "answers_equal": True})
        res[name]["gpu_over_cpu_nodes"] = res[name]["nodes_per_s"]["median"] / res[name]["cpu_host_build"]["nodes_per_s"]
        save(res)

    for name in shapes:
        compare(name)
        say(name, res[name]["ms_median"], res[name]["gpu_over_cpu_nodes"])
    t0 = time.perf_counter()
    sub, off = solver.sub_puzzles(full[idx], kb, allowed=allowed)
    torch.cuda.synchronize()
    say("sub_puzzles done")
    res["b_sub_puzzles"] = {"grids": int(idx.shape[0]), "k": kb, "candidates": shapes["b_kernel"][0].total,
                            "proper_puzzles": int(sub.shape[0]), "seconds_host_clock": time.perf_counter() - t0}
    save(res)
    # ---- a small batch: one family of shape a alone
    one = Shape(solver, fam[0][:fam[1][1]], fam[1][:2], fam[2][:1], fam[3][:1], ks[1], False)
    ts = [one.probe_seconds]
    for _ in range(2):
        t0 = time.perf_counter()
        one.run()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    secs, _, hcount, hnodes = host_run(lib, hfam, 0, 1, ks[1], 0, 3)
    assert int(hcount[0]) == one.total
    say("small batch", ts, secs)
    res["small_batch_one_family"] = {"k": ks[1], "count": one.total, "nodes": int(hnodes[0]),
                                     "gpu_seconds_median_of_3_host_clock": statistics.median(ts), "host_one_thread_seconds": secs}
    save(res)
    # ---- c
    p = torch.from_numpy(np.array([[int(ch) for ch in gen.hard17_classes()[0]]], dtype=np.uint8)).to(dev)
    for d in (1, 2, 3):
        t0 = time.perf_counter()
        nb, _ = gen.neighbourhood(p, d)
        torch.cuda.synchronize()
        say("neighbourhood", d, nb.shape[0], time.perf_counter() - t0)
        res[f"c_neighbourhood_d{d}"] = {"puzzle": "hard17_classes()[0]", "families": [17, 136, 680][d - 1],
                                        "neighbours": int(nb.shape[0]), "seconds_host_clock": time.perf_counter() - t0}
        save(res)
    # ---- d
    _, grid = solver.count_solutions(p, limit=2, return_first=True)
    famd = families(solver, grid)
    t0 = time.perf_counter()
    k = int(host_tau(lib, to_host(famd), 0, 1, 8)[0])
    say("d: tau", k, time.perf_counter() - t0)
    res["d_rising_k"] = {"grid": "the solution of hard17_classes()[0]", "sets": int(famd[0].shape[0]), "tau": k,
                         "tau_host_one_thread_seconds": time.perf_counter() - t0, "steps": []}
    while k <= 32:
        s = Shape(solver, *famd, k, False)
        say("d", k, s.total, s.probe_seconds)
        res["d_rising_k"]["steps"].append({"k": k, "count": s.total, "seconds": s.probe_seconds})
        save(res)
        if s.probe_seconds * 8 > budget:  # (a k has cost up to eight times the one before)
            break
        k += 1
    t0 = time.perf_counter()
    got = int(gen.min_hitting_clues(grid, max_size=12)[0].item())
    assert got == res["d_rising_k"]["tau"]
    res["d_rising_k"]["min_hitting_clues_seconds_host_clock"] = time.perf_counter() - t0
    save(res)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--budget", type=float, default=2.0, help="seconds a launch may take (shapes a and d)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hit_rate.json"))
    a = ap.parse_args()
    if a.launches < 10:
        ap.error("at least 10 timed launches")

    def save(res):
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(measure(a.launches, a.warmup, a.budget, save)))


if __name__ == "__main__":
    main()
