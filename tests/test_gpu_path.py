"""GPU checks of the solving path (path_wave_kernel through BatchSolver.path
and the C ABI) against the fixture tests/golden/path_cases.json, which the
plain-Python definition of path_cases.py made, against the host build of
path.h, and against the rest of the library.  Every check is an equality."""
import numpy as np
import pytest
import torch

import logic_cases as G
import path_cases as P
from abi_arena import IN_FILL, OUT_FILL, Arena, _poisons

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)  # a single wave's claim, more boards than some grids hold, several claims a wave


@pytest.fixture(scope="module")
def fx():
    return P.load_fixture()


@pytest.fixture(scope="module")
def host():
    import test_path_host as H
    from native_build import host_lib
    lib = host_lib("path_host")
    return lambda boards, start, rules=P.ALL, max_rounds=0: H.run(lib, boards, start, rules, max_rounds)


def dev_inputs(solver, b, s):
    return (None if b is None else torch.from_numpy(np.array(b, dtype=np.uint8)).to(solver.device),
            None if s is None else torch.from_numpy(np.array(s, dtype=np.uint16).view(np.int16)).to(solver.device))


def gpu_path(solver, b, s, rules=P.ALL, max_rounds=0, **kw):
    db, ds = dev_inputs(solver, b, s)
    ev, off, status, marks, hist = solver.path(db, rules=rules, start=ds, max_rounds=max_rounds, return_marks=True,
                                               return_hist=True, **kw)
    assert ev.dtype == torch.int32 and off.dtype == torch.int64 and status.dtype == torch.int32 and marks.dtype == torch.int16
    ev = ev.cpu().numpy()
    rounds = np.array([ev[a:b_][ev[a:b_][:, 7] == 0][:, 0].max(initial=0) for a, b_ in zip(off.tolist()[:-1], off.tolist()[1:])],
                      dtype=np.int32)
    return {"events": ev, "offsets": off.cpu().numpy(), "status": status.cpu().numpy(), "rounds": rounds,
            "marks": marks.cpu().numpy().view(np.uint16), "hist": hist.cpu().numpy()}


def assert_run(names, got, want):
    for key in ("status", "rounds", "hist", "marks", "offsets", "events"):
        if not np.array_equal(got[key], want[key]):
            bad = [names[i] for i in range(len(names)) if key in ("offsets", "events") or not np.array_equal(got[key][i], want[key][i])]
            raise AssertionError((key, bad[:6]))


def names_of(fx, idx):
    return [fx["names"][i] for i in idx]


def mix(fx, n, seed=0):
    """Fixture indices of n states, one per status of the full path (dead,
    solved, stuck) in rotation."""
    rng = np.random.default_rng(seed)
    st = fx["runs"][0]["status"]
    by = [rng.permutation(np.nonzero(st == k)[0]) for k in (P.DEAD, P.SOLVED, P.STUCK)]
    return np.array([by[j % 3][(j // 3) % len(by[j % 3])] for j in range(n)])


def kernel_rounds(solver, b, s, rules=P.ALL, max_rounds=0):
    """d_rounds (and d_status, d_count) as the kernel writes them: a counting call of the C ABI."""
    db, ds = dev_inputs(solver, b, s)
    rc, out = raw_call(solver, db, ds, len(b if b is not None else s), rules, max_rounds, 0, None, hist=False, marks=False)
    assert rc == 0
    return out["rounds"].cpu().numpy(), out["status"].cpu().numpy(), out["count"].cpu().numpy()


def test_fixture(solver, fx):
    """Every run of the fixture: events, offsets, status, marks and hist, and
    the kernel's own rounds, status and count."""
    for run in fx["runs"]:
        b, s = P.inputs(fx, run["idx"])
        assert_run(names_of(fx, run["idx"]), gpu_path(solver, b, s, run["rules"], run["max_rounds"]), run)
        rounds, status, count = kernel_rounds(solver, b, s, run["rules"], run["max_rounds"])
        assert np.array_equal(rounds, run["rounds"]) and np.array_equal(status, run["status"])
        assert np.array_equal(count, np.diff(run["offsets"]))


@pytest.mark.parametrize("rules", [G.N, G.N | G.H | G.F2 | G.F3, G.NHL | G.S2 | G.S3, G.N | G.L | G.S2 | G.F4],
                         ids=lambda m: "0x%x" % m)
def test_other_masks_against_the_host_build(solver, fx, host, rules):
    idx = np.arange(len(fx["names"]))
    b, s = P.inputs(fx, idx)
    for max_rounds in (0, 4):
        want = host(b, s, rules, max_rounds)
        assert_run(fx["names"], gpu_path(solver, b, s, rules, max_rounds), want)
        rounds, status, count = kernel_rounds(solver, b, s, rules, max_rounds)
        assert np.array_equal(rounds, want["rounds"]) and np.array_equal(status, want["status"]) and np.array_equal(count, want["count"])


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(solver, fx, host, n):
    """One state per status in rotation; with max_rounds = 3 the LIMITED ones
    join them."""
    idx = mix(fx, n, seed=n)
    b, s = P.inputs(fx, idx)
    full = fx["runs"][0]
    got = gpu_path(solver, b, s)
    assert np.array_equal(got["status"], full["status"][idx]) and np.array_equal(got["marks"], full["marks"][idx])
    assert np.array_equal(got["hist"], full["hist"][idx])
    for k, i in enumerate(idx):
        assert np.array_equal(got["events"][got["offsets"][k]:got["offsets"][k + 1]],
                              full["events"][full["offsets"][i]:full["offsets"][i + 1]]), fx["names"][i]
    cut, want = gpu_path(solver, b, s, P.ALL, 3), host(b, s, P.ALL, 3)
    assert_run(names_of(fx, idx), cut, want)
    for mr, ref in ((0, full["rounds"][idx]), (3, want["rounds"])):
        rounds, status, count = kernel_rounds(solver, b, s, P.ALL, mr)
        assert np.array_equal(rounds, ref) and np.array_equal(status, (got if mr == 0 else cut)["status"])
    assert n < 63 or set(cut["status"].tolist()) == {P.DEAD, P.SOLVED, P.STUCK, P.LIMITED}


def test_max_waves_one_gives_the_same_sets(solver, fx):
    idx = mix(fx, 130, seed=5)
    b, s = P.inputs(fx, idx)
    a, c = gpu_path(solver, b, s), gpu_path(solver, b, s, max_waves=1)
    assert_run(names_of(fx, idx), c, a)
    d = gpu_path(solver, b, s, G.N | G.S4 | G.F4, 2, max_waves=3)
    assert_run(names_of(fx, idx), d, gpu_path(solver, b, s, G.N | G.S4 | G.F4, 2))


def raw_call(solver, db, ds, n, rules, max_rounds, capacity, rows, scratch=None, hist=True, marks=True, outs=None, max_waves=0):
    """sdk_path_batch itself; returns rc and the outputs."""
    L = solver.lib
    dev = solver.device
    new = (lambda nbytes, item, name: outs.carve(nbytes, itemsize=item, name=name)) if outs is not None else \
        (lambda nbytes, item, name: torch.full((nbytes // item,), 0x5A5A5A5A, dtype=torch.int32 if item == 4 else torch.int64,
                                               device=dev))
    count, rounds, status = new(4 * n, 4, "count"), new(4 * n, 4, "rounds"), new(4 * n, 4, "status")
    h = new(36 * n, 4, "hist") if hist else None
    if marks:
        m = outs.carve(162 * n, offset_mod4=2, name="marks") if outs is not None else torch.zeros(81 * n, dtype=torch.int16, device=dev)
    else:
        m = None
    info = new(16, 8, "info")
    need = int(L.sdk_path_scratch_bytes(n, max_waves))
    sc = scratch if scratch is not None else torch.empty(need, dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        rc = L.sdk_path_batch(ptr(db), ptr(ds), rules, max_rounds, n, ptr(rows), capacity, count.data_ptr(), rounds.data_ptr(),
                              status.data_ptr(), ptr(h), ptr(m), info.data_ptr(), sc.data_ptr(), need, max_waves,
                              int(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    return rc, {"count": count, "rounds": rounds, "status": status, "hist": h, "marks": m, "info": info}


def sorted_rows(rows):
    r = rows.cpu().numpy().view(np.uint32).reshape(-1, 4)
    return r[np.lexsort((r[:, 3], r[:, 2], r[:, 1], r[:, 0]))]


def test_capacity(solver, fx):
    """capacity == total lists every row; one less lists `capacity` rows, each
    a true event, and leaves the guard row behind them alone; 0 with a NULL
    list counts only."""
    idx = mix(fx, 65, seed=2)
    b, s = P.inputs(fx, idx)
    db, ds = dev_inputs(solver, b, s)
    n = len(idx)
    rc, out = raw_call(solver, db, ds, n, P.ALL, 0, 0, None)
    assert rc == 0
    total, listed = out["info"].tolist()
    full = fx["runs"][0]
    want_count = np.diff(full["offsets"])[idx]
    assert listed == 0 and total == int(want_count.sum()) and np.array_equal(out["count"].cpu().numpy(), want_count)
    assert np.array_equal(out["status"].cpu().numpy(), full["status"][idx]) and np.array_equal(out["rounds"].cpu().numpy(), full["rounds"][idx])
    rows = torch.full((total + 1, 4), -1515870811, dtype=torch.int32, device=solver.device)  # 0xA5A5A5A5
    rc, out = raw_call(solver, db, ds, n, P.ALL, 0, total, rows)
    assert rc == 0 and out["info"].tolist() == [total, total] and bool((rows[total] == -1515870811).all())
    every = sorted_rows(rows[:total])
    assert len(np.unique(every, axis=0)) == total
    import test_path_host as H
    ev, off = H.csr(*H.decode(every), n)
    for k, i in enumerate(idx):
        assert np.array_equal(ev[off[k]:off[k + 1]], full["events"][full["offsets"][i]:full["offsets"][i + 1]]), fx["names"][i]
    rows.fill_(-1515870811)
    rc, out = raw_call(solver, db, ds, n, P.ALL, 0, total - 1, rows)
    assert rc == 0 and out["info"].tolist() == [total, total - 1] and bool((rows[total - 1:] == -1515870811).all())
    some = sorted_rows(rows[:total - 1])
    have = {tuple(r) for r in every.tolist()}
    assert len(np.unique(some, axis=0)) == total - 1 and all(tuple(r) in have for r in some.tolist())
    assert np.array_equal(out["count"].cpu().numpy(), want_count)


def test_empty_boards_with_start_alone(solver, fx, host):
    """boards=None: pencil marks on empty boards; and the boards alone."""
    run = fx["runs"][0]
    sel = np.nonzero(~fx["has_board"])[0]
    got = gpu_path(solver, None, fx["start"][sel])
    assert_run(names_of(fx, sel), got, {k: (run[k][sel] if k not in ("events", "offsets") else got[k]) for k in
                                        ("status", "rounds", "hist", "marks", "offsets", "events")})
    assert_run(names_of(fx, sel), got, host(None, fx["start"][sel]))
    sel = np.nonzero(~fx["has_start"])[0]
    assert_run(names_of(fx, sel), gpu_path(solver, fx["boards"][sel], None), host(fx["boards"][sel], None))
    z = gpu_path(solver, np.zeros((3, 81), dtype=np.uint8), None)
    assert z["status"].tolist() == [P.STUCK] * 3 and len(z["events"]) == 0 and (z["marks"] == 0x1FF).all()
    e, off, st = solver.path(torch.zeros((0, 81), dtype=torch.uint8))
    assert e.shape == (0, 8) and off.tolist() == [0] and st.shape == (0,)
    with pytest.raises(ValueError):
        solver.path(None, start=None)
    for bad in (G.H, 0x201, 0):
        with pytest.raises(ValueError):
            solver.path(torch.zeros((1, 81), dtype=torch.uint8), rules=bad)


def test_given_capacity_that_overflows_raises(solver, fx):
    from sudoku_solver_distributed_amd.solver import SudokuHipError
    idx = mix(fx, 9, seed=1)
    db, ds = dev_inputs(solver, *P.inputs(fx, idx))
    total = int(np.diff(fx["runs"][0]["offsets"])[idx].sum())
    ev, off, st = solver.path(db, start=ds, capacity=total)
    assert ev.shape[0] == total
    with pytest.raises(SudokuHipError, match=f"capacity={total}"):
        solver.path(db, start=ds, capacity=total - 1)
    ev, off, st = solver.path(db, start=ds, capacity=0)
    assert ev.shape == (0, 8) and np.array_equal(st.cpu().numpy(), fx["runs"][0]["status"][idx])


def test_invalid_bytes_and_marks(solver, fx):
    idx = mix(fx, 18, seed=3)
    b, s = (a.copy() for a in P.inputs(fx, idx))
    b[1, 0], b[3, 80], s[5, 40], s[7, 17] = 10, 255, 0x200, 0x8001
    hit = [1, 3, 5, 7]
    got = gpu_path(solver, b, s)
    assert (got["status"][hit] == P.INVALID).all() and (np.diff(got["offsets"])[hit] == 0).all()
    assert (got["hist"][hit] == 0).all() and (got["marks"][hit] == 0).all()
    rounds, status, count = kernel_rounds(solver, b, s)
    assert (rounds[hit] == 0).all() and (status[hit] == P.INVALID).all() and (count[hit] == 0).all()
    rest = np.array([k for k in range(18) if k not in hit])
    full = fx["runs"][0]
    assert np.array_equal(rounds[rest], full["rounds"][idx[rest]])
    assert np.array_equal(got["status"][rest], full["status"][idx[rest]]) and np.array_equal(got["marks"][rest], full["marks"][idx[rest]])
    for k in rest:
        i = idx[k]
        assert np.array_equal(got["events"][got["offsets"][k]:got["offsets"][k + 1]],
                              full["events"][full["offsets"][i]:full["offsets"][i + 1]])


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_byte_offset_inputs_and_guard_bytes(solver, fx, offset):
    """d_boards at every address mod 4 inside an arena of bytes > 9, d_start
    and d_marks at 2 mod 4; the outputs, the list and the scratch inside
    arenas whose other bytes must not change; the inputs unchanged."""
    n = 67
    idx = mix(fx, n, seed=40 + offset)
    dev = solver.device
    inputs, outs, scratch = Arena(dev, IN_FILL, 1 << 16), Arena(dev, OUT_FILL, 1 << 20), Arena(dev, OUT_FILL, 1 << 12)
    b, s = P.inputs(fx, idx)
    d = inputs.boards(n, offset_mod4=offset, name="boards")
    d.copy_(torch.from_numpy(b))
    ds = inputs.carve(162 * n, offset_mod4=2, name="start")
    ds.copy_(torch.from_numpy(np.ascontiguousarray(s).view(np.uint8).reshape(-1)))
    assert d.data_ptr() % 4 == offset and ds.data_ptr() % 4 == 2
    full = fx["runs"][0]
    total = int(np.diff(full["offsets"])[idx].sum())
    rows = outs.carve(16 * total, name="rows", align=16)
    sc = scratch.carve(int(solver.lib.sdk_path_scratch_bytes(n, 0)), name="scratch", align=8)
    rc, out = raw_call(solver, d, ds, n, P.ALL, 0, total, rows, scratch=sc, outs=outs)
    assert rc == 0 and out["marks"].data_ptr() % 4 == 2 and out["info"].tolist() == [total, total]
    for a in (inputs, outs, scratch):
        a.assert_guards()
    assert np.array_equal(d.cpu().numpy(), b) and np.array_equal(ds.cpu().numpy().view(np.uint16).reshape(n, 81), s)
    assert np.array_equal(out["status"].cpu().numpy(), full["status"][idx])
    assert np.array_equal(out["marks"].cpu().numpy().view(np.uint16).reshape(n, 81), full["marks"][idx])
    assert np.array_equal(out["hist"].cpu().numpy().reshape(n, 9), full["hist"][idx])
    import test_path_host as H
    ev, off = H.csr(*H.decode(sorted_rows(rows.view(torch.int32))), n)
    for k, i in enumerate(idx):
        assert np.array_equal(ev[off[k]:off[k + 1]], full["events"][full["offsets"][i]:full["offsets"][i + 1]])
    # the optional outputs left out
    outs2 = Arena(dev, OUT_FILL, 1 << 14)
    rc, out = raw_call(solver, d, ds, n, P.ALL, 0, 0, None, scratch=sc, hist=False, marks=False, outs=outs2)
    assert rc == 0 and out["info"].tolist() == [total, 0]
    for a in (inputs, outs2, scratch):
        a.assert_guards()


def test_bad_arguments_launch_nothing(solver, fx):
    """Every refused call returns -2 and leaves the outputs and the scratch as
    they were."""
    n = 64
    dev = solver.device
    L = solver.lib
    outs = Arena(dev, OUT_FILL, 1 << 17)
    db, ds = dev_inputs(solver, *P.inputs(fx, np.arange(n)))
    c, r, st = (outs.carve(4 * n, itemsize=4, name=k) for k in ("count", "rounds", "status"))
    h = outs.carve(36 * n, itemsize=4, name="hist")
    m = outs.carve(162 * n, name="marks")
    rows = outs.carve(16 * 64, name="rows", align=16)
    info = outs.carve(16, itemsize=8, name="info")
    need = int(L.sdk_path_scratch_bytes(n, 0))
    sc = outs.carve(need, name="scratch", align=8)

    def call(**kw):
        a = {"b": db.data_ptr(), "s": ds.data_ptr(), "rules": P.ALL, "mr": 0, "n": n, "rows": rows.data_ptr(), "cap": 64,
             "c": c.data_ptr(), "r": r.data_ptr(), "st": st.data_ptr(), "h": h.data_ptr(), "m": m.data_ptr(),
             "info": info.data_ptr(), "sc": sc.data_ptr(), "bytes": need, "waves": 0}
        a.update(kw)
        return L.sdk_path_batch(a["b"], a["s"], a["rules"], a["mr"], a["n"], a["rows"], a["cap"], a["c"], a["r"], a["st"], a["h"],
                                a["m"], a["info"], a["sc"], a["bytes"], a["waves"], None)

    with torch.cuda.device(dev):
        for kw in ({"rules": G.H}, {"rules": 0x201}, {"mr": -1}, {"cap": -1}, {"cap": (2 ** 63 - 1) // 16 + 1}, {"waves": -1}, {"n": -1}, {"b": None, "s": None},
                   {"rows": None}, {"c": None}, {"r": None}, {"st": None}, {"info": None}, {"sc": None}, {"bytes": need - 1},
                   {"s": ds.data_ptr() + 1}, {"m": m.data_ptr() + 1}, {"rows": rows.data_ptr() + 8}, {"c": c.data_ptr() + 2},
                   {"r": r.data_ptr() + 2}, {"st": st.data_ptr() + 2}, {"h": h.data_ptr() + 2}, {"info": info.data_ptr() + 4},
                   {"sc": sc.data_ptr() + 4}):
            assert call(**kw) == -2, kw
    torch.cuda.synchronize(dev)
    assert bool((outs.buf == OUT_FILL).all())


def test_back_to_back_calls_share_one_scratch(solver, fx, host):
    """Calls on one stream with the one cached scratch, nothing between them,
    with different n, rules and max_rounds: every call's heads are re-armed in
    stream order."""
    idx = mix(fx, 131, seed=9)
    b, s = P.inputs(fx, idx)
    a = gpu_path(solver, b, s)
    c = gpu_path(solver, b[:65], s[:65], G.N | G.L, 0)
    d = gpu_path(solver, b[:7], s[:7], P.ALL, 1)
    e = gpu_path(solver, b, s)
    assert_run(names_of(fx, idx), e, a)
    assert_run(names_of(fx, idx[:65]), c, host(b[:65], s[:65], G.N | G.L, 0))
    assert_run(names_of(fx, idx[:7]), d, host(b[:7], s[:7], P.ALL, 1))


def test_poisoned_scratch(solver, fx):
    """The scratch's contents before the call are irrelevant."""
    idx = mix(fx, 33, seed=11)
    db, ds = dev_inputs(solver, *P.inputs(fx, idx))
    n = len(idx)
    full = fx["runs"][0]
    total = int(np.diff(full["offsets"])[idx].sum())
    sc = torch.zeros(int(solver.lib.sdk_path_scratch_bytes(n, 0)), dtype=torch.uint8, device=solver.device)
    want = None
    for name, poison in _poisons(sc):
        poison()
        rows = torch.zeros((total, 4), dtype=torch.int32, device=solver.device)
        rc, out = raw_call(solver, db, ds, n, P.ALL, 0, total, rows, scratch=sc)
        assert rc == 0 and out["info"].tolist() == [total, total], name
        assert np.array_equal(out["status"].cpu().numpy(), full["status"][idx]), name
        got = sorted_rows(rows)
        want = got if want is None else want
        assert np.array_equal(got, want), name


def test_replay_and_logic_agree(solver, fx):
    """gen.apply_events over the whole batch reproduces the end marks, and the
    end marks are BatchSolver.logic's with ladder=[rules]; the exact
    candidates of the boards survive in the end marks (the rules are sound)."""
    from sudoku_solver_distributed_amd import gen
    idx = np.arange(len(fx["names"]))
    b, s = P.inputs(fx, idx)
    db, ds = dev_inputs(solver, b, s)
    for rules in (P.ALL, G.N | G.S4 | G.F4):
        ev, off, status, marks = solver.path(db, rules=rules, start=ds, return_marks=True)
        step, lm = solver.logic(db, [rules], ds, return_marks=True)
        assert torch.equal(marks, lm)
        assert torch.equal(status == P.DEAD, step == 0) and torch.equal(status == P.SOLVED, step == 1)
        start = np.array([P.start_marks(b[k] if fx["has_board"][k] else None, s[k]) for k in idx], dtype=np.int16)
        end = gen.apply_events(torch.from_numpy(start).to(solver.device), ev, off)
        live = status != P.DEAD
        assert end.device == marks.device and torch.equal(end[live], marks[live])
    boards = np.nonzero(fx["has_board"] & ~fx["has_start"])[0]
    ev, off, status, marks = solver.path(db[boards], return_marks=True)
    exact = solver.candidates(db[boards])
    live = status != P.DEAD
    assert int(live.sum()) >= 30 and bool(((exact[live] & ~marks[live]) == 0).all())


def test_symmetry_images_keep_the_rounds(solver, fx):
    import symmetry_cases as S
    import test_path_host as H
    idx = mix(fx, 48, seed=77)
    rng = np.random.default_rng(5)
    b, s = P.inputs(fx, idx)
    syms = [S.random_symmetry(rng) for _ in idx]
    ib = np.stack([S.image_board(x, t) for x, t in zip(b, syms)])
    is_ = np.stack([S.image_marks(x, t) for x, t in zip(s, syms)])
    a, c = gpu_path(solver, b, s), gpu_path(solver, ib, is_)
    for key in ("status", "rounds", "hist", "offsets"):
        assert np.array_equal(a[key], c[key]), key
    for k in range(len(idx)):
        assert H.rounds_summary(a, k) == H.rounds_summary(c, k), fx["names"][idx[k]]
    assert np.array_equal(c["marks"], np.stack([S.image_marks(m, t) for m, t in zip(a["marks"], syms)]))


def test_hint_explain_and_technique_counts(solver, fx):
    from sudoku_solver_distributed_amd import gen, solver as sol
    assert sol.PATH_COLUMNS == P.COLUMNS and sol.PATH_CLASSES == P.CLASS_NAMES and len(gen.PATH_CLASS_NAMES) == 9
    idx = np.arange(len(fx["names"]))
    db, ds = dev_inputs(solver, *P.inputs(fx, idx))
    ev, off, status = gen.hint(db, ds)
    full = fx["runs"][0]
    e, off = ev.cpu().numpy(), off.tolist()
    for k in idx:
        w = full["events"][full["offsets"][k]:full["offsets"][k + 1]]
        mine = e[off[k]:off[k + 1]]
        assert np.array_equal(mine[mine[:, 7] == 0], w[(w[:, 0] == 1) & (w[:, 7] == 0)]), fx["names"][k]
        assert len(np.unique(mine[mine[:, 7] == 0][:, 1])) <= 1
    assert np.array_equal(gen.technique_counts(db, ds).cpu().numpy(), full["hist"])
    for run in fx["runs"]:
        lines = gen.explain(run["events"])
        assert len(lines) == len(run["events"]) and all(isinstance(x, str) and len(x) > 10 for x in lines)
        assert all(("contradiction" in x) == bool(c) for x, c in zip(lines, run["events"][:, 7]))
    pair = np.array([[3, 3, 45 + 3, 0b10010, 0b1000100, 3, 200, 0]], dtype=np.int32)
    assert gen.explain(pair) == ["naked pair {3,7} in row 4, columns 2 and 5: 3 candidates leave"]
    assert gen.path_class_names([0, 3, 6, 8]) == ["naked single", "pair", "X-wing", "jellyfish"]
