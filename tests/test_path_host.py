"""CPU checks of the solving path (csrc/path.h, the schedule
path_wave_kernel's waves run): the header compiled for the host
(tests/native/path_host.cpp) against the fixture tests/golden/path_cases.json
and, live, against the plain-Python definition of path_cases.py; replay of the
events by gen.apply_events; agreement with the host build of logic.h; prefixes
under max_rounds; symmetry images; rule L against logic::pass_l; and the C
ABI's argument checks through ctypes (no GPU).  Every check is an equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import logic_cases as G
import native_build
import path_cases as P

_vp, _i64 = ctypes.c_void_p, ctypes.c_int64
# in (NULL ok), start (NULL ok), rules, max_rounds, n, rows (NULL ok iff capacity 0), capacity, count, rounds, status,
# hist (NULL ok), marks (NULL ok), info -> 0 / -2
native_build.PROTOS.setdefault("path_host", {
    "path_host_batch": ([_vp, _vp, ctypes.c_uint32, ctypes.c_int, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "path_host_rule_l": ([_vp, _vp, _i64, _vp, _vp], _i64)})
native_build.PROTOS.setdefault("logic_host", {"logic_host_batch": (
    [_vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int64], ctypes.c_int)})


@pytest.fixture(scope="module")
def host():
    return native_build.host_lib("path_host")


@pytest.fixture(scope="module")
def fx():
    return P.load_fixture()


def decode(rows):
    """Raw rows (k, 4) uint32 -> (owner (k,), events (k, 8) int64 in path_cases.COLUMNS)."""
    w = rows.astype(np.int64)
    w1, w2 = w[:, 1], w[:, 2]
    ev = np.stack([w1 & 0xFFFF, (w1 >> 16) & 15, w2 & 0xFF, (w2 >> 8) & 0x1FF, (w2 >> 17) & 0x7FFF, (w1 >> 24) & 0xFF, w[:, 3],
                   (w1 >> 20) & 1], axis=1)
    return w[:, 0], ev


def csr(owner, ev, n):
    """Events sorted by (owner, round, m, I, u) and their offsets."""
    order = np.lexsort((ev[:, 4], ev[:, 3], ev[:, 2], ev[:, 0], owner))
    return ev[order].astype(np.int32), np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))]).astype(np.int64)


def run(lib, boards, start, rules=P.ALL, max_rounds=0, hist=True, marks=True):
    """path_host_batch, a counting call and then the list at its exact size
    with a guard row behind it: dict of events, offsets, count, rounds,
    status, hist, marks (None for an output left out)."""
    b = None if boards is None else np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 81)
    s = None if start is None else np.ascontiguousarray(start, dtype=np.uint16).reshape(-1, 81)
    n = len(b) if b is not None else len(s)
    ptr = lambda a: None if a is None else a.ctypes.data
    out = {}
    for cap in (0, None):
        cap = int(out["info"][0]) if cap is None else cap
        rows = np.full((cap + 1, 4), 0xA5A5A5A5, dtype=np.uint32)
        c, r, st = (np.full(n, 12345, dtype=np.int32) for _ in range(3))
        h = np.full((n, 9), 12345, dtype=np.int32) if hist else None
        m = np.full((n, 81), 0xFFFF, dtype=np.uint16) if marks else None
        info = np.zeros(2, dtype=np.int64)
        assert lib.path_host_batch(ptr(b), ptr(s), rules, max_rounds, n, rows.ctypes.data if cap else None, cap, c.ctypes.data,
                                   r.ctypes.data, st.ctypes.data, ptr(h), ptr(m), info.ctypes.data) == 0
        assert info[1] == min(info[0], cap) and (rows[cap] == 0xA5A5A5A5).all()
        if out:
            assert info[0] == out["info"][0] and np.array_equal(c, out["count"]) and np.array_equal(st, out["status"])
        out = {"info": info, "count": c, "rounds": r, "status": st, "hist": h, "marks": m}
    owner, ev = decode(rows[:cap])
    out["events"], out["offsets"] = csr(owner, ev, n)
    assert np.array_equal(np.diff(out["offsets"]), c) and int(c.sum()) == cap
    return out


def assert_run(names, got, want):
    for key in ("status", "rounds", "hist", "marks", "offsets", "events"):
        if got[key] is None:
            continue
        if not np.array_equal(got[key], want[key]):
            bad = [i for i in range(len(names)) if key in ("offsets", "events") or not np.array_equal(got[key][i], want[key][i])]
            raise AssertionError((key, [names[i] for i in bad[:6]]))


def spread(fx, count=60):
    """About `count` states of the fixture over all kinds: every other one."""
    step = max(1, len(fx["names"]) // count)
    return np.arange(0, len(fx["names"]), step)


def test_fixture_is_what_the_design_lists(fx):
    """The recorded paths themselves: the coverage the generator asserts."""
    f = fx["facts"]
    assert f["states"] == len(fx["names"]) == 104 and all(v > 0 for v in f["events_by_class"]) and all(f["l_directions"])
    assert f["size1_contradictions"] and f["hall_contradictions"] and f["boards_with_parallel_events"] and f["boards_cut_mid_path"]
    assert set(f["status_tally"]) == {"0", "1", "2", "3"}
    assert [(r["rules"], r["max_rounds"]) for r in fx["runs"]] == [(P.ALL, 0), (7, 0), (G.N | G.S4 | G.F4, 0), (G.N | G.L, 0), (P.ALL, 2)]
    for run_ in fx["runs"]:
        ev = run_["events"]
        assert (ev[:, 1] <= 8).all() and ((ev[:, 5] > 0) | (ev[:, 7] == 1)).all()
        assert np.array_equal(run_["hist"].sum(1), np.diff(run_["offsets"]) - (run_["status"] == P.DEAD))
        assert (run_["marks"][run_["status"] == P.DEAD] == 0).all()
        # one class a round, one `left` a round, and every round removes something
        for k in range(len(run_["idx"])):
            e = ev[run_["offsets"][k]:run_["offsets"][k + 1]]
            e = e[e[:, 7] == 0]
            for r in np.unique(e[:, 0]):
                assert len(np.unique(e[e[:, 0] == r][:, [1, 6]], axis=0)) == 1


def test_host_matches_fixture(host, fx):
    """Every run of the fixture bit for bit as sorted event sets, with all
    outputs and with each optional output NULL."""
    for run_ in fx["runs"]:
        b, s = P.inputs(fx, run_["idx"])
        names = [fx["names"][i] for i in run_["idx"]]
        assert_run(names, run(host, b, s, run_["rules"], run_["max_rounds"]), run_)
    run_ = fx["runs"][1]
    b, s = P.inputs(fx, run_["idx"])
    for hist, marks in ((False, True), (True, False), (False, False)):
        got = run(host, b, s, run_["rules"], hist=hist, marks=marks)
        assert (got["hist"] is None) == (not hist) and (got["marks"] is None) == (not marks)
        assert_run([fx["names"][i] for i in run_["idx"]], got, run_)


def test_null_inputs(host, fx):
    """The boards alone and the pencil marks alone: the NULL inputs."""
    run_ = fx["runs"][0]
    for key, only in (("has_start", False), ("has_board", False)):
        sel = np.nonzero(fx[key] == only)[0]
        b, s = P.inputs(fx, sel)
        got = run(host, b if key == "has_start" else None, s if key == "has_board" else None)
        both = run(host, b, s)
        assert len(sel) >= 20
        for k in ("status", "rounds", "hist", "marks", "offsets", "events"):
            assert np.array_equal(got[k], both[k]), (key, k)
        assert np.array_equal(got["status"], run_["status"][sel])
    assert host.path_host_batch(None, None, P.ALL, 0, 1, None, 0, None, None, None, None, None, None) == -2


@pytest.mark.parametrize("rules", P.MASKS, ids=lambda m: "0x%x" % m)
def test_host_matches_the_python_definition_live(host, fx, rules):
    """About 60 states over all kinds against path_cases.path run now, with
    and without a round limit."""
    sel = spread(fx)
    assert len(sel) >= 50
    b, s = P.inputs(fx, sel)
    for max_rounds in (0, 3):
        got = run(host, b, s, rules, max_rounds)
        for k, i in enumerate(sel):
            ev, status, rounds, hist, marks = P.path(b[k] if fx["has_board"][i] else None, s[k] if fx["has_start"][i] else None,
                                                     rules, max_rounds)
            mine = got["events"][got["offsets"][k]:got["offsets"][k + 1]]
            assert [tuple(e) for e in mine.tolist()] == ev, (fx["names"][i], rules, max_rounds)
            assert (int(got["status"][k]), int(got["rounds"][k]), got["hist"][k].tolist(), got["marks"][k].tolist()) == \
                (status, rounds, hist, marks), (fx["names"][i], rules, max_rounds)


def test_replay_reproduces_every_round(fx):
    """gen.apply_events round by round from the start marks: every round's
    `left`, and the end marks, from the events alone; and the same from
    path_cases.replay."""
    from sudoku_solver_distributed_amd import gen
    for run_ in fx["runs"][:3]:
        for k, i in enumerate(run_["idx"]):
            ev = run_["events"][run_["offsets"][k]:run_["offsets"][k + 1]]
            marks = np.array(P.start_marks(fx["boards"][i] if fx["has_board"][i] else None, fx["start"][i]), dtype=np.uint16)
            for r in range(1, int(run_["rounds"][k]) + 1):
                mine = ev[(ev[:, 0] == r) & (ev[:, 7] == 0)]
                assert len(mine)
                before = marks
                marks = gen.apply_events(marks, mine)
                assert int(np.unpackbits(marks.view(np.uint8)).sum()) == int(mine[0, 6]), (fx["names"][i], r)
                removed = [int(np.unpackbits(before.view(np.uint8)).sum() - np.unpackbits(gen.apply_events(before, e[None]).view(np.uint8)).sum())
                           for e in mine[:3]]
                assert removed == mine[:3, 5].tolist()
            if run_["status"][k] != P.DEAD:
                assert np.array_equal(marks, run_["marks"][k]), fx["names"][i]
                assert P.replay(P.start_marks(fx["boards"][i] if fx["has_board"][i] else None, fx["start"][i]), ev) == marks.tolist()
    # the batch form: all states at once through the offsets
    run_ = fx["runs"][0]
    b, s = P.inputs(fx, run_["idx"])
    start = np.array([P.start_marks(b[k] if fx["has_board"][i] else None, s[k]) for k, i in enumerate(run_["idx"])], dtype=np.uint16)
    end = gen.apply_events(start, run_["events"], run_["offsets"])
    live = run_["status"] != P.DEAD
    assert np.array_equal(end[live], run_["marks"][live])


def logic_host(boards, start, ladder):
    lib = native_build.host_lib("logic_host")
    n = len(boards)
    lad = np.array(ladder, dtype=np.uint32)
    st = np.zeros(n, dtype=np.int32)
    m = np.zeros((n, 81), dtype=np.uint16)
    assert lib.logic_host_batch(np.ascontiguousarray(boards).ctypes.data, np.ascontiguousarray(start).ctypes.data, lad.ctypes.data,
                                len(lad), st.ctypes.data, None, None, m.ctypes.data, n) == 0
    return st, m


@pytest.mark.parametrize("rules", P.MASKS, ids=lambda m: "0x%x" % m)
def test_end_state_is_logics_fixpoint(host, fx, rules):
    """The end marks equal logic_host's under ladder=[rules] for STUCK and
    SOLVED, and DEAD holds exactly when that ladder's step is 0."""
    b, s = P.inputs(fx, np.arange(len(fx["names"])))
    got = run(host, b, s, rules)
    step, marks = logic_host(b, s, [rules])
    assert np.array_equal(got["status"] == P.DEAD, step == 0)
    assert np.array_equal(got["status"] == P.SOLVED, step == 1)
    assert np.array_equal(got["marks"], marks)
    assert set(got["status"].tolist()) <= {P.DEAD, P.SOLVED, P.STUCK}


def test_highest_class_is_logics_grade(host, fx):
    """For the boards ALL solves, the default ladder's step that holds the
    path's highest class is logic's default grade."""
    b, s = P.inputs(fx, np.arange(len(fx["names"])))
    got = run(host, b, s)
    step, _ = logic_host(b, s, G.DEFAULT_LADDER)
    solved = np.nonzero(got["status"] == P.SOLVED)[0]
    assert len(solved) >= 20
    for k in solved:
        top = max(c for c in range(9) if got["hist"][k][c]) if got["hist"][k].any() else 0
        grade = next(j + 1 for j, m in enumerate(G.DEFAULT_LADDER) if m >> top & 1)
        assert grade == step[k], fx["names"][k]
    assert len({int(step[k]) for k in solved}) >= 5


def test_counts(host, fx):
    """hist sums to count minus the contradiction events; rounds is the last
    event's round."""
    b, s = P.inputs(fx, np.arange(len(fx["names"])))
    for rules in P.MASKS:
        got = run(host, b, s, rules)
        contra = np.array([int(got["events"][got["offsets"][k]:got["offsets"][k + 1]][:, 7].sum()) for k in range(len(b))])
        assert np.array_equal(got["hist"].sum(1), got["count"] - contra)
        assert np.array_equal(contra, (got["status"] == P.DEAD).astype(int))
        for k in range(len(b)):
            e = got["events"][got["offsets"][k]:got["offsets"][k + 1]]
            e = e[e[:, 7] == 0]
            assert int(got["rounds"][k]) == (int(e[:, 0].max()) if len(e) else 0)
            assert np.array_equal(np.bincount(e[:, 1], minlength=9), got["hist"][k])


def test_max_rounds_gives_a_prefix(host, fx):
    """The non-contradiction events of max_rounds = r are exactly the rounds
    <= r of the full path, for r = 1, 2 and a middle round."""
    b, s = P.inputs(fx, np.arange(len(fx["names"])))
    full = run(host, b, s)
    middle = max(3, int(np.median(full["rounds"])) // 2)
    for r in (1, 2, middle):
        got = run(host, b, s, P.ALL, r)
        for k in range(len(b)):
            e = got["events"][got["offsets"][k]:got["offsets"][k + 1]]
            w = full["events"][full["offsets"][k]:full["offsets"][k + 1]]
            assert np.array_equal(e[e[:, 7] == 0], w[(w[:, 7] == 0) & (w[:, 0] <= r)]), (fx["names"][k], r)
            if full["rounds"][k] > r:
                assert got["status"][k] == P.LIMITED and got["rounds"][k] == r
            elif full["rounds"][k] == r and (full["status"][k] == P.STUCK or (w[:, 7] & (w[:, 1] >= 3)).any()):
                # the limit (step 3) comes before the classes (step 4): no STUCK and no Hall contradiction at round r
                assert got["status"][k] == P.LIMITED and got["rounds"][k] == r
            else:
                assert got["status"][k] == full["status"][k] and np.array_equal(e, w)
        assert (got["status"] == P.LIMITED).any()


def rounds_summary(out, k):
    e = out["events"][out["offsets"][k]:out["offsets"][k + 1]]
    e = e[e[:, 7] == 0]
    return [(int(r), int(e[e[:, 0] == r][0, 1]), int((e[:, 0] == r).sum()), int(e[e[:, 0] == r][0, 6])) for r in np.unique(e[:, 0])]


def test_symmetry_images_keep_the_rounds(host, fx):
    """Relabelled, permuted and transposed images (the pencil marks carried
    by image_marks): the same status, rounds and hist, and per round the same
    (class, event count, left)."""
    import symmetry_cases as S
    sel = spread(fx, 40)
    rng = np.random.default_rng(27)
    b, s = P.inputs(fx, sel)
    syms = [S.random_symmetry(rng) for _ in sel]
    ib = np.stack([S.image_board(x, t) for x, t in zip(b, syms)])
    is_ = np.stack([S.image_marks(x, t) for x, t in zip(s, syms)])
    for rules in (P.ALL, G.N | G.S4 | G.F4):
        a, c = run(host, b, s, rules), run(host, ib, is_, rules)
        for key in ("status", "rounds", "hist", "count"):
            assert np.array_equal(a[key], c[key]), key
        for k in range(len(sel)):
            assert rounds_summary(a, k) == rounds_summary(c, k), fx["names"][sel[k]]
        assert np.array_equal(c["marks"], np.stack([S.image_marks(m, t) for m, t in zip(a["marks"], syms)]))


def test_rule_l_firings_are_pass_l(host, fx):
    """The union of the L firings' removals on a state is what logic::pass_l
    removes from it: on the start states and on the N|H fixpoints."""
    b, s = P.inputs(fx, np.arange(len(fx["names"])))
    _, closed = logic_host(b, s, [G.N | G.H])
    fired = 0
    for boards, start in ((b, s), (None, closed[(closed != 0).all(1)])):
        n = len(start)
        ml, mp = np.zeros((n, 81), dtype=np.uint16), np.zeros((n, 81), dtype=np.uint16)
        fired += host.path_host_rule_l(None if boards is None else np.ascontiguousarray(boards).ctypes.data,
                                       np.ascontiguousarray(start).ctypes.data, n, ml.ctypes.data, mp.ctypes.data)
        assert np.array_equal(ml, mp)
        assert (ml != start).any()
    assert fired > 100


def test_bytes_above_9_and_marks_above_0x1ff_are_invalid(host, fx):
    b, s = P.inputs(fx, np.arange(12))
    b, s = b.copy(), s.copy()
    b[1, 0], b[3, 80], s[5, 40], s[7, 17] = 10, 255, 0x200, 0x8001
    hit = [1, 3, 5, 7]
    rest = [k for k in range(12) if k not in hit]
    for rules in (P.ALL, G.N):
        got = run(host, b, s, rules)
        assert (got["status"][hit] == P.INVALID).all() and (got["count"][hit] == 0).all() and (got["rounds"][hit] == 0).all()
        assert (got["hist"][hit] == 0).all() and (got["marks"][hit] == 0).all()
    got = run(host, b, s)
    want = fx["runs"][0]
    assert np.array_equal(got["status"][rest], want["status"][rest]) and np.array_equal(got["marks"][rest], want["marks"][rest])
    for k in rest:
        assert np.array_equal(got["events"][got["offsets"][k]:got["offsets"][k + 1]],
                              want["events"][want["offsets"][k]:want["offsets"][k + 1]])
    assert (run(host, None, s)["status"][[5, 7]] == P.INVALID).all()


def test_host_refuses_bad_arguments(host):
    z = np.zeros(81, dtype=np.uint8)
    out = np.zeros(16, dtype=np.int64)

    def call(rules=P.ALL, max_rounds=0, b=z, cap=0, rows=None):
        return host.path_host_batch(None if b is None else b.ctypes.data, None, rules, max_rounds, 1, rows, cap, out.ctypes.data,
                                    out.ctypes.data, out.ctypes.data, None, None, out.ctypes.data)

    assert call() == 0 and call(G.N) == 0 and call(G.N | G.F4, 5) == 0
    assert call(G.H) == -2 and call(0x201) == -2 and call(0) == -2       # a mask without N or outside 0x1FF
    assert call(max_rounds=-1) == -2 and call(cap=-1) == -2 and call(cap=4) == -2 and call(b=None) == -2


def test_standalone_program_under_sanitizers(tmp_path, fx):
    """tests/native/path_host.cpp as a program of its own (-DPATH_HOST_MAIN)
    built with -fsanitize=address,undefined: a state of every status and
    kind under two masks and a round limit, no report, the fixture's
    events."""
    exe = str(tmp_path / "path_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DPATH_HOST_MAIN", "-o", exe,
                           os.path.join(native_build.NATIVE, "path_host.cpp")])
    for run_ in (fx["runs"][0], fx["runs"][2], fx["runs"][4]):
        pick = np.arange(0, len(run_["idx"]), 3 if run_ is fx["runs"][0] else 1)[:30]
        assert set(run_["status"][pick].tolist()) >= ({P.DEAD, P.SOLVED, P.STUCK} if not run_["max_rounds"] else {P.LIMITED})
        text = ""
        for k in pick:
            i = run_["idx"][k]
            text += ("s" + G.marks_text(fx["start"][i]) if fx["has_start"][i] else "".join(str(int(v)) for v in fx["boards"][i])) + "\n"
        out = subprocess.run([exe, str(run_["rules"]), str(run_["max_rounds"])], input=text, capture_output=True, text=True)
        assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
        lines = out.stdout.strip().split("\n")
        assert len(lines) == len(pick)
        for line, k in zip(lines, pick):
            head, rows = line.split()[:3], line.split()[3:]
            assert [int(v) for v in head] == [run_["status"][k], run_["rounds"][k], run_["offsets"][k + 1] - run_["offsets"][k]]
            raw = np.array([[0] + [int(v, 16) for v in r.split(":")] for r in rows], dtype=np.uint32).reshape(-1, 4)
            ev, _ = csr(*decode(raw), 1)
            assert np.array_equal(ev, run_["events"][run_["offsets"][k]:run_["offsets"][k + 1]]), fx["names"][run_["idx"][k]]


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    from sudoku_solver_distributed_amd import _lib
    f = L.sdk_path_batch
    assert (_lib.SDK_PATH_DEAD, _lib.SDK_PATH_SOLVED, _lib.SDK_PATH_STUCK, _lib.SDK_PATH_LIMITED) == (P.DEAD, P.SOLVED, P.STUCK,
                                                                                                    P.LIMITED)
    need = int(L.sdk_path_scratch_bytes(100, 0))

    def call(b=16, s=16, rules=P.ALL, mr=0, n=100, rows=16, cap=10, c=16, r=16, st=16, h=None, m=None, info=16, sc=16, size=need,
             waves=0):
        return f(b, s, rules, mr, n, rows, cap, c, r, st, h, m, info, sc, size, waves, None)

    assert call(rules=G.H) == -2 and call(rules=0x201) == -2 and call(rules=0x400 | G.N) == -2 and call(rules=0) == -2
    assert call(mr=-1) == -2 and call(cap=-1) == -2 and call(waves=-1) == -2
    assert call(cap=(2 ** 63 - 1) // 16 + 1) == -2                        # a list whose bytes do not fit an int64
    assert call(n=-1) == -2 and call(n=1 << 31) == -2                     # n negative, above 2^31 - 1
    assert call(b=None, s=None) == -2                                     # both inputs NULL
    assert call(rows=None) == -2                                          # a capacity without a list
    assert call(c=None) == -2 and call(r=None) == -2 and call(st=None) == -2 and call(info=None) == -2 and call(sc=None) == -2
    assert call(size=need - 1) == -2                                      # scratch one byte short
    assert call(s=17) == -2 and call(m=17) == -2                          # d_start / d_marks at an odd address
    assert call(rows=24) == -2 and call(c=18) == -2 and call(r=18) == -2 and call(st=18) == -2 and call(h=18) == -2
    assert call(info=20) == -2 and call(sc=20) == -2
    assert call(b=None, s=None, rows=None, cap=0, c=None, r=None, st=None, info=None, n=0, sc=None, size=0) == 0   # n == 0
    assert call(n=0, rules=G.H) == -2 and call(n=0, mr=-1) == -2 and call(n=0, cap=-1) == -2   # ... still checks the scalars


def test_scratch_bytes(L):
    sb = L.sdk_path_scratch_bytes
    assert sb(100, 0) == sb(1, 7) == sb(2 ** 31 - 1, 0) == sb(0, 0) == 64
    assert sb(-1, 0) == 0 and sb(1, -1) == 0 and sb(1 << 31, 0) == 0
