"""CPU checks of the hitting sets (csrc/hit.h, what the hit kernels run): the
fixture tests/golden/hit_cases.json itself -- brute force and the cell-by-cell
restatement, neither of which hit.h had a part in -- recomputed where that is
quick; the header compiled for the host (tests/native/hit_host.cpp) against
the fixture in rows, counts and statuses, with the packing prune and without
it, with the coarse and the fine task cut, with the families shuffled, listing
and counting; the limit; the stand-alone program under the sanitizers; and the
C ABI's argument checks through ctypes (no GPU).  Every check is an equality.
"""
import ctypes
import os
import subprocess
from math import comb

import numpy as np
import pytest

import hit_cases as H
import native_build
import ua_cases as U

_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
native_build.PROTOS.setdefault("hit_host", {
    # sets, offsets, allowed, required, n, k, limit, rows, capacity, count, status, info (2 x int64), nodes (NULL ok),
    # mode (bit 0: fine tasks, bit 1: count only) -> 0 / -2
    "hit_host_batch": ([_vp, _vp, _vp, _vp, _i64, _int, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _int], _int),
})
FILL32 = 0xA5A5A5A5


@pytest.fixture(scope="module", params=["prune", "noprune"])
def host(request):
    return native_build.host_lib("hit_host", defines=() if request.param == "prune" else ("SDK_HIT_PRUNE=0",), openmp=True)


@pytest.fixture(scope="module")
def cases():
    return H.load_fixture()


def run_host(lib, cases, k, mode=0, limit=0, capacity=1 << 17):
    """hit_host_batch on these cases as one batch: (masks per family, count,
    status, (total, listed), nodes)."""
    sets, offsets, A, R = H.batch_arrays(cases)
    n = len(cases)
    rows = np.full((max(capacity, 1), 4), FILL32, dtype=np.uint32)
    count = np.full(n, 12345, dtype=np.int64)
    status = np.full(n, 12345, dtype=np.int32)
    info = np.zeros(2, dtype=np.int64)
    nodes = np.zeros(n, dtype=np.uint64)
    before = [a.copy() for a in (sets, offsets, A, R)]
    rc = lib.hit_host_batch(sets.ctypes.data, offsets.ctypes.data, A.ctypes.data, R.ctypes.data, n, k, limit,
                            rows.ctypes.data, capacity, count.ctypes.data, status.ctypes.data, info.ctypes.data,
                            nodes.ctypes.data, mode)
    assert rc == 0
    assert all(np.array_equal(a, b) for a, b in zip(before, (sets, offsets, A, R)))
    assert (rows[info[1]:] == FILL32).all()
    got = [[] for _ in range(n)]
    for r, m in zip(rows[:info[1]], U.words_to_masks(rows[:info[1]])):
        got[int(r[3])].append(m)
    return got, count, status, (int(info[0]), int(info[1])), nodes


def by_k(cases):
    ks = sorted({k for c in cases for k in c.answers})
    return [(k, [c for c in cases if k in c.answers]) for k in ks]


def test_fixture_is_what_the_design_lists(cases):
    """The recorded answers themselves: the families the issue names, the two
    methods equal again on the small cases, the corner cases by the definition
    and tau against the greedy packing."""
    names = [c.name for c in cases]
    real = [f"hard17_{k}" for k in range(4)] + [f"random_{k}" for k in range(4)]
    assert names[:3] == ["cyclic", "cyclic_shuffled", "cyclic_repeats"]
    for g in real:
        assert {f"{g}_at6", f"{g}_at12", f"{g}_required", f"{g}_tau6"} <= set(names)
    by = {c.name: c for c in cases}
    assert len(by["cyclic"].sets) == 81 and all(H.popcount(m) == 6 for m in by["cyclic"].sets)
    assert sorted(by["cyclic_shuffled"].sets) == sorted(by["cyclic"].sets) != by["cyclic_shuffled"].sets
    for k in by["cyclic_shuffled"].answers:
        assert by["cyclic_shuffled"].answers[k] == by["cyclic"].answers[k] == by["cyclic_repeats"].answers[k]
        assert by["cyclic"].answers[k][0] > 0
    assert min(by["cyclic_wide"].answers.values())[0] == 0 < max(by["cyclic_wide"].answers.values())[0]
    for c in cases:
        assert c.status == H.status_of(c.A, c.R), c.name
        for k, (count, rows, dig) in c.answers.items():
            assert dig is not None or (rows is None and c.name.endswith("_tau6")), c.name
            if rows is not None:
                assert len(rows) == count and rows == sorted(set(rows), key=U.sort_key), c.name
                assert all(H.popcount(m) == k and not m & ~c.A and not c.R & ~m and all(m & u for u in c.sets) for m in rows)
            if len(c.sets) <= 30 and H.popcount(c.A) <= 62 and comb(H.popcount(c.A), k) <= 1 << 14:
                again = H.brute_rows(c.sets, c.A, c.R, k)
                assert again == H.restated_rows(c.sets, c.A, c.R, k) and len(again) == count, (c.name, k)
                assert again == rows, (c.name, k)
    e = by["empty_family"]
    assert [e.answers[k][0] for k in (0, 1, 2, 3, 5, 20, 21)] == [0, 0, 1, 18, comb(18, 3), 1, 0]
    assert by["empty_family_all_cells"].answers[2][0] == comb(81, 2) and by["empty_family_all_cells"].answers[0][0] == 1
    assert [by["one_cell"].answers[k][0] for k in (0, 1, 2)] == [0, 1, 19]
    assert [by["all_cells"].answers[k][0] for k in (0, 1, 6, 7)] == [0, 6, 1, 0]
    assert all(v[0] == 0 for name in ("outside_allowed", "zero_mask", "zero_mask_alone", "required_outside", "bit81_allowed",
                                      "bit81_required") for v in by[name].answers.values())
    assert [by[n].status for n in ("required_outside", "bit81_allowed", "bit81_required")] == [H.INVALID] * 3
    assert [by["k32"].answers[k][0] for k in (31, 32)] == [19, 15]
    for g in real:
        t = by[f"{g}_tau6"]
        used, packed = 0, 0
        for m in t.sets:
            if not m & used:
                used, packed = used | m, packed + 1
        assert t.answers[t.tau - 1][0] == 0 and t.answers[t.tau][0] == t.minimum > 0 and t.tau >= packed, g
        for size in (6, 12):
            c = by[f"{g}_at{size}"]
            assert 20 <= H.popcount(c.A) <= 24 and not c.puzzle & ~c.A and all(c.puzzle & u for u in c.sets), c.name
            rows = c.answers[H.popcount(c.puzzle)][1]
            assert rows is None or c.puzzle in rows, c.name


@pytest.mark.parametrize("mode", [0, 1])
def test_host_matches_fixture(host, cases, mode):
    """Every case at every k it records, as one batch a k: the coarse task
    cut (mode 0) and the fine one (mode 1), invalid and empty families among
    the others."""
    for k, group in by_k(cases):
        group = [c for c in group if c.answers[k][0] <= 1 << 16]
        got, count, status, (total, listed), _ = run_host(host, group, k, mode=mode, capacity=1 << 18)
        assert total == listed == sum(c.answers[k][0] for c in group)
        for i, c in enumerate(group):
            H.check_answer(c, k, got[i], int(count[i]), int(status[i]))


def test_count_mode_equals_list_mode(host, cases):
    """Count only (leaves add binomials): the fixture's counts, the large
    ones of the tau cases included; the nodes never above the listing walk's."""
    for k, group in by_k(cases):
        _, count, status, (total, listed), nodes = run_host(host, group, k, mode=2, capacity=0)
        assert listed == 0 and total == sum(c.answers[k][0] for c in group)
        assert count.tolist() == [c.answers[k][0] for c in group] and status.tolist() == [c.status for c in group]
        _, count1, _, _, nodes1 = run_host(host, group, k, mode=3, capacity=0)
        assert np.array_equal(count, count1)
    # the binomial where nothing is walked: the empty family on all cells, and where an int64 ends
    sets, off = np.zeros((0, 4), np.uint32), np.zeros(2, np.int64)
    A, R = H.masks_to_words([H.ALL81]), H.masks_to_words([0])
    for k in (0, 1, 2, 13, 16):
        count, status, info = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(2, np.int64)
        assert host.hit_host_batch(sets.ctypes.data, off.ctypes.data, A.ctypes.data, R.ctypes.data, 1, k, 0, None, 0,
                                   count.ctypes.data, status.ctypes.data, info.ctypes.data, None, 2) == 0
        assert count[0] == info[0] == comb(81, k), k


def test_shuffled_and_repeated_sets_change_nothing(host, cases):
    """Each real family at 12 cells in three seeded orders, one of them with
    sets repeated: the same rows."""
    rng = np.random.default_rng(7)
    picked = [c for c in cases if c.name.endswith("_at12") or c.name.endswith("_required")]
    for c in picked:
        k = max(c.answers, key=lambda kk: c.answers[kk][0])
        for trial in range(3):
            d = H.Case()
            d.__dict__.update(c.__dict__)
            d.sets = [c.sets[j] for j in rng.permutation(len(c.sets))]
            if trial == 2:
                d.sets += [d.sets[j] for j in rng.integers(0, len(d.sets), 9)]
            got, count, status, _, _ = run_host(host, [d], k, mode=trial & 1)
            H.check_answer(c, k, got[0], int(count[0]), int(status[0]))


def test_limit(host, cases):
    """limit = 1, 2 and count - 1: count == limit, status LIMITED, every row
    one of the full list; a limit at or above the count leaves DONE only
    above it."""
    picked = [c for c in cases if c.name in ("cyclic", "hard17_1_at12", "random_2_at6", "edge_cells", "empty_family")]
    assert len(picked) == 5
    for c in picked:
        k = max(c.answers, key=lambda kk: c.answers[kk][0] if c.answers[kk][1] is not None else -1)
        full, rows, _ = c.answers[k]
        assert full >= 4
        for mode in (0, 1):
            for limit in (1, 2, full - 1, full, full + 1):
                got, count, status, (total, listed), _ = run_host(host, [c], k, mode=mode, limit=limit)
                want = min(limit, full)
                assert count[0] == total == listed == want == len(got[0]), (c.name, limit)
                assert status[0] == (H.LIMITED if limit <= full else H.DONE), (c.name, limit)
                assert len(set(got[0])) == want and set(got[0]) <= set(rows), (c.name, limit)


def test_capacity_and_bad_arguments_of_the_host_model(host, cases):
    c = next(c for c in cases if c.name == "edge_cells")
    got, count, _, (total, _), _ = run_host(host, [c], 4)
    got2, count2, _, info2, _ = run_host(host, [c], 4, capacity=total - 1)
    assert info2 == (total, total - 1) and np.array_equal(count, count2) and set(got2[0]) <= set(got[0])
    _, count0, _, info0, _ = run_host(host, [c], 4, capacity=0)
    assert info0 == (total, 0) and np.array_equal(count, count0)
    z = np.zeros(8, dtype=np.int64)
    p = z.ctypes.data
    for kw in (dict(k=-1), dict(k=33), dict(limit=-1), dict(cap=-1), dict(n=-1), dict(mode=2, limit=1)):
        a = dict(n=1, k=3, limit=0, cap=0, mode=0)
        a.update(kw)
        assert host.hit_host_batch(p, p, p, p, a["n"], a["k"], a["limit"], None, a["cap"], p, p, p, None, a["mode"]) == -2, kw


def test_standalone_program_under_sanitizers(tmp_path, cases):
    """tests/native/hit_host.cpp as a program of its own (-DHIT_HOST_MAIN)
    built with -fsanitize=address,undefined: real, hand-made and invalid
    families at the edges of k, both task cuts, no report."""
    exe = str(tmp_path / "hit_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-DHIT_HOST_MAIN", "-o", exe,
                           os.path.join(native_build.NATIVE, "hit_host.cpp")])
    by = {c.name: c for c in cases}
    pick = [(by["cyclic"], None), (by["hard17_0_at12"], 17), (by["random_1_required"], None), (by["k32"], 32), (by["k32"], 31),
            (by["all_cells"], 6), (by["empty_family"], 0), (by["empty_family"], 21), (by["zero_mask"], 2),
            (by["bit81_required"], 3), (by["required_outside"], 2), (by["edge_cells_required"], 1)]
    richest = lambda c: max((kk for kk in c.answers if c.answers[kk][0] <= 4000), key=lambda kk: c.answers[kk][0])
    pick = [(c, k if k is not None else richest(c)) for c, k in pick]
    text = "".join("%d 0 %x %x%s\n" % (k, c.A, c.R, "".join(" %x" % m for m in c.sets)) for c, k in pick)
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(pick)
    for line, (c, k) in zip(lines, pick):
        n = c.answers[k][0]
        assert line == " ".join(["%d %d %d %d" % (c.status, n, n, n)] * 2), (c.name, k, line)


# ---- the C ABI's argument checks (no device call before them)

@pytest.fixture(scope="module")
def L():
    from sudoku_solver_distributed_amd import _lib, build
    build.build()
    return _lib.load()


def test_abi_argument_checks(L):
    from sudoku_solver_distributed_amd import _lib
    f, sb = L.sdk_hitting_sets_batch, L.sdk_hitting_sets_scratch_bytes
    assert _lib.SDK_HIT_MAX_CLUES == 32 and _lib.SDK_HIT_DONE == 1 and _lib.SDK_HIT_LIMITED == 2
    assert sb(100, 0) == 64 == sb(100, 7) == sb(0, 0) == sb(2 ** 31 - 1, 0)
    assert sb(-1, 0) == 0 and sb(1, -1) == 0 and sb(1 << 31, 0) == 0 and sb(2 ** 63 - 1, 0) == 0
    ok = dict(s=16, o=16, a=16, q=16, n=100, k=17, lim=0, r=16, cap=10, c=16, st=16, i=16, sc=16, nb=64, w=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["s"], a["o"], a["a"], a["q"], a["n"], a["k"], a["lim"], a["r"], a["cap"], a["c"], a["st"], a["i"], a["sc"],
                 a["nb"], a["w"], None)
    assert call(k=-1) == -2 and call(k=33) == -2                  # k out of range
    assert call(n=-1) == -2 and call(n=1 << 31) == -2             # n negative / above 2^31 - 1
    assert call(cap=-1) == -2 and call(w=-1) == -2 and call(lim=-1) == -2
    assert call(cap=2 ** 63 - 1) == -2                            # 16 * capacity past an int64
    assert call(nb=63) == -2                                      # scratch one byte short
    for name in ("o", "a", "q", "c", "st", "i", "sc", "r"):       # a required pointer is NULL
        assert call(**{name: None}) == -2, name
    assert call(r=24) == -2 and call(r=24, cap=0) == -2           # d_rows not 16-byte aligned
    assert call(s=24) == -2 and call(a=24) == -2 and call(q=24) == -2   # d_sets / d_allowed / d_required likewise
    assert call(o=20) == -2 and call(c=20) == -2 and call(i=20) == -2 and call(sc=20) == -2   # 8-byte alignment
    assert call(st=18) == -2                                      # d_status misaligned
    none = (None,) * 4
    assert f(*none, 0, 17, 0, None, 0, None, None, None, None, 0, 0, None) == 0     # n == 0
    assert f(*none, 0, 33, 0, None, 0, None, None, None, None, 0, 0, None) == -2    # ... still checks k
    assert f(*none, 0, 17, 0, None, -1, None, None, None, None, 0, 0, None) == -2
