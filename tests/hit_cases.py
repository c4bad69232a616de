"""What the hitting-set tests share (test_hit_host.py on the CPU,
test_gpu_hit.py on the GPU): the loader of tests/golden/hit_cases.json and
hit_cases.npz (the listed rows, as masks of 11 bytes)
(written by tests/golden/make_hit_cases.py, which csrc/hit.h has no part in),
the families it names rebuilt from tests/golden/ua_cases.npz, and the
definition of DESIGN.md §25 in plain Python twice over -- brute force over the
k-subsets of A that hold R, and a cell-by-cell restatement (cell c in or out,
in cell order) that lists or, with a memo, counts.  A cell set is a Python int
here, cell c its bit c; the C ABI's words are {m & M32, m >> 32 & M32, m >> 64,
ignored}.  Loaded once per process and shared, never modified.
"""
import functools
import hashlib
import itertools
import json
import os
from math import comb

import numpy as np

import ua_cases as U

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "hit_cases.json")
FIXTURE_ROWS = os.path.join(HERE, "golden", "hit_cases.npz")
DONE, LIMITED, INVALID = 1, 2, -1       # SDK_HIT_DONE, SDK_HIT_LIMITED, SDK_INVALID
MAX_CLUES = 32                          # SDK_HIT_MAX_CLUES
M32 = 0xFFFFFFFF
ALL81 = (1 << 81) - 1
BRUTE_CAP = 1 << 20                     # k-subsets a brute-forced case may have
LIST_CAP = 1500                         # rows a case lists in hit_cases.npz; beyond it their number and digest alone


def status_of(A, R):
    return INVALID if (A | R) >> 81 or R & ~A else DONE


def popcount(m):
    return bin(m).count("1")


def brute_rows(sets, A, R, k):
    """The rows by the definition: every k-subset of A that holds R, tested
    against every set (numpy over the subsets, the cells of A \\ R renumbered
    0..).  None when there are more than BRUTE_CAP subsets or more than 62
    such cells."""
    if status_of(A, R) != DONE:
        return []
    free = U.cells_of(A & ~R)
    r = k - popcount(R)
    if r < 0 or r > len(free):
        return []
    if comb(len(free), r) > BRUTE_CAP or len(free) > 62:
        return None
    need = {m & A for m in sets if not m & R}
    if 0 in need:
        return []
    pos = {c: j for j, c in enumerate(free)}
    local = sorted({sum(1 << pos[c] for c in U.cells_of(m)) for m in need})
    combos = np.fromiter((sum(1 << j for j in t) for t in itertools.combinations(range(len(free)), r)), dtype=np.int64,
                         count=comb(len(free), r))
    ok = np.ones(len(combos), dtype=bool)
    for m in local:
        ok &= (combos & m) != 0
    out = []
    for v in combos[ok].tolist():
        out.append(R | U.mask_of(free[j] for j in range(len(free)) if (v >> j) & 1))
    return sorted(out, key=U.sort_key)


def _prepared(sets, A, R):
    """The distinct sets R misses, each cut to A, by their last cell."""
    need = sorted({m & A for m in sets if not m & R})
    closing = [[] for _ in range(81)]
    for j, m in enumerate(need):
        if m:
            closing[m.bit_length() - 1].append(j)
    return need, closing


def _counter(sets, A, R):
    """rec(c, left, unhit): how many ways cells c.. complete a choice with
    `left` clues to place and the sets `unhit` (a bit a set) still to meet,
    with a memo; and the per-cell tables it uses."""
    need, closing = _prepared(sets, A, R)
    hits = [sum(1 << j for j in range(len(need)) if need[j] >> c & 1) for c in range(81)]
    close = [sum(1 << j for j in closing[c]) for c in range(81)]
    free = A & ~R

    @functools.lru_cache(maxsize=None)
    def rec(c, left, unhit):
        if c == 81:
            return int(left == 0)
        if not unhit:
            return comb(popcount(free >> c), left)
        total = 0
        if free >> c & 1 and left:
            total += rec(c + 1, left - 1, unhit & ~hits[c])
        if not unhit & close[c]:  # a set whose last allowed cell is c stays unhit: the branch ends
            total += rec(c + 1, left, unhit)
        return total

    return rec, need, hits, close, free


def restated_count(sets, A, R, k):
    """How many rows, by the restatement: cell 0, 1, ... each in or out; a
    set whose last allowed cell passes unhit ends the branch."""
    if status_of(A, R) != DONE or k < popcount(R) or k > popcount(A):
        return 0
    rec, need, _, _, _ = _counter(sets, A, R)
    return 0 if 0 in need else rec(0, k - popcount(R), (1 << len(need)) - 1)


def restated_rows(sets, A, R, k):
    """The rows by the restatement, the walk entering only the branches the
    count finds a row in."""
    if status_of(A, R) != DONE or k < popcount(R) or k > popcount(A):
        return []
    rec, need, hits, close, free = _counter(sets, A, R)
    if 0 in need:
        return []
    out = []

    def walk(c, S, left, unhit):
        if c == 81:
            out.append(S)
            return
        if free >> c & 1 and left and rec(c + 1, left - 1, unhit & ~hits[c]):
            walk(c + 1, S | 1 << c, left - 1, unhit & ~hits[c])
        if not unhit & close[c] and rec(c + 1, left, unhit):
            walk(c + 1, S, left, unhit)

    if rec(0, k - popcount(R), (1 << len(need)) - 1):
        walk(0, R, k - popcount(R), (1 << len(need)) - 1)
    return sorted(out, key=U.sort_key)


def digest(masks):
    """The sorted rows as one sha256 (cases beyond LIST_CAP rows)."""
    h = hashlib.sha256()
    for m in sorted(masks, key=U.sort_key):
        h.update(m.to_bytes(11, "little"))
    return h.hexdigest()


def family_of(spec):
    """The sets a case's "family" entry names, as a list of masks in order."""
    if "ua" in spec:
        case = {c.name: c for c in U.load_fixture()}[spec["ua"]]
        sets = case.minimal(spec["size"])
    else:
        sets = [int(s, 16) for s in spec["sets"]]
    if "shuffle" in spec:
        rng = np.random.default_rng(spec["shuffle"])
        sets = [sets[j] for j in rng.permutation(len(sets))]
    if "repeat" in spec:
        sets = sets + [sets[j] for j in spec["repeat"]]
    return sets


class Case:
    """name, sets (list of masks), A, R, status and answers: {k: (count,
    rows or None, digest or None)}; tau / minimum for the cases that record
    the least k with a row and the rows there; puzzle: the cells of the
    proper puzzle a real case's A was grown from."""

    def words(self):
        return U.rows_to_words(self.sets, owner=0xDEADBEEF)


def masks_to_words(masks):
    """(n, 4) uint32 with the fourth word a filler the ABI ignores."""
    return np.array([[m & M32, (m >> 32) & M32, (m >> 64) & M32, 0x5A5A5A5A] for m in masks], dtype=np.uint32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def load_fixture():
    with open(FIXTURE) as f:
        doc = json.load(f)["cases"]
    arrays = np.load(FIXTURE_ROWS)
    out = []
    for d in doc:
        c = Case()
        c.name, c.spec = d["name"], d["family"]
        c.sets = family_of(d["family"])
        c.A, c.R, c.status = int(d["A"], 16), int(d["R"], 16), int(d["status"])
        c.answers = {}
        for k, a in d["k"].items():
            key = "%s/%s" % (d["name"], k)
            rows = [int.from_bytes(bytes(r), "little") for r in arrays[key]] if key in arrays else None
            assert rows is None or (len(rows) == int(a["count"]) and digest(rows) == a["digest"]), key
            c.answers[int(k)] = (int(a["count"]), rows, a.get("digest"))
        c.tau, c.minimum = d.get("tau"), d.get("minimum")
        c.puzzle = int(d["puzzle"], 16) if "puzzle" in d else None
        out.append(c)
    return out


def batch_arrays(cases):
    """(sets (S, 4) uint32, offsets (n + 1,) int64, allowed (n, 4), required
    (n, 4)) of these cases as one call's arguments."""
    sets = np.concatenate([c.words() for c in cases] + [np.zeros((0, 4), np.uint32)])
    offsets = np.concatenate([[0], np.cumsum([len(c.sets) for c in cases])]).astype(np.int64)
    return (np.ascontiguousarray(sets), offsets, masks_to_words([c.A for c in cases]), masks_to_words([c.R for c in cases]))


def check_answer(case, k, got_masks, count, status):
    """A family's listed rows, count and status against the fixture."""
    want_count, rows, dig = case.answers[k]
    assert status == case.status, (case.name, k, status)
    assert count == want_count == len(got_masks), (case.name, k, count, want_count, len(got_masks))
    assert len(set(got_masks)) == len(got_masks), (case.name, k)
    if rows is not None:
        assert sorted(got_masks, key=U.sort_key) == rows, (case.name, k)
    elif dig is not None:
        assert digest(got_masks) == dig, (case.name, k)
    for m in got_masks[:50] if rows is not None or dig is not None else got_masks:  # (a tau case records the number alone)
        assert popcount(m) == k and not m & ~case.A and not case.R & ~m and all(m & u for u in case.sets), (case.name, k)
