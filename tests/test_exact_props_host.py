"""CPU side of the exact count's property tests (test_gpu_exact_props.py runs
the same inputs on the GPU): the ring arithmetic that ships (plane_exact.h's
exact_slot, exact_advance and exact_reserve, swept through
tests/native/exact_host.cpp's exact_ring_sweep); the conditions the GPU tests'
inputs are chosen for, from the fixture, the oracle and the host model alone,
each with its measured value; and the properties themselves -- PARTIAL as a
lower bound, the placement identities, place independence, the knobs' corners --
on the host model at one and two waves.  Every check is an equality or an
inequality of the contract.  The host model does not run H2.

The host runs are serial and cost seconds each, so they are computed once, side
by side on threads (the entry keeps no state and ctypes releases the GIL)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import exact_cases as E
import test_uniq_host as UH
from native_build import host_lib
from oracle import oracle as O

GRIDS = (1, 2)  # simulated waves


@pytest.fixture(scope="module")
def host():
    return host_lib("exact_host")


def _place_batches():
    h1 = E.load_fixture()["h1"][0]
    batch, src = E.placed(130, h1, (0, 63, 64, -1), E.light(126))
    return batch, src


@pytest.fixture(scope="module")
def runs(host):
    """name -> (count, status, stats) of every heavy host run of this file."""
    h1 = E.load_fixture()["h1"][0]
    mix = E.budget_mix()[0]
    batch, _ = _place_batches()
    light = E.pool()[0][E.light(128)]
    kids = E.placements()[1]
    jobs = {"h1": (h1[None], E.host_knobs(**E.H1_BUDGET))}
    for w in GRIDS:
        # 3(b) at the GPU test's knobs on two waves; one wave runs the same rounds (half the passes)
        jobs["mix", w] = (mix, E.host_knobs(**dict(E.MIX_BUDGET, max_waves=w)))
        jobs["place", w] = (batch, E.host_knobs(256, max_waves=w))
        jobs["reversed", w] = (batch[::-1], E.host_knobs(256, max_waves=w))
        jobs["two-lines", w] = (light, E.host_knobs(4, max_waves=w, max_tasks=1))
        jobs["one-round", w] = (light, E.host_knobs(2 ** 31 - 1, max_rounds=1, max_waves=w))
        jobs["kids", w] = (kids, E.host_knobs(**dict(E.TINY, max_waves=w)))
    names = list(jobs)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        res = list(ex.map(lambda k: E.host_exact(host, jobs[k][0], **jobs[k][1]), names))
    for k, r in zip(names, res):
        s = jobs[k][1]["slice"]
        assert r[2]["max_passes"] <= s + E.RUN_MAX, (k, r[2])
    return dict(zip(names, res))


# ---- the ring arithmetic that ships

def test_ring_arithmetic_sweep(host):
    """10 000 seeded rounds for every ring of 2..130 lines: see
    exact_ring_sweep for the five checks; 0 means none failed."""
    assert host.exact_ring_sweep(20271, 10000, 2, 130) == 0
    assert host.exact_ring_sweep(7, 2000, 2, 2) == 0  # max_tasks = 1 alone, another seed


# ---- the inputs' conditions

def test_symmetry_budgets_and_sizes():
    """From the fixture's and the oracle's counts alone.  Measured: the
    default-knob launch holds 806 boards (34 of set b) and 3 221 rows with
    11 737 108 completions; the tiny-knob launch 778 boards (6 of set b),
    3 109 rows, 1 073 724 completions."""
    _, count, status = E.pool()
    for budget, min_b, min_all in ((E.SYM_BUDGET, 24, 200), (E.SYM_TINY_BUDGET, 4, 200)):
        sel = E.symmetry_selection(budget)
        rows, source, syms = E.symmetry_rows(budget)
        is_b = E.pool_sets()[sel] == "b"
        total = int(count[source].sum())
        print(budget, len(sel), int(is_b.sum()), len(rows), total)
        assert total <= budget
        assert is_b.sum() >= min_b and len(sel) >= min_all
        assert len(set(sel.tolist())) == len(sel) and is_b[:is_b.sum()].all()  # pool order, set b first
        assert len(rows) == (E.SYM_IMAGES + 1) * len(sel) - E.SYM_IMAGES * int((status[sel] == E.INVALID).sum())
        # an image is a board with the same givens count, and the oracle counts the same on a few light ones
        for r in list(syms)[:24]:
            assert (rows[r] != 0).sum() == (E.pool()[0][source[r]] != 0).sum()
            if count[source[r]] <= 1022:
                assert O.count_solutions(rows[r], E.NO_LIMIT) == count[source[r]]
    assert E.SYM_BUDGET == 12_000_000 and E.SYM_TINY_BUDGET == 1_500_000


def test_h1_budget_leaves_a_positive_partial_count(runs):
    """3(a).  Measured on the host model: 2 726 completions after the 8
    rounds, 770 lines donated, 267 parks."""
    count, status, stats = runs["h1"]
    bound = E.pass_bound(**E.H1_BUDGET)
    assert E.H1_BUDGET == dict(slice=32, max_rounds=8, max_waves=1) and bound == 58368 < E.H1_COUNT
    print(int(count[0]), stats)
    assert status[0] == E.PARTIAL and stats["rounds"] == 8
    assert 0 < count[0] <= bound


@pytest.mark.parametrize("waves", GRIDS)
def test_mixed_budget_on_the_host_model(runs, waves):
    """3(b): slice 8192, 24 rounds.  DONE => exact, PARTIAL => a lower
    bound, nothing else -- and on two waves, the GPU test's grid, between 25
    and 75 % of set b PARTIAL.  Measured on two waves: 73 % of set b (186 of
    256) and 20 of the 64 light boards PARTIAL; on one wave 224 and 45 --
    boards queue behind the lanes' parked stacks, so the light ones are not
    the first to finish.  (Slice 4096 with 64 rounds leaves 178 and costs a
    third more passes; with 44 rounds it leaves 192, the 75 % itself.)"""
    assert E.MIX_BUDGET == dict(slice=8192, max_rounds=24, max_waves=2)
    boards, want, is_b = E.budget_mix()
    assert is_b.sum() == 256 and (~is_b).sum() == 64 and set(E.pool_sets()[E.light(64, "cd")]) == {"c", "d"}
    count, status, stats = runs["mix", waves]
    part = E.check_bounds(count, status, want)
    share = part[is_b].mean()
    print(waves, stats, "PARTIAL: set b", int(part[is_b].sum()), "others", int(part[~is_b].sum()))
    assert part[want > E.pass_bound(**dict(E.MIX_BUDGET, max_waves=waves))].all()
    assert part[is_b].any() and (~part[is_b]).any()
    if waves == E.MIX_BUDGET["max_waves"]:
        assert 0.25 <= share <= 0.75, share


def test_placement_inputs_and_identities(runs):
    """Item 6 against the oracle's counter: the host model's count of every
    child equals the oracle's (0 for a digit that clashes with a given), the
    identities with the host build of plane_uniq.h hold, and neither direction
    is vacuous.  Measured: 7 200 children, 203 with one completion, 928 with
    several."""
    sel, kids, parent, cell, digit = E.placements()
    boards, count, _ = E.pool()
    assert (E.pool_sets()[sel] == "d").all() and count[sel].min() >= 2 and count[sel].max() <= 64
    want = np.array([0 if E.clue_clashes(boards[sel[p]], c, d) else O.count_solutions(k, E.NO_LIMIT)
                     for k, p, c, d in zip(kids, parent, cell, digit)], dtype=np.int64)
    once, marks, _ = UH.uniq(host_lib("uniq_host"), boards[sel])
    ones, several = E.check_placements(want, once, marks, count[sel])
    print(len(kids), ones, several)
    assert ones >= 200 and several >= 200
    for w in GRIDS:
        child, status, stats = runs["kids", w]
        assert (status == E.DONE).all() and np.array_equal(child, want)
        assert E.check_placements(child, once, marks, count[sel]) == (ones, several)


# ---- the properties on the host model

@pytest.mark.parametrize("waves", GRIDS)
def test_h1_counts_the_same_wherever_it_stands(runs, waves):
    _, want, _ = E.pool()
    batch, src = _place_batches()
    assert (src < 0).sum() == 4 and src[0] == src[63] == src[64] == src[129] == -1
    expect = np.where(src < 0, E.H1_COUNT, want[np.maximum(src, 0)])
    for name, exp in (("place", expect), ("reversed", expect[::-1])):
        count, status, stats = runs[name, waves]
        assert (status == E.DONE).all() and np.array_equal(count, exp), name
        assert stats["donated"] > 0 and stats["rounds"] > 1


@pytest.mark.parametrize("waves", GRIDS)
def test_knob_corners(runs, waves):
    """A ring of two lines: deeper stacks can only park.  A slice above any
    pass count: one round, nothing donated, nothing parked."""
    _, want, _ = E.pool()
    idx = E.light(128)
    assert want[idx].max() <= 1022 and (want[idx] > 1).sum() >= 32 and len(set(E.pool_sets()[idx])) == 4
    count, status, stats = runs["two-lines", waves]
    print(stats)
    assert (status == E.DONE).all() and np.array_equal(count, want[idx])
    assert stats["parks"] > 0
    count, status, stats = runs["one-round", waves]
    assert (status == E.DONE).all() and np.array_equal(count, want[idx])
    assert (stats["rounds"], stats["donated"], stats["parks"]) == (1, 0, 0)
