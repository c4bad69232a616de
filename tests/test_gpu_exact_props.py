"""GPU checks of the exact completion count's contract that its fixture cannot
show (exact_kernel through BatchSolver.count_exact and the C ABI): the buffer
contract, a scratch reused after a PARTIAL call, PARTIAL as a lower bound,
additivity over a cell's digits on H2, invariance under Sudoku's symmetries,
agreement with count_solutions, candidates and unique_candidates, independence
of a board's place and batch, the knobs' corners and two callers at once.
Every expected value is the fixture's, the oracle's or an identity between
calls; every check is an equality or an inequality of the contract.  The inputs
are exact_cases.py's, and test_exact_props_host.py asserts on the CPU what they
are chosen for."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import exact_cases as E
import symmetry_cases as S
from abi_arena import IN_FILL, OUT_FILL, Arena

pytestmark = pytest.mark.gpu

EMPTY_MORE = np.iinfo(np.int64).max  # the empty board's count is above any lower bound a call can report


def _run(solver, boards, **kw):
    count, status, stats = solver.count_exact(torch.from_numpy(np.array(boards, dtype=np.uint8)), return_status=True,
                                              return_stats=True, **kw)
    if "slice" in kw:
        assert stats["max_passes"] <= kw["slice"] + E.RUN_MAX, stats
    return count.cpu().numpy(), status.cpu().numpy(), stats


def _need(solver, n, max_waves, max_tasks):
    return int(solver.lib.sdk_count_exact_scratch_bytes(n, max_waves, max_tasks))


def _raw(solver, d_boards, d_count, d_status, scratch, size, slice, max_rounds, max_tasks, max_waves, stream=None,
         stats=None):
    """sdk_count_exact_batch as a C caller reaches it: (return code, stats
    dict).  stats: a pointer to four int64 on the host, or None for an array
    of its own."""
    n = d_boards.shape[0]
    own = (ctypes.c_int64 * 4)()
    with torch.cuda.device(solver.device):
        st = int((stream or torch.cuda.current_stream(solver.device)).cuda_stream)
        rc = solver.lib.sdk_count_exact_batch(d_boards.data_ptr(), d_count.data_ptr(), d_status.data_ptr(), n, slice,
                                              max_rounds, max_tasks, scratch.data_ptr(), size, max_waves, st,
                                              stats if stats is not None else own)
    got = dict(zip(("rounds", "donated", "parks", "max_passes"), (int(v) for v in own)))
    if stats is None:
        assert got["max_passes"] <= slice + E.RUN_MAX, got
    return rc, got


def _outputs(solver, n):
    return (torch.full((n,), -12345, dtype=torch.int64, device=solver.device),
            torch.full((n,), 12345, dtype=torch.int32, device=solver.device))


def _same(count, status, idx):
    _, want, want_status = E.pool()
    count, status = np.asarray(count), np.asarray(status)
    bad = np.nonzero((count != want[idx]) | (status != want_status[idx]))[0]
    assert len(bad) == 0, [(int(i), int(idx[i]), int(count[i]), int(want[idx[i]]), int(status[i])) for i in bad[:10]]


# ---- 1. the buffer contract

@pytest.mark.parametrize("offset", (0, 1, 2, 3))
def test_buffer_contract(solver, offset):
    """d_boards at every address mod 4 among bytes > 9 (exact_load_words
    reads the aligned dwords that hold a board: the 1..3 neighbouring bytes
    must never reach an answer); d_count, d_status and a scratch of exactly
    the stated size among 0xA5 bytes, none of which may change; 68 boards, so
    that the last open-task counter ends at the guard; the tiny knobs, so that
    the ring, the park words and the counters are all written.

    The scratch arrives dirty (0xA5: every park word would read as a parked
    stack of 0xA5A5A5A5 levels).  What a round reads before it writes, as
    exact_init_kernel and exact_kernel stand: d_count, d_status and the
    open-task counters of all n boards, the park words of all 64 * waves
    lanes and the 32 words of the head block -- exact_init_kernel arms every
    one of them, in stream order before the first round; the ring only in
    [head0, limit), which is empty in the first round and afterwards holds
    lines that an earlier round of the same call wrote (exact_reserve keeps
    appends out of it); a lane's stack lines only at levels it pushed before
    (a taken task line is pushed as level 0, a parked stack was pushed in the
    round before, the park word arming says there is none at the start).  No
    gap: the init kernel is as it was."""
    _, want, want_status = E.pool()
    boards, idx = E.mixed(68)
    n, dev = len(boards), solver.device
    knobs = dict(E.TINY)
    need = _need(solver, n, knobs["max_waves"], knobs["max_tasks"])
    assert need == 256 + 2 * (64 * 81 * 128 + 64 * 8) + 2 * 64 * 128 + 4 * n and (4 * n) % 16 == 0
    inputs, outs, scratch = Arena(dev, IN_FILL, 1 << 14), Arena(dev, OUT_FILL, 1 << 12), Arena(dev, OUT_FILL, 1 << 21)
    d = inputs.boards(n, offset, name="boards")
    d.copy_(torch.from_numpy(boards))
    before = inputs.buf.clone()
    count = outs.carve(8 * n, itemsize=8, name="count")
    status = outs.carve(4 * n, itemsize=4, name="status")
    sc = scratch.carve(need, name="scratch", align=16)
    assert d.data_ptr() % 4 == offset and sc.data_ptr() % 16 == 0
    host = np.full(12, -7, dtype=np.int64)
    rc, _ = _raw(solver, d, count, status, sc, need, stats=host[4:].ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                 **knobs)
    torch.cuda.synchronize(dev)
    assert rc == 0
    _same(count.cpu().numpy(), status.cpu().numpy(), idx)
    rounds, donated, parks, most = (int(v) for v in host[4:8])
    print(offset, rounds, donated, parks, most)
    assert parks > 0 and donated > 0 and rounds > 1 and 0 < most <= knobs["slice"] + E.RUN_MAX
    assert (host[:4] == -7).all() and (host[8:] == -7).all()
    for a in (inputs, outs, scratch):
        a.assert_guards()
    assert torch.equal(inputs.buf, before)


# ---- 2. one scratch, reused after a PARTIAL call

def test_scratch_reused_after_a_partial_call(solver):
    """Call A leaves stacks parked and lines queued (the empty board and H1
    after four rounds); call B, same layout, and call C, another layout in
    the same bytes, each arm what they read: every answer exact."""
    boards, want, _ = E.pool()
    h1 = E.load_fixture()["h1"][0]
    light = E.light(40)
    sizes = [_need(solver, 68, 2, 64), _need(solver, 32, 2, 64), _need(solver, 40, 1, 16)]
    sc = torch.full((max(sizes),), 0x5A, dtype=torch.uint8, device=solver.device)
    a = np.concatenate([np.zeros((1, 81), np.uint8), h1[None], boards[light[:30]]])
    count, status = _outputs(solver, len(a))
    rc, stats = _raw(solver, torch.from_numpy(a).to(solver.device), count, status, sc, sizes[1], slice=32, max_rounds=4,
                     max_tasks=64, max_waves=2)
    assert rc == 0 and stats["rounds"] == 4 and stats["parks"] > 0, stats
    count, status = count.cpu().numpy(), status.cpu().numpy()
    assert status[0] == E.PARTIAL and status[1] == E.PARTIAL
    E.check_bounds(count, status, np.concatenate([[EMPTY_MORE, E.H1_COUNT], want[light[:30]]]))
    b, idx = E.mixed(68)
    count, status = _outputs(solver, len(b))
    rc, stats = _raw(solver, torch.from_numpy(b).to(solver.device), count, status, sc, sizes[0], slice=32,
                     max_rounds=E.MANY, max_tasks=64, max_waves=2)
    assert rc == 0
    _same(count.cpu().numpy(), status.cpu().numpy(), idx)
    count, status = _outputs(solver, 40)
    rc, stats = _raw(solver, torch.from_numpy(boards[light]).to(solver.device), count, status, sc, sizes[2], slice=32,
                     max_rounds=E.MANY, max_tasks=16, max_waves=1)
    assert rc == 0
    _same(count.cpu().numpy(), status.cpu().numpy(), light)


# ---- 3. PARTIAL is a lower bound, DONE is exact, neither disturbs the other

def test_h1_out_of_budget_is_a_positive_lower_bound(solver):
    """H1 alone on one wave, 8 rounds of 32 passes: fewer than 8 x (32 + 82) x
    64 = 58 368 passes, and a completion costs a pass, so H1's 885 469 cannot
    be reached: PARTIAL, 0 < count <= 58 368."""
    h1, want = E.load_fixture()["h1"]
    bound = E.pass_bound(**E.H1_BUDGET)
    assert bound == 58368 < want
    count, status, stats = _run(solver, h1[None], **E.H1_BUDGET)
    print(int(count[0]), stats)
    assert status[0] == E.PARTIAL and stats["rounds"] == 8
    assert 0 < count[0] <= bound


def test_mixed_budget_done_is_exact_partial_is_a_lower_bound(solver):
    """Set b among light boards at a budget that leaves a mix (chosen on the
    host model, where 25..75 % of set b come back PARTIAL): DONE => the exact
    count, PARTIAL => 0 <= count <= the exact count, no other status; at least
    one of each among set b; a board with more completions than the call has
    passes is PARTIAL.  The shares themselves are not asserted: which lane
    reserves first is not fixed."""
    boards, want, is_b = E.budget_mix()
    count, status, stats = _run(solver, boards, **E.MIX_BUDGET)
    part = E.check_bounds(count, status, want)
    print(stats, "PARTIAL in set b:", int(part[is_b].sum()), "elsewhere:", int(part[~is_b].sum()))
    assert part[is_b].any() and (~part[is_b]).any()
    # (none at this budget: a budget below set b's largest count finishes next to none of it, lanes serve boards in
    # their order, not by size; test_h1_out_of_budget_is_a_positive_lower_bound is where the bound bites)
    assert part[want > E.pass_bound(**E.MIX_BUDGET)].all()


# ---- 4. additivity on H2

def test_h2_is_the_sum_of_its_children(solver):
    """H2 (7 299 350, the fixture) with one more clue at each of three empty
    cells: the nine children of a cell add up to H2's count; then the 81
    children of two cells at once, whose rows add up to the one-clue
    children.  No child's count is recorded anywhere."""
    boards, want, _ = E.pool()
    h2, total = E.load_fixture()["h2"]
    assert total == E.H2_COUNT
    cells = [int(c) for c in np.nonzero(h2 == 0)[0][list(E.H2_CELLS)]]
    light = E.light(36)
    batch = np.concatenate([E.with_clue(h2, (c,)) for c in cells] + [h2[None], boards[light]])
    order = np.random.default_rng(4).permutation(len(batch))
    count, status, stats = _run(solver, batch[order])
    print("one clue", stats)
    back = np.empty_like(order)
    back[order] = np.arange(len(order))
    count, status = count[back], status[back]
    assert (status == E.DONE).all()
    one = count[:27].reshape(3, 9)
    assert one.sum(1).tolist() == [total] * 3, one.tolist()
    assert ((one > 0).sum(1) >= 2).all()
    for k, c in enumerate(cells):
        for d in range(1, 10):
            assert not E.clue_clashes(h2, c, d) or one[k, d - 1] == 0, (c, d)
    assert int(count[27]) == total
    assert np.array_equal(count[28:], want[light])
    two, status, stats = _run(solver, E.with_clue(h2, cells[:2]))
    print("two clues", stats)
    assert (status == E.DONE).all()
    assert int(two.sum()) == total and np.array_equal(two.reshape(9, 9).sum(1), one[0])
    assert np.array_equal(two.reshape(9, 9).sum(0), one[1])


# ---- 5. invariance under symmetry

def test_image_board_is_apply_symmetry():
    """The images the invariance test launches follow gen.apply_symmetry's
    convention (symmetry_cases pins it in full on the CPU)."""
    from sudoku_solver_distributed_amd.gen import CANON_SYMMETRIES, apply_symmetry
    boards = E.pool()[0][E.symmetry_selection(E.SYM_TINY_BUDGET)[:8]]
    sym = np.random.default_rng(12).integers(0, CANON_SYMMETRIES, size=len(boards))
    images, maps = apply_symmetry(boards, sym)
    for b, s, m, img in zip(boards, sym, maps, images):
        assert np.array_equal(S.image_board(b, S.from_number(s, m)), img)


@pytest.mark.parametrize("knobs", ("default", "tiny"))
def test_images_count_what_their_boards_count(solver, knobs):
    """Every selected pool board and its three seeded images in one shuffled
    launch: count and status of a board and of all its images are equal, and
    equal to the fixture's or the oracle's."""
    rows, source, syms = E.symmetry_rows(E.SYM_BUDGET if knobs == "default" else E.SYM_TINY_BUDGET)
    assert len(syms) > len(rows) // 2 and all((rows[r] != E.pool()[0][source[r]]).any() for r in list(syms)[:64])
    count, status, stats = _run(solver, rows, **({} if knobs == "default" else E.TINY))
    print(knobs, len(rows), stats)
    _same(count, status, source)
    if knobs == "tiny":
        assert stats["parks"] > 0 and stats["donated"] > 0


# ---- 6. agreement with the other entries

@pytest.fixture(scope="module")
def pool_exact(solver):
    """The whole pool at the default knobs, once: equal to the fixture and
    the oracle (test_gpu_exact.py asserts that; here too)."""
    boards, want, want_status = E.pool()
    count, status, _ = _run(solver, boards)
    _same(count, status, np.arange(len(boards)))
    return count, status


def test_capped_count_and_candidates_agree_with_the_exact_count(solver, pool_exact):
    exact, status = pool_exact
    d = torch.from_numpy(E.pool()[0].copy()).to(solver.device)
    invalid = status == E.INVALID
    assert invalid.sum() == 1 and (status[~invalid] == E.DONE).all()
    for limit in (2, 64, 1024):
        capped = solver.count_solutions(d, limit=limit).cpu().numpy()
        assert np.array_equal(capped == -1, invalid)
        assert np.array_equal(capped[~invalid], np.minimum(limit, exact[~invalid]))
    _, k = solver.candidates(d, return_count=True)
    k = k.cpu().numpy()
    assert np.array_equal(k == -1, invalid) and np.array_equal(k[~invalid], np.minimum(2, exact[~invalid]))


def test_every_placement_agrees_with_unique_candidates(solver, pool_exact):
    """16 boards of set d and all their children "board plus (c, d)": a
    child has a completion exactly where marks has the bit, exactly one
    exactly where once has it, and the nine children of a cell add up to the
    board's own count."""
    sel, kids, parent, cell, digit = E.placements()
    child, status, stats = _run(solver, kids)
    print(len(kids), stats)
    assert (status == E.DONE).all()
    once, marks = solver.unique_candidates(torch.from_numpy(E.pool()[0][sel]).to(solver.device), return_marks=True)
    ones, several = E.check_placements(child, once.cpu().numpy().view(np.uint16), marks.cpu().numpy().view(np.uint16),
                                       pool_exact[0][sel])
    assert ones >= 200 and several >= 200, (ones, several)


# ---- 7. place and batch independence

def test_h1_counts_the_same_wherever_it_stands(solver):
    """H1 first, last of the first wave, first of the second and last of 130
    boards on three waves, then the same batch reversed."""
    _, want, _ = E.pool()
    h1, total = E.load_fixture()["h1"]
    batch, src = E.placed(130, h1, (0, 63, 64, -1), E.light(126))
    assert (src < 0).sum() == 4 and src[0] == src[63] == src[64] == src[129] == -1
    expect = np.where(src < 0, total, want[np.maximum(src, 0)])
    for boards, exp in ((batch, expect), (batch[::-1], expect[::-1])):
        count, status, stats = _run(solver, boards, max_waves=3, max_rounds=E.MANY)
        print(stats)
        assert (status == E.DONE).all() and np.array_equal(count, exp)


# ---- 8. the knobs' corners

def test_ring_of_two_lines(solver):
    """max_tasks = 1: a stack of more than two levels can only park."""
    idx = E.light(128)
    count, status, stats = _run(solver, E.pool()[0][idx], max_tasks=1, slice=4, max_waves=2, max_rounds=E.MANY)
    print(stats)
    _same(count, status, idx)
    assert stats["parks"] > 0


def test_one_round_does_it_all(solver):
    """A slice above any pass count (the largest the 2^63 check lets through
    with one round): one round, nothing donated, nothing parked."""
    idx = E.light(128)
    count, status, stats = _run(solver, E.pool()[0][idx], slice=2 ** 31 - 1, max_rounds=1, max_waves=2)
    _same(count, status, idx)
    assert (stats["rounds"], stats["donated"], stats["parks"]) == (1, 0, 0), stats


# ---- 9. two callers

def test_two_threads_call_at_once(solver):
    """Two threads, each with its own stream, scratch and outputs, start on a
    barrier: the library runs one launch sequence at a time, both return 0
    with exact answers."""
    boards, idx = E.mixed(68)
    perms = [np.arange(68), np.random.default_rng(9).permutation(68)]
    need = _need(solver, 68, E.TINY["max_waves"], E.TINY["max_tasks"])
    jobs = []
    for p in perms:
        jobs.append(dict(d=torch.from_numpy(np.ascontiguousarray(boards[p])).to(solver.device), out=_outputs(solver, 68),
                         sc=torch.full((need,), 0xA5, dtype=torch.uint8, device=solver.device),
                         stream=torch.cuda.Stream(solver.device), idx=idx[p]))
    torch.cuda.synchronize(solver.device)
    barrier = threading.Barrier(2)

    def call(job):
        barrier.wait()
        job["rc"], job["stats"] = _raw(solver, job["d"], *job["out"], job["sc"], need, stream=job["stream"], **E.TINY)

    threads = [threading.Thread(target=call, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize(solver.device)
    for j in jobs:
        assert j.get("rc") == 0, j.get("rc")
        _same(j["out"][0].cpu().numpy(), j["out"][1].cpu().numpy(), j["idx"])
        assert j["stats"]["parks"] > 0
