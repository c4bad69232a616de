// Host build of sudoku_solver_distributed_amd/csrc/plane_cand.h (the exact
// candidates: cand_iter, cand_marks, cand_board -- what cand_kernel's lane loop
// runs) for the CPU test-suite (tests/test_cand_host.py), checked against the
// oracle's counter asked once per cell and digit.  Not a product path.
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"
#include "../../sudoku_solver_distributed_amd/csrc/plane_cand.h"

static_assert((int)host::LineStack::LEVELS >= (int)plane::CAND_LEVELS, "a lane's lines");
// cand_kernel's per-lane lines: the search's levels, R's line and W's
static host::LineStack lines;

// marks[81 i + c] = the digits some valid completion of board i puts into cell
// c (bit d-1 for digit d); count[i] (may be NULL) = 0 / 1 / 2 as the marks
// say, -1 for a byte > 9, 0 for clashing givens, -3 (and zero marks) if a
// search needed more than max_depth (<= 81) levels.  sweep: completions before
// the targeted searches (0: the compiled SDK_CAND_SWEEP).  stats (may be NULL):
// passes, targeted searches, deepest stack depth, summed / maximal over the boards.
extern "C" void cand_host_batch(const uint8_t *in, uint16_t *marks, int32_t *count, int64_t n, uint32_t max_depth,
                                uint32_t sweep, uint64_t *stats)
{
    plane::CandStats st = {0, 0, 0};
    if (max_depth > (uint32_t)plane::COUNT_MAX_DEPTH) max_depth = plane::COUNT_MAX_DEPTH;
    if (!sweep) sweep = SDK_CAND_SWEEP;
    for (int64_t i = 0; i < n; ++i) {
        uint16_t *dst = marks + i * 81;
        uint32_t x[21], given[3];
        host::words_of(in + i * 81, x);
        plane::Board B;
        bool clash = false;
        int32_t c;
        if (!plane::load_words(B, x, clash, given)) {
            c = -1;
        } else if (clash) {
            c = 0;
        } else {
            c = plane::cand_board(B, given, lines, max_depth, sweep, [&](int cell, uint32_t m) { dst[cell] = (uint16_t)m; },
                                  st);
            if (count) count[i] = c;
            continue;
        }
        for (int cell = 0; cell < 81; ++cell) dst[cell] = 0;
        if (count) count[i] = c;
    }
    if (stats) {
        stats[0] = st.passes;
        stats[1] = st.searches;
        stats[2] = st.max_depth;
    }
}
