// Host build of sudoku_solver_distributed_amd/csrc/plane_uniq.h (the unique
// candidates: uniq_iter, uniq_count, uniq_board -- what uniq_kernel's lane loop
// runs) for the CPU test-suite (tests/test_uniq_host.py), checked against the
// oracle's counter asked once per cell and digit.  Not a product path.
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"
#include "../../sudoku_solver_distributed_amd/csrc/plane_uniq.h"

static_assert((int)host::LineStack::LEVELS >= (int)plane::UNIQ_LEVELS, "a lane's lines");
// uniq_kernel's per-lane lines: the search's levels and the lines of R, V, U, W / T
static host::LineStack lines;

// once[81 i + c] = the digits exactly one valid completion of board i puts
// into cell c (bit d-1 for digit d); marks (may be NULL) = the digits at least
// one does; count[i] (may be NULL) = 0 / 1 / 2 as the marks say, -1 for a byte
// > 9, 0 for clashing givens, -3 (and zero arrays) if a search needed more
// than max_depth (<= 81) levels.  sweep: completions before the targeted
// searches (0: the compiled SDK_UNIQ_SWEEP).  stats (may be NULL): passes,
// passes in the sweep, targeted searches, deepest stack depth, summed /
// maximal over the boards, and the most passes of one board.  board_passes
// (may be NULL): n numbers, each board's passes.
extern "C" void uniq_host_batch(const uint8_t *in, uint16_t *once, uint16_t *marks, int32_t *count, int64_t n,
                                uint32_t max_depth, uint32_t sweep, uint64_t *stats, uint64_t *board_passes)
{
    plane::UniqStats st = {0, 0, 0, 0};
    uint64_t worst = 0;
    if (max_depth > (uint32_t)plane::COUNT_MAX_DEPTH) max_depth = plane::COUNT_MAX_DEPTH;
    if (!sweep) sweep = SDK_UNIQ_SWEEP;
    if (sweep < 2) sweep = 2;  // plane_uniq.h: a target is an undetermined cell of R
    for (int64_t i = 0; i < n; ++i) {
        uint16_t *o = once + i * 81, *m = marks ? marks + i * 81 : nullptr;
        uint32_t x[21], given[3];
        host::words_of(in + i * 81, x);
        plane::Board B;
        bool clash = false;
        int32_t c;
        if (board_passes) board_passes[i] = 0;
        if (!plane::load_words(B, x, clash, given)) {
            c = -1;
        } else if (clash) {
            c = 0;
        } else {
            const uint64_t p0 = st.passes;
            c = plane::uniq_board(B, given, lines, max_depth, sweep,
                                  [&](int cell, uint32_t mk) {
                                      if (m) m[cell] = (uint16_t)mk;
                                  },
                                  [&](int cell, uint32_t on) { o[cell] = (uint16_t)on; }, st);
            if (st.passes - p0 > worst) worst = st.passes - p0;
            if (board_passes) board_passes[i] = st.passes - p0;
            if (count) count[i] = c;
            continue;
        }
        for (int cell = 0; cell < 81; ++cell) {
            o[cell] = 0;
            if (m) m[cell] = 0;
        }
        if (count) count[i] = c;
    }
    if (stats) {
        stats[0] = st.passes;
        stats[1] = st.sweep_passes;
        stats[2] = st.searches;
        stats[3] = st.max_depth;
        stats[4] = worst;
    }
}
