// Host build of sudoku_solver_distributed_amd/csrc/plane_min.h (redundant
// givens: min_start, min_iter, min_board -- what min_kernel's lane loop runs)
// for the CPU test-suite (tests/test_min_host.py), checked against the
// definition written as the plain loop over the oracle's counter.  Not a
// product path.
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"
#include "../../sudoku_solver_distributed_amd/csrc/plane_min.h"

static_assert((int)host::LineStack::LEVELS >= (int)plane::MIN_LEVELS, "a lane's lines");
// min_kernel's per-lane lines: the search's levels and the puzzle's line
static host::LineStack lines;

// the lane's view of its board: the turn order and the working copy in `out`
struct HostIo {
    const uint8_t *turns;  // NULL: turn t takes cell t
    uint8_t *out;
    uint32_t order(uint32_t t) const { return turns ? turns[t] : t; }
    uint32_t digit(uint32_t c) const { return out[c]; }
    void erase(uint32_t c) const { out[c] = 0; }
};

// sdk_minimize_batch on the host: out[81 i ..] = board i minimised (mode 0,
// the turns from order[81 i ..] or cell by cell when order is NULL, until
// max_empty cells are empty) or with every individually redundant given erased
// (mode 1); status[i] = min(2, completions), -1 for a byte > 9, -3 (out =
// input) if a search needed more than max_depth (<= 81) levels; removed (may
// be NULL).  stats (may be NULL): passes, tests started, deepest stack depth,
// summed / maximal over the boards.
extern "C" void min_host_batch(const uint8_t *in, const uint8_t *order, uint8_t *out, int32_t *status, int32_t *removed,
                               int64_t n, int mode, int max_empty, uint32_t max_depth, uint64_t *stats)
{
    plane::MinStats st = {0, 0, 0};
    if (max_depth > (uint32_t)plane::COUNT_MAX_DEPTH) max_depth = plane::COUNT_MAX_DEPTH;
    const bool probe = mode == 1;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t *src = in + i * 81;
        uint8_t *dst = out + i * 81;
        memcpy(dst, src, 81);
        uint32_t x[21], given[3], gone = 0;
        host::words_of(src, x);
        plane::Board B;
        bool clash = false;
        int32_t s;
        if (!plane::load_words(B, x, clash, given)) {
            s = -1;
        } else if (clash) {
            s = 0;
        } else {
            const HostIo io = {order && !probe ? order + i * 81 : nullptr, dst};
            s = plane::min_board(B, given, lines, max_depth, probe, (uint32_t)max_empty, io, gone, st);
            if (s == (int32_t)plane::COUNT_FAULT) {
                memcpy(dst, src, 81);
                gone = 0;
            }
        }
        status[i] = s;
        if (removed) removed[i] = (int32_t)gone;
    }
    if (stats) {
        stats[0] = st.passes;
        stats[1] = st.tests;
        stats[2] = st.max_depth;
    }
}
