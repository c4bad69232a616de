// Host build of sudoku_solver_distributed_amd/csrc/plane_count.h (the capped
// completion count: count_step, count_iter, count_board -- what count_kernel's
// lane loop runs) for the CPU test-suite (tests/test_count_host.py), checked
// against the oracle's counter.  Not a product path.
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"
#include "../../sudoku_solver_distributed_amd/csrc/plane_count.h"

// count_kernel's per-lane stack lines
static host::LineStack lines;

// count[i] = min(limit, completions of board i), -1 for a byte > 9, 0 for
// clashing givens, -3 if the search needed more than max_depth (<= 81)
// levels.  first (may be NULL): the first completion met for count >= 1, the
// input board otherwise.  deepest: the deepest stack depth reached.
extern "C" void count_host_batch(const uint8_t *in, int32_t *count, uint8_t *first, int64_t n, int32_t limit,
                                 uint32_t max_depth, uint64_t *passes, uint32_t *deepest)
{
    plane::CountStats st = {0, 0};
    if (max_depth > (uint32_t)plane::COUNT_MAX_DEPTH) max_depth = plane::COUNT_MAX_DEPTH;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t *src = in + i * 81;
        uint8_t *dst = first ? first + i * 81 : nullptr;
        uint32_t x[21], given[3];
        host::words_of(src, x);
        plane::Board B;
        bool clash = false;
        int32_t c;
        if (!plane::load_words(B, x, clash, given)) {
            c = -1;
        } else if (clash) {
            c = 0;
        } else {
            c = plane::count_board(
                B, given, lines, limit, max_depth,
                [&](const plane::Board &S) {
                    if (dst) plane::store_values(S, [&](int cell, uint32_t v) { dst[cell] = (uint8_t)v; });
                },
                st);
        }
        count[i] = c;
        if (dst && c <= 0) memcpy(dst, src, 81);
    }
    *passes = st.passes;
    *deepest = st.max_depth;
}
