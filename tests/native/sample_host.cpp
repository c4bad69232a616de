// Host build of sudoku_solver_distributed_amd/csrc/plane_sample.h (the random
// completion: sample_choose, sample_step, sample_iter, sample_board -- what
// sample_kernel's lane loop runs) for the CPU test-suite
// (tests/test_sample_host.py), checked against the oracle and against the
// rule restated in the test.  Not a product path.
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"
#include "../../sudoku_solver_distributed_amd/csrc/plane_sample.h"

// sample_kernel's per-lane stack lines
static host::LineStack lines;

// sdk_sample_batch on the host: item q = board q / per_board (in == NULL:
// the empty board) under key first_key + q; out[81 q ..] = its completion and
// status[q] = 1, or the input board with 0 (no completion, clashing givens
// included), -1 (a byte > 9) or -3 (the search needed more than max_depth
// (<= 81) levels).  passes, deepest, draws (each may be NULL): per item the
// passes run, the deepest stack depth reached and the draws made.
extern "C" void sample_host_batch(const uint8_t *in, uint8_t *out, int32_t *status, int64_t n, int per_board,
                                  uint64_t seed, uint64_t first_key, uint32_t max_depth, uint64_t *passes,
                                  uint32_t *deepest, uint32_t *draws)
{
    static const uint8_t empty[81] = {0};
    if (max_depth > (uint32_t)plane::COUNT_MAX_DEPTH) max_depth = plane::COUNT_MAX_DEPTH;
    const int64_t items = n * per_board;
    for (int64_t q = 0; q < items; ++q) {
        const uint8_t *src = in ? in + (q / per_board) * 81 : empty;
        uint8_t *dst = out + q * 81;
        plane::SampleStats st = {0, 0, 0};
        uint32_t x[21], given[3];
        host::words_of(src, x);
        plane::Board B;
        bool clash = false;
        int32_t s;
        if (!plane::load_words(B, x, clash, given)) {
            s = -1;
        } else if (clash) {
            s = 0;
        } else {
            const int k = plane::sample_board(B, given, lines, max_depth, plane::sample_stream(seed, first_key + (uint64_t)q), st);
            s = k == plane::P_FOUND ? 1 : k == plane::P_NONE ? 0 : (int32_t)plane::COUNT_FAULT;
        }
        if (s == 1) plane::store_values(B, [&](int cell, uint32_t v) { dst[cell] = (uint8_t)v; });
        else memcpy(dst, src, 81);
        status[q] = s;
        if (passes) passes[q] = st.passes;
        if (deepest) deepest[q] = st.max_depth;
        if (draws) draws[q] = st.draws;
    }
}

// choose(mask) for draw number t of the item (seed, key): the digit bit
extern "C" uint32_t sample_host_pick(uint32_t mask, uint64_t seed, uint64_t key, uint32_t t)
{
    return plane::sample_choose(mask, plane::sample_stream(seed, key), t);
}
