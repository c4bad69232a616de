// Host build of the root rule of
// sudoku_solver_distributed_amd/csrc/plane_solver.h (search_step_impl's
// root_full: an all-single root is taken as solved without its verifying
// pass, and plane::grid_complete tests the answer, as the plane kernel's
// outbox flush does) for the CPU test-suite (tests/test_root_full.py) and the
// fixture search (tests/golden/make_root_full_cases.py).  Not a product path.
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"

// The look-ahead lane solver (host_model.h's driver) on each board, without
// the rule and with it.  Per board: the answers and statuses of both runs
// (1 solved, 0 no completion, -1 invalid byte, 2 left to the wave kernel), the
// passes of both, whether the board ended by the rule and whether
// grid_complete then rejected it.
extern "C" void rootfull_compare(const uint8_t *in, int64_t n, int node_order, uint32_t max_depth, uint32_t mrv_after,
                                 uint8_t *out_off, int32_t *st_off, uint8_t *out_on, int32_t *st_on,
                                 uint32_t *passes_off, uint32_t *passes_on, uint8_t *by_rule, uint8_t *rejected)
{
    host::Counts c;
    host::BoardInfo *info = new host::BoardInfo[n > 0 ? n : 1];
    host::solve_batch(in, out_off, st_off, n, true, host::LANE_ONLY, node_order, max_depth, mrv_after, c, false, info);
    for (int64_t i = 0; i < n; ++i) passes_off[i] = info[i].passes;
    host::solve_batch(in, out_on, st_on, n, true, host::LANE_ONLY, node_order, max_depth, mrv_after, c, true, info);
    for (int64_t i = 0; i < n; ++i) {
        passes_on[i] = info[i].passes;
        by_rule[i] = info[i].by_rule;
        rejected[i] = info[i].rejected;
    }
    delete[] info;
}

// plane::solve_ahead, the lane solver's own driver, with the rule: 1 solved,
// 0 no completion, -1 left to the wave kernel (-2: a byte > 9 or clashing
// givens, not run)
extern "C" void rootfull_solve_ahead(const uint8_t *in, uint8_t *out, int32_t *status, int64_t n, int node_order,
                                     uint32_t max_depth, uint32_t mrv_after, int root_full)
{
    static host::LineStack lines;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t x[21];
        host::words_of(in + i * 81, x);
        memcpy(out + i * 81, in + i * 81, 81);
        plane::Board B;
        bool clash = false;
        if (!plane::load_words(B, x, clash) || clash) { status[i] = -2; continue; }
        plane::Stats st = {0, 0};
        status[i] = plane::solve_ahead(B, lines, node_order, max_depth, st, mrv_after, root_full != 0);
        if (status[i] == 1) plane::store_values(B, [&](int cell, uint32_t v) { out[i * 81 + cell] = (uint8_t)v; });
    }
}

// plane::grid_complete on full grids given as bytes 1..9 (through the value
// bit-slices, as the kernel's outbox records hold them)
extern "C" void rootfull_grid_complete(const uint8_t *in, int64_t n, uint8_t *ok)
{
    for (int64_t i = 0; i < n; ++i) {
        uint32_t x[21], V[4][3];
        host::words_of(in + i * 81, x);
        const uint32_t bad = plane::slices_from_words(x, V);
        ok[i] = !bad && plane::grid_complete(V);
    }
}
