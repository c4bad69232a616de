// Host build of rule D's box -> row table of
// sudoku_solver_distributed_amd/csrc/plane_solver.h (lock_fill, lock_index,
// lock_entry, and the passes that take the table) for the CPU test-suite
// (tests/test_lock_table.py): the lookup against point_rows_apply on every
// 27-bit band word, and plane::pass_ahead with the table in lockstep with
// plane::pass_ahead without it along host_model.h's searches.  Not a product
// path.
#include <stdint.h>
#include <string.h>

#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"

// the table as the plane kernel fills it: `nthreads` threads, each its share
extern "C" void lock_table_fill(uint32_t *tbl, uint32_t nthreads)
{
    for (uint32_t t = 0; t < nthreads; ++t) plane::lock_fill(tbl, t, nthreads);
}

extern "C" uint32_t lock_table_index(uint32_t y) { return plane::lock_index(y); }

// every band word (27 cells, guard bits clear): words on which
// y & tbl[lock_index(y)] differs from point_rows_apply(y), or whose index is
// out of the table; *first = the first such word
extern "C" int64_t lock_table_check_all(const uint32_t *tbl, uint32_t *first)
{
    int64_t bad = 0;
    for (uint32_t r2 = 0; r2 < 512; ++r2)
        for (uint32_t r1 = 0; r1 < 512; ++r1)
            for (uint32_t r0 = 0; r0 < 512; ++r0) {
                const uint32_t y = r0 | (r1 << 10) | (r2 << 20);
                const uint32_t i = plane::lock_index(y);
                if (i >= (uint32_t)plane::LOCK_ENTRIES || (y & tbl[i]) != plane::point_rows_apply(y)) {
                    if (!bad) *first = y;
                    bad++;
                }
            }
    return bad;
}

static bool same(const plane::Board &A, const plane::Board &B)
{
    for (int d = 0; d < 9; ++d)
        for (int b = 0; b < 3; ++b)
            if (A.P[d][b] != B.P[d][b]) return false;
    return true;
}

// The look-ahead lane solver (host_model.h's lane phase, the root rule on as in
// the plane kernel's unordered launches) over n boards; every pass is run
// twice from the same state, without and with the table.  Returns the passes
// after which the planes, the verdict, und[] or nd[] differ; *passes = all.
extern "C" int64_t lock_table_lockstep(const uint8_t *in, int64_t n, const uint32_t *tbl, int node_order,
                                       uint32_t max_depth, uint32_t mrv_after, uint64_t *passes)
{
    static host::LineStack lines;
    const plane::WordStack<host::LineStack> ls = {lines};
    int64_t bad = 0;
    *passes = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t x[21], und[3], nd[3];
        host::words_of(in + i * 81, x);
        plane::Board B;
        bool clash = false;
        if (!plane::load_words(B, x, clash, nd) || clash) continue;
        for (int b = 0; b < 3; ++b) und[b] = plane::ROWS & ~nd[b];
        uint32_t depth = 0, lg = 0, mst = 0;
        int s = plane::S_CONT;
        while (s == plane::S_CONT) {
            plane::Board T = B;
            uint32_t tu[3] = {und[0], und[1], und[2]}, tn[3] = {nd[0], nd[1], nd[2]};
            const int r = plane::pass_ahead(B, und, nd);
            const int rt = plane::pass_ahead(T, tu, tn, tbl);
            ++*passes;
            bad += r != rt || !same(B, T) || memcmp(und, tu, sizeof und) || memcmp(nd, tn, sizeof nd);
            s = plane::search_step_ahead(B, und, nd, r, depth, mst, ls, node_order, max_depth, mrv_after, lg, true);
        }
    }
    return bad;
}

// plane::pass with the table against plane::pass on n random plane states
// (the pass before the look-ahead one keeps its table overload too)
extern "C" int64_t lock_table_pass_random(const uint32_t *tbl, int64_t n, uint64_t seed)
{
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); };
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i) {
        plane::Board A;
        const int dens = (int)(rnd() % 3);  // sparse, half, dense planes
        for (int d = 0; d < 9; ++d)
            for (int b = 0; b < 3; ++b) {
                uint32_t w = rnd() ^ (rnd() << 11);
                if (dens == 0) w &= rnd() ^ (rnd() << 11);
                if (dens == 2) w |= rnd() ^ (rnd() << 11);
                A.P[d][b] = w & plane::ROWS;
            }
        for (int b = 0; b < 3; ++b) A.Det[b] = 0;
        plane::Board T = A;
        uint32_t ua[3], ut[3];
        const int r = plane::pass(A, ua), rt = plane::pass(T, ut, tbl);
        bad += r != rt || !same(A, T) || memcmp(ua, ut, sizeof ua) || memcmp(A.Det, T.Det, sizeof A.Det);
    }
    return bad;
}
