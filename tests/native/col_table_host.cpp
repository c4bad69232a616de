// Host build of rule C's column table of
// sudoku_solver_distributed_amd/csrc/plane_solver.h (col_fill, col_entry,
// col_offset, and the passes that take plane::PassTables) for the CPU
// test-suite (tests/test_col_table.py): the entries against the arithmetic of
// pass_body() on every 9-bit column pattern, and plane::pass_ahead_tables in
// lockstep with plane::pass_ahead along host_model.h's searches.  Not a
// product path.
#include <stdint.h>
#include <string.h>

#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"

extern "C" int col_table_entries() { return plane::COL_ENTRIES; }
extern "C" uint32_t col_table_box_shift() { return plane::COL_BOX_SHIFT; }

// both tables as the plane kernel fills them: `nthreads` threads, each its share
extern "C" void col_table_fill(uint32_t *lock, uint16_t *col, uint32_t nthreads)
{
    for (uint32_t t = 0; t < nthreads; ++t) {
        plane::lock_fill(lock, t, nthreads);
        plane::col_fill(col, t, nthreads);
    }
}

// the byte offset the pass reads for a band's column word o (junk above bit 8 allowed)
extern "C" uint32_t col_table_offset(uint32_t o) { return plane::col_offset(o); }

// pass_body()'s arithmetic on the column pattern o (plane_solver.h, rule C):
// *vp = the columns of the boxes with exactly one occupied column, *boxes =
// the "box has a place" bits 0 / 3 / 6.  Restated here with plain operators.
extern "C" void col_table_arith(uint32_t o, uint32_t *vp, uint32_t *boxes)
{
    const uint32_t o1 = o >> 1, o2 = o >> 2;
    const uint32_t ob = o | o1 | o2;
    const uint32_t mo = (o & o1) | (o2 & (o | o1));
    const uint32_t vb = (o ^ o1 ^ o2) & ~mo & plane::BOXC;
    *vp = o & (vb * 7u);
    *boxes = ob & plane::BOXC;
}

static bool same(const plane::Board &A, const plane::Board &B)
{
    for (int d = 0; d < 9; ++d)
        for (int b = 0; b < 3; ++b)
            if (A.P[d][b] != B.P[d][b]) return false;
    return true;
}

// The look-ahead lane solver (host_model.h's lane phase, the root rule on as in
// the plane kernel's unordered launches) over n boards, boards with clashing
// givens included (a pass is a function of its planes whatever they mean);
// every pass is run twice from the same state, without tables and with both.
// Returns the passes after which the planes, the verdict, und[] or nd[]
// differ; *passes = all.  Then each board is solved a second time on the
// tables alone: tot[0..1] = passes and guesses without tables, tot[2..3] with,
// tot[4] = boards whose end (verdict or planes) differs.
extern "C" int64_t col_table_lockstep(const uint8_t *in, int64_t n, const uint32_t *lock, const uint16_t *col,
                                      int node_order, uint32_t max_depth, uint32_t mrv_after, uint64_t *passes,
                                      uint64_t *tot)
{
    static host::LineStack lines, lines_t;
    const plane::WordStack<host::LineStack> ls = {lines}, lt = {lines_t};
    const plane::PassTables T = {lock, col};
    int64_t bad = 0;
    *passes = 0;
    for (int k = 0; k < 5; ++k) tot[k] = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t x[21], und[3], nd[3], und0[3], nd0[3];
        host::words_of(in + i * 81, x);
        plane::Board B;
        bool clash = false;
        if (!plane::load_words(B, x, clash, nd)) continue;
        for (int b = 0; b < 3; ++b) und[b] = plane::ROWS & ~nd[b];
        const plane::Board B0 = B;
        memcpy(und0, und, sizeof und);
        memcpy(nd0, nd, sizeof nd);
        uint32_t depth = 0, lg = 0, mst = 0;
        int s = plane::S_CONT;
        while (s == plane::S_CONT) {
            plane::Board C = B;
            uint32_t tu[3] = {und[0], und[1], und[2]}, tn[3] = {nd[0], nd[1], nd[2]};
            const int r = plane::pass_ahead(B, und, nd);
            const int rt = plane::pass_ahead_tables<1>(C, tu, tn, T);
            ++*passes;
            ++tot[0];
            bad += r != rt || !same(B, C) || memcmp(und, tu, sizeof und) || memcmp(nd, tn, sizeof nd);
            s = plane::search_step_ahead(B, und, nd, r, depth, mst, ls, node_order, max_depth, mrv_after, lg, true);
        }
        tot[1] += lg;
        // the same search on the tables alone
        plane::Board C = B0;
        uint32_t tu[3] = {und0[0], und0[1], und0[2]}, tn[3] = {nd0[0], nd0[1], nd0[2]};
        uint32_t dt = 0, lgt = 0, mt = 0;
        int st = plane::S_CONT;
        while (st == plane::S_CONT) {
            const int rt = plane::pass_ahead_tables<1>(C, tu, tn, T);
            ++tot[2];
            st = plane::search_step_ahead(C, tu, tn, rt, dt, mt, lt, node_order, max_depth, mrv_after, lgt, true);
        }
        tot[3] += lgt;
        tot[4] += st != s || (s == plane::S_SOLVED && !same(B, C));
    }
    return bad;
}

// n random plane states (sparse, half, dense): plane::pass and
// plane::pass_ahead with both tables against the same passes without.
extern "C" int64_t col_table_pass_random(const uint32_t *lock, const uint16_t *col, int64_t n, uint64_t seed)
{
    const plane::PassTables T = {lock, col};
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); };
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i) {
        plane::Board A;
        const int dens = (int)(rnd() % 3);
        for (int d = 0; d < 9; ++d)
            for (int b = 0; b < 3; ++b) {
                uint32_t w = rnd() ^ (rnd() << 11);
                if (dens == 0) w &= rnd() ^ (rnd() << 11);
                if (dens == 2) w |= rnd() ^ (rnd() << 11);
                A.P[d][b] = w & plane::ROWS;
            }
        for (int b = 0; b < 3; ++b) A.Det[b] = 0;
        plane::Board C = A, A2 = A, C2 = A;
        uint32_t ua[3], ut[3];
        const int r = plane::pass(A, ua), rt = plane::pass_tables<1>(C, ut, T);
        bad += r != rt || !same(A, C) || memcmp(ua, ut, sizeof ua) || memcmp(A.Det, C.Det, sizeof A.Det);
        // the look-ahead pass from the same planes: und / nd as rule A gives them
        uint32_t single[3], u1[3], n1[3], u2[3], n2[3];
        plane::rule_a(A2, single);
        for (int b = 0; b < 3; ++b) {
            u1[b] = u2[b] = plane::ROWS & ~single[b];
            n1[b] = n2[b] = single[b];
        }
        const int q = plane::pass_ahead(A2, u1, n1), qt = plane::pass_ahead_tables<1>(C2, u2, n2, T);
        bad += q != qt || !same(A2, C2) || memcmp(u1, u2, sizeof u1) || memcmp(n1, n2, sizeof n1);
    }
    return bad;
}

// The overloads that take a bare table pointer read the 512 lock words and
// nothing after them: n random states through plane::pass and
// plane::pass_ahead with `tbl` (512 words followed by whatever the caller put
// there) against the same passes on a private copy of the 512 words.
extern "C" int64_t col_table_old_overloads(const uint32_t *tbl, int64_t n, uint64_t seed)
{
    uint32_t own[plane::LOCK_ENTRIES];
    memcpy(own, tbl, sizeof own);
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); };
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i) {
        plane::Board A;
        for (int d = 0; d < 9; ++d)
            for (int b = 0; b < 3; ++b) A.P[d][b] = (rnd() ^ (rnd() << 11)) & (rnd() | (rnd() << 11)) & plane::ROWS;
        for (int b = 0; b < 3; ++b) A.Det[b] = 0;
        plane::Board C = A, A2 = A, C2 = A;
        uint32_t ua[3], ut[3];
        const int r = plane::pass(A, ua, own), rt = plane::pass(C, ut, tbl);
        bad += r != rt || !same(A, C) || memcmp(ua, ut, sizeof ua);
        uint32_t single[3], u1[3], n1[3], u2[3], n2[3];
        plane::rule_a(A2, single);
        for (int b = 0; b < 3; ++b) {
            u1[b] = u2[b] = plane::ROWS & ~single[b];
            n1[b] = n2[b] = single[b];
        }
        const int q = plane::pass_ahead(A2, u1, n1, own), qt = plane::pass_ahead(C2, u2, n2, tbl);
        bad += q != qt || !same(A2, C2) || memcmp(u1, u2, sizeof u1) || memcmp(n1, n2, sizeof n1);
        // and they are the arithmetic passes
        plane::Board A3 = A2;  // (A2 already passed: one more pass of each)
        plane::Board C3 = A2;
        uint32_t u3[3] = {u1[0], u1[1], u1[2]}, n3[3] = {n1[0], n1[1], n1[2]};
        uint32_t u4[3] = {u1[0], u1[1], u1[2]}, n4[3] = {n1[0], n1[1], n1[2]};
        const int p = plane::pass_ahead(A3, u3, n3), pt = plane::pass_ahead(C3, u4, n4, tbl);
        bad += p != pt || !same(A3, C3);
    }
    return bad;
}
