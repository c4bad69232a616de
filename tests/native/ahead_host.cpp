// Host build of the look-ahead path of
// sudoku_solver_distributed_amd/csrc/plane_solver.h (pass_ahead,
// search_step_ahead: what the plane kernel's lane loop runs) for the CPU
// test-suite (tests/test_pass_ahead.py): checked pass by pass against
// plane::pass, and as a solver (host_model.h's driver) against the same
// driver on plane::pass, the oracle and the wave-wide solver's continuation.
// Not a product path.
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"

using host::words_of;

// The lane solver alone (host_model.h's driver): on plane::pass (ahead = 0)
// or on the look-ahead pass (1).  status: 1 solved, 0 no completion, -1
// invalid byte, 2 left to the wave kernel (clashing givens or depth overflow).
extern "C" void ahead_solve_batch(const uint8_t *in, uint8_t *out, int32_t *status, int64_t n, int node_order,
                                  uint32_t max_depth, uint32_t mrv_after, int ahead, uint64_t *guesses,
                                  uint64_t *passes)
{
    host::Counts c;
    host::solve_batch(in, out, status, n, ahead != 0, host::LANE_ONLY, node_order, max_depth, mrv_after, c);
    *guesses = c.guesses;
    *passes = c.passes_lane;
}

// `lane_guesses` guesses (or the whole search, if it ends first) on the
// look-ahead lane path, stepping exactly like plane_kernel, then the rest of
// the search on the wave-wide solver from the same planes, stack and depth
// (und / nd dropped, as the kernel's tail records drop them).  Statuses as
// ahead_solve_batch.
extern "C" void ahead_wide_batch(const uint8_t *in, uint8_t *out, int32_t *status, int64_t n, int node_order,
                                 uint32_t max_depth, uint32_t mrv_after, uint32_t lane_guesses, uint64_t *passes_lane,
                                 uint64_t *passes_wide)
{
    host::Counts c;
    host::solve_batch(in, out, status, n, true, lane_guesses, node_order, max_depth, mrv_after, c);
    *passes_lane = c.passes_lane;
    *passes_wide = c.passes_wide;
}

// ---- lock-step: pass_ahead against plane::pass

// rule A as a plain loop: the cells with one candidate, the cells with none
static uint32_t plain_rule_a(const plane::Board &B, uint32_t (&single)[3])
{
    uint32_t empty = 0;
    for (int b = 0; b < 3; ++b) {
        uint32_t o = 0, t = 0;
        for (int d = 0; d < 9; ++d) {
            t |= o & B.P[d][b];
            o |= B.P[d][b];
        }
        empty |= plane::ROWS & ~o;
        single[b] = o & ~t;
    }
    return empty;
}

// One pass of both from the state A (planes and Det): false if pass_ahead
// from A's planes and nd = single & ~Det leaves other planes than
// plane::pass, another verdict than that pass's upgraded by rule A on the
// result, or other und' / nd' than the next plane::pass would compute.  A is
// advanced by plane::pass; ra / ua are its verdict and undetermined cells.
static bool lockstep(plane::Board &A, int &ra, uint32_t (&ua)[3])
{
    plane::Board B = A;
    uint32_t single[3], und[3], nd[3];
    plain_rule_a(A, single);
    bool any_nd = false;
    for (int b = 0; b < 3; ++b) {
        nd[b] = single[b] & ~A.Det[b];
        und[b] = plane::ROWS & ~single[b];
        any_nd |= nd[b] != 0;
        B.Det[b] = 0xDEADBEEFu;  // not used on this path
    }
    ra = plane::pass(A, ua);
    const int rb = plane::pass_ahead(B, und, nd);
    for (int d = 0; d < 9; ++d)
        for (int b = 0; b < 3; ++b)
            if (A.P[d][b] != B.P[d][b]) return false;
    // what the next plane::pass computes first: rule A on the new planes
    // against Det = the cells determined when this pass began
    uint32_t s2[3], nd2[3];
    const uint32_t empty2 = plain_rule_a(A, s2);
    bool any2 = false;
    for (int b = 0; b < 3; ++b) {
        nd2[b] = s2[b] & ~A.Det[b];
        any2 |= nd2[b] != 0;
        if (und[b] != (plane::ROWS & ~s2[b]) || nd[b] != nd2[b]) return false;
    }
    int want;
    if (ra == plane::DEAD || empty2) {
        want = plane::DEAD;
    } else if (ra == plane::SOLVED) {
        want = plane::SOLVED;
    } else {
        // a hidden single placed by a pass that is not dead is a cell that
        // became determined: STUCK is "no cell became determined"
        want = any2 ? plane::OPEN : plane::STUCK;
        // plane::pass is OPEN without a newly determined cell on entry only
        // when it placed a hidden single
        if (ra == plane::OPEN && !any_nd && !any2) return false;
    }
    return rb == want;
}

// Along each board's search (branching on the first undetermined cell at a
// fixpoint, as plane_host.cpp's plane_check_pass) and from `nrand` random
// plane states: the number of passes that fail lockstep().
extern "C" int64_t ahead_check_pass(const uint8_t *in, int64_t n, int64_t nrand, uint64_t seed)
{
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t x[21];
        words_of(in + i * 81, x);
        plane::Board A;
        bool clash = false;
        if (!plane::load_words(A, x, clash)) continue;
        for (int step = 0; step < 400; ++step) {
            uint32_t ua[3];
            int ra;
            if (!lockstep(A, ra, ua)) { bad++; break; }
            if (ra == plane::DEAD || ra == plane::SOLVED) break;
            if (ra == plane::STUCK) {
                int band, pos;
                plane::pick_cell(ua, (int)(i & 1), band, pos);
                const uint32_t cand = plane::cell_cand(A, band, pos);
                if (!cand) break;  // (rule D emptied the cell: the next pass is DEAD)
                // mostly the lowest digit; every third board the highest (more dead ends)
                uint32_t d = cand & (0u - cand);
                if (i % 3 == 2) d = 1u << (31 - __builtin_clz(cand));
                plane::set_cell(A, band, pos, d);
            }
        }
    }
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); };
    for (int64_t i = 0; i < nrand; ++i) {
        plane::Board A;
        const int density = (int)(rnd() % 4);  // sparse to dense planes
        for (int d = 0; d < 9; ++d)
            for (int k = 0; k < 3; ++k) {
                uint32_t w = rnd();
                for (int j = 0; j < density; ++j) w |= rnd();
                A.P[d][k] = w & plane::ROWS;
            }
        for (int k = 0; k < 3; ++k) A.Det[k] = (rnd() & rnd()) & plane::ROWS;
        for (int step = 0; step < 8; ++step) {
            uint32_t ua[3];
            int ra;
            if (!lockstep(A, ra, ua)) { bad++; break; }
        }
    }
    return bad;
}
