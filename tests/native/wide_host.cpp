// Host build of sudoku_solver_distributed_amd/csrc/plane_wide.h (the wave-wide
// tail solver of plane_kernel) for the CPU test-suite
// (tests/test_plane_solver.py): the same source, over an emulated 64-lane
// wave, is checked against the lane solver (plane_solver.h) and the oracle
// before the GPU runs it.  Not a product path.
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"

using host::to_wave;
using host::words_of;

// `lane_guesses` guesses (or the whole search, if it ends first) on the lane
// solver's reference pass (plane::pass + search_step; plane_kernel's lanes run
// the look-ahead pass, whose hand-over ahead_host.cpp's ahead_wide_batch
// models), then the rest of the search on the wave-wide solver from the same
// state and stack (host_model.h's driver).  status: 1 solved, 0 no completion, -1 invalid
// byte, 2 left to the wave kernel (clashing givens or depth overflow).
// guesses: lane and wide together.
extern "C" void wide_solve_batch(const uint8_t *in, uint8_t *out, int32_t *status, int64_t n, int node_order,
                                 uint32_t max_depth, uint32_t mrv_after, uint32_t lane_guesses, uint64_t *guesses,
                                 uint64_t *passes_lane, uint64_t *passes_wide)
{
    host::Counts c;
    host::solve_batch(in, out, status, n, false, lane_guesses, node_order, max_depth, mrv_after, c);
    *guesses = c.guesses;
    *passes_lane = c.passes_lane;
    *passes_wide = c.passes_wide;
}

// Fixpoints of the wide pass against the lane pass, from each loaded board
// and from `trials` random mid-search states per board (random cells fixed to
// a random candidate between propagations).  Both passes are iterated until
// the state stops changing (a STUCK pass may still have removed places by
// rule D, which neither pass counts as progress; the orders differ, the
// closure does not).  Returns the number of states where the two
// disagree (verdict, planes or undetermined cells) and the STUCK side holds
// no two determined cells with one digit in a unit: such a pair is a
// contradiction neither rule set flags at once, and which pass meets it
// first depends on the order singles are applied (both stay sound).
static bool determined_clash(const plane::Board &E)
{
    uint32_t det[3];
    for (int b = 0; b < 3; ++b) {
        uint32_t o = 0, t = 0;
        for (int d = 0; d < 9; ++d) {
            t |= o & E.P[d][b];
            o |= E.P[d][b];
        }
        det[b] = o & ~t;
    }
    return plane::givens_clash(E, det);
}

extern "C" int64_t wide_check_fixpoint(const uint8_t *in, int64_t n, int trials, uint32_t seed)
{
    const wide::Lanes L = wide::lanes();
    int64_t bad = 0;
    uint32_t rs = seed * 2654435761u + 1u;
    auto rnd = [&rs]() { rs ^= rs << 13; rs ^= rs >> 17; rs ^= rs << 5; return rs; };
    for (int64_t i = 0; i < n; ++i) {
        uint32_t x[21];
        words_of(in + i * 81, x);
        plane::Board B0;
        bool clash = false;
        if (!plane::load_words(B0, x, clash) || clash) continue;
        for (int trial = 0; trial <= trials; ++trial) {
            plane::Board B = B0;
            uint32_t ul[3];
            int rl = plane::STUCK;
            const int guesses = trial ? 1 + (int)(rnd() % 4) : 0;
            for (int k = 0; k < guesses; ++k) {
                while ((rl = plane::pass(B, ul)) == plane::OPEN) {}
                if (rl != plane::STUCK) break;
                int band, pos;
                plane::pick_cell(ul, (int)(rnd() & 1u), band, pos);
                uint32_t d = plane::cell_cand(B, band, pos);
                for (uint32_t j = rnd() % (uint32_t)__builtin_popcount(d); j; --j) d &= d - 1;
                plane::set_cell(B, band, pos, d & (0u - d));
            }
            if (rl != plane::STUCK) continue;
            wide::V w = to_wave(B, L), det(0u), und;
            for (int k = 0; k < 64; ++k)
                if (L.b.x[k] < 3) det.x[k] = B.Det[L.b.x[k]];
            int rw;
            for (;;) {
                const plane::Board prev = B;
                rl = plane::pass(B, ul);
                if (rl == plane::OPEN || (rl == plane::STUCK && memcmp(prev.P, B.P, sizeof B.P) != 0)) continue;
                break;
            }
            for (;;) {
                const wide::V prev = w;
                rw = wide::pass(w, det, und, L);
                bool moved = false;
                for (int k = 0; k < 64; ++k) moved |= prev.x[k] != w.x[k];
                if (rw == wide::OPEN || (rw == wide::STUCK && moved)) continue;
                break;
            }
            bool diff = rl != rw;
            if (!diff && rl == plane::STUCK) {
                const wide::V want = to_wave(B, L);
                for (int k = 0; k < 64; ++k) diff |= want.x[k] != w.x[k];
                for (int b = 0; b < 3; ++b) diff |= ul[b] != und.x[16 * b];
            }
            if (diff) {
                plane::Board E = B;  // the STUCK side's planes
                if (rw == wide::STUCK)
                    for (int k = 0; k < 64; ++k)
                        if ((L.valid.m >> k) & 1) E.P[L.d.x[k]][L.b.x[k]] = w.x[k];
                bad += !determined_clash(E);
            }
        }
    }
    return bad;
}
