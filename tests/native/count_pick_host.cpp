// Host build of the count mode's branch rule of
// sudoku_solver_distributed_amd/csrc/plane_solver.h (pick_count_masks: the
// band with the fewest two-candidate cells) for the CPU test-suite
// (tests/test_count_pick_host.py): the lane pick and the wave-wide solver's
// pick against a plain per-cell loop on random plane states, and the solvers
// that branch on it (host_model.h's driver).  Not a product path.
//
// PICK_VARIANT (the rule the two callers use, through SDK_PLANE_COUNT_PICK):
//   0  the header's rule
//   1  mutant: the band with the MOST cells of S
//   2  mutant: the tie-break reversed (the FEWEST undetermined cells)
//   3  the header's rule, counting its calls
//   4  the previous rule (plane::pick_mrv_masks)
#include <stdint.h>

#ifndef PICK_VARIANT
#define PICK_VARIANT 0
#endif
#if PICK_VARIANT
namespace plane {
static inline void variant_pick(const uint32_t (&e2)[3], const uint32_t (&e3)[3], const uint32_t und[3], int &band,
                                int &pos);
}
#define SDK_PLANE_COUNT_PICK variant_pick
#endif
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"

static uint64_t g_calls;

#if PICK_VARIANT
namespace plane {
static inline void variant_pick(const uint32_t (&e2)[3], const uint32_t (&e3)[3], const uint32_t und[3], int &band,
                                int &pos)
{
#if PICK_VARIANT == 3
    g_calls++;
    pick_count_masks(e2, e3, und, band, pos);
#elif PICK_VARIANT == 4
    pick_mrv_masks(e2, e3, und, band, pos);
#else
    const bool a2 = (e2[0] | e2[1] | e2[2]) != 0, a3 = (e3[0] | e3[1] | e3[2]) != 0;
    const uint32_t *s = a2 ? e2 : a3 ? e3 : und;
    band = -1;
    for (int b = 0; b < 3; ++b) {
        if (!s[b]) continue;
        const int n = __builtin_popcount(s[b]), u = __builtin_popcount(und[b]);
        const int bn = band < 0 ? 0 : __builtin_popcount(s[band]), bu = band < 0 ? 0 : __builtin_popcount(und[band]);
#if PICK_VARIANT == 1
        if (band < 0 || n > bn || (n == bn && u > bu)) band = b;
#else
        if (band < 0 || n < bn || (n == bn && u < bu)) band = b;
#endif
    }
    pos = __builtin_ctz(s[band]);
#endif
}
}  // namespace plane
#endif

extern "C" uint64_t pick_calls(void) { return g_calls; }

// ---- the rule by definition, cell by cell

// candidates of the cell at (band, pos), counted over the nine planes
static int cell_count(const plane::Board &B, int band, int pos)
{
    int n = 0;
    for (int d = 0; d < 9; ++d) n += (int)((B.P[d][band] >> pos) & 1u);
    return n;
}

struct Want {
    int band, pos;
    bool tie_s, tie_u;  // two bands share the fewest cells of S; and the most undetermined cells among them
};

static Want plain_pick(const plane::Board &B, const uint32_t und[3], int &level)
{
    // S: the undetermined cells with two candidates if there is one anywhere,
    // else those with three, else all of them
    int cnt[3][10] = {{0}};
    for (int b = 0; b < 3; ++b)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 9; ++c)
                if ((und[b] >> (10 * r + c)) & 1u) {
                    int n = cell_count(B, b, 10 * r + c);
                    cnt[b][n > 9 ? 9 : n]++;
                }
    level = (cnt[0][2] + cnt[1][2] + cnt[2][2]) ? 2 : (cnt[0][3] + cnt[1][3] + cnt[2][3]) ? 3 : 0;
    auto in_s = [&](int b, int p) { return ((und[b] >> p) & 1u) && (level == 0 || cell_count(B, b, p) == level); };
    int ns[3], nu[3];
    for (int b = 0; b < 3; ++b) {
        ns[b] = nu[b] = 0;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 9; ++c) {
                nu[b] += (int)((und[b] >> (10 * r + c)) & 1u);
                ns[b] += in_s(b, 10 * r + c) ? 1 : 0;
            }
    }
    Want w = {-1, -1, false, false};
    for (int b = 0; b < 3; ++b) {
        if (!ns[b]) continue;
        if (w.band < 0 || ns[b] < ns[w.band] || (ns[b] == ns[w.band] && nu[b] > nu[w.band])) w.band = b;
    }
    for (int b = 0; b < 3; ++b)
        if (b != w.band && ns[b] == ns[w.band]) {
            w.tie_s = true;
            if (nu[b] == nu[w.band]) w.tie_u = true;
        }
    for (int r = 0; r < 3 && w.pos < 0; ++r)
        for (int c = 0; c < 9; ++c)
            if (in_s(w.band, 10 * r + c)) { w.pos = 10 * r + c; break; }
    return w;
}

// n random plane states: the lane pick (plane::pick_count) and the wave-wide
// solver's pick (wide::pick_count on the emulated wave) against the plain
// loop.  bad[0] / bad[1]: states on which the lane / the wide pick differs.
// seen[]: states 0 with a two-candidate cell, 1 with none but a
// three-candidate one, 2 with neither, 3 with a tie in the first key, 4 with
// a tie in both keys, 5 with a single undetermined cell.
extern "C" void pick_check(int64_t n, uint64_t seed, int64_t *bad, int64_t *seen)
{
    const wide::Lanes L = wide::lanes();
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); };
    bad[0] = bad[1] = 0;
    for (int k = 0; k < 6; ++k) seen[k] = 0;
    for (int64_t i = 0; i < n; ++i) {
        // the state cell by cell: a candidate set per cell, its size drawn by
        // the state's profile
        const int profile = (int)(rnd() % 8);
        const int p2 = (int)(rnd() % 40);  // per cent of two-candidate cells where the profile has them
        plane::Board B;
        uint32_t und[3] = {0, 0, 0};
        for (int d = 0; d < 9; ++d)
            for (int b = 0; b < 3; ++b) B.P[d][b] = 0;
        const int lone = (int)(rnd() % 81);
        for (int cell = 0; cell < 81; ++cell) {
            const int b = cell / 27, p = 10 * ((cell / 9) % 3) + cell % 9;
            int size;
            const int roll = (int)(rnd() % 100);
            switch (profile) {
            case 0: size = 1 + (int)(rnd() % 9); break;                                // anything
            case 1: size = roll < p2 ? 2 : roll < 70 ? 1 : 3 + (int)(rnd() % 3); break;  // mid-search: singles, pairs, a few more
            case 2: size = roll < 60 ? 1 : 3 + (int)(rnd() % 5); break;                // no pair
            case 3: size = roll < 60 ? 1 : 4 + (int)(rnd() % 6); break;                // no pair, no triple
            case 4: size = cell == lone ? 2 + (int)(rnd() % 4) : 1; break;             // one undetermined cell
            case 5: size = roll < 6 ? 2 : roll < 50 ? 1 : 3 + (int)(rnd() % 3); break;  // few pairs: ties in the first key
            case 6: size = roll < 3 ? 3 : roll < 50 ? 1 : 4 + (int)(rnd() % 3); break;  // few triples, no pair
            default: size = (cell % 27) % 13 == 0 ? 2 : (cell % 9 < 4 ? 1 : 4); break;  // the same pattern in every band
            }
            uint32_t set = 0;
            while (__builtin_popcount(set) < size) set |= 1u << (rnd() % 9);
            for (int d = 0; d < 9; ++d)
                if ((set >> d) & 1u) B.P[d][b] |= 1u << p;
            if (size >= 2) und[b] |= 1u << p;
        }
        // (the solvers call the pick with und = the cells of two or more
        // candidates; a cell of und dropped now and then must not matter)
        if (profile == 0 && (rnd() & 1)) und[rnd() % 3] &= rnd() | rnd();
        if (!(und[0] | und[1] | und[2])) continue;
        int level;
        const Want want = plain_pick(B, und, level);
        seen[level == 2 ? 0 : level == 3 ? 1 : 2]++;
        seen[3] += want.tie_s;
        seen[4] += want.tie_u;
        seen[5] += __builtin_popcount(und[0]) + __builtin_popcount(und[1]) + __builtin_popcount(und[2]) == 1;
        int band = -1, pos = -1;
        plane::pick_count(B, und, band, pos);
        bad[0] += band != want.band || pos != want.pos;
        const wide::V w = host::to_wave(B, L);
        wide::V u(0u);
        for (int l = 0; l < 48; ++l) u.x[l] = und[l >> 4];
        band = pos = -1;
        wide::pick_count(w, u, L, band, pos);
        bad[1] += band != want.band || pos != want.pos;
    }
}

// host_model.h's driver: the lane solver on plane::pass (ahead = 0) or on the
// look-ahead pass (1), handed to the wave-wide solver after `lane_guesses`
// guesses (0xFFFFFFFF: never).  Statuses as host::solve_batch.
extern "C" void pick_solve_batch(const uint8_t *in, uint8_t *out, int32_t *status, int64_t n, int node_order,
                                 uint32_t max_depth, uint32_t mrv_after, int ahead, uint32_t lane_guesses,
                                 uint64_t *guesses, uint64_t *passes_lane, uint64_t *passes_wide)
{
    host::Counts c;
    host::solve_batch(in, out, status, n, ahead != 0, lane_guesses, node_order, max_depth, mrv_after, c);
    *guesses = c.guesses;
    *passes_lane = c.passes_lane;
    *passes_wide = c.passes_wide;
}

// the look-ahead lane solver with the root rule, as the plane kernel's lane
// loop runs it: per board its passes and guesses
extern "C" void pick_lane_totals(const uint8_t *in, uint8_t *out, int32_t *status, int64_t n, int node_order,
                                 uint32_t max_depth, uint32_t mrv_after, uint64_t *guesses, uint64_t *passes,
                                 uint32_t *board_passes)
{
    host::Counts c;
    host::BoardInfo *info = new host::BoardInfo[n > 0 ? n : 1];
    host::solve_batch(in, out, status, n, true, host::LANE_ONLY, node_order, max_depth, mrv_after, c, true, info);
    for (int64_t i = 0; i < n; ++i) board_passes[i] = info[i].passes;
    delete[] info;
    *guesses = c.guesses;
    *passes = c.passes_lane;
}
