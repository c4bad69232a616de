// pick_study.cpp -- which band should the completion count (search mode
// M_COUNT of plane_solver.h) branch in?  The lane solver on the host
// (host_model.h's driver, the look-ahead path) with the branch rule replaced
// through SDK_PLANE_COUNT_PICK, for scripts/pick_study.py.  Tooling only.
//
// Every rule takes S = e2 if any band has a two-candidate cell, else e3 if
// any has a three-candidate one, else und, and branches on the lowest cell of
// S in the band (and, rules 7 / 8, the row) it chooses:
//   0  the first band with a cell of S (plane::pick_mrv_masks, the rule before)
//   1  the band with the most cells of S
//   2  the band with the fewest undetermined cells
//   3  the band with the fewest cells of S
//   4  3, ties to the most undetermined cells (plane::pick_count_masks)
//   5  the band with the most undetermined cells
//   6  5, ties to the fewest cells of S
//   7  4, then the band's row with the fewest cells of S
//   8  3, then the band's row with the fewest cells of S
#include <stdint.h>

namespace plane {
static inline void study_pick(const uint32_t (&e2)[3], const uint32_t (&e3)[3], const uint32_t und[3], int &band,
                              int &pos);
}
#define SDK_PLANE_COUNT_PICK study_pick
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"

static int g_rule;

namespace plane {
static inline void study_pick(const uint32_t (&e2)[3], const uint32_t (&e3)[3], const uint32_t und[3], int &band,
                              int &pos)
{
    if (g_rule == 0) return pick_mrv_masks(e2, e3, und, band, pos);
    if (g_rule == 4) return pick_count_masks(e2, e3, und, band, pos);
    const uint32_t *s = (e2[0] | e2[1] | e2[2]) ? e2 : (e3[0] | e3[1] | e3[2]) ? e3 : und;
    long best = 0;
    band = -1;
    for (int b = 0; b < 3; ++b) {
        if (!s[b]) continue;
        const long n = __builtin_popcount(s[b]), u = __builtin_popcount(und[b]);
        long key;  // the smallest wins, the lowest band among equals
        switch (g_rule) {
        case 1: key = -n; break;
        case 2: key = u; break;
        case 3: case 8: key = n; break;
        case 5: key = -u; break;
        case 6: key = -u * 64 + n; break;
        default: key = n * 64 - u; break;  // 7 (and 4)
        }
        if (band < 0 || key < best) { band = b; best = key; }
    }
    uint32_t w = s[band];
    if (g_rule >= 7) {
        int row = -1, rn = 0;
        for (int k = 0; k < 3; ++k) {
            const int n = __builtin_popcount(w & (0x1FFu << (10 * k)));
            if (n && (row < 0 || n < rn)) { row = k; rn = n; }
        }
        w &= 0x1FFu << (10 * row);
    }
    pos = __builtin_ctz(w);
}
}  // namespace plane

// per board: passes and guesses (branch nodes) of the lane solver under
// `rule`; root_full: with the root rule, as the plane kernel runs it.
// Returns the boards whose answer or status differs from rule 0's (ref_out /
// ref_status, filled by the call with rule 0).
extern "C" int64_t pick_study(const uint8_t *in, int64_t n, int rule, int node_order, uint32_t max_depth,
                              uint32_t mrv_after, int root_full, uint32_t *passes, uint64_t *guesses,
                              uint8_t *ref_out, int32_t *ref_status)
{
    g_rule = rule;
    int64_t differ = 0;
    uint64_t g = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint8_t out[81];
        int32_t st;
        host::Counts c;
        host::BoardInfo info;
        host::solve_batch(in + i * 81, out, &st, 1, true, host::LANE_ONLY, node_order, max_depth, mrv_after, c,
                          root_full != 0, &info);
        passes[i] = info.passes;
        g += c.guesses;
        if (rule == 0) {
            memcpy(ref_out + i * 81, out, 81);
            ref_status[i] = st;
        } else {
            differ += st != ref_status[i] || memcmp(out, ref_out + i * 81, 81) != 0;
        }
    }
    *guesses = g;
    return differ;
}
