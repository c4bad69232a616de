// plane_cand.h -- the exact candidates of one board on digit planes:
//
//     marks[c] bit d-1  <=>  some completion of the board that is a valid
//                            Sudoku grid (every row, column and box holds 1..9
//                            once, the givens kept) puts digit d into cell c
//
// and count = min(2, completions): 0 when all marks are zero, 1 when every
// cell has one bit, 2 otherwise.  Built from plane_count.h's pieces, none of
// them changed: the count's loop (plane::pass_ahead, plane::count_step), run
// in two phases over three sets of 27 plane words -- B, the search's planes;
// R, the closed root; W, the witnessed candidates.
//
// Sweep.  The count's search from the givens.  Every SOLVED state is OR-ed
// into W (one completion witnesses 81 candidates at once).  The first STUCK
// verdict is at depth 0 (levels are pushed at STUCK verdicts only): its planes
// are the root's closure under rules A-D and are kept as R with their und[].
// The sweep ends when the search is exhausted (C_DONE: W holds every
// completion, so W is the answer; this is every board with fewer than `sweep`
// completions) or at `sweep` completions.
//
// Targeted searches.  While R & ~W has a bit (cell, d): B = R with the cell
// fixed to d, depth 0, and the same loop to its first SOLVED state (OR-ed into
// W) or to C_DONE (no completion holds d there: the bit leaves R).  At most
// 648 searches, each no harder than a solve; at the end R == W.
//
// Exactness.  (1) Every bit of W comes from a SOLVED state: a grid in which
// every unit holds every digit, reached from the givens by fixing cells, so a
// valid completion that keeps the givens.  (2) Rules A-D only remove
// candidates that no valid completion uses, so R as saved holds every true
// candidate, and a bit leaves R only after an exhaustive search of the root
// with that cell fixed found no completion: R always holds every true
// candidate.  (3) The loop ends only when R & ~W is empty; with (1), W is a
// subset of the true candidates, with (2) those are a subset of R, so R == W
// == the answer.  Nothing depends on `sweep`, on which bit of R & ~W is taken
// (SDK_CAND_DESCEND, test builds only: the highest instead of the lowest) or
// on the branching order.  A targeted search starts only after a completion
// was met, so every determined cell of R is witnessed already and a target is
// always an undetermined cell of R; und_R without it is what pass_ahead takes
// (a cell that a refutation left with one candidate is still listed in und_R:
// pass_ahead's closing rule A finds it, as it finds every new single).
//
// The two lines.  R and W live in the lane's stack lines, levels
// COUNT_MAX_DEPTH and COUNT_MAX_DEPTH + 1, written and read through the same
// stack interface as the search's levels (push / pop with und[]; W's und[] and
// both entries are unused).  W's line is first written at the first
// completion: a board that ends without one has all marks zero.
//
// Stack depth: the count's argument (plane_count.h).  A targeted search
// starts with one more cell fixed than the sweep, so COUNT_MAX_DEPTH levels
// hold it too; a push past max_depth still ends the board with K_FAULT
// (SDK_FAULT in the count, zero marks), never with marks.
//
// Plain C++ for host and device: the CPU tests compile it with g++
// (tests/native/cand_host.cpp) against the oracle's counter asked once per
// cell and digit.
#ifndef SDK_PLANE_CAND_H
#define SDK_PLANE_CAND_H

#include "plane_count.h"

// completions after which the sweep hands over to the targeted searches
// (results never depend on it)
#ifndef SDK_CAND_SWEEP
#define SDK_CAND_SWEEP 2
#endif
// 1: the highest bit of the last non-zero word of R & ~W is the next target
// instead of the lowest bit of the first (test builds: same marks)
#ifndef SDK_CAND_DESCEND
#define SDK_CAND_DESCEND 0
#endif
static_assert(SDK_CAND_SWEEP >= 1 && SDK_CAND_SWEEP <= 32767, "SDK_CAND_SWEEP");

namespace plane {

enum {
    CAND_ROOT_LEVEL = COUNT_MAX_DEPTH,     // R and its und[]
    CAND_WIT_LEVEL = COUNT_MAX_DEPTH + 1,  // W
    CAND_LEVELS = COUNT_MAX_DEPTH + 2,     // lines of a lane
};
enum { K_CONT = 0, K_DONE = 1, K_FAULT = 2 };
// a board's mode word: bits 0-4 pos, 5-6 band, 8-11 digit of the targeted
// search's candidate; the phase; R saved; W written; the sweep's completions
enum : uint32_t { CM_TARGET_BITS = 0xFFFu, CM_TARGET = 1u << 12, CM_ROOT = 1u << 13, CM_WIT = 1u << 14, CM_FOUND_SHIFT = 16 };

// A fixed line's level as a value made where it is used: as a constant, the
// line's offset (lane offset + 128 level) is loop-invariant and the kernel
// would keep one register per line alive across its whole loop.
PS_FN uint32_t cand_level(uint32_t level)
{
    PS_PIN(level);
    return level;
}

// One iteration on a board in flight: a pass, then the step or the change of
// phase.  mode starts at 0.  Returns K_CONT, K_DONE (the answer is W: the line
// CAND_WIT_LEVEL if mode has CM_WIT, else all zero) or K_FAULT.  The GPU
// kernel's lane loop and the host driver both run this.
template <class Stack>
PS_FN int cand_iter(Board &B, uint32_t (&und)[3], uint32_t (&nd)[3], uint32_t &depth, uint32_t &mode, const Stack &stk,
                    uint32_t max_depth, uint32_t sweep)
{
    int r = pass_ahead(B, und, nd);
    if (r == OPEN) return K_CONT;
    bool pick = false, refuted = false;
    if (r == SOLVED) {
        // W |= the completion (B is dead from here: the step below replaces it)
        if (mode & CM_WIT) {
            Board T;
            uint32_t tu[3];
            stk.pop(cand_level(CAND_WIT_LEVEL), T, tu);
#pragma unroll
            for (int d = 0; d < 9; ++d)
#pragma unroll
                for (int b = 0; b < 3; ++b) B.P[d][b] |= T.P[d][b];
        }
        stk.push(cand_level(CAND_WIT_LEVEL), B, und, 0u);
        mode |= CM_WIT;
        if (mode & CM_TARGET) {
            pick = true;  // the target is witnessed
        } else {
            mode += 1u << CM_FOUND_SHIFT;
            if ((mode >> CM_FOUND_SHIFT) >= sweep) {
                // solved with no STUCK verdict before: the closure itself is the one completion
                if (!(mode & CM_ROOT)) return K_DONE;
                pick = true;
            } else {
                r = DEAD;  // and look for another
            }
        }
    }
    if (!pick) {
        if (r == STUCK && !(mode & CM_ROOT)) {  // the sweep's first fixpoint: depth 0, the closed root
            stk.push(cand_level(CAND_ROOT_LEVEL), B, und, 0u);
            mode |= CM_ROOT;
        }
        const int s = count_step(B, und, nd, r, depth, stk, max_depth);
        if (s == C_CONT) return K_CONT;
        if (s == C_FAULT) return K_FAULT;
        if (!(mode & CM_TARGET)) return K_DONE;  // the sweep met every completion
        refuted = true;                          // no completion holds the target
    }
    // the next target: a bit of R & ~W
    stk.pop(cand_level(CAND_ROOT_LEVEL), B, und);
    if (refuted) {
        const uint32_t td = (mode >> 8) & 15u, tb = (mode >> 5) & 3u, cb = 1u << (mode & 31u);
#pragma unroll
        for (int d = 0; d < 9; ++d)
#pragma unroll
            for (int b = 0; b < 3; ++b) B.P[d][b] = andn(B.P[d][b], (td == (uint32_t)d && tb == (uint32_t)b) ? cb : 0u);
        stk.push(cand_level(CAND_ROOT_LEVEL), B, und, 0u);
    }
    uint32_t x = 0, idx = 0;
    {
        Board T;
        uint32_t tu[3];
        stk.pop(cand_level(CAND_WIT_LEVEL), T, tu);
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const int w = SDK_CAND_DESCEND ? k : 26 - k;  // the last word that overwrites wins
            const uint32_t y = andn(B.P[w / 3][w % 3], T.P[w / 3][w % 3]);
            x = y ? y : x;
            idx = y ? (uint32_t)w : idx;
        }
    }
    if (!x) return K_DONE;  // R == W
    const int pos = SDK_CAND_DESCEND ? 31 - __builtin_clz(x) : __builtin_ctz(x);
    const uint32_t d = idx / 3u;
    const int band = (int)(idx - 3u * d);
    set_cell(B, band, pos, 1u << d);
    const uint32_t cb = 1u << pos;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        nd[b] = band == b ? cb : 0u;
        und[b] = andn(und[b], nd[b]);
    }
    depth = 0;
    mode = (mode & ~CM_TARGET_BITS) | CM_TARGET | (uint32_t)pos | ((uint32_t)band << 5) | (d << 8);
    return K_CONT;
}

// The marks of the planes W (bit d-1 of put(cell, marks) for digit d) and the
// count they imply.
template <class Put>
PS_FN int32_t cand_marks(const Board &W, Put put)
{
    uint32_t any = 0, multi = 0;
#pragma unroll
    for (int i = 0; i < 81; ++i) {
        // cell_cand at a fixed (band, pos): the cell's bit of the digit's one
        // word, shifts by constants only (cell_cand's band masks would be 27
        // constants held in registers across the kernel's loop)
        const int b = cell_band(i), p = cell_pos(i);
        uint32_t m = 0;
#pragma unroll
        for (int d = 8; d >= 0; --d) m = m + m + ((W.P[d][b] >> p) & 1u);
        any |= m;
        multi |= m & (m - 1u);
        put(i, m);
    }
    return any ? (multi ? 2 : 1) : 0;
}

struct CandStats {
    uint64_t passes;
    uint32_t max_depth;  // deepest stack depth reached (levels in use)
    uint32_t searches;   // targeted searches started
};

// Host / reference driver: the marks of a loaded board whose givens are clean
// (given[] from load_words) through put(cell, marks).  The stack holds
// CAND_LEVELS lines.  Returns the count, or COUNT_FAULT (put gets zeros).
template <typename Stack, class Put>
PS_FN int32_t cand_board(Board &B, const uint32_t (&given)[3], Stack &stk, uint32_t max_depth, uint32_t sweep, Put put,
                         CandStats &st)
{
    const WordStack<Stack> ws = {stk};
    uint32_t depth = 0, mode = 0, und[3], nd[3];
    for (int b = 0; b < 3; ++b) {
        nd[b] = given[b];
        und[b] = andn(ROWS, given[b]);
    }
    for (;;) {
        const uint32_t before = mode & (CM_TARGET | CM_TARGET_BITS);
        const int k = cand_iter(B, und, nd, depth, mode, ws, max_depth, sweep);
        st.passes++;
        if (depth > st.max_depth) st.max_depth = depth;
        if (k == K_CONT) {
            if ((mode & (CM_TARGET | CM_TARGET_BITS)) != before) st.searches++;
            continue;
        }
        Board W;
        uint32_t tu[3];
        if (k == K_DONE && (mode & CM_WIT)) {
            ws.pop(cand_level(CAND_WIT_LEVEL), W, tu);
        } else {
            for (int d = 0; d < 9; ++d)
                for (int b = 0; b < 3; ++b) W.P[d][b] = 0u;
        }
        const int32_t c = cand_marks(W, put);
        return k == K_FAULT ? (int32_t)COUNT_FAULT : c;
    }
}

}  // namespace plane

#endif  // SDK_PLANE_CAND_H
