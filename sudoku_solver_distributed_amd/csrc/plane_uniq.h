// plane_uniq.h -- the unique candidates of one board on digit planes:
//
//     marks[c] bit d-1  <=>  at least one completion of the board (a valid
//                            Sudoku grid that keeps the givens) puts d into c
//     once[c]  bit d-1  <=>  EXACTLY one completion puts d into c
//
// and count = min(2, completions), as plane_cand.h.  marks is plane_cand.h's
// answer; for an empty cell, once says that the board with that clue added is
// a proper puzzle.  Built from plane_count.h's pieces, none of them changed:
// the count's loop (plane::pass_ahead, plane::count_step), run in two phases
// over B, the search's planes, and five sets of 27 plane words kept in the
// lane's stack lines:
//     R  the closed root, a superset of the true candidates
//     W  witnessed at least once (the sweep only)
//     V  witnessed by two DISTINCT completions
//     U  the bits of R still open: in R, not in V, not yet settled
//     T  the first completion of a targeted search (shares W's line)
// The bits settled as "exactly one" are X = R & ~V & ~U; they need no line.
//
// Sweep.  The count's search from the givens.  The first STUCK verdict is at
// depth 0: its planes are the root's closure under rules A-D, kept as R with
// their und[].  Every SOLVED state S does V |= W & S, then W |= S.  The
// leaves of one depth-first search are distinct completions (each is met
// once, in exactly one branch: plane_count.h), so a bit enters V exactly when
// a second completion of the sweep holds it.  If the search is exhausted
// (C_DONE) before SDK_UNIQ_SWEEP completions, W holds every completion and V
// every placement two of them share: marks = W, once = W & ~V.  Otherwise, at
// the SDK_UNIQ_SWEEP-th completion, U = R & ~V and the targeted searches begin.
//
// Targeted searches.  While U has a bit (cell, d): B = R with the cell fixed
// to d, depth 0, and the count's loop to two completions:
//   - exhausted with none:  no completion holds d there; the bit leaves R and U;
//   - exhausted after one:  exactly one completion holds d there; the bit
//     leaves U and stays in R & ~V (settled);
//   - two, T1 then T2:      two leaves of one search, so distinct: V |= T1 & T2
//     and U &= ~(T1 & T2).  Both hold d at the cell, so the target itself goes.
// Every search removes its target from U, so there are at most 729 of them.
// At the end marks = R and once = R & ~V.
// V |= W & S is NOT sound inside a targeted search: S may be the very
// completion that put the bit into W (an earlier search, or the sweep, may
// have met the same grid), so the two witnesses need not be distinct.  Only
// two leaves of ONE search are known to differ; W is not used after the sweep.
//
// Exactness.  (1) R holds every true candidate: rules A-D only remove
// candidates that no valid completion uses, and a bit leaves R only after an
// exhaustive search of the root with that cell fixed found no completion.
// (2) V only ever receives placements shared by two distinct completions, so
// V is a subset of "at least two".  (3) A bit is settled (leaves U while
// staying in R & ~V) only after an exhaustive search with it fixed met exactly
// one completion; no later step can put it into V, by (2).  (4) The loop ends
// only when U is empty: every bit of R is then in V (at least two), settled
// (exactly one), and the bits refuted are gone, so R is exactly the true
// candidates (each remaining bit has a witness) and R & ~V exactly "one".
// Nothing depends on SDK_UNIQ_SWEEP, on which bit of U is taken
// (SDK_UNIQ_DESCEND, test builds only) or on the branching order.
//
// Targets are undetermined cells of R.  With SDK_UNIQ_SWEEP >= 2 (asserted
// below) two distinct completions are met before the first targeted search;
// a cell that R determines holds its digit in both, so the bit is in V and
// never in U.  A cell that refutations left with one candidate is still
// listed in und_R: pass_ahead's closing rule A finds it, as in plane_cand.h.
// Two completions also mean a branch, so R was saved before the sweep ends.
//
// The lines.  R (with its und[]), V, U and W / T are the lane's stack lines
// at levels COUNT_MAX_DEPTH .. COUNT_MAX_DEPTH + 3, written and read through
// the search's own stack interface (the other lines' und[] and every entry
// are unused).  They are never held in registers across a pass: plane_cand.h
// and DESIGN.md §15 say why.  W and V are first written at the sweep's first
// completion: a board that ends without one has all bits zero.  When a board
// finishes, once = marks & ~V is written into U's line, which is spent by
// then: the caller converts one line at a time (uniq_kernels.hip says why).
//
// Stack depth: the count's argument (plane_count.h).  A push past max_depth
// ends the board with K_FAULT (SDK_FAULT, zero arrays), never with an answer.
//
// Plain C++ for host and device: the CPU tests compile it with g++
// (tests/native/uniq_host.cpp) against the oracle's counter asked once per
// cell and digit.
#ifndef SDK_PLANE_UNIQ_H
#define SDK_PLANE_UNIQ_H

#include "plane_cand.h"

// completions after which the sweep hands over to the targeted searches
// (results never depend on it; DESIGN.md §18 has the table behind the value)
#ifndef SDK_UNIQ_SWEEP
#define SDK_UNIQ_SWEEP 16
#endif
// 1: the highest bit of the last non-zero word of U is the next target
// instead of the lowest bit of the first (test builds: same answers)
#ifndef SDK_UNIQ_DESCEND
#define SDK_UNIQ_DESCEND 0
#endif
// >= 2: a target is always an undetermined cell of R (above)
static_assert(SDK_UNIQ_SWEEP >= 2 && SDK_UNIQ_SWEEP <= 32767, "SDK_UNIQ_SWEEP");

namespace plane {

enum {
    UNIQ_ROOT_LEVEL = COUNT_MAX_DEPTH,      // R and its und[]
    UNIQ_TWO_LEVEL = COUNT_MAX_DEPTH + 1,   // V
    UNIQ_OPEN_LEVEL = COUNT_MAX_DEPTH + 2,  // U
    UNIQ_WIT_LEVEL = COUNT_MAX_DEPTH + 3,   // W in the sweep, T in a targeted search
    UNIQ_LEVELS = COUNT_MAX_DEPTH + 4,      // lines of a lane
};
// a board's mode word: bits 0-4 pos, 5-6 band, 8-11 digit of the targeted
// search's candidate; the phase; R saved; W and V written; T written (the
// targeted search has met one completion); the sweep's completions
enum : uint32_t {
    UM_TARGET_BITS = 0xFFFu,
    UM_TARGET = 1u << 12,
    UM_ROOT = 1u << 13,
    UM_WIT = 1u << 14,
    UM_FIRST = 1u << 15,
    UM_FOUND_SHIFT = 16,
};

// One iteration on a board in flight: a pass, then the step or the change of
// phase.  mode starts at 0.  Returns K_CONT, K_DONE or K_FAULT.  At K_DONE
// marks is the line UNIQ_ROOT_LEVEL if mode has UM_TARGET, else UNIQ_WIT_LEVEL
// if it has UM_WIT, and once = marks & ~V has been written into U's line,
// UNIQ_OPEN_LEVEL (U is spent by then), so that the caller converts one line
// at a time; with neither flag both answers are all zero.  The count is
// uniq_count(mode).  The GPU kernel's lane loop and the host driver both run
// this.
template <class Stack>
PS_FN int uniq_iter(Board &B, uint32_t (&und)[3], uint32_t (&nd)[3], uint32_t &depth, uint32_t &mode, const Stack &stk,
                    uint32_t max_depth, uint32_t sweep)
{
    int r = pass_ahead(B, und, nd);
    if (r == OPEN) return K_CONT;
    Board T;  // the bits that leave U
    uint32_t tu[3];
    bool pick = false;
    // the answer's second line: once = marks & ~V
    auto finish = [&](uint32_t level) {
        stk.pop(cand_level(level), B, tu);
        stk.pop(cand_level(UNIQ_TWO_LEVEL), T, tu);
#pragma unroll
        for (int d = 0; d < 9; ++d)
#pragma unroll
            for (int b = 0; b < 3; ++b) B.P[d][b] = andn(B.P[d][b], T.P[d][b]);
        stk.push(cand_level(UNIQ_OPEN_LEVEL), B, tu, 0u);
    };
    if (r == SOLVED) {
        // (B is dead from here: the step or the pick below replaces it)
        if (!(mode & UM_TARGET)) {
            if (mode & UM_WIT) {
                // V |= W & S; W |= S
                stk.pop(cand_level(UNIQ_WIT_LEVEL), T, tu);
#pragma unroll
                for (int d = 0; d < 9; ++d)
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        const uint32_t s = B.P[d][b], w = T.P[d][b];
                        B.P[d][b] = s | w;
                        T.P[d][b] = s & w;
                    }
                stk.push(cand_level(UNIQ_WIT_LEVEL), B, und, 0u);
                stk.pop(cand_level(UNIQ_TWO_LEVEL), B, tu);
#pragma unroll
                for (int d = 0; d < 9; ++d)
#pragma unroll
                    for (int b = 0; b < 3; ++b) B.P[d][b] |= T.P[d][b];
            } else {
                stk.push(cand_level(UNIQ_WIT_LEVEL), B, und, 0u);
#pragma unroll
                for (int d = 0; d < 9; ++d)
#pragma unroll
                    for (int b = 0; b < 3; ++b) B.P[d][b] = 0u;
                mode |= UM_WIT;
            }
            stk.push(cand_level(UNIQ_TWO_LEVEL), B, und, 0u);
            mode += 1u << UM_FOUND_SHIFT;
            if ((mode >> UM_FOUND_SHIFT) >= sweep) {
                // U = R & ~V: R's copy goes into U's line, V leaves it below
                // (sweep >= 2: a branch was taken, so R is saved)
#pragma unroll
                for (int d = 0; d < 9; ++d)
#pragma unroll
                    for (int b = 0; b < 3; ++b) T.P[d][b] = B.P[d][b];
                stk.pop(cand_level(UNIQ_ROOT_LEVEL), B, tu);
                stk.push(cand_level(UNIQ_OPEN_LEVEL), B, tu, 0u);
                mode |= UM_TARGET;
                pick = true;
            } else {
                r = DEAD;  // and look for another
            }
        } else if (!(mode & UM_FIRST)) {
            stk.push(cand_level(UNIQ_WIT_LEVEL), B, und, 0u);  // T1
            mode |= UM_FIRST;
            r = DEAD;  // and look for a second
        } else {
            // two distinct completions hold the target: V |= T1 & T2
            stk.pop(cand_level(UNIQ_WIT_LEVEL), T, tu);
#pragma unroll
            for (int d = 0; d < 9; ++d)
#pragma unroll
                for (int b = 0; b < 3; ++b) T.P[d][b] &= B.P[d][b];
            stk.pop(cand_level(UNIQ_TWO_LEVEL), B, tu);
#pragma unroll
            for (int d = 0; d < 9; ++d)
#pragma unroll
                for (int b = 0; b < 3; ++b) B.P[d][b] |= T.P[d][b];
            stk.push(cand_level(UNIQ_TWO_LEVEL), B, tu, 0u);
            pick = true;
        }
    }
    if (!pick) {
        if (r == STUCK && !(mode & UM_ROOT)) {  // the sweep's first fixpoint: depth 0, the closed root
            stk.push(cand_level(UNIQ_ROOT_LEVEL), B, und, 0u);
            mode |= UM_ROOT;
        }
        const int s = count_step(B, und, nd, r, depth, stk, max_depth);
        if (s == C_CONT) return K_CONT;
        if (s == C_FAULT) return K_FAULT;
        if (!(mode & UM_TARGET)) {  // the sweep met every completion
            if (mode & UM_WIT) finish(UNIQ_WIT_LEVEL);
            return K_DONE;
        }
        // the targeted search is exhausted: its bit leaves U, and R too if no
        // completion held it
        const uint32_t td = (mode >> 8) & 15u, tb = (mode >> 5) & 3u, cb = 1u << (mode & 31u);
#pragma unroll
        for (int d = 0; d < 9; ++d)
#pragma unroll
            for (int b = 0; b < 3; ++b) T.P[d][b] = (td == (uint32_t)d && tb == (uint32_t)b) ? cb : 0u;
        if (!(mode & UM_FIRST)) {
            stk.pop(cand_level(UNIQ_ROOT_LEVEL), B, tu);
#pragma unroll
            for (int d = 0; d < 9; ++d)
#pragma unroll
                for (int b = 0; b < 3; ++b) B.P[d][b] = andn(B.P[d][b], T.P[d][b]);
            stk.push(cand_level(UNIQ_ROOT_LEVEL), B, tu, 0u);
        }
    }
    // U &= ~T, and the next target: a bit of U
    uint32_t x = 0, idx = 0;
    stk.pop(cand_level(UNIQ_OPEN_LEVEL), B, tu);
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        const int w = SDK_UNIQ_DESCEND ? k : 26 - k;  // the last word that overwrites wins
        const uint32_t y = andn(B.P[w / 3][w % 3], T.P[w / 3][w % 3]);
        B.P[w / 3][w % 3] = y;
        x = y ? y : x;
        idx = y ? (uint32_t)w : idx;
    }
    if (!x) {  // every bit of R is in V or settled
        finish(UNIQ_ROOT_LEVEL);
        return K_DONE;
    }
    stk.push(cand_level(UNIQ_OPEN_LEVEL), B, tu, 0u);
    stk.pop(cand_level(UNIQ_ROOT_LEVEL), B, und);
    const int pos = SDK_UNIQ_DESCEND ? 31 - __builtin_clz(x) : __builtin_ctz(x);
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
    mode = (mode & ~(UM_TARGET_BITS | UM_FIRST)) | UM_TARGET | (uint32_t)pos | ((uint32_t)band << 5) | (d << 8);
    return K_CONT;
}

// The count of a board that ended with K_DONE, from its mode word: the
// sweep's completions if it met them all, else two or more.
PS_FN int32_t uniq_count(uint32_t mode)
{
    const uint32_t found = mode >> UM_FOUND_SHIFT;
    return (mode & UM_TARGET) || found >= 2u ? 2 : (int32_t)found;
}

struct UniqStats {
    uint64_t passes;        // all iterations
    uint64_t sweep_passes;  // ... of them in the sweep
    uint32_t max_depth;     // deepest stack depth reached (levels in use)
    uint32_t searches;      // targeted searches started
};

// Host / reference driver: the answer of a loaded board whose givens are
// clean (given[] from load_words) through put_marks(cell, marks) and
// put_once(cell, once).  The stack holds UNIQ_LEVELS lines.  Returns the
// count, or COUNT_FAULT (both get zeros).
template <typename Stack, class PutM, class PutO>
PS_FN int32_t uniq_board(Board &B, const uint32_t (&given)[3], Stack &stk, uint32_t max_depth, uint32_t sweep,
                         PutM put_marks, PutO put_once, UniqStats &st)
{
    const WordStack<Stack> ws = {stk};
    uint32_t depth = 0, mode = 0, und[3], nd[3];
    for (int b = 0; b < 3; ++b) {
        nd[b] = given[b];
        und[b] = andn(ROWS, given[b]);
    }
    for (;;) {
        const uint32_t before = mode & (UM_TARGET | UM_TARGET_BITS);
        const int k = uniq_iter(B, und, nd, depth, mode, ws, max_depth, sweep);
        st.passes++;
        if (!(before & UM_TARGET)) st.sweep_passes++;
        if (depth > st.max_depth) st.max_depth = depth;
        if (k == K_CONT) {
            if ((mode & (UM_TARGET | UM_TARGET_BITS)) != before) st.searches++;
            continue;
        }
        Board M;
        uint32_t tu[3];
        const bool answer = k == K_DONE && (mode & (UM_TARGET | UM_WIT));
        for (int half = 0; half < 2; ++half) {
            if (answer) {
                ws.pop(cand_level(half ? UNIQ_OPEN_LEVEL : (mode & UM_TARGET) ? UNIQ_ROOT_LEVEL : UNIQ_WIT_LEVEL), M, tu);
            } else {
                for (int d = 0; d < 9; ++d)
                    for (int b = 0; b < 3; ++b) M.P[d][b] = 0u;
            }
            if (half) cand_marks(M, put_once);
            else cand_marks(M, put_marks);
        }
        const int32_t c = answer ? uniq_count(mode) : 0;
        return k == K_FAULT ? (int32_t)COUNT_FAULT : c;
    }
}

}  // namespace plane

#endif  // SDK_PLANE_UNIQ_H
