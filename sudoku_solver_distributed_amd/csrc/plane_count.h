// plane_count.h -- capped completion count of one board on digit planes.
//
//     count = min(limit, number of completions of the board that are valid
//                        Sudoku grids: every row, column and box holds 1..9
//                        once, the givens kept)
//
// Built from plane_solver.h's pieces, none of them changed: one look-ahead
// pass (plane::pass_ahead) per iteration, branching at a fixpoint on a
// fewest-candidates cell (plane::pick_mrv), digits ascending.  Rules A-D only
// remove candidates that no valid completion uses, and a SOLVED verdict is a
// grid in which every unit holds every digit, so on a board whose givens do
// not repeat a digit in a unit the count is exact: every completion is met
// once, in exactly one branch.  A board whose givens clash has no valid
// completion; load_words reports the clash and the caller answers 0 without a
// search (the solve kernels' walk never tests givens and may fill such a
// board: the count deliberately differs there).
//
// Stack depth.  A level is pushed only at a fixpoint with an undetermined
// cell left, and the push fixes one of them; und[] only shrinks along a
// branch and a level restores the und[] it was pushed with.  With L levels in
// use at least L cells of the 81 are fixed, so a push happens at depth <= 80:
// COUNT_MAX_DEPTH = 81 levels can never overflow.  count_step still tests the
// depth it is given: a push at depth == max_depth ends the board with C_FAULT
// (SDK_FAULT), never with a count.
//
// Plain C++ for host and device, like plane_solver.h: the CPU tests compile
// it with g++ (tests/native/count_host.cpp) against the oracle's counter.
#ifndef SDK_PLANE_COUNT_H
#define SDK_PLANE_COUNT_H

#include "plane_solver.h"

namespace plane {

enum { COUNT_MAX_DEPTH = 81, COUNT_FAULT = -3 /* SDK_FAULT */ };
enum { C_CONT = 0, C_DONE = 1, C_FAULT = 2 };

// The search step after a pass_ahead() whose verdict r is STUCK or DEAD (the
// driver turns SOLVED into DEAD once it has counted the completion; OPEN
// needs no step).  Stack: the look-ahead layout of WordStack -- push(level,
// B, und, entry), pop(level, B, und) -> entry, put_entry(level, e).
//   STUCK: branch on a fewest-candidates cell: the level keeps the planes,
//          und[] and the cell's other candidates; the lowest one is fixed.
//   DEAD:  back to the deepest level, which always has an untried digit: a
//          level whose LAST digit is taken is given up at once (the search
//          continues at its depth and the next push overwrites its line), so
//          no level below `depth` is ever exhausted and the scan down ends
//          at its first line.  No level left: the count is final (C_DONE).
// Returns C_CONT (pass again; nd[] = the one cell fixed), C_DONE, or C_FAULT
// (a push past max_depth, or a stack line that breaks the invariant above).
template <class Stack>
PS_FN int count_step(Board &B, uint32_t (&und)[3], uint32_t (&nd)[3], int r, uint32_t &depth, const Stack &stk,
                     uint32_t max_depth)
{
    int band = 0, pos = 0;
    uint32_t fix_d = 0;
    if (r == STUCK) {
        if (depth >= max_depth) return C_FAULT;
        pick_mrv(B, und, band, pos);
        const uint32_t cand = cell_cand(B, band, pos);  // >= 2 digits: rule A ran on these planes
        fix_d = cand & (0u - cand);
        stk.push(depth, B, und, make_entry(band, pos, cand ^ fix_d));
        depth++;
    } else {
        if (depth == 0) return C_DONE;
        const uint32_t level = depth - 1;
        const uint32_t e = stk.pop(level, B, und);
        const uint32_t rem = (e >> 8) & 0x1FFu;
        if (!rem) return C_FAULT;
        fix_d = rem & (0u - rem);
        if (rem == fix_d) depth = level;  // the level's last digit: its line is free again
        else stk.put_entry(level, e & ~(fix_d << 8));
        band = (int)((e >> 5) & 3u);
        pos = (int)(e & 31u);
    }
    set_cell(B, band, pos, fix_d);
    const uint32_t cb = 1u << pos;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        nd[b] = band == b ? cb : 0u;
        und[b] = andn(und[b], nd[b]);
    }
    return C_CONT;
}

// One iteration of the count on a board in flight: a pass, the completion
// counted (emit(B) on the first one, while the planes still hold it), then the
// step.  Returns true when the board is finished: found = its count, or
// COUNT_FAULT.  The GPU kernel's lane loop and the host driver both run this.
template <class Stack, class Emit>
PS_FN bool count_iter(Board &B, uint32_t (&und)[3], uint32_t (&nd)[3], uint32_t &depth, int32_t &found, int32_t limit,
                      const Stack &stk, uint32_t max_depth, Emit emit)
{
    int r = pass_ahead(B, und, nd);
    if (r == OPEN) return false;
    if (r == SOLVED) {
        if (found == 0) emit(B);
        if (++found >= limit) return true;
        r = DEAD;  // and look for another
    }
    const int s = count_step(B, und, nd, r, depth, stk, max_depth);
    if (s == C_CONT) return false;
    if (s == C_FAULT) found = COUNT_FAULT;
    return true;
}

struct CountStats {
    uint64_t passes;
    uint32_t max_depth;  // deepest stack depth reached (levels in use)
};

// Host / reference driver: count the completions of a loaded board whose
// givens are clean (given[] from load_words), to `limit`.  emit(B) receives
// the first completion.  Returns the count, or COUNT_FAULT.
template <typename Stack, class Emit>
PS_FN int32_t count_board(Board &B, const uint32_t (&given)[3], Stack &stk, int32_t limit, uint32_t max_depth,
                          Emit emit, CountStats &st)
{
    const WordStack<Stack> ws = {stk};
    uint32_t depth = 0, und[3], nd[3];
    int32_t found = 0;
    for (int b = 0; b < 3; ++b) {
        nd[b] = given[b];
        und[b] = andn(ROWS, given[b]);
    }
    for (;;) {
        const bool done = count_iter(B, und, nd, depth, found, limit, ws, max_depth, emit);
        st.passes++;
        if (depth > st.max_depth) st.max_depth = depth;
        if (done) return found;
    }
}

}  // namespace plane

#endif  // SDK_PLANE_COUNT_H
