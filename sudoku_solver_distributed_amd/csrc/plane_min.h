// plane_min.h -- redundant givens of one board on digit planes: a puzzle with
// exactly one completion S is minimised (greedy: givens are erased turn by
// turn while the puzzle keeps its one completion) or probed (every given is
// tested alone against the input board).  Built from plane_count.h's pieces,
// none of them changed: the count's loop (plane::pass_ahead,
// plane::count_step), run in two phases.
//
// Phase 0.  The count's search from the givens to two completions.  It ends
// the board with status 0 (none) or 2 (several), or hands a board with
// exactly one completion to phase 1.  On a full grid it is one pass.
//
// Phase 1, turn by turn.  The current puzzle P's LOADED planes -- a given is
// its one bit, an empty cell all nine (plane::planes_from_slices) -- are kept
// in one extra stack line, level MIN_ROOT_LEVEL, whose und[] slot carries the
// mask of P's givens.  A turn takes the next cell c that is a given of P,
// digit s.  The search root is rebuilt from the line: cell c opened to all
// digits but s, und[] / nd[] as after a load (every other given still to be
// removed from its peers, c undetermined), depth 0.  The shared loop then runs
// to its first SOLVED verdict (the given is needed) or to C_DONE (redundant).
// In greedy mode a redundant given leaves P: in the saved line the cell is set
// to all nine digits and its bit leaves the given mask.
//
// Exactness.  P has exactly one completion S, and s = S[c].  The completions
// of P without c are S and the completions of P without c that put another
// digit into c, which are exactly what the test searches: rules A-D only
// remove candidates that no valid completion uses and a SOLVED verdict is a
// valid grid that keeps the test root's givens, so the test meets such a
// completion if and only if one exists.  Exhausted: P without c still has the
// one completion S, and greedy goes on with it.  A completion met: P without c
// has two, c stays, and it stays needed under further removals, since those
// only add completions -- one pass over the turns suffices.  S is never
// searched for again and is stored nowhere: the digit under test is the given
// itself.  Probe mode never changes the saved line, so every test is against
// the input board.
//
// Stack depth: the count's argument (plane_count.h).  A level is pushed only
// at a fixpoint with an undetermined cell left and fixes one of them, so with
// L levels in use L cells are fixed and a push happens at depth <= 80, whatever
// the givens are: COUNT_MAX_DEPTH levels hold every test.  A push at max_depth
// still ends the board with N_FAULT (SDK_FAULT, the input board back), never
// with a partial result.
//
// Plain C++ for host and device: the CPU tests compile it with g++
// (tests/native/min_host.cpp) against the definition written as the plain loop
// over the oracle's counter.
#ifndef SDK_PLANE_MIN_H
#define SDK_PLANE_MIN_H

#include "plane_count.h"

namespace plane {

enum {
    MIN_ROOT_LEVEL = COUNT_MAX_DEPTH,  // P's loaded planes; und[] = P's givens
    MIN_LEVELS = COUNT_MAX_DEPTH + 1,  // lines of a lane
};
enum { N_CONT = 0, N_DONE = 1, N_FAULT = 2 };
// a board's mode word: bits 0-6 the cell under test, 7-13 the next turn,
// 14-20 the givens removed, 21-22 phase 0's completions; bit 23: phase 1
enum : uint32_t {
    MN_CELL = 0x7Fu,
    MN_TURN_SHIFT = 7,
    MN_TURN = 0x7Fu << MN_TURN_SHIFT,
    MN_REMOVED_SHIFT = 14,
    MN_FOUND_SHIFT = 21,
    MN_TEST = 1u << 23,
};

// The saved line's level as a value made where it is used (plane_cand.h's
// cand_level: as a constant, the line's offset would be kept in a register
// across the kernel's whole loop).
PS_FN uint32_t min_root_level()
{
    uint32_t level = MIN_ROOT_LEVEL;
    PS_PIN(level);
    return level;
}

// what a finished board's mode word says: min(2, completions) and the givens removed
PS_FN int32_t min_status(uint32_t mode) { return (mode & MN_TEST) ? 1 : (int32_t)((mode >> MN_FOUND_SHIFT) & 3u); }
PS_FN uint32_t min_removed(uint32_t mode) { return (mode & MN_TEST) ? (mode >> MN_REMOVED_SHIFT) & 0x7Fu : 0u; }

// A loaded board (clean givens, given[] from load_words) set up for its first
// iteration: the loaded planes saved as P's line, und / nd as after a load.
template <class Stack>
PS_FN void min_start(Board &B, const uint32_t (&given)[3], uint32_t (&und)[3], uint32_t (&nd)[3], uint32_t &depth,
                     uint32_t &mode, const Stack &stk)
{
    stk.push(min_root_level(), B, given, 0u);
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        nd[b] = given[b];
        und[b] = andn(ROWS, given[b]);
    }
    depth = 0;
    mode = 0;
}

// One iteration on a board in flight: a pass, then the step, the change of
// phase or the next turn.  io: order(t) -> the cell of turn t (a value above
// 80 skips the turn), digit(c) -> P[c], erase(c): P[c] = 0 -- the caller's
// working copy of the board, which ends as the answer.  probe: every given
// against the input board (io.order(t) must be t; max_empty is not read).
// Returns N_CONT, N_DONE (min_status / min_removed of mode) or N_FAULT (the
// caller puts the input board back).  The GPU kernel's lane loop and the host
// driver both run this.
template <class Stack, class Io>
PS_FN int min_iter(Board &B, uint32_t (&und)[3], uint32_t (&nd)[3], uint32_t &depth, uint32_t &mode, const Stack &stk,
                   uint32_t max_depth, bool probe, uint32_t max_empty, const Io &io)
{
    int r = pass_ahead(B, und, nd);
    if (r == OPEN) return N_CONT;
    const bool test = (mode & MN_TEST) != 0;
    bool needed = false, refuted = false;
    if (r == SOLVED) {
        if (test) {
            needed = true;  // a completion with another digit in the cell
        } else {
            mode += 1u << MN_FOUND_SHIFT;
            if (((mode >> MN_FOUND_SHIFT) & 3u) >= 2u) return N_DONE;
            r = DEAD;  // and look for another
        }
    }
    if (!needed) {
        const int s = count_step(B, und, nd, r, depth, stk, max_depth);
        if (s == C_CONT) return N_CONT;
        if (s == C_FAULT) return N_FAULT;
        if (test) {
            refuted = true;  // no completion holds another digit there
        } else {
            if (!((mode >> MN_FOUND_SHIFT) & 3u)) return N_DONE;  // no completion
            mode |= MN_TEST;                                       // exactly one: turn 0 is next
        }
    }
    // the next turn, from P's line
    uint32_t gm[3];
    stk.pop(min_root_level(), B, gm);
    if (refuted) {
        const uint32_t c = mode & MN_CELL;
        io.erase(c);
        mode += 1u << MN_REMOVED_SHIFT;
        if (!probe) {
            const uint32_t band = c / 27u, q = c - 27u * band, cb = 1u << (q + q / 9u);
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const uint32_t m = band == (uint32_t)b ? cb : 0u;
                gm[b] = andn(gm[b], m);
#pragma unroll
                for (int d = 0; d < 9; ++d) B.P[d][b] |= m;  // an empty cell: all nine
            }
            stk.push(min_root_level(), B, gm, 0u);
        }
    }
    uint32_t turn = (mode >> MN_TURN_SHIFT) & 0x7Fu, c = 0, band = 0, cb = 0;
    bool got = false;
    const uint32_t empties = 81u - (uint32_t)(__builtin_popcount(gm[0]) + __builtin_popcount(gm[1]) + __builtin_popcount(gm[2]));
    if (probe || empties < max_empty) {
        while (turn < 81u) {
            c = io.order(turn);
            ++turn;
            if (c > 80u) continue;
            band = c / 27u;
            const uint32_t q = c - 27u * band;
            cb = 1u << (q + q / 9u);
            if (band_word(gm, (int)band) & cb) {  // a given of P
                got = true;
                break;
            }
        }
    }
    if (!got) return N_DONE;
    // the test's root: cell c open to every digit but its own
    const uint32_t s = io.digit(c) - 1u;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const uint32_t m = band == (uint32_t)b ? cb : 0u;
#pragma unroll
        for (int d = 0; d < 9; ++d) B.P[d][b] = s == (uint32_t)d ? andn(B.P[d][b], m) : (B.P[d][b] | m);
        nd[b] = andn(gm[b], m);
        und[b] = andn(ROWS, nd[b]);
    }
    depth = 0;
    mode = (mode & ~(MN_CELL | MN_TURN)) | c | (turn << MN_TURN_SHIFT);
    return N_CONT;
}

struct MinStats {
    uint64_t passes;
    uint32_t max_depth;  // deepest stack depth reached (levels in use)
    uint32_t tests;      // tests started
};

// Host / reference driver: a loaded board whose givens are clean (given[]
// from load_words) minimised or probed through io, the caller's working copy.
// The stack holds MIN_LEVELS lines.  Returns min(2, completions) with
// removed = the givens erased, or COUNT_FAULT (the caller puts the input back).
template <typename Stack, class Io>
PS_FN int32_t min_board(Board &B, const uint32_t (&given)[3], Stack &stk, uint32_t max_depth, bool probe,
                        uint32_t max_empty, const Io &io, uint32_t &removed, MinStats &st)
{
    const WordStack<Stack> ws = {stk};
    uint32_t depth, mode, und[3], nd[3];
    min_start(B, given, und, nd, depth, mode, ws);
    removed = 0;
    for (;;) {
        const uint32_t turn = mode & MN_TURN;
        const int k = min_iter(B, und, nd, depth, mode, ws, max_depth, probe, max_empty, io);
        st.passes++;
        if (depth > st.max_depth) st.max_depth = depth;
        if (k == N_CONT) {
            if ((mode & MN_TURN) != turn) st.tests++;  // a turn was taken
            continue;
        }
        if (k == N_FAULT) return (int32_t)COUNT_FAULT;
        removed = min_removed(mode);
        return min_status(mode);
    }
}

}  // namespace plane

#endif  // SDK_PLANE_MIN_H
