// plane_sample.h -- a random completion of one board on digit planes: the
// count's search (plane_count.h) with the digit of every branch drawn from a
// seeded, counter-based hash instead of taken in ascending order.
//
// An item is a board and a 64-bit key.  Its answer is a function of the
// board's 81 bytes, the seed and the key alone: every draw is a hash of
// (seed, key, t), t the number of draws the item has made so far, so it does
// not matter which lane runs the item, in which batch it came or what the
// lanes beside it do.
//
// Search.  Built from plane_solver.h's and plane_count.h's pieces, none of
// them changed: one look-ahead pass (plane::pass_ahead) per iteration; at a
// STUCK fixpoint a level is pushed on the cell plane::pick_mrv picks (the cell
// choice is deterministic); at DEAD the deepest level is popped; the first
// SOLVED verdict ends the item.  The one difference from count_step is the
// digit: on a push it is drawn from the cell's candidates (two or more), on a
// pop from the level's remaining digits.  With all arithmetic mod 2^64:
//
//     mix(x):   x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;
//               x *= 0x94D049BB133111EB;  x ^= x >> 31
//     h       = mix(mix(seed) + key)
//     r_t     = mix(h + (t + 1) * 0x9E3779B97F4A7C15)      t = 0, 1, 2, ...
//     index   = ((r_t >> 32) * popcount(mask)) >> 32
//     digit   = the index-th lowest set bit of mask
//
// Every choice advances t, push or pop, also when the mask has one bit.  The
// chosen digit leaves the level's remaining mask, as in count_step, and a
// level whose last digit is taken is freed at once; the stack entry format,
// COUNT_MAX_DEPTH and its depth argument are the count's (plane_count.h): a
// push at max_depth is a fault, never an answer.
//
// What this is.  Each branch picks uniformly among the digits left in the
// cell.  Every completion of the board has positive probability: choosing a
// completion's own digit at every branch never dies, because rules A-D only
// remove digits that no completion uses.  The search is complete, so it ends
// with a completion whenever the board has one and with none otherwise.  The
// distribution over completions is that of a randomised search; it is NOT
// uniform.
//
// Plain C++ for host and device, like plane_count.h: the CPU tests compile it
// with g++ (tests/native/sample_host.cpp).
#ifndef SDK_PLANE_SAMPLE_H
#define SDK_PLANE_SAMPLE_H

#include "plane_count.h"

namespace plane {

enum { P_CONT = 0, P_FOUND = 1, P_NONE = 2, P_FAULT = 3 };

PS_FN uint64_t sample_mix(uint64_t x)
{
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// an item's stream: h of the rule above
PS_FN uint64_t sample_stream(uint64_t seed, uint64_t key) { return sample_mix(sample_mix(seed) + key); }

// choose(mask): the item's draw number t out of mask (one to nine digit bits)
// as a digit bit; t advances
PS_FN uint32_t sample_choose(uint32_t mask, uint64_t h, uint32_t &t)
{
    const uint64_t r = sample_mix(h + ((uint64_t)t + 1u) * 0x9E3779B97F4A7C15ull);
    ++t;
    const uint32_t index = (uint32_t)(((r >> 32) * (uint64_t)(uint32_t)__builtin_popcount(mask)) >> 32);
    uint32_t m = mask;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) m = k < index ? m & (m - 1u) : m;  // index <= 8: drop that many low bits
    return m & (0u - m);
}

// count_step with the drawn digit: the search step after a pass_ahead() whose
// verdict r is STUCK or DEAD.  Returns C_CONT (pass again; nd[] = the one cell
// fixed), C_DONE (no level left: the board has no completion) or C_FAULT (a
// push at max_depth, or a stack line that breaks count_step's invariant).
template <class Stack>
PS_FN int sample_step(Board &B, uint32_t (&und)[3], uint32_t (&nd)[3], int r, uint32_t &depth, const Stack &stk,
                      uint32_t max_depth, uint64_t h, uint32_t &t)
{
    int band = 0, pos = 0;
    uint32_t fix_d = 0;
    if (r == STUCK) {
        if (depth >= max_depth) return C_FAULT;
        pick_mrv(B, und, band, pos);
        const uint32_t cand = cell_cand(B, band, pos);  // >= 2 digits: rule A ran on these planes
        fix_d = sample_choose(cand, h, t);
        stk.push(depth, B, und, make_entry(band, pos, cand ^ fix_d));
        depth++;
    } else {
        if (depth == 0) return C_DONE;
        const uint32_t level = depth - 1;
        const uint32_t e = stk.pop(level, B, und);
        const uint32_t rem = (e >> 8) & 0x1FFu;
        if (!rem) return C_FAULT;
        fix_d = sample_choose(rem, h, t);
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

// One iteration on an item in flight: a pass, then the step.  P_FOUND: the
// planes hold the completion (the caller stores it now); P_NONE: the board has
// none; P_FAULT.  The GPU kernel's lane loop and the host driver both run this.
template <class Stack>
PS_FN int sample_iter(Board &B, uint32_t (&und)[3], uint32_t (&nd)[3], uint32_t &depth, const Stack &stk,
                      uint32_t max_depth, uint64_t h, uint32_t &t)
{
    const int r = pass_ahead(B, und, nd);
    if (r == OPEN) return P_CONT;
    if (r == SOLVED) return P_FOUND;
    const int s = sample_step(B, und, nd, r, depth, stk, max_depth, h, t);
    return s == C_CONT ? P_CONT : s == C_DONE ? P_NONE : P_FAULT;
}

struct SampleStats {
    uint64_t passes;
    uint32_t max_depth;  // deepest stack depth reached (levels in use)
    uint32_t draws;      // t at the end
};

// Host / reference driver: a loaded board whose givens are clean (given[] from
// load_words) searched under stream h.  Returns P_FOUND with the completion in
// B's planes, P_NONE or P_FAULT.
template <typename Stack>
PS_FN int sample_board(Board &B, const uint32_t (&given)[3], Stack &stk, uint32_t max_depth, uint64_t h,
                       SampleStats &st)
{
    const WordStack<Stack> ws = {stk};
    uint32_t depth = 0, t = 0, und[3], nd[3];
    for (int b = 0; b < 3; ++b) {
        nd[b] = given[b];
        und[b] = andn(ROWS, given[b]);
    }
    for (;;) {
        const int k = sample_iter(B, und, nd, depth, ws, max_depth, h, t);
        st.passes++;
        if (depth > st.max_depth) st.max_depth = depth;
        st.draws = t;
        if (k != P_CONT) return k;
    }
}

}  // namespace plane

#endif  // SDK_PLANE_SAMPLE_H
