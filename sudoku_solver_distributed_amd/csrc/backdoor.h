// backdoor.h -- the smallest sets of cells that unlock a puzzle, on rate.h's
// rule closures.  DESIGN.md §23 is the specification; in short, for a board
// b, a valid grid g that keeps b's givens and a level L in 1..3: a set S of
// cells is a backdoor when closure_L of b with the cells of S filled from g
// is solved.  Asked for are the smallest size of a backdoor up to max_size,
// how many there are of that size, the lexicographically first of them and
// the cells that lie in one.
//
// The rules are monotone, so (a) every superset of a backdoor is one and (b) a
// minimum backdoor holds only cells that closure_L(b) leaves with two or more
// candidates (a cell with one candidate there holds g's digit -- the rules are
// sound and g is a completion -- so fixing it changes nothing and the set
// without it is a backdoor too).  By (b) the search runs over the k-subsets
// of the n open cells of closure_L(b), k = 1, 2, ..., each started from that
// closure instead of from b (closure_L(b + S) is the closure of closure_L(b)
// with S fixed, the same fixpoint); a subset is named by its rank in the
// lexicographic order of the k-subsets of 0..n-1, the indices of the open
// cells in cell order.
//
// Plain C++ for host and device: tests/native/backdoor_host.cpp compiles it
// with g++, backdoor_kernels.hip runs it on the GPU.
#ifndef SDK_BACKDOOR_H
#define SDK_BACKDOOR_H

#include "rate.h"

namespace backdoor {

using plane::Board;

enum { MAX_SIZE = 4, MAX_LEVEL = 3, INVALID = -1, MISMATCH = -2 };

// C(n, j) for n <= 81, j <= 4 (at most C(81, 4) = 1 663 740; the products stay
// below 2^32: 81 * 80 * 79 * 78 = 39 929 760).  Zero for n < j.
PS_FN constexpr uint32_t choose(uint32_t n, int j)
{
    return j == 0   ? 1u
           : j == 1 ? n
           : j == 2 ? n * (n - 1u) / 2u
           : j == 3 ? n * (n - 1u) * (n - 2u) / 6u
                    : n * (n - 1u) * (n - 2u) * (n - 3u) / 24u;
}

// The K-subset of 0..n-1 with lexicographic rank r < C(n, K), ascending in
// idx[0..K-1].  The subsets whose first element is x come C(n-1-x, K-1) at a
// time; the last element is what is left of the rank.
template <int K>
PS_FN void unrank(uint32_t r, uint32_t n, uint32_t (&idx)[MAX_SIZE])
{
    uint32_t x = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int rem = K - 1 - j;
        if (rem > 0) {
            for (;;) {
                const uint32_t c = choose(n - 1u - x, rem);
                if (r < c) break;
                r -= c;
                ++x;
            }
        } else {
            x += r;
        }
        idx[j] = x;
        ++x;
    }
#pragma unroll
    for (int j = K; j < MAX_SIZE; ++j) idx[j] = 0xFFu;
}
PS_FN void unrank_k(int k, uint32_t r, uint32_t n, uint32_t (&idx)[MAX_SIZE])
{
    if (k == 1) unrank<1>(r, n, idx);
    else if (k == 2) unrank<2>(r, n, idx);
    else if (k == 3) unrank<3>(r, n, idx);
    else unrank<4>(r, n, idx);
}

// Validate g from its 21 words: 0 for a valid grid, INVALID for a byte outside
// 1..9, else MISMATCH.  A full grid is valid exactly when N finds no two equal
// digits in a unit: one pass, nothing to remove.
PS_FN int validate_grid(const uint32_t (&xg)[21])
{
    Board G;
    uint32_t V[4][3], given[3];
    const uint32_t bad = plane::slices_from_words(xg, V);
    plane::planes_from_slices(G, V, given);
    if (bad || (given[0] & given[1] & given[2]) != (uint32_t)plane::ROWS) return INVALID;
    int open;
    return rate::pass(G, 1, open) == rate::R_SOLVED ? 0 : MISMATCH;
}

// g keeps b's givens: where a byte of b (0..9) is not zero, g's byte equals it
PS_FN bool keeps_givens(const uint32_t (&xb)[21], const uint32_t (&xg)[21])
{
    uint32_t diff = 0;
#pragma unroll
    for (int k = 0; k < 21; ++k) {
        const uint32_t x = xb[k];
        const uint32_t nz = (x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x01010101u;  // bit 0 of every byte that is not zero
        diff |= (x ^ xg[k]) & (nz * 0xFFu) & (k == 20 ? 0xFFu : 0xFFFFFFFFu);
    }
    return diff == 0;
}

// Validate (b, g) from their 21 words each and leave b's start state in B.
// 0 when g is a valid grid that keeps b's givens; INVALID for a byte > 9 in b
// or outside 1..9 in g; else MISMATCH.
PS_FN int validate(Board &B, const uint32_t (&xb)[21], const uint32_t (&xg)[21])
{
    const int code = validate_grid(xg);
    const bool keeps = keeps_givens(xb, xg);
    const bool ok_b = rate::load(B, xb);
    if (code == INVALID || !ok_b) return INVALID;
    return code == 0 && keeps ? 0 : MISMATCH;
}

// The cells closure_L leaves with two or more candidates, as band words (bit
// plane::cell_pos(c) of word plane::cell_band(c)), and how many they are.
PS_FN uint32_t open_cells(const Board &B, uint32_t (&open)[3])
{
    uint32_t single[3];
    plane::rule_a(B, single);
    uint32_t n = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        open[b] = plane::andn((uint32_t)plane::ROWS, single[b]);
        n += (uint32_t)__builtin_popcount(open[b]);
    }
    return n;
}

// An open cell and g's digit there, as the trials read them: cell | digit << 8
PS_FN uint32_t entry_of(int cell, uint32_t digit) { return (uint32_t)cell | (digit << 8); }

// Fix the K cells of the subset with rank r on T (a copy of closure_L(b)):
// entry(i) is the i-th open cell's entry.  cov[]: the subset as band words.
template <int K, typename Entry>
PS_FN void fix_subset(Board &T, uint32_t r, uint32_t n, Entry entry, uint32_t (&cov)[3])
{
    uint32_t idx[MAX_SIZE];
    unrank<K>(r, n, idx);
    cov[0] = cov[1] = cov[2] = 0u;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint32_t e = entry(idx[j]);
        const int cell = (int)(e & 0xFFu);
        const int band = plane::cell_band(cell), pos = plane::cell_pos(cell);
        plane::set_cell(T, band, pos, 1u << ((e >> 8) - 1u));
        const uint32_t bit = 1u << pos;
        cov[0] |= band == 0 ? bit : 0u;
        cov[1] |= band == 1 ? bit : 0u;
        cov[2] |= band == 2 ? bit : 0u;
    }
}

// One board's answer, as sdk_backdoor_batch documents it
struct Answer {
    int32_t size, count;
    uint8_t first[MAX_SIZE];
    uint8_t cover[81];
};

PS_FN void answer_code(Answer &A, int32_t size, int32_t count)
{
    A.size = size;
    A.count = count;
    for (int j = 0; j < MAX_SIZE; ++j) A.first[j] = 0xFFu;
    for (int c = 0; c < 81; ++c) A.cover[c] = 0;
}

// Host / reference driver: every subset of every size in rank order, one
// after the other (the kernels spread the same ranks over the device).
template <int K>
inline bool host_size(const Board &C, const uint32_t *entries, uint32_t n, int level, Answer &A)
{
    const uint32_t ranks = choose(n, K);
    uint32_t cover[3] = {0u, 0u, 0u}, first = 0xFFFFFFFFu;
    int32_t count = 0;
    for (uint32_t r = 0; r < ranks; ++r) {
        Board T = C;
        uint32_t cov[3];
        fix_subset<K>(T, r, n, [&](uint32_t i) { return entries[i]; }, cov);
        int open;
        if (rate::close_level(T, level, open) != rate::R_SOLVED) continue;
        ++count;
        if (r < first) first = r;
        for (int b = 0; b < 3; ++b) cover[b] |= cov[b];
    }
    if (!count) return false;
    A.size = K;
    A.count = count;
    uint32_t idx[MAX_SIZE];
    unrank<K>(first, n, idx);
    for (int j = 0; j < K; ++j) A.first[j] = (uint8_t)(entries[idx[j]] & 0xFFu);
    for (int c = 0; c < 81; ++c) A.cover[c] = (uint8_t)((cover[plane::cell_band(c)] >> plane::cell_pos(c)) & 1u);
    return true;
}

inline void host_board(const uint32_t (&xb)[21], const uint32_t (&xg)[21], const uint8_t *g, int level, int max_size,
                       Answer &A)
{
    Board B;
    const int v = validate(B, xb, xg);
    if (v != 0) return answer_code(A, v, 0);
    int op;
    const int r = rate::close_level(B, level, op);
    if (r == rate::R_SOLVED) return answer_code(A, 0, 1);
    if (r == rate::R_DEAD) return answer_code(A, MISMATCH, 0);  // (never: g is a completion and the rules are sound)
    uint32_t open[3], entries[81];
    const uint32_t n = open_cells(B, open);
    uint32_t k = 0;
    for (int c = 0; c < 81; ++c)
        if ((open[plane::cell_band(c)] >> plane::cell_pos(c)) & 1u) entries[k++] = entry_of(c, g[c]);
    answer_code(A, max_size + 1, 0);
    if (host_size<1>(B, entries, n, level, A) || max_size < 2) return;
    if (host_size<2>(B, entries, n, level, A) || max_size < 3) return;
    if (host_size<3>(B, entries, n, level, A) || max_size < 4) return;
    host_size<4>(B, entries, n, level, A);
}

}  // namespace backdoor

#endif  // SDK_BACKDOOR_H
