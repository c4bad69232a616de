// path.h -- the solving path: every deduction of a state, round by round, on
// top of logic.h's matrices and Hall step.  DESIGN.md §27 is the
// specification; in short:
//
// The nine CLASSES are the bit indices of a rule mask: 0 N, 1 H, 2 L, 3 S2,
// 4 S3, 5 S4, 6 F2, 7 F3, 8 F4.  A FIRING is
//   a Hall firing (m, I, u): on matrix m (logic.h's numbering) the k-subset I
//     of rows (a row mask) with union u, |u| == k; u leaves every row outside
//     I.  N is size 1 on the naked matrices 45..71, H size 1 on the hidden
//     matrices 18..44, S_k size k on 18..71, F_k size k on 0..17;
//   an L firing (dir, d, line, box): digit d has a place in the three cells
//     the line (0..8 a row, 9..17 a column) shares with the box and, dir 0,
//     none elsewhere in the box: d leaves the rest of the line; dir 1, none
//     elsewhere in the line: d leaves the rest of the box.
// A firing is EFFECTIVE on a state when it removes a candidate there; a
// VIOLATION is a k-subset with |u| < k (size 1: an empty row of a matrix
// 18..71, the rating's dead).
//
// The schedule of one board, r = 0 rounds done:
//   1 dead: stop, DEAD, one contradiction event (class 0, round r + 1, the
//     smallest (m, I) among 18..71 with an empty row, u = 0);
//   2 solved: stop, SOLVED;  3 max_rounds > 0 and r == max_rounds: LIMITED;
//   4 the classes of `rules` in ascending order: an S_k or F_k with a
//     violation stops the board, DEAD, with a contradiction event of that
//     class, the smallest (m, I) and its u; the first class with an effective
//     firing is the round's class; none: STUCK;
//   5 ++r; every effective firing of the class, all evaluated on the round's
//     start state, is one event of round r; the new state is the start state
//     minus the union of their removals.
// (m, I) compares m first, then the row mask I as a number.
//
// An event is three words beside its owner:
//   w1 = round | class << 16 | contradiction << 20 | removed << 24
//   w2 = m | I << 8 | u << 17; for L m = 72 + dir, I = 1 << (d - 1),
//        u = line | box << 5
//   w3 = the candidates left after the event's round (contradiction: before).
//
// Plain C++ for host and device: tests/native/path_host.cpp compiles it with
// g++, path_kernels.hip runs it on the GPU with one wave a board.  A matrix
// is nine words STRIDE apart, as in logic.h.
#ifndef SDK_PATH_HEADER
#define SDK_PATH_HEADER

#include "logic.h"
#include "rate.h"

namespace path {

enum { DEAD = 0, SOLVED = 1, STUCK = 2, LIMITED = 3, INVALID = -1 };
enum { CLASSES = 9, C_N = 0, C_H = 1, C_L = 2, M_L = 72, L_PAIRS = 81 };
enum : uint32_t { NO_VIOLATION = 0xFFFFFFFFu };

struct Out {
    int32_t count, rounds, status;
    int32_t hist[CLASSES];
};

// the subset size of a Hall class (0 for L)
PS_FN int class_size(int c) { return c < 2 ? 1 : c == 2 ? 0 : (c - 3) % 3 + 2; }
// does matrix m take part in the Hall class c
PS_FN bool class_has(int c, int m)
{
    return c == C_N ? m >= 45 : c == C_H ? (m >= 18 && m < 45) : c < 6 ? m >= 18 : m < 18;
}

PS_FN uint32_t word1(int round, int cls, bool contradiction, int removed)
{
    return (uint32_t)round | ((uint32_t)cls << 16) | ((uint32_t)contradiction << 20) | ((uint32_t)removed << 24);
}
PS_FN uint32_t hall_word(int m, uint32_t I, uint32_t u) { return (uint32_t)m | (I << 8) | (u << 17); }
PS_FN uint32_t l_word(int dir, int d, int line, int box)
{
    return (uint32_t)(M_L + dir) | ((1u << d) << 8) | (((uint32_t)line | ((uint32_t)box << 5)) << 17);
}

PS_FN int left_of(const uint32_t *W)
{
    int n = 0;
    for (int w = 0; w < 27; ++w) n += __builtin_popcount(W[w] & plane::ROWS);
    return n;
}

// what the firing (I, u) removes on M: the elements of u in the rows outside I
template <int STRIDE>
PS_FN int removed(const uint32_t *M, uint32_t I, uint32_t u)
{
    int n = 0;
    for (int r = 0; r < 9; ++r)
        if (!((I >> r) & 1u)) n += __builtin_popcount(M[r * STRIDE] & u);
    return n;
}

// every k-subset I of the rows of M whose union u has at most k elements:
// f(I, u, |u|).  A union only grows, so a subset past k is not extended.
template <int STRIDE, typename F>
PS_FN void subsets(const uint32_t *M, int k, F f)
{
    for (int a = 0; a < 9; ++a) {
        const uint32_t u1 = M[a * STRIDE];
        const int p1 = __builtin_popcount(u1);
        if (p1 > k) continue;
        if (k == 1) {
            f(1u << a, u1, p1);
            continue;
        }
        for (int b = a + 1; b < 9; ++b) {
            const uint32_t u2 = u1 | M[b * STRIDE];
            const int p2 = __builtin_popcount(u2);
            if (p2 > k) continue;
            const uint32_t I2 = (1u << a) | (1u << b);
            if (k == 2) {
                f(I2, u2, p2);
                continue;
            }
            for (int c = b + 1; c < 9; ++c) {
                const uint32_t u3 = u2 | M[c * STRIDE];
                const int p3 = __builtin_popcount(u3);
                if (p3 > k) continue;
                const uint32_t I3 = I2 | (1u << c);
                if (k == 3) {
                    f(I3, u3, p3);
                    continue;
                }
                for (int e = c + 1; e < 9; ++e) {
                    const uint32_t u4 = u3 | M[e * STRIDE];
                    const int p4 = __builtin_popcount(u4);
                    if (p4 <= 4) f(I3 | (1u << e), u4, p4);
                }
            }
        }
    }
}

// The Hall class of size k on M: emit(I, u, removed) for every effective
// firing.  Returns the smallest violation as I << 9 | u, or NO_VIOLATION.
template <int STRIDE, typename Emit>
PS_FN uint32_t hall_class(const uint32_t *M, int k, Emit emit)
{
    uint32_t bad = NO_VIOLATION;
    subsets<STRIDE>(M, k, [&](uint32_t I, uint32_t u, int p) {
        if (p < k) {
            const uint32_t key = (I << 9) | u;
            bad = key < bad ? key : bad;
        } else {
            const int n = removed<STRIDE>(M, I, u);
            if (n) emit(I, u, n);
        }
    });
    return bad;
}

// the lowest empty row of M as a row mask, 0 for none
template <int STRIDE>
PS_FN uint32_t empty_row(const uint32_t *M)
{
    for (int r = 0; r < 9; ++r)
        if (!M[r * STRIDE]) return 1u << r;
    return 0u;
}

// every row of M holds one element
template <int STRIDE>
PS_FN bool all_single(const uint32_t *M)
{
    bool ok = true;
    for (int r = 0; r < 9; ++r) ok = ok && __builtin_popcount(M[r * STRIDE]) == 1;
    return ok;
}

// Rule L for digit d (0-based) and one box: emit(dir, line, t, idx, mask) for
// every effective firing, `mask` the places of d that leave unit idx of type t
// (bit k = the unit's k-th cell).
template <typename Emit>
PS_FN void l_pair(const uint32_t *W, int d, int box, Emit emit)
{
    const uint32_t bs = logic::slice(W, logic::T_BOX, d, box);
    if (!bs) return;
    for (int j = 0; j < 6; ++j) {
        const bool col = j >= 3;
        const int idx = col ? 3 * (box % 3) + (j - 3) : 3 * (box / 3) + j;
        // the three shared cells, as bits of the box and as bits of the line
        const uint32_t in_box = col ? 0x49u << (j - 3) : 7u << (3 * j);
        const uint32_t in_line = 7u << (3 * (col ? box / 3 : box % 3));
        if (!(bs & in_box)) continue;
        const uint32_t ls = logic::slice(W, col ? logic::T_COL : logic::T_ROW, d, idx);
        const uint32_t box_rest = bs & ~in_box, line_rest = ls & ~in_line;
        const int line = col ? 9 + idx : idx;
        if (!box_rest && line_rest) emit(0, line, col ? logic::T_COL : logic::T_ROW, idx, line_rest);
        if (!line_rest && box_rest) emit(1, line, (int)logic::T_BOX, box, box_rest);
    }
}

// the cells of `mask` in unit idx of type t: clear(band, pos)
template <typename Clear>
PS_FN void unit_cells(int t, int idx, uint32_t mask, Clear clear)
{
    while (mask) {
        const int k = __builtin_ctz(mask);
        mask &= mask - 1u;
        int band, pos;
        logic::unit_cell(t, idx, k, band, pos);
        clear(band, pos);
    }
}

// what the Hall firing (I, u) on matrix m (rows M) removes: clear(d, band, pos)
template <int STRIDE, typename Clear>
PS_FN void hall_cells(int m, const uint32_t *M, uint32_t I, uint32_t u, Clear clear)
{
    const int kind = m / 9, idx = m % 9;
    for (int i = 0; i < 9; ++i) {
        uint32_t rem = ((I >> i) & 1u) ? 0u : u & M[i * STRIDE];
        while (rem) {
            const int j = __builtin_ctz(rem);
            rem &= rem - 1u;
            const int d = kind < 2 ? idx : kind < 5 ? i : j;
            const int t = kind < 2 ? kind : kind < 5 ? kind - 2 : kind - 5;
            int band, pos;
            logic::unit_cell(t, kind < 2 ? i : idx, kind < 5 ? j : i, band, pos);
            clear(d, band, pos);
        }
    }
}

// ---- one board on the host (the reference schedule; path_wave_kernel spreads
// the matrices of a class over a wave)
// W: the start state's 27 words, the end state on return.  row(w1, w2, w3) is
// called for every event.
template <typename Row>
PS_FN void run_board(uint32_t (&W)[27], uint32_t rules, int max_rounds, Out &O, Row row)
{
    O.count = O.rounds = 0;
    for (int c = 0; c < CLASSES; ++c) O.hist[c] = 0;
    uint32_t M[9];
    for (;;) {
        // 1, 2: dead, solved
        bool solved = true;
        for (int m = 18; m < logic::MATRICES; ++m) {
            logic::build<1>(W, m, M);
            const uint32_t I = empty_row<1>(M);
            if (I) {
                row(word1(O.rounds + 1, 0, true, 0), hall_word(m, I, 0u), (uint32_t)left_of(W));
                ++O.count;
                O.status = DEAD;
                return;
            }
            if (m >= 45 && m < 54) solved = solved && all_single<1>(M);
        }
        if (solved) {
            O.status = SOLVED;
            return;
        }
        if (max_rounds > 0 && O.rounds == max_rounds) {
            O.status = LIMITED;
            return;
        }
        // 4, 5: the first class that fires; its removals gather in S
        uint32_t S[27];
        for (int w = 0; w < 27; ++w) S[w] = W[w];
        int fired = -1, events = 0;
        for (int c = 0; c < CLASSES && fired < 0; ++c) {
            if (!((rules >> c) & 1u)) continue;
            if (c == C_L) {
                for (int q = 0; q < L_PAIRS; ++q)
                    l_pair(W, q / 9, q % 9, [&](int, int, int t, int idx, uint32_t mask) {
                        ++events;
                        unit_cells(t, idx, mask, [&](int band, int pos) { S[3 * (q / 9) + band] &= ~(1u << pos); });
                    });
            } else {
                const int k = class_size(c);
                for (int m = 0; m < logic::MATRICES; ++m) {
                    if (!class_has(c, m)) continue;
                    logic::build<1>(W, m, M);
                    const uint32_t bad = hall_class<1>(M, k, [&](uint32_t I, uint32_t u, int) {
                        ++events;
                        hall_cells<1>(m, M, I, u, [&](int d, int band, int pos) { S[3 * d + band] &= ~(1u << pos); });
                    });
                    if (bad != NO_VIOLATION && k > 1) {
                        row(word1(O.rounds + 1, c, true, 0), hall_word(m, bad >> 9, bad & 0x1FFu), (uint32_t)left_of(W));
                        ++O.count;
                        O.status = DEAD;
                        return;
                    }
                }
            }
            if (events) fired = c;
        }
        if (fired < 0) {
            O.status = STUCK;
            return;
        }
        ++O.rounds;
        const uint32_t left = (uint32_t)left_of(S);
        if (fired == C_L) {
            for (int q = 0; q < L_PAIRS; ++q)
                l_pair(W, q / 9, q % 9, [&](int dir, int line, int, int, uint32_t mask) {
                    row(word1(O.rounds, C_L, false, __builtin_popcount(mask)), l_word(dir, q / 9, line, q % 9), left);
                });
        } else {
            for (int m = 0; m < logic::MATRICES; ++m) {
                if (!class_has(fired, m)) continue;
                logic::build<1>(W, m, M);
                hall_class<1>(M, class_size(fired), [&](uint32_t I, uint32_t u, int n) {
                    row(word1(O.rounds, fired, false, n), hall_word(m, I, u), left);
                });
            }
        }
        O.count += events;
        O.hist[fired] += events;
        for (int w = 0; w < 27; ++w) W[w] = S[w];
    }
}

}  // namespace path

#endif  // SDK_PATH_HEADER
