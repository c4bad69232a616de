// logic.h -- the named techniques (subsets and fish) as monotone rule steps
// on top of rate.h's N, H and L, on the digit-plane layout of plane::Board.
// DESIGN.md §26 is the specification; in short:
//
// The Hall step of size k on a 9x9 0/1 matrix with row sets M[0..8]: for every
// k-subset I of rows with u = the union of its rows, |u| < k makes the state
// dead (pigeonhole) and |u| == k takes u out of every row outside I.  Rows of
// any size take part.
//   S_k  subsets, k = 2, 3, 4: in each of the 27 units the step on cells x
//        candidate digits (naked) and on digits x cells (hidden);
//   F_k  fish, k = 2, 3, 4: per digit the step on rows x columns and on
//        columns x rows (X-wing, swordfish, jellyfish, both orientations).
// The step only removes and is monotone with dead as the bottom state (the
// "< k is dead" clause is what makes it so), so a rule set's fixpoint -- and
// whether it is dead -- depends on no order; tests/logic_cases.py, per cell
// and by the text, reaches the same states bit for bit.
//
// A rule set is a bit mask (N = 1 ... F4 = 256), a ladder a list of 1..8 rule
// sets, each holding N and a proper superset of the one before; step j's
// closure is computed on the closure of the step before.
//
// The 72 matrices of a sweep are slices of three tables of 9-bit values: per
// digit d and row r the columns where d has a place in r ("hidden subsets in
// row r": fix r, vary d; "row fish of d": fix d, vary r), likewise per column
// and per box; the naked matrices are the transposes of the hidden ones.
// Matrix m = 9 kind + idx:
//   kind 0  row fish of digit idx        M[i] = slice(ROW, idx, i)
//   kind 1  column fish of digit idx     M[i] = slice(COL, idx, i)
//   kind 2-4  hidden in row / column / box idx   M[i] = slice(t, i, idx)
//   kind 5-7  naked in row / column / box idx    the transpose of kind - 3
//
// Plain C++ for host and device: tests/native/logic_host.cpp compiles it with
// g++, logic_kernels.hip runs it on the GPU.  The state is read as 27 words
// W[3 d + b] = P[d][b]; a matrix and its removals as nine words STRIDE apart
// (1 on the host, 64 in a wave's LDS, one column a lane).
// (SDK_LOGIC_H is the rule H of include/sudoku_hip.h)
#ifndef SDK_LOGIC_HEADER
#define SDK_LOGIC_HEADER

#include "rate.h"

// test-only: matrices, rows and subsets in descending order and a sweep's
// removals all taken from the sweep's first state (another schedule of the
// same rules; tests/test_logic_host.py checks that nothing depends on it)
#ifndef SDK_LOGIC_DESCEND
#define SDK_LOGIC_DESCEND 0
#endif

namespace logic {

using plane::Board;

enum { MAX_STEPS = 8, NOT_RUN = -2, INVALID = -1, MATRICES = 72 };
enum : uint32_t { N = 1, H = 2, L = 4, S2 = 8, S3 = 16, S4 = 32, F2 = 64, F3 = 128, F4 = 256, ALL = 0x1FF, NHL = 7, HALL = ALL & ~NHL };
enum { T_ROW = 0, T_COL = 1, T_BOX = 2 };
enum { SW_NONE = 0, SW_CHANGED = 1, SW_DEAD = 2 };

struct Result {
    int32_t step;
    int32_t open[MAX_STEPS];
    int32_t left[MAX_STEPS];
};

// 1..8 masks inside 0x1FF, each with N, each a proper superset of the one before
PS_FN bool ladder_ok(const uint32_t *ladder, int steps)
{
    if (!ladder || steps < 1 || steps > MAX_STEPS) return false;
    uint32_t prev = 0;
    for (int j = 0; j < steps; ++j) {
        const uint32_t m = ladder[j];
        if ((m & ~(uint32_t)ALL) || !(m & N) || m == prev || (m & prev) != prev) return false;
        prev = m;
    }
    return true;
}

// rate.h's level of a rule set that is one (N, N|H, N|H|L), else 0
PS_FN int rate_level(uint32_t rules) { return rules == N ? 1 : rules == (N | H) ? 2 : rules == NHL ? 3 : 0; }

// ---- the slicings
// the places of digit d in unit u of type t, bit k = the unit's k-th cell
PS_FN uint32_t slice(const uint32_t *W, int t, int d, int u)
{
    if (t == T_ROW) return (W[3 * d + u / 3] >> (10 * (u % 3))) & 0x1FFu;
    if (t == T_COL) {
        uint32_t s = 0;
        for (int b = 0; b < 3; ++b) {
            const uint32_t w = W[3 * d + b] >> u;
            s |= ((w & 1u) | ((w >> 9) & 2u) | ((w >> 18) & 4u)) << (3 * b);
        }
        return s;
    }
    const uint32_t w = W[3 * d + u / 3] >> (3 * (u % 3));
    return (w & 7u) | ((w >> 7) & 0x38u) | ((w >> 14) & 0x1C0u);
}

// the k-th cell of unit u of type t as (band, bit position)
PS_FN void unit_cell(int t, int u, int k, int &band, int &pos)
{
    const int r = t == T_ROW ? u : t == T_COL ? k : 3 * (u / 3) + k / 3;
    const int c = t == T_ROW ? k : t == T_COL ? u : 3 * (u % 3) + k % 3;
    band = r / 3;
    pos = 10 * (r % 3) + c;
}

// the sizes matrix m takes part in under `rules`: bit 0 size 2, bit 1 size 3, bit 2 size 4
PS_FN uint32_t sizes(int m, uint32_t rules) { return (m < 18 ? rules >> 6 : rules >> 3) & 7u; }

template <int STRIDE>
PS_FN void build(const uint32_t *W, int m, uint32_t *M)
{
    const int kind = m / 9, idx = m % 9;
    if (kind < 2) {
        for (int i = 0; i < 9; ++i) M[i * STRIDE] = slice(W, kind, idx, i);
    } else if (kind < 5) {
        for (int i = 0; i < 9; ++i) M[i * STRIDE] = slice(W, kind - 2, i, idx);
    } else {
        uint32_t s[9];
#pragma unroll
        for (int d = 0; d < 9; ++d) s[d] = slice(W, kind - 5, d, idx);
        for (int i = 0; i < 9; ++i) {
            uint32_t v = 0;
#pragma unroll
            for (int d = 0; d < 9; ++d) v |= ((s[d] >> i) & 1u) << d;
            M[i * STRIDE] = v;
        }
    }
}

// ---- the Hall step
PS_FN constexpr int row_at(int a) { return SDK_LOGIC_DESCEND ? 8 - a : a; }

// the subset I (a row mask) fired with the union u: u leaves every other row
template <int STRIDE>
PS_FN void fire(uint32_t *C, uint32_t I, uint32_t u)
{
    for (int r = 0; r < 9; ++r)
        if (!((I >> r) & 1u)) C[r * STRIDE] |= u;
}

// The sizes `ks` on the matrix M: C[i] |= what leaves row i; true = dead.  A
// union can only grow, so a subset whose union is larger than the largest
// size asked for is not extended.
template <int STRIDE>
PS_FN bool hall(const uint32_t *M, uint32_t *C, uint32_t ks)
{
    const int kmax = (ks & 4u) ? 4 : (ks & 2u) ? 3 : 2;
    for (int a = 0; a < 8; ++a) {
        const int i = row_at(a);
        const uint32_t u1 = M[i * STRIDE];
        if (__builtin_popcount(u1) > kmax) continue;
        for (int b = a + 1; b < 9; ++b) {
            const int j = row_at(b);
            const uint32_t u2 = u1 | M[j * STRIDE];
            const int p2 = __builtin_popcount(u2);
            if (p2 > kmax) continue;
            const uint32_t I2 = (1u << i) | (1u << j);
            if (ks & 1u) {
                if (p2 < 2) return true;
                if (p2 == 2) fire<STRIDE>(C, I2, u2);
            }
            if (!(ks & 6u)) continue;
            for (int c = b + 1; c < 9; ++c) {
                const int l = row_at(c);
                const uint32_t u3 = u2 | M[l * STRIDE];
                const int p3 = __builtin_popcount(u3);
                if (p3 > kmax) continue;
                const uint32_t I3 = I2 | (1u << l);
                if (ks & 2u) {
                    if (p3 < 3) return true;
                    if (p3 == 3) fire<STRIDE>(C, I3, u3);
                }
                if (!(ks & 4u)) continue;
                for (int e = c + 1; e < 9; ++e) {
                    const int q = row_at(e);
                    const uint32_t u4 = u3 | M[q * STRIDE];
                    const int p4 = __builtin_popcount(u4);
                    if (p4 < 4) return true;
                    if (p4 == 4) fire<STRIDE>(C, I3 | (1u << q), u4);
                }
            }
        }
    }
    return false;
}

// The removals C of matrix m (whose rows are M) as cells of the board:
// clear(d, band, pos) for every place that leaves.  True when there is one.
template <int STRIDE, typename Clear>
PS_FN bool apply(int m, const uint32_t *M, const uint32_t *C, Clear clear)
{
    const int kind = m / 9, idx = m % 9;
    bool any = false;
    for (int i = 0; i < 9; ++i) {
        uint32_t rem = C[i * STRIDE] & M[i * STRIDE];
        while (rem) {
            const int j = __builtin_ctz(rem);
            rem &= rem - 1u;
            // (kind 0, 1: digit idx, unit i, cell j; 2-4: digit i, unit idx, cell j; 5-7: digit j, unit idx, cell i)
            const int d = kind < 2 ? idx : kind < 5 ? i : j;
            const int t = kind < 2 ? kind : kind < 5 ? kind - 2 : kind - 5;
            int band, pos;
            unit_cell(t, kind < 2 ? i : idx, kind < 5 ? j : i, band, pos);
            clear(d, band, pos);
            any = true;
        }
    }
    return any;
}

// ---- closures
// Rule L alone on every digit (a rule set with L and without H: rate::pass
// has no such level).  True when something was removed.
PS_FN bool pass_l(Board &B)
{
    using namespace plane;
    uint32_t chg = 0;
    for (int d = 0; d < 9; ++d) {
        uint32_t y[3], o[3], vp[3], clear[3];
        for (int b = 0; b < 3; ++b) {
            y[b] = B.P[d][b];
            o[b] = or3(y[b], y[b] >> 10, y[b] >> 20) & 0x1FFu;
            const uint32_t o1 = o[b] >> 1, o2 = o[b] >> 2;
            vp[b] = o[b] & box_cols(box_one(xor3(o[b], o1, o2), maj3(o[b], o1, o2)));
        }
        rate::locked(y, o, vp, maj3(o[0], o[1], o[2]), clear);
        for (int b = 0; b < 3; ++b) {
            chg |= y[b] & clear[b];
            B.P[d][b] = andn(y[b], clear[b]);
        }
    }
    return chg != 0;
}

// the closure under the N, H and L of `rules` (a rate:: verdict, never R_OPEN)
PS_FN int close_nhl(Board &B, uint32_t rules, int &open)
{
    const int level = !(rules & H) ? 1 : (rules & L) ? 3 : 2;
    const bool l_alone = (rules & L) && !(rules & H);
    for (;;) {
        const int r = rate::close_level(B, level, open);
        if (r != rate::R_FIX || !l_alone || !pass_l(B)) return r;
    }
}

PS_FN void words_of(const Board &B, uint32_t (&W)[27])
{
    for (int w = 0; w < 27; ++w) W[w] = B.P[w / 3][w % 3];
}

// One sweep of the Hall steps of `rules` over the 72 matrices, one board at a
// time (the host's schedule; logic_wave_kernel gives every lane a matrix).
PS_FN int sweep(Board &B, uint32_t rules)
{
    bool changed = false;
    uint32_t W[27];
    words_of(B, W);
    for (int a = 0; a < MATRICES; ++a) {
        const int m = SDK_LOGIC_DESCEND ? MATRICES - 1 - a : a;
        const uint32_t ks = sizes(m, rules);
        if (!ks) continue;
#if !SDK_LOGIC_DESCEND
        words_of(B, W);
#endif
        uint32_t M[9], C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        build<1>(W, m, M);
        if (hall<1>(M, C, ks)) return SW_DEAD;
        if (apply<1>(m, M, C, [&](int d, int band, int pos) { B.P[d][band] &= ~(1u << pos); })) changed = true;
    }
    return changed ? SW_CHANGED : SW_NONE;
}

// the closure under `rules`: N, H and L to their fixpoint, then a sweep of the
// Hall steps, until a sweep removes nothing
PS_FN int close_rules(Board &B, uint32_t rules, int &open)
{
    for (;;) {
        const int r = close_nhl(B, rules, open);
        if (r != rate::R_FIX || !(rules & HALL)) return r;
        const int s = sweep(B, rules);
        if (s == SW_DEAD) return rate::R_DEAD;
        if (s == SW_NONE) return rate::R_FIX;
    }
}

PS_FN int candidates_left(const Board &B)
{
    int n = 0;
#pragma unroll
    for (int w = 0; w < 27; ++w) n += __builtin_popcount(B.P[w / 3][w % 3] & plane::ROWS);
    return n;
}

// ---- answers
PS_FN void start(Result &R)
{
    R.step = 0;
#pragma unroll
    for (int k = 0; k < MAX_STEPS; ++k) R.open[k] = R.left[k] = NOT_RUN;
}
PS_FN void invalid(Result &R)
{
    R.step = INVALID;
#pragma unroll
    for (int k = 0; k < MAX_STEPS; ++k) R.open[k] = R.left[k] = INVALID;
}

// Enter the verdict r (never R_OPEN) of step j's closure (j 0-based) into R;
// true when the board's answer is settled, false when step j + 1 has to run.
PS_FN bool settle(Result &R, int j, int r, int open, int left, int steps)
{
    const bool fix = r == rate::R_FIX;
    const int32_t vo = fix ? open : r == rate::R_DEAD ? -1 : 0, vl = fix ? left : r == rate::R_DEAD ? -1 : 81;
#pragma unroll
    for (int k = 0; k < MAX_STEPS; ++k) {
        // (masked selects, not open[j]: indexed by a lane's own step the entries would live in scratch)
        const int32_t m = -(int32_t)(fix ? k == j : (k >= j && k < steps));
        R.open[k] = (vo & m) | (R.open[k] & ~m);
        R.left[k] = (vl & m) | (R.left[k] & ~m);
    }
    R.step = fix ? steps + 1 : r == rate::R_DEAD ? 0 : j + 1;
    return !fix || j == steps - 1;
}

// Host / reference driver: B = the start state; on return the deepest
// closure computed (meaningless when R.step == 0).
PS_FN void run_board(Board &B, const uint32_t *ladder, int steps, Result &R)
{
    start(R);
    int open = 0;
    for (int j = 0; j < steps; ++j) {
        const int r = close_rules(B, ladder[j], open);
        if (settle(R, j, r, open, candidates_left(B), steps)) return;
    }
}

// ---- the start state
PS_FN void empty_board(Board &B)
{
#pragma unroll
    for (int d = 0; d < 9; ++d)
#pragma unroll
        for (int b = 0; b < 3; ++b) B.P[d][b] = plane::ROWS;
#pragma unroll
    for (int b = 0; b < 3; ++b) B.Det[b] = 0;
}

// B &= the pencil marks get(cell) (bit d-1 = digit d).  False for a bit above 0x1FF.
template <typename Get>
PS_FN bool and_marks(Board &B, Get get)
{
    uint32_t Q[9][3], bad = 0;
#pragma unroll
    for (int d = 0; d < 9; ++d)
#pragma unroll
        for (int b = 0; b < 3; ++b) Q[d][b] = 0;
#pragma unroll
    for (int i = 0; i < 81; ++i) {
        const uint32_t m = get(i);
        bad |= m;
#pragma unroll
        for (int d = 0; d < 9; ++d) Q[d][plane::cell_band(i)] |= ((m >> d) & 1u) << plane::cell_pos(i);
    }
#pragma unroll
    for (int d = 0; d < 9; ++d)
#pragma unroll
        for (int b = 0; b < 3; ++b) B.P[d][b] &= Q[d][b];
    return (bad & ~(uint32_t)ALL) == 0;
}

}  // namespace logic

#endif  // SDK_LOGIC_HEADER
