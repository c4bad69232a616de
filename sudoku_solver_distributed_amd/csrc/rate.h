// rate.h -- how hard a puzzle is, as fixpoints of rule sets on the digit-plane
// layout of plane::Board (plane_solver.h: 27 words, guard bits).  DESIGN.md
// §14 is the specification; in short, per cell a candidate set, and
//   N  a cell with one candidate d removes d from its 20 peers;
//   H  a digit with one place in a unit becomes that cell's only candidate;
//   L  locked candidates, all four forms (box -> row, box -> column,
//      row -> box, column -> box);
//   T  fix a candidate of a cell with two or more: if the {N, H, L} closure
//      of that state is dead, the candidate goes (one level of trial).
// Level 1 is {N}, 2 {N, H}, 3 {N, H, L}, 4 {N, H, L, T}.  A state is dead
// when a cell has no candidate or a unit has no place for a digit.  Every
// rule only removes candidates and is monotone, so a level's fixpoint -- and
// whether it is dead -- does not depend on the order the rules fire in: the
// schedule below (Gauss-Seidel over the digits, as plane::pass_body's) is one
// of many, and tests/rate_cases.py, per cell and rule by rule, reaches the
// same states bit for bit.
//
// plane::pass is not used: it fuses its rules for the solve path, keeps the
// cells that clash (its callers never pass such givens) and has three of the
// four locked-candidate forms.  Here every rule is applied in full: where two
// applications of a rule empty each other's cell or unit, the pass reports
// the state dead at once (the rules would get there one step later).
//
// Plain C++ for host and device: tests/native/rate_host.cpp compiles it with
// g++, rate_kernels.hip runs it on the GPU.  The three-input logic goes
// through plane_solver.h's v_bitop3 helpers (VGPR operands only).
#ifndef SDK_RATE_H
#define SDK_RATE_H

#include "plane_solver.h"

// test-only: the digits, cells and trials in descending order and the trials
// of a sweep all on the sweep's starting state (another schedule of the same
// rules; tests/test_rate_host.py checks that nothing depends on it)
#ifndef SDK_RATE_DESCEND
#define SDK_RATE_DESCEND 0
#endif

namespace rate {

using plane::Board;

enum { MAX_LEVEL = 4, NOT_RUN = -2, INVALID = -1 };
// a pass's verdict: something was removed (pass again); the state is dead;
// nothing to remove and every cell has one candidate; nothing to remove
enum { R_OPEN = 0, R_DEAD = 1, R_SOLVED = 2, R_FIX = 3 };

struct Result {
    int32_t rating;
    int32_t open[MAX_LEVEL];
};

PS_FN constexpr int digit_at(int i) { return SDK_RATE_DESCEND ? 8 - i : i; }

// 3-bit groups of a 9-bit set rotated by one and by two places, together:
// bit i = another bit of i's group is set
PS_FN uint32_t group_others(uint32_t c)
{
    return ((c & 0xDBu) << 1) | ((c & 0x124u) >> 2) | ((c & 0x49u) << 2) | ((c & 0x1B6u) >> 1);
}

// Rule L on one digit's three band words y[] (read only): the cells to clear.
//   o[b]  columns with a place in band b, vp[b] the column of every box of
//         band b whose places lie in one column, mo3 columns with places in
//         two or more bands (all from the caller's unit tallies).
PS_FN void locked(const uint32_t (&y)[3], const uint32_t (&o)[3], const uint32_t (&vp)[3], uint32_t mo3,
                  uint32_t (&clear)[3])
{
    const uint32_t one_band = plane::andn(plane::xor3(o[0], o[1], o[2]), mo3);  // columns with places in one band
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        // box -> column: the column's cells in the other two bands
        uint32_t ec = vp[(b + 1) % 3] | vp[(b + 2) % 3];
        // column -> box: a column whose places lie in this band clears the
        // other two columns of its box here
        ec |= group_others(o[b] & one_band);
        const uint32_t w = y[b];
        // r3: bit 10k + 3j = row k of the band has a place in box j
        const uint32_t r3 = plane::or3(w, w >> 1, w >> 2) & 0x4912449u;
        // box -> row: boxes with places in one row clear that row outside
        // the box; two boxes pointing into one row clear all of it
        const uint32_t a1 = r3 >> 10, a2 = r3 >> 20;
        const uint32_t hbox = plane::box_one(plane::xor3(r3, a1, a2), plane::maj3(r3, a1, a2));
        const uint32_t area = plane::mul24(hbox, 0x701C07u);
        const uint32_t seg = r3 & area;
        const uint32_t rows = plane::guard_rows(plane::row_nonzero(seg));
        const uint32_t rows2 = plane::guard_rows(plane::row_nonzero(seg & (seg + plane::ROWS)));
        // row -> box: a row with places in one box clears the box's other rows
        const uint32_t b1 = r3 >> 3, b2 = r3 >> 6;
        const uint32_t one = plane::andn(plane::xor3(r3, b1, b2), plane::maj3(r3, b1, b2)) & plane::ONES;
        const uint32_t s = r3 & plane::mul24(one, 0x1FFu);
        const uint32_t sc = plane::or3(s, s << 1, s << 2);  // the box's three columns, in the pointing row
        const uint32_t other_rows = (plane::or3(sc >> 10, sc >> 20, sc << 10) | (sc << 20)) & plane::ROWS;
        clear[b] = plane::or3(plane::mul24(ec, 0x100401u), plane::andn(rows, area) | rows2, other_rows);
    }
}

// One pass of the level's rules over the whole board.  open: the cells
// without exactly one candidate in the state the pass started from (the
// state it leaves too when the verdict is R_SOLVED or R_FIX).
PS_FN int pass(Board &B, int level, int &open)
{
    using namespace plane;
    uint32_t single[3];
    uint32_t dead = rule_a(B, single);  // cells with no candidate
    open = 81 - (__builtin_popcount(single[0]) + __builtin_popcount(single[1]) + __builtin_popcount(single[2]));
    const uint32_t mh = level >= 2 ? ~0u : 0u, ml = level >= 3 ? ~0u : 0u;
    // per unit kind, "the digit has a place": row guard bits, columns, box bits 0/3/6
    uint32_t rowall = GUARDS, colall = 0x1FFu, boxall = BOXC;
    uint32_t hall[3] = {0u, 0u, 0u};  // hidden singles placed so far this pass
    uint32_t chg = 0;
    pin_board(B);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int d = digit_at(i);
        uint32_t y[3], x[3], f[3];
        // ---- H of the digits before d: their single places are no place of d
        // ---- N: the cells whose one candidate is d clear d from their peers
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            y[b] = andn(B.P[d][b], hall[b]);
            x[b] = single[b] & y[b];
            const uint32_t s1 = x[b] >> 10, s2 = x[b] >> 20;
            f[b] = or3(x[b], s1, s2) & 0x1FFu;  // columns holding such a cell
            // two of them in one row, column or box of the band empty each other
            dead |= (x[b] & (x[b] + ROWS)) | (maj3(x[b], s1, s2) & 0x1FFu) | (maj3(f[b], f[b] >> 1, f[b] >> 2) & BOXC);
        }
        dead |= maj3(f[0], f[1], f[2]);  // ... or in one column across bands
        const uint32_t cpeer = mul24(or3(f[0], f[1], f[2]), 0x100401u);
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const uint32_t g = or3(f[b], f[b] >> 1, f[b] >> 2) & BOXC;
            const uint32_t peer = or3(guard_rows(row_nonzero(x[b])), cpeer, mul24(g, 0x701C07u));
            y[b] = sel(peer, x[b], y[b]);
        }
        // ---- the units' tallies of d: no place (dead), one place (H), lines of a box (L)
        uint32_t o[3], t[3], gr[3], vp[3], hb[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const uint32_t y1 = y[b] + ROWS;  // row guard set iff the row has a place
            rowall &= y1;
            gr[b] = guard_rows(row_nonzero(y[b] & y1));  // rows with two or more places
            const uint32_t s1 = y[b] >> 10, s2 = y[b] >> 20;
            o[b] = or3(y[b], s1, s2) & 0x1FFu;   // columns with a place in the band
            t[b] = maj3(y[b], s1, s2) & 0x1FFu;  // ... with two or more
            const uint32_t o1 = o[b] >> 1, o2 = o[b] >> 2;
            boxall &= or3(o[b], o1, o2);
            const uint32_t vb = box_one(xor3(o[b], o1, o2), maj3(o[b], o1, o2));  // boxes with places in one column
            vp[b] = o[b] & box_cols(vb);
            hb[b] = andn(vp[b], t[b]);  // ... and one place in it: the box's single place
        }
        const uint32_t O = or3(o[0], o[1], o[2]);
        colall &= O;
        const uint32_t mo3 = maj3(o[0], o[1], o[2]);
        const uint32_t hc = andn2(O, or3(t[0], t[1], t[2]), mo3);  // columns with one place
        // ---- L, from the same tallies
        uint32_t clear[3];
        locked(y, o, vp, mo3, clear);
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            // d's single places in a row, a box or a column
            const uint32_t hs = bop3_nor(gr[b], mul24(hb[b] | hc, 0x100401u), 0u);
            hall[b] = or_and(hall[b], y[b] & hs, mh);
            y[b] = andn_and(y[b], clear[b], ml);
            chg |= B.P[d][b] ^ y[b];
            B.P[d][b] = y[b];
        }
        pin_board(B);
        PS_PIN(rowall);
        PS_PIN(colall);
        PS_PIN(boxall);
        PS_PIN(dead);
        PS_PIN(chg);
#pragma unroll
        for (int b = 0; b < 3; ++b) PS_PIN(hall[b]);
    }
    // H for the digits after: a cell that is some digit's single place has
    // left every plane treated after that digit's; it now leaves every plane
    // treated before it that a later plane still holds.  (A cell that is the
    // single place of two digits kept the earlier one: the later digit's
    // unit has no place left, dead as it must be.)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        uint32_t later = B.P[digit_at(8)][b];
#pragma unroll
        for (int i = 7; i >= 0; --i) {
            const int e = digit_at(i);
            const uint32_t p = andn_and(B.P[e][b], hall[b], later);
            chg |= B.P[e][b] ^ p;
            B.P[e][b] = p;
            later |= p;
        }
    }
    dead |= or3(rowall ^ GUARDS, colall ^ 0x1FFu, boxall ^ BOXC);
    if (dead) return R_DEAD;
    if (chg) return R_OPEN;
    return and3(single[0], single[1], single[2]) == ROWS ? R_SOLVED : R_FIX;
}

// closure of level 1..3: passes until nothing changes or the state is dead
PS_FN int close_level(Board &B, int level, int &open)
{
    for (;;) {
        const int r = pass(B, level, open);
        if (r != R_OPEN) return r;
    }
}
template <int LEVEL>
PS_FN int close(Board &B, int &open)
{
    static_assert(LEVEL >= 1 && LEVEL <= 3, "level 4 is close_trials");
    return close_level(B, LEVEL, open);
}

// Level 4 on a level-3 fixpoint, one board at a time (the host's schedule;
// rate_trial_kernel spreads a sweep's trials over a wave): sweeps over the
// candidates of the cells with two or more, a dead trial's candidate goes and
// level 3 closes the board again, until a sweep removes nothing.
PS_FN int close_trials(Board &B, int &open)
{
    for (;;) {
        bool removed = false;
#if SDK_RATE_DESCEND
        const Board S = B;  // every trial of the sweep from the sweep's start
#endif
        for (int k = 0; k < 81 * 9; ++k) {
            const int kk = SDK_RATE_DESCEND ? 81 * 9 - 1 - k : k;
            const int cell = kk / 9, d = kk % 9;
            const int band = plane::cell_band(cell), pos = plane::cell_pos(cell);
#if SDK_RATE_DESCEND
            const uint32_t c = plane::cell_cand(S, band, pos);
#else
            const uint32_t c = plane::cell_cand(B, band, pos);
#endif
            if (!((c >> d) & 1u) || (c & (c - 1u)) == 0) continue;
#if SDK_RATE_DESCEND
            Board T = S;
#else
            Board T = B;
#endif
            plane::set_cell(T, band, pos, 1u << d);
            int o;
            if (close<3>(T, o) != R_DEAD) continue;
            B.P[d][band] &= ~(1u << pos);
            removed = true;
#if !SDK_RATE_DESCEND
            const int r = close<3>(B, open);
            if (r != R_FIX) return r;
#endif
        }
        if (!removed) return R_FIX;
#if SDK_RATE_DESCEND
        const int r = close<3>(B, open);
        if (r != R_FIX) return r;
#endif
    }
}

PS_FN void start(Result &R)
{
    R.rating = 0;
#pragma unroll
    for (int k = 0; k < MAX_LEVEL; ++k) R.open[k] = NOT_RUN;
}
PS_FN void invalid(Result &R)
{
    R.rating = INVALID;
#pragma unroll
    for (int k = 0; k < MAX_LEVEL; ++k) R.open[k] = INVALID;
}

// Enter the verdict r (never R_OPEN) of closure_level into R; true when the
// board's rating is settled, false when level + 1 has to run.
PS_FN bool settle(Result &R, int level, int r, int open, int max_level)
{
    if (r == R_FIX) {
#pragma unroll
        for (int k = 1; k <= MAX_LEVEL; ++k) {
            // (a masked select, not open[level - 1]: indexed by a lane's own level the entries would live in scratch)
            const int32_t m = -(int32_t)(k == level);
            R.open[k - 1] = (open & m) | (R.open[k - 1] & ~m);
        }
        R.rating = max_level + 1;
        return level == max_level;
    }
    R.rating = r == R_DEAD ? 0 : level;
#pragma unroll
    for (int k = 1; k <= MAX_LEVEL; ++k)
        if (k >= level && k <= max_level) R.open[k - 1] = r == R_DEAD ? -1 : 0;
    return true;
}

// Host / reference driver: B = the start state of a board (plane::
// planes_from_slices); on return the deepest closure computed (meaningless
// when R.rating == 0: the marks of a dead closure are zero).
PS_FN void rate_board(Board &B, int max_level, Result &R)
{
    start(R);
    int open = 0;  // (close_trials leaves level 3's count where no trial dies)
    for (int level = 1; level <= max_level; ++level) {
        const int r = level <= 3 ? close_level(B, level, open) : close_trials(B, open);
        if (settle(R, level, r, open, max_level)) return;
    }
}

// the start state from a board's 21 words (plane::load_words' input, without
// its test of the givens: N deals with givens that repeat a digit).  False
// for a byte > 9.
PS_FN bool load(Board &B, const uint32_t (&x)[21])
{
    uint32_t V[4][3], given[3];
    const uint32_t bad = plane::slices_from_words(x, V);
    plane::planes_from_slices(B, V, given);
    return bad == 0;
}

// marks: per cell, bit d-1 set when d is a candidate, through put(cell, mask)
template <typename Put>
PS_FN void store_marks(const Board &B, uint32_t keep, Put put)
{
#pragma unroll
    for (int i = 0; i < 81; ++i) {
        const int b = plane::cell_band(i), p = plane::cell_pos(i);
        uint32_t m = 0;
#pragma unroll
        for (int d = 8; d >= 0; --d) m = m + m + ((B.P[d][b] >> p) & 1u);
        put(i, m & keep);
    }
}

}  // namespace rate

#endif  // SDK_RATE_H
