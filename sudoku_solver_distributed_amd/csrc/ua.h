// ua.h -- the unavoidable sets of a solution grid, by a depth-bounded repair
// search.  DESIGN.md §24 is the specification; in short, for a valid grid g
// and a size m: a NEIGHBOUR is a valid grid g' != g, D(g') the cells where it
// differs; two cells of D are LINKED when they are peers and one's new digit
// is the other's old one; a ROW is the D of a neighbour with |D| <= m whose D
// is connected under links.  Every minimal unavoidable set of at most m cells
// is the D of a row (§24 proves it), so the rows, filtered to those without a
// proper subset among them, are exactly the minimal sets.
//
// The search: a TASK is (seed cell s, seed digit d != g[s]).  The state is the
// changed cells D with their new digits and the PENDING cells: unchanged cells
// whose digit a changed peer now holds, which therefore must change.  A step
// takes the lowest pending cell c and gives it every digit that is neither
// g[c] nor held by a changed peer; the unchanged peers of c that hold the new
// digit in g -- pos_g[d] & peers[c], at most three -- become pending.  A
// pending cell below the seed ends the branch (the seed is the least cell of
// D, so each connected neighbour is met once, from its least cell), and so
// does |D| + |pending| > m.  No pending cell left: D is a row.
//
// Cell c is bit c & 31 of word c >> 5 in every 81-bit mask here.  The state
// of a task is six mask words and a stack of one word and one 16-bit digit
// set per changed cell; where they live is the caller's: `Mem` hands out the
// grid's nine digit masks, the peer table and the stack (LDS on the GPU,
// plain arrays on the host).  step() is ONE node of the walk, so lanes of a
// wave advance tasks of their own side by side.
//
// Plain C++ for host and device: tests/native/ua_host.cpp compiles it with
// g++, ua_kernels.hip runs it on the GPU.
#ifndef SDK_UA_H
#define SDK_UA_H

#include <stdint.h>

#ifndef PS_FN
#ifdef __HIPCC__
#define PS_FN __host__ __device__ __forceinline__
#else
#define PS_FN static inline
#endif
#endif

namespace ua {

enum { MIN_SIZE = 4, MAX_SIZE = 16, TASKS = 648, SPLIT = 8, DONE = 1, INVALID = -1, NOT_A_GRID = -2 };
enum { NO_CELL = 127 };

PS_FN int popc(uint32_t x) { return __builtin_popcount(x); }

// the 20 peers of cell c
PS_FN void peer_mask(int c, uint32_t (&out)[3])
{
    const int r = c / 9, k = c % 9;
    uint32_t o0 = 0u, o1 = 0u, o2 = 0u;
    for (int a = 0; a < 81; ++a) {
        const int ra = a / 9, ka = a % 9;
        if (a != c && (ra == r || ka == k || (ra / 3 == r / 3 && ka / 3 == k / 3))) {
            const uint32_t bit = 1u << (a & 31);
            o0 |= a < 32 ? bit : 0u;
            o1 |= a >= 32 && a < 64 ? bit : 0u;
            o2 |= a >= 64 ? bit : 0u;
        }
    }
    out[0] = o0, out[1] = o1, out[2] = o2;
}

// The status of the 81 bytes byte_at(0..80): INVALID for a byte outside 1..9,
// NOT_A_GRID when a digit repeats in a row, column or box, DONE otherwise.
template <class F>
PS_FN int validate(F byte_at)
{
    bool bad = false;
    for (int c = 0; c < 81; ++c) {
        const uint32_t v = byte_at(c);
        bad |= v < 1u || v > 9u;
    }
    if (bad) return INVALID;
    bool rep = false;
    for (int u = 0; u < 9; ++u) {
        uint32_t row = 0, col = 0, box = 0;
        for (int k = 0; k < 9; ++k) {
            row |= 1u << byte_at(9 * u + k);
            col |= 1u << byte_at(9 * k + u);
            box |= 1u << byte_at(27 * (u / 3) + 3 * (u % 3) + 9 * (k / 3) + k % 3);
        }
        rep |= row != 0x3FEu || col != 0x3FEu || box != 0x3FEu;
    }
    return rep ? NOT_A_GRID : DONE;
}

// word w of the cells that hold digit d (1..9)
template <class F>
PS_FN uint32_t digit_word(F byte_at, int d, int w)
{
    uint32_t m = 0;
    const int end = w == 2 ? 81 : 32 * w + 32;
    for (int c = 32 * w; c < end; ++c) m |= (uint32_t)(byte_at(c) == (uint32_t)d) << (c & 31);
    return m;
}

// a stack entry: the level's cell, its digit now (0: none tried yet) and the
// cells that digit made pending (NO_CELL in the unused places)
PS_FN uint32_t entry(int c, int d, uint32_t made) { return (uint32_t)c | (uint32_t)d << 7 | made << 11; }
constexpr uint32_t MADE_NONE = NO_CELL | NO_CELL << 7 | NO_CELL << 14;

struct State {
    uint32_t D[3];  // the changed cells
    uint32_t P[3];  // the pending cells
    int32_t seed;
    int32_t depth;  // levels on the stack; 0: no task
    int32_t max_size;
    int32_t only;   // a split task: the one digit level 1 takes; 0: all of them
};

template <class M>
PS_FN int digit_of(M &mem, int c)
{
    int d = 0;
    for (int k = 0; k < 9; ++k) d += (int)((mem.gm(k, c >> 5) >> (c & 31)) & 1u) * (k + 1);
    return d;
}

// Level `level`'s cell c takes digit d.  Returns 1 when D is a row now.
template <class M>
PS_FN int place(State &S, M &mem, int level, int c, int d)
{
    uint32_t nw[3];
    uint32_t low = 0;
    const int sw = S.seed >> 5;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        nw[w] = mem.gm(d - 1, w) & mem.peer(c, w) & ~S.D[w] & ~S.P[w];
        const uint32_t below = w < sw ? 0xFFFFFFFFu : w == sw ? (1u << (S.seed & 31)) - 1u : 0u;
        low |= nw[w] & below;
    }
    if (low) {  // a cell below the seed would have to change
        mem.stk(level) = entry(c, d, MADE_NONE);
        return 0;
    }
    uint32_t made = 0;
    int k = 0;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        uint32_t x = nw[w];
        while (x) {  // (three cells at the most: one a row, a column and a box)
            made |= (uint32_t)(32 * w + __builtin_ctz(x)) << (7 * k++);
            x &= x - 1u;
        }
        S.P[w] |= nw[w];
    }
    for (; k < 3; ++k) made |= (uint32_t)NO_CELL << (7 * k);
    mem.stk(level) = entry(c, d, made);
    const int cells = popc(S.D[0]) + popc(S.D[1]) + popc(S.D[2]) + popc(S.P[0]) + popc(S.P[1]) + popc(S.P[2]);
    if (cells > S.max_size) return 0;
    if (!(S.P[0] | S.P[1] | S.P[2])) return 1;
    // the lowest pending cell is the next level; the digits it cannot take
    const int w2 = S.P[0] ? 0 : S.P[1] ? 1 : 2;
    const int c2 = 32 * w2 + __builtin_ctz(S.P[0] ? S.P[0] : S.P[1] ? S.P[1] : S.P[2]);
    const uint32_t bit = 1u << (c2 & 31);
#pragma unroll
    for (int w = 0; w < 3; ++w) {  // (selects, not branches: the masks stay in registers)
        const uint32_t hit = w == w2 ? bit : 0u;
        S.P[w] &= ~hit;
        S.D[w] |= hit;
    }
    uint32_t taken = 1u << (digit_of(mem, c2) - 1);
    for (int l = 0; l <= level; ++l) {
        const uint32_t e = mem.stk(l);
        const int a = (int)(e & 127u);
        if ((mem.peer(c2, a >> 5) >> (a & 31)) & 1u) taken |= 1u << (((e >> 7) & 15u) - 1u);
    }
    mem.fb(level + 1) = (uint16_t)taken;
    mem.stk(level + 1) = entry(c2, 0, MADE_NONE);
    S.depth = level + 2;
    return 0;
}

// Begin task (seed, k): the seed takes the k-th digit (k = 0..7) that is not
// its own.  depth stays 0 when the task ends at once.  k2 = 0..7 makes it a
// SPLIT task, an eighth of that one: level 1 -- the seed's lowest pending
// cell, whose own digit is the seed's new one -- takes only the k2-th digit
// that is not its own (k2 < 0: all of them).  The eight split tasks of a task
// walk its subtrees, each once: the rows are the same.
template <class M>
PS_FN void start(State &S, M &mem, int seed, int k, int k2, int max_size)
{
    const int own = digit_of(mem, seed);
    const int d = k + 1 + (k + 1 >= own ? 1 : 0);
    S.only = k2 < 0 ? 0 : k2 + 1 + (k2 + 1 >= d ? 1 : 0);
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        S.D[w] = w == (seed >> 5) ? 1u << (seed & 31) : 0u;
        S.P[w] = 0u;
    }
    S.seed = seed;
    S.max_size = max_size;
    S.depth = 1;
    place(S, mem, 0, seed, d);  // (never a row: the seed's digit stands elsewhere in its row)
    if (S.depth != 2) S.depth = 0;
}

// One node of a running task (depth >= 1): the top level drops its digit and
// takes its next one, or leaves the stack.  Returns 1 when S.D is a row.
template <class M>
PS_FN int step(State &S, M &mem)
{
    const int level = S.depth - 1;
    if (level == 0) {  // back at the seed: the task is over
        S.depth = 0;
        return 0;
    }
    const uint32_t e = mem.stk(level);
    const int c = (int)(e & 127u), d = (int)((e >> 7) & 15u);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint32_t a = (e >> (11 + 7 * j)) & 127u;
        const uint32_t bit = a == (uint32_t)NO_CELL ? 0u : 1u << (a & 31u);
#pragma unroll
        for (int w = 0; w < 3; ++w) S.P[w] &= ~((a >> 5) == (uint32_t)w ? bit : 0u);
    }
    uint32_t avail = ~(uint32_t)mem.fb(level) & 0x1FFu & (0x1FFu << d);  // digits above d
    if (level == 1 && S.only) avail = d ? 0u : avail & (1u << (S.only - 1));
    if (!avail) {  // the cell goes back among the pending ones
        const uint32_t bit = 1u << (c & 31);
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const uint32_t hit = (c >> 5) == w ? bit : 0u;
            S.D[w] &= ~hit;
            S.P[w] |= hit;
        }
        S.depth = level;
        return 0;
    }
    return place(S, mem, level, c, __builtin_ctz(avail) + 1);
}

// keep[k] of the filter entry by its definition: no row of the group is a
// proper subset of row k, and no row of lower index equals it (rows: four
// words each, the fourth ignored)
PS_FN bool subset_of(const uint32_t *a, const uint32_t *b)
{
    return !((a[0] & ~b[0]) | (a[1] & ~b[1]) | (a[2] & ~b[2]));
}
PS_FN bool same_cells(const uint32_t *a, const uint32_t *b)
{
    return a[0] == b[0] && a[1] == b[1] && a[2] == b[2];
}

#ifndef __HIP_DEVICE_COMPILE__
// ------------------------------------------------------------- host model
struct HostMem {
    uint32_t g[27];
    uint32_t p[81][3];
    uint32_t s[MAX_SIZE];
    uint16_t f[MAX_SIZE];
    uint32_t gm(int k, int w) const { return g[3 * k + w]; }
    uint32_t peer(int c, int w) const { return p[c][w]; }
    uint32_t &stk(int l) { return s[l]; }
    uint16_t &fb(int l) { return f[l]; }
};

// Every row of `grid` (status DONE) at max_size, task by task in cell order:
// emit(D) per row.  Returns the nodes of the walk (place() calls).  split:
// every task as its eight split tasks (the same rows; the seed's digit is
// then placed eight times).
template <class E>
static inline uint64_t host_grid(const uint8_t *grid, int max_size, E emit, bool split = false)
{
    HostMem mem;
    auto byte_at = [&](int c) { return (uint32_t)grid[c]; };
    for (int d = 1; d <= 9; ++d)
        for (int w = 0; w < 3; ++w) mem.g[3 * (d - 1) + w] = digit_word(byte_at, d, w);
    for (int c = 0; c < 81; ++c) peer_mask(c, mem.p[c]);
    uint64_t nodes = 0;
    for (int t = 0; t < (split ? TASKS * SPLIT : TASKS); ++t) {
        State S;
        if (split)
            start(S, mem, t >> 6, (t >> 3) & 7, t & 7, max_size);
        else
            start(S, mem, t >> 3, t & 7, -1, max_size);
        ++nodes;
        while (S.depth) {
            const int before = S.depth;
            if (step(S, mem)) emit(S.D);
            if (S.depth >= before && before > 1) ++nodes;  // (a level that left the stack placed nothing)
        }
    }
    return nodes;
}
#endif

}  // namespace ua

#endif  // SDK_UA_H
