// hit.h -- the k-cell hitting sets of a family of cell sets.  DESIGN.md §25
// is the specification; in short, a FAMILY is a list of 81-bit cell sets F, an
// allowed mask A and a required mask R, and a ROW at size k is a set S with
// R <= S <= A, |S| = k and S & U != 0 for every U in F.  The rows are a set,
// each listed once, a function of (F as a set of masks, A, R, k) alone.
//
// The search: the state is the chosen cells C (they contain R), the dead
// cells X and a stack of one level per cell chosen beyond R.  A node scans the
// family from its parent's set on for the first set U with U & C == 0 (every
// set before it is hit, so the scan along a path is linear in the family):
//   - such a U and no clue left: the branch ends;
//   - such a U: its cells (U & A) \ X in ascending order u_0 < u_1 < ...;
//     branch j chooses u_j and makes u_0 .. u_{j-1} dead below it;
//   - no such U: the r clues left are every r-subset of A \ C \ X, walked in
//     ascending cell order (a FREE level takes a cell above its parent's).
// Every S is reached once: at every set node the branch taken is the least
// cell of U \ X that S holds (§25 proves it).  One prune that removes only
// branches without a row (SDK_HIT_PRUNE=0 switches it off): past U the scan
// packs unhit sets greedily, each restricted to A \ X and disjoint from those
// taken, over the next SDK_HIT_PRUNE_WINDOW sets; a set with no cell left, or
// more packed sets than clues left, ends the branch.
//
// Cell c is bit c & 31 of word c >> 5 in every mask.  A level is four stack
// words: the set's index (FREE: a free level), the cells the level made dead
// (three words, undone exactly when it leaves), and in the third word's spare
// bits the cell it holds now.  Where the stack, the family and A live is the
// caller's: `Mem` hands them out (LDS and global memory on the GPU, arrays on
// the host).  step() is ONE node, so lanes of a wave advance tasks of their
// own side by side; the mask updates are selects on the word index, never
// branches.
//
// Plain C++ for host and device: tests/native/hit_host.cpp compiles it with
// g++, hit_kernels.hip runs it on the GPU.
#ifndef SDK_HIT_H
#define SDK_HIT_H

#include <stdint.h>

#ifndef PS_FN
#ifdef __HIPCC__
#define PS_FN __host__ __device__ __forceinline__
#else
#define PS_FN static inline
#endif
#endif

#ifndef SDK_HIT_PRUNE
#define SDK_HIT_PRUNE 1
#endif
#ifndef SDK_HIT_PRUNE_WINDOW
#define SDK_HIT_PRUNE_WINDOW 48  // sets past the first unhit one that the packing looks at
#endif

namespace hit {

enum { MAX_CLUES = 32, DONE = 1, LIMITED = 2, INVALID = -1 };
enum { NO_CELL = 127, COARSE = 81, FINE = 81 * 81 };
constexpr uint32_t FREE = 0xFFFFFFFFu;
constexpr uint64_t COUNT_MAX = 0x7FFFFFFFFFFFFFFFull;

PS_FN int popc(uint32_t x) { return __builtin_popcount(x); }
PS_FN int popc3(const uint32_t *m) { return popc(m[0]) + popc(m[1]) + popc(m[2]); }

// the bit of cell c in word w (0 in the other words; NO_CELL: bit 31 of word 3, never asked for)
PS_FN uint32_t bitw(int c, int w) { return (c >> 5) == w ? 1u << (c & 31) : 0u; }

// the cells above c in word w (c = -1: every cell)
PS_FN uint32_t above(int c, int w)
{
    const int t = c + 1 - 32 * w;  // the first cell wanted, counted from the word's first
    return t <= 0 ? 0xFFFFFFFFu : t >= 32 ? 0u : 0xFFFFFFFFu << t;
}

PS_FN int lowest(const uint32_t *m)
{
    return m[0] ? __builtin_ctz(m[0]) : m[1] ? 32 + __builtin_ctz(m[1]) : m[2] ? 64 + __builtin_ctz(m[2]) : (int)NO_CELL;
}

// C(n, r), COUNT_MAX where it does not fit an int64 (n <= 81)
PS_FN uint64_t binomial(int n, int r)
{
    if (r < 0 || r > n) return 0;
    if (r > n - r) r = n - r;
    uint64_t v = 1;
    for (int i = 1; i <= r; ++i) {
        // v is C(n - r + i - 1, i - 1), so v m / i is whole: with v = q i + t it is q m + t m / i
        const uint64_t m = (uint64_t)(n - r + i), q = v / (uint64_t)i, t = v % (uint64_t)i;
        if (q > (COUNT_MAX - 81u * 81u) / m) return COUNT_MAX;
        v = q * m + t * m / (uint64_t)i;
    }
    return v;
}

// The status of a family's masks: INVALID for a bit at or above 81 in A or R,
// or R not inside A.
PS_FN int validate(const uint32_t *A, const uint32_t *R)
{
    const bool bad = ((A[2] | R[2]) >> 17) != 0u || ((R[0] & ~A[0]) | (R[1] & ~A[1]) | (R[2] & ~A[2])) != 0u;
    return bad ? (int)INVALID : (int)DONE;
}

struct State {
    uint32_t C[3];  // the chosen cells
    uint32_t X[3];  // the dead cells
    int32_t depth;  // levels on the stack; 0: no task
    int32_t k;
    int32_t only0;  // a task: the one cell level 0 takes
    int32_t only1;  // a fine task: the one cell level 1 takes; -1: all of them
    int32_t count_only;  // a free leaf adds its binomial instead of being walked
};

// a level's fourth word: the dead cells of word 2, the cell held (NO_CELL:
// none; on a free level not yet chosen: the floor) and whether one is chosen
PS_FN uint32_t tail(uint32_t a2, int cell, bool chosen) { return a2 | (uint32_t)cell << 17 | (chosen ? 1u << 24 : 0u); }

// Sets first .. first + BATCH - 1 of the family, the loads independent of one
// another (an index past the family reads its last set again; the caller
// ignores it).  nsets >= 1.
enum { BATCH = 8 };
template <class M>
PS_FN void load_batch(const M &mem, uint32_t first, uint32_t nsets, uint32_t (&b)[BATCH][3])
{
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
        const uint32_t i = first + (uint32_t)j;
        mem.load(i < nsets ? i : nsets - 1u, b[j]);
    }
}

// The node below a choice (or the root): scans from set `from` (FREE: every
// set is hit), cells above `floor` for a free level.  Returns the rows found
// here (1: S.C is one; in count_only also a leaf's binomial) and pushes the
// node's level `level` when it has branches.
template <class M>
PS_FN uint64_t descend(State &S, M &mem, int level, uint32_t from, int floor, bool prune)
{
    const int r = S.k - popc3(S.C);
    const uint32_t nsets = mem.nsets();
    uint32_t idx = from;
    uint32_t u[3] = {0u, 0u, 0u};
    if (from != FREE) {
        bool found = false;
        while (idx < nsets && !found) {  // BATCH loads in flight, then the first unhit set among them
            uint32_t b[BATCH][3];
            load_batch(mem, idx, nsets, b);
            int sel = BATCH;
#pragma unroll
            for (int j = BATCH - 1; j >= 0; --j) {
                const bool unhit = idx + (uint32_t)j < nsets && !((b[j][0] & S.C[0]) | (b[j][1] & S.C[1]) | (b[j][2] & S.C[2]));
                sel = unhit ? j : sel;
#pragma unroll
                for (int w = 0; w < 3; ++w) u[w] = unhit ? b[j][w] : u[w];
            }
            found = sel < BATCH;
            idx += (uint32_t)sel;
        }
        if (!found) idx = FREE, floor = -1;
    }
    if (idx == FREE) {  // every set is hit: the clues left are free
        if (r == 0) return 1;
        uint32_t rest[3];
#pragma unroll
        for (int w = 0; w < 3; ++w) rest[w] = mem.allowed(w) & ~S.C[w] & ~S.X[w] & above(floor, w);
        const int n = popc3(rest);
        if (n < r) return 0;
        if (S.count_only) return binomial(n, r);
        mem.stk(level, 0) = FREE;
        mem.stk(level, 3) = tail(0u, floor < 0 ? (int)NO_CELL : floor, false);
        S.depth = level + 1;
        return 0;
    }
    if (r == 0) return 0;
#if SDK_HIT_PRUNE
    if (prune) {
        uint32_t P[3];
#pragma unroll
        for (int w = 0; w < 3; ++w) P[w] = u[w] & mem.allowed(w) & ~S.X[w];
        if (!(P[0] | P[1] | P[2])) return 0;
        int packed = 1;
        const uint32_t end = nsets - idx - 1u > (uint32_t)SDK_HIT_PRUNE_WINDOW ? idx + 1u + SDK_HIT_PRUNE_WINDOW : nsets;
        for (uint32_t j0 = idx + 1u; j0 < end; j0 += BATCH) {
            uint32_t b[BATCH][3];
            load_batch(mem, j0, nsets, b);
#pragma unroll
            for (int j = 0; j < BATCH; ++j) {
                uint32_t v[3];
#pragma unroll
                for (int w = 0; w < 3; ++w) v[w] = b[j][w] & mem.allowed(w) & ~S.X[w];
                const bool unhit = j0 + (uint32_t)j < end && !((b[j][0] & S.C[0]) | (b[j][1] & S.C[1]) | (b[j][2] & S.C[2]));
                if (unhit && !(v[0] | v[1] | v[2])) return 0;  // an unhit set with no cell left
                const bool take = unhit && !((v[0] & P[0]) | (v[1] & P[1]) | (v[2] & P[2]));
#pragma unroll
                for (int w = 0; w < 3; ++w) P[w] |= take ? v[w] : 0u;
                packed += take ? 1 : 0;
            }
            if (packed > r) return 0;
        }
    }
#else
    (void)prune;
#endif
    mem.stk(level, 0) = idx;
    mem.stk(level, 1) = 0u;
    mem.stk(level, 2) = 0u;
    mem.stk(level, 3) = tail(0u, NO_CELL, false);
    S.depth = level + 1;
    return 0;
}

// One node of a running task (depth >= 1): the top level drops its cell and
// takes its next one, or leaves the stack.  Returns the rows found (see
// descend).
template <class M>
PS_FN uint64_t step(State &S, M &mem)
{
    const int level = S.depth - 1;
    const uint32_t idx = mem.stk(level, 0);
    const bool free_ = idx == FREE;
    const uint32_t e = mem.stk(level, 3);
    uint32_t a[3] = {free_ ? 0u : mem.stk(level, 1), free_ ? 0u : mem.stk(level, 2), e & 0x1FFFFu};
    const int cell = (int)((e >> 17) & 127u);
    const bool chosen = ((e >> 24) & 1u) != 0u;
    if (chosen) {  // the cell leaves C and, on a set level, is dead for the later branches
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const uint32_t b = bitw(cell, w);
            S.C[w] &= ~b;
            S.X[w] |= free_ ? 0u : b;
            a[w] |= free_ ? 0u : b;
        }
    }
    const int floor = cell == (int)NO_CELL ? -1 : cell;
    uint32_t u[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (!free_) mem.load(idx, u);
    uint32_t cand[3];
#pragma unroll
    for (int w = 0; w < 3; ++w) cand[w] = u[w] & mem.allowed(w) & ~S.C[w] & ~S.X[w] & above(floor, w);
    const int only = level == 0 ? S.only0 : level == 1 ? S.only1 : -1;
    if (only >= 0) {  // a task's level: its one cell, the candidates below it dead
        const bool has = !chosen && (((cand[0] & bitw(only, 0)) | (cand[1] & bitw(only, 1)) | (cand[2] & bitw(only, 2))) != 0u);
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const uint32_t low = has && !free_ ? cand[w] & ~above(only - 1, w) : 0u;
            S.X[w] |= low;
            a[w] |= low;
            cand[w] = has ? bitw(only, w) : 0u;
        }
    }
    const int c = lowest(cand);
    if (c == (int)NO_CELL || (free_ && only < 0 && popc3(cand) < S.k - popc3(S.C))) {
#pragma unroll
        for (int w = 0; w < 3; ++w) S.X[w] &= ~a[w];
        S.depth = level;
        return 0;
    }
#pragma unroll
    for (int w = 0; w < 3; ++w) S.C[w] |= bitw(c, w);
    if (!free_) {
        mem.stk(level, 1) = a[0];
        mem.stk(level, 2) = a[1];
    }
    mem.stk(level, 3) = tail(a[2], c, true);
    return descend(S, mem, level + 1, free_ ? FREE : idx + 1u, c, true);
}

// Begin task (c1, c2) of the family `mem` describes, with required cells R:
// level 0 takes cell c1 alone and level 1 cell c2 alone (c2 < 0: a coarse
// task, level 1 takes every cell).  The tasks of a family, c1 = 0..80 and for
// a fine cut c2 = 0..80 as well, walk disjoint subtrees that cover the tree:
// what the root itself, or the node below c1 of a fine task, yields without a
// level belongs to the task with c1 = 0, or c2 = 0.  Returns like step();
// depth stays 0 when the task ends at once.
template <class M>
PS_FN uint64_t start(State &S, M &mem, const uint32_t *R, int k, int c1, int c2, int count_only)
{
#pragma unroll
    for (int w = 0; w < 3; ++w) S.C[w] = R[w], S.X[w] = 0u;
    S.depth = 0;
    S.k = k;
    S.only0 = c1;
    S.only1 = c2;
    S.count_only = count_only;
    if (k < popc3(R)) return 0;
    uint64_t add = descend(S, mem, 0, 0u, -1, false);
    if (S.depth == 0) return c1 == 0 && c2 <= 0 ? add : 0;
    add = step(S, mem);
    if (S.depth < 2) {  // no level 1: the task is over
        S.depth = 0;
        if (c2 > 0) add = 0;
    }
    return add;
}

#ifndef __HIP_DEVICE_COMPILE__
// ------------------------------------------------------------- host model
struct HostMem {
    const uint32_t *sets;  // the family's rows of four words
    uint32_t n;
    uint32_t A[3];
    uint32_t s[MAX_CLUES][4];
    uint32_t nsets() const { return n; }
    void load(uint32_t i, uint32_t *u) const { u[0] = sets[4 * (uint64_t)i], u[1] = sets[4 * (uint64_t)i + 1], u[2] = sets[4 * (uint64_t)i + 2]; }
    uint32_t allowed(int w) const { return A[w]; }
    uint32_t &stk(int l, int j) { return s[l][j]; }
};

// Every row of one family (status DONE), task by task: emit(C) per row, or
// emit(NULL, add) per count in count_only.  `limit` > 0 stops after that many
// rows.  Returns the nodes of the walk: the start() and step() calls.
template <class E>
static inline uint64_t host_family(const uint32_t *sets, int64_t nsets, const uint32_t *A, const uint32_t *R, int k,
                                   bool fine, bool count_only, int64_t limit, E emit)
{
    HostMem mem;
    mem.sets = sets, mem.n = (uint32_t)nsets;
    for (int w = 0; w < 3; ++w) mem.A[w] = A[w];
    uint64_t nodes = 0;
    int64_t rows = 0;
    for (int t = 0; t < (fine ? (int)FINE : (int)COARSE); ++t) {
        State S;
        uint64_t add = start(S, mem, R, k, fine ? t / 81 : t, fine ? t % 81 : -1, count_only);
        ++nodes;
        for (;;) {
            if (add) {
                emit(S.C, add);
                rows += (int64_t)add;
                if (limit > 0 && rows >= limit) return nodes;
            }
            if (!S.depth) break;
            add = step(S, mem);
            ++nodes;
        }
    }
    return nodes;
}
#endif

}  // namespace hit

#endif  // SDK_HIT_H
