// canon.h -- canonical (minlex) form of a board under Sudoku's symmetries.
//
// Board: 81 bytes, row-major, values 0..9 (validity plays no part).
// Line permutation p in [0, 1296): p = ((bp*6 + a)*6 + b)*6 + d, with
// PERM3 = {012, 021, 102, 120, 201, 210} and in = (a, b, d):
//     perm_p[k] = 3*PERM3[bp][k/3] + PERM3[in[k/3]][k%3]
// Symmetry sym = (t*1296 + ri)*1296 + ci, t in {0, 1}, R = perm_ri,
// C = perm_ci: image cell (i, j) = g[R[i]][C[j]] (t == 0) or g[C[j]][R[i]]
// (t == 1); the image's non-zero digits are then relabelled 1, 2, ... in
// order of first appearance (row-major), zeros stay.
//     canon(g) = the smallest image (bytes compared 0 < 1 < ... < 9)
//     sym(g)   = the smallest sym whose image is canon(g)
//     autos(g) = the number of sym whose image is canon(g)
// -- scripts/hard17/hard17_search.c canon(), bit for bit.
//
// The search is exhaustive with exact pruning only.  A "row variant" is
// rv = t*1296 + ri.  The 36 consecutive rv of a BLOCK share (t, bp, a); the
// blocks of bp = 2k and 2k + 1 both put band k first, so the two of them (a
// SUPER-BLOCK: t, k, a) share the image's first three rows; the six rv of a
// (block, b) share rows 3..5.  One (super-block, ci) is walked as prefix(),
// rows 0..2 once, then complete() for each of its twelve (bp, b): rows 3..5
// once, rows 6..8 per d, the digit map carried along; a level is left as soon
// as the rows so far are GREATER than the running best's.  A second prune
// works across the searchers of one board: `key` is the smallest 16-cell
// prefix (row 0 and seven cells of row 1, 64 bits) any of them has met; a
// prefix that is strictly greater cannot start the canon.  Only strictly
// greater candidates are ever dropped, so every tie survives.
//
// Plain C++ for host and device, like plane_count.h: the CPU tests compile
// it with g++ (tests/native/canon_host.cpp).
#ifndef SDK_CANON_H
#define SDK_CANON_H

#include <stdint.h>

#ifndef PS_FN
#ifdef __HIPCC__
#define PS_FN __host__ __device__ __forceinline__
#else
#define PS_FN static inline
#endif
#endif

namespace canon {

enum {
    LINE_PERMS = 1296,
    ROW_VARIANTS = 2592,      // t*1296 + ri
    SYMMETRIES = 3359232,     // 2 * 1296 * 1296
    BLOCK = 36,               // row variants that share (t, bp, a)
    SUPER_BLOCKS = 36,        // (t, first band, a): two blocks each
    RECORD_WORDS = 16,        // a packed partial record: 64 bytes
    STAGE_BYTES = 162,        // the board and its transpose
};

// PERM3[p][k], the three columns of the table as 2-bit fields
PS_FN int perm3(int p, int k)
{
    const uint32_t T0 = 0u | 0u << 2 | 1u << 4 | 1u << 6 | 2u << 8 | 2u << 10;
    const uint32_t T1 = 1u | 2u << 2 | 0u << 4 | 2u << 6 | 0u << 8 | 1u << 10;
    const uint32_t T2 = 2u | 1u << 2 | 2u << 4 | 0u << 6 | 1u << 8 | 0u << 10;
    const uint32_t T = k == 0 ? T0 : k == 1 ? T1 : T2;
    return (int)((T >> (2 * p)) & 3u);
}

// perm_p[0..8]
PS_FN void line_perm(int p, int (&out)[9])
{
    const int in[3] = {(p / 36) % 6, (p / 6) % 6, p % 6};
    const int bp = p / 216;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = 3 * perm3(bp, k / 3) + perm3(in[k / 3], k % 3);
}

// The board and its transpose, so that image cell (i, j) is
// bt[81*t + 9*R[i] + C[j]] for both t.  false: a byte > 9.
PS_FN bool stage(const uint8_t *g, uint8_t *bt)
{
    bool ok = true;
    for (int i = 0; i < 81; ++i) {
        const uint8_t x = g[i];
        ok = ok && x <= 9;
        bt[i] = x;
        bt[81 + 9 * (i % 9) + i / 9] = x;
    }
    return ok;
}

// One image row: the source row's cells gathered through C and relabelled.
// map: nibble x = the label of source digit x (0: none yet; nibble 0 stays
// 0, so an empty cell maps to 0), nine nibbles in use; next: the next label.
// The row comes back as nine nibbles, cell 0 in the most significant.
PS_FN uint64_t image_row(const uint8_t *src, const int (&C)[9], uint64_t &map, uint32_t &next)
{
    uint32_t head = 0, m = 0;  // cells 0..7, then cell 8
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const uint32_t x = src[C[j]], sh = 4u * x;
        head = head << 4 | m;
        m = (uint32_t)(map >> sh) & 15u;
        const bool fresh = x != 0u && m == 0u;
        m = fresh ? next : m;
        map |= fresh ? (uint64_t)next << sh : 0ull;
        next += fresh ? 1u : 0u;
    }
    return (uint64_t)head << 4 | m;
}

// A partial result: the smallest image met (nine rows of nine nibbles), the
// smallest sym that gave it and how many did.  Empty: rows all ones (greater
// than any image row), no ties.
struct Record {
    uint64_t row[9];
    uint32_t sym, ties;
};

PS_FN void clear(Record &r)
{
#pragma unroll
    for (int i = 0; i < 9; ++i) r.row[i] = 0xFFFFFFFFFull;  // survives pack / unpack as it is
    r.sym = ~0u;
    r.ties = 0u;
}

// rows a[0..2] against b[0..2]: < 0, 0, > 0
PS_FN int cmp3(const uint64_t *a, const uint64_t *b)
{
    if (a[0] != b[0]) return a[0] < b[0] ? -1 : 1;
    if (a[1] != b[1]) return a[1] < b[1] ? -1 : 1;
    if (a[2] != b[2]) return a[2] < b[2] ? -1 : 1;
    return 0;
}

// smaller canon wins; on equal canon the ties add up and the smaller sym stays
PS_FN void merge(Record &a, const Record &b)
{
    int c = cmp3(a.row, b.row);
    if (c == 0) c = cmp3(a.row + 3, b.row + 3);
    if (c == 0) c = cmp3(a.row + 6, b.row + 6);
    if (c > 0) {
        a = b;
    } else if (c == 0) {
        a.ties += b.ties;
        a.sym = b.sym < a.sym ? b.sym : a.sym;
    }
}

// 64 bytes: words 0..8 = cells 0..7 of each row, word 9 = cell 8 of rows
// 0..7, word 10 = cell 8 of row 8, word 11 = sym, word 12 = ties, word 13 =
// 1 for a board with a byte > 9 (no search was done), words 14..15 zero.
PS_FN void pack(const Record &r, uint32_t (&w)[RECORD_WORDS])
{
    uint32_t last = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        w[i] = (uint32_t)(r.row[i] >> 4);
        if (i < 8) last = last << 4 | ((uint32_t)r.row[i] & 15u);
    }
    w[9] = last;
    w[10] = (uint32_t)r.row[8] & 15u;
    w[11] = r.sym;
    w[12] = r.ties;
    w[13] = w[14] = w[15] = 0u;
}

PS_FN void unpack(const uint32_t *w, Record &r)
{
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const uint32_t last = i < 8 ? (w[9] >> (4 * (7 - i))) & 15u : w[10] & 15u;
        r.row[i] = (uint64_t)w[i] << 4 | last;
    }
    r.sym = w[11];
    r.ties = w[12];
}

// a board's S packed records merged.  false: the board had a byte > 9.
PS_FN bool reduce(const uint32_t *w, int S, Record &out)
{
    clear(out);
    if (w[13]) return false;
    for (int s = 0; s < S; ++s) {
        Record r;
        unpack(w + (int64_t)s * RECORD_WORDS, r);
        merge(out, r);
    }
    return true;
}

// the record's image as 81 bytes
template <class Put>
PS_FN void store_cells(const Record &r, Put put)
{
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) put(9 * i + j, (uint32_t)(r.row[i] >> (4 * (8 - j))) & 15u);
}

// Super-block sb in [0, 36) = (t*3 + k)*6 + a; its blocks are number
// t*36 + 12k + a (bp = 2k) and that + 6 (bp = 2k + 1).
PS_FN int super_first_block(int sb) { return (sb / 18) * 36 + 12 * ((sb % 18) / 6) + sb % 6; }

// slice s of S: [s*2592/S, (s+1)*2592/S)
PS_FN int slice_lo(int s, int S) { return (int)((int64_t)s * ROW_VARIANTS / S); }

// the super-blocks with a row variant in [lo, hi), ascending; returns how many
PS_FN int list_super_blocks(int lo, int hi, uint8_t *list)
{
    const int b0 = lo / BLOCK, b1 = (hi + BLOCK - 1) / BLOCK;
    int n = 0;
    for (int sb = 0; sb < SUPER_BLOCKS; ++sb) {
        const int f = super_first_block(sb);
        if ((f >= b0 && f < b1) || (f + 6 >= b0 && f + 6 < b1)) list[n++] = (uint8_t)sb;
    }
    return n;
}

// The state of one (super-block, ci) after its first three image rows.
struct Prefix {
    uint64_t r[3], map;
    uint32_t next;
    uint16_t sb, ci;
};

PS_FN uint64_t prefix_key(const Prefix &p) { return p.r[0] << 28 | p.r[1] >> 8; }

// Rows 0..2 of (super-block sb, column permutation ci).  false: the item is
// dead, its 16-cell prefix is greater than one already met.
// Key: load() -> the smallest 16-cell prefix met so far by anyone searching
// this board (all ones at the start), lower(k) -> make it at most k.
template <class Key>
PS_FN bool prefix(const uint8_t *bt, int sb, int ci, Prefix &p, Key &key)
{
    const int t = sb / 18, band = (sb % 18) / 6, a = sb % 6;
    const uint8_t *g = bt + 81 * t;
    int C[9];
    line_perm(ci, C);
    p.map = 0;
    p.next = 1;
    p.sb = (uint16_t)sb;
    p.ci = (uint16_t)ci;
    const uint64_t k = key.load();
    p.r[0] = image_row(g + 9 * (3 * band + perm3(a, 0)), C, p.map, p.next);
    if (p.r[0] > (k >> 28)) return false;
    p.r[1] = image_row(g + 9 * (3 * band + perm3(a, 1)), C, p.map, p.next);
    const uint64_t mine = prefix_key(p);
    if (mine > k) return false;
    if (mine < k) key.lower(mine);  // the prefix of real images: of every (bp, b, d) of this super-block
    p.r[2] = image_row(g + 9 * (3 * band + perm3(a, 2)), C, p.map, p.next);
    return true;
}

// The row variants of one (bp, b) of a live prefix -- hb = 0..11 is
// bp = 2*band + hb / 6, b = hb % 6 -- that lie in [lo, hi), against `best`:
// rows 3..5 once, rows 6..8 for each of the six d.
template <class Key>
PS_FN void complete(const uint8_t *bt, const Prefix &p, int hb, int lo, int hi, Record &best, Key &key)
{
    const int sb = p.sb, ci = p.ci;
    const int t = sb / 18, band = (sb % 18) / 6, a = sb % 6;
    const int bp = 2 * band + hb / 6, b = hb % 6;
    const int rvb = (t * 36 + bp * 6 + a) * BLOCK + 6 * b;
    if (rvb + 6 <= lo || rvb >= hi) return;
    if (prefix_key(p) > key.load()) return;  // the key has moved on since the prefix was made
    int c3 = cmp3(p.r, best.row);
    if (c3 > 0) return;
    const uint8_t *g = bt + 81 * t;
    int C[9];
    line_perm(ci, C);
    uint64_t r[6], map1 = p.map;
    uint32_t next1 = p.next;
#pragma unroll
    for (int q = 0; q < 3; ++q) r[q] = image_row(g + 9 * (3 * perm3(bp, 1) + perm3(b, q)), C, map1, next1);
    int c6 = c3 ? c3 : cmp3(r, best.row + 3);
    if (c6 > 0) return;
#pragma unroll 1
    for (int d = 0; d < 6; ++d) {
        const int rv = rvb + d;
        if (rv < lo || rv >= hi) continue;
        uint64_t map2 = map1;
        uint32_t next2 = next1;
#pragma unroll
        for (int q = 0; q < 3; ++q) r[3 + q] = image_row(g + 9 * (3 * perm3(bp, 2) + perm3(d, q)), C, map2, next2);
        const int c9 = c6 ? c6 : cmp3(r + 3, best.row + 6);
        if (c9 > 0) continue;
        const uint32_t sym = (uint32_t)rv * LINE_PERMS + (uint32_t)ci;
        if (c9 < 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) best.row[i] = p.r[i];
#pragma unroll
            for (int i = 0; i < 6; ++i) best.row[3 + i] = r[i];
            best.sym = sym;
            best.ties = 1u;
            c6 = 0;  // the best now starts with this candidate's own rows 0..5
        } else {
            best.ties++;
            best.sym = sym < best.sym ? sym : best.sym;
        }
    }
}

// One (super-block, ci) of the search, start to end.
template <class Key>
PS_FN void search_super(const uint8_t *bt, int sb, int ci, int lo, int hi, Record &best, Key &key)
{
    Prefix p;
    if (!prefix(bt, sb, ci, p, key)) return;
    for (int hb = 0; hb < 12; ++hb) complete(bt, p, hb, lo, hi, best, key);
}

struct HostKey {
    uint64_t v;
    uint64_t load() const { return v; }
    void lower(uint64_t k) { v = k < v ? k : v; }
};

// Host driver: the record of the row variants [lo, hi) of board g, walked the
// way one workgroup of canon_kernel walks a slice.  false: a byte > 9 (no
// search; out is empty).
static inline bool canon_board(const uint8_t *g, int lo, int hi, Record &out)
{
    uint8_t bt[STAGE_BYTES];
    clear(out);
    if (!stage(g, bt)) return false;
    HostKey key = {~0ull};
    uint8_t list[SUPER_BLOCKS];
    const int count = list_super_blocks(lo, hi, list);
    for (int it = 0; it < count * LINE_PERMS; ++it)
        search_super(bt, list[it / LINE_PERMS], it % LINE_PERMS, lo, hi, out, key);
    return true;
}

}  // namespace canon

#endif  // SDK_CANON_H
