// host_model.h -- the lane solvers stepped on the host, the way the kernels
// step them: a board's bytes as load_words takes them, a lane's stack lines,
// the wave-wide solver's view of the same lines over an emulated wave, and one
// driver from the load to the answer.  Host only: the CPU tests
// (tests/native/*.cpp) and the tooling (scripts/native/*.cpp) include it, no
// .hip unit does.  Not a product path.
#ifndef SDK_HOST_MODEL_H
#define SDK_HOST_MODEL_H

#include <stdint.h>
#include <string.h>

#include "plane_wide.h"

namespace host {

// the 21 little-endian words of a board's 81 bytes (plane::load_words' input)
inline void words_of(const uint8_t *src, uint32_t (&x)[21])
{
    uint8_t buf[84] = {0};
    memcpy(buf, src, 81);
    for (int k = 0; k < 21; ++k)
        x[k] = (uint32_t)buf[4 * k] | ((uint32_t)buf[4 * k + 1] << 8) | ((uint32_t)buf[4 * k + 2] << 16) |
               ((uint32_t)buf[4 * k + 3] << 24);
}

// One lane's stack lines in the kernels' layout (plane_stack.h): word 3d+b =
// P[d][b], word 27 = the branch entry, words 28-30 = the level's undetermined
// cells (the look-ahead path only).  The put / get plane::WordStack wraps.
// deepest: the most levels in use since the caller last zeroed it.
struct LineStack {
    // (the unique candidates' lanes: 81 levels and the four set lines of
    // plane_uniq.h; the candidates' lanes use 83 of them, plane_cand.h)
    enum { LEVELS = 85 };
    uint32_t w[LEVELS * plane::STACK_LINE_WORDS];
    uint32_t deepest = 0;
    void put(uint32_t level, int k, uint32_t v)
    {
        w[level * plane::STACK_LINE_WORDS + k] = v;
        if (level + 1 > deepest) deepest = level + 1;
    }
    uint32_t get(uint32_t level, int k) const { return w[level * plane::STACK_LINE_WORDS + k]; }
};

// the wave-wide solver's view of the same lines: it never reads words 28-30
struct WStack {
    uint32_t *w;
    uint32_t &at(uint32_t level, uint32_t k) const { return w[level * plane::STACK_LINE_WORDS + k]; }
    void push(uint32_t level, const wide::V &v, const wide::Lanes &L, uint32_t entry) const
    {
        for (int i = 0; i < 64; ++i)
            if ((L.valid.m >> i) & 1) at(level, L.word.x[i]) = v.x[i];
        at(level, plane::STACK_ENTRY) = entry;
    }
    uint32_t entry(uint32_t level) const { return at(level, plane::STACK_ENTRY); }
    wide::V restore(uint32_t level, const wide::Lanes &L) const
    {
        wide::V r(0u);
        for (int i = 0; i < 64; ++i)
            if ((L.valid.m >> i) & 1) r.x[i] = at(level, L.word.x[i]);
        return r;
    }
    void put_entry(uint32_t level, uint32_t e) const { at(level, plane::STACK_ENTRY) = e; }
};

inline wide::V to_wave(const plane::Board &B, const wide::Lanes &L)
{
    wide::V w(0u);
    for (int i = 0; i < 64; ++i)
        if ((L.valid.m >> i) & 1) w.x[i] = B.P[L.d.x[i]][L.b.x[i]];
    return w;
}

// the store path of plane_kernel's wide tail: value slices per band -> bytes
inline void store_wave(const wide::V &w, const wide::Lanes &L, uint8_t *dst)
{
    wide::V s[4];
    wide::value_slices(w, L, s);
    for (int c = 0; c < 81; ++c) {
        const int b = plane::cell_band(c), p = plane::cell_pos(c);
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k) v |= ((s[k].x[16 * b] >> p) & 1u) << k;
        dst[c] = (uint8_t)v;
    }
}

struct Counts {
    uint64_t guesses, passes_lane, passes_wide;  // guesses: lane and wide together
};
enum : uint32_t { LANE_ONLY = 0xFFFFFFFFu };  // lane_guesses: no hand-over
// per board (solve_batch's `info`): lane passes, whether the board ended by the
// root rule (plane::search_step_impl's root_full), whether grid_complete()
// then rejected its all-single root
struct BoardInfo {
    uint32_t passes;
    uint8_t by_rule, rejected;
};

// Solve each board.  The lane phase steps one pass and one search step per
// iteration, as a lane of plane_kernel does: the look-ahead pass the kernel
// runs (ahead: plane::pass_ahead + search_step_ahead, und / nd starting from
// the givens as at the kernel's refill) or the pass it ran before
// (plane::pass + search_step, kept as the look-ahead pass's reference).  Once
// `lane_guesses` guesses are made and the search has not ended, the wave-wide
// solver continues from the same planes, stack, depth and search mode (Det,
// und and nd dropped, as the kernel's tail drops them); LANE_ONLY: never.
// out: the completion, or the input back.  status: 1 solved, 0 no completion,
// -1 a byte > 9, 2 left to the wave kernel (clashing givens, a search deeper
// than max_depth <= LineStack::LEVELS, or -- root_full, the look-ahead path
// only, as the plane kernel's unordered lane loop runs it -- an all-single
// root that plane::grid_complete rejects, as the kernel's outbox flush does).
inline void solve_batch(const uint8_t *in, uint8_t *out, int32_t *status, int64_t n, bool ahead, uint32_t lane_guesses,
                        int node_order, uint32_t max_depth, uint32_t mrv_after, Counts &c, bool root_full = false,
                        BoardInfo *info = nullptr)
{
    static LineStack lines;
    const plane::WordStack<LineStack> ls = {lines};
    const WStack ws = {lines.w};
    const wide::Lanes L = wide::lanes();
    c = {0, 0, 0};
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t *src = in + i * 81;
        uint8_t *dst = out + i * 81;
        memcpy(dst, src, 81);
        uint32_t x[21], und[3], nd[3];
        words_of(src, x);
        plane::Board B;
        bool clash = false;
        if (!plane::load_words(B, x, clash, nd)) { status[i] = -1; continue; }
        if (clash) { status[i] = 2; continue; }
        for (int b = 0; b < 3; ++b) und[b] = plane::ROWS & ~nd[b];  // (plane::pass computes its own und)
        uint32_t depth = 0, lg = 0, mst = 0;
        int s = plane::S_CONT;
        bool by_rule = false;
        const uint64_t p0 = c.passes_lane;
        if (info) info[i] = {0u, 0, 0};
        while (s == plane::S_CONT && lg < lane_guesses) {
            if (ahead) {
                const int r = plane::pass_ahead(B, und, nd);
                s = plane::search_step_ahead(B, und, nd, r, depth, mst, ls, node_order, max_depth, mrv_after, lg,
                                             root_full);
                by_rule = s == plane::S_SOLVED && r == plane::OPEN;  // (only the rule ends an OPEN pass)
            } else {
                const int r = plane::pass(B, und);
                s = plane::search_step(B, und, r, depth, mst, ls, node_order, max_depth, mrv_after, lg);
            }
            c.passes_lane++;
        }
        c.guesses += lg;
        if (info) {
            info[i].passes = (uint32_t)(c.passes_lane - p0);
            info[i].by_rule = by_rule;
        }
        if (by_rule && !plane::grid_complete(B)) {
            if (info) info[i].rejected = 1;
            status[i] = 2;
            continue;
        }
        if (s != plane::S_CONT) {
            if (s == plane::S_SOLVED) plane::store_values(B, [&](int cell, uint32_t v) { dst[cell] = (uint8_t)v; });
            status[i] = s == plane::S_SOLVED ? 1 : s == plane::S_NONE ? 0 : 2;
            continue;
        }
        wide::V w = to_wave(B, L);
        wide::Stats st = {0, 0, 0};
        wide::NoCancel hk;
        const int r = wide::solve(w, depth, ws, L, node_order, max_depth, st, hk, mst, mrv_after);
        c.guesses += st.guesses;
        c.passes_wide += st.passes;
        if (r == wide::W_SOLVED) store_wave(w, L, dst);
        status[i] = r == wide::W_SOLVED ? 1 : r == wide::W_UNSOLVABLE ? 0 : 2;
    }
}

}  // namespace host

#endif  // SDK_HOST_MODEL_H
