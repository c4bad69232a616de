// Host model of the completion list (csrc/plane_enum.h, what enum_kernel's
// lanes run) for the CPU test-suite (tests/test_enum_host.py): W simulated
// waves of 64 lanes, stepped serially, wave after wave, round after round,
// with the kernel's take / drop / stop / donate / park / flush rules, the same
// ring and counters (plane_exact.h's functions: the code that ships) and the
// same list: one cursor, a row and its owner written when the slot is below
// the capacity, the per-board limit through the board's count as a ticket
// (plane::enum_emit, enum_dropped, enum_final).  Not a product path.
// With -DENUM_HOST_MAIN the file is a program of its own (a few boards, their
// lists checked) for a sanitizer build.
#include <vector>

#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"
#include "../../sudoku_solver_distributed_amd/csrc/plane_enum.h"

namespace {

struct Atomics {
    uint64_t load(const uint64_t *p) const { return *p; }
    bool cas(uint64_t *p, uint64_t &expected, uint64_t desired) const
    {
        if (*p != expected) {
            expected = *p;
            return false;
        }
        *p = desired;
        return true;
    }
};

// the ring and the head block, as the kernel's lanes see them in one round
struct Shared {
    uint64_t *head;
    uint32_t *ring;
    uint64_t cap, head0, limit, target;
    uint32_t slot0;  // head0's slot
    bool wants() const { return head[plane::XH_TAIL] - limit < target; }
    uint64_t reserve(uint32_t k) const
    {
        return plane::exact_reserve(Atomics(), &head[plane::XH_TAIL], head0, cap, k);
    }
    uint32_t *line(uint64_t pos) const
    {
        return ring + plane::exact_slot(pos, head0, slot0, cap) * plane::STACK_LINE_WORDS;
    }
    void put(uint64_t pos, const plane::Board &B, const uint32_t (&und)[3], uint32_t entry, uint32_t board) const
    {
        uint32_t *w = line(pos);
        for (int k = 0; k < 27; ++k) w[k] = B.P[k / 3][k % 3];
        w[plane::STACK_ENTRY] = entry;
        for (int b = 0; b < 3; ++b) w[plane::STACK_UND + b] = und[b];
        w[plane::STACK_BOARD] = board;
    }
    uint32_t get(uint64_t pos, plane::Board &B, uint32_t (&und)[3], uint32_t &board) const
    {
        const uint32_t *w = line(pos);
        for (int k = 0; k < 27; ++k) B.P[k / 3][k % 3] = w[k];
        for (int b = 0; b < 3; ++b) und[b] = w[plane::STACK_UND + b];
        board = w[plane::STACK_BOARD];
        return w[plane::STACK_ENTRY];
    }
};

// the list, as plane::enum_emit reaches it
struct Out {
    int64_t *count;
    uint64_t *head;
    uint8_t *grids;
    int32_t *owner;
    uint64_t ticket(uint32_t board) const { return (uint64_t)count[board]++; }
    uint64_t slot() const { return head[plane::XH_TOTAL]++; }
    void write(uint64_t slot, const plane::Board &B, uint32_t board) const
    {
        uint8_t *dst = grids + slot * 81;
        plane::store_values(B, [&](int c, uint32_t v) { dst[c] = (uint8_t)v; });
        owner[slot] = (int32_t)board;
    }
};

struct Lane {
    plane::Board B;
    uint32_t und[3], nd[3], depth, found, board, passes;
    bool active, resume;
};

struct Park {
    uint32_t depth, board;
};

}  // namespace

// grids / owner / count[i] / status[i] / info as sdk_enumerate_batch documents
// them (status 1 DONE, 2 PARTIAL, 3 LIMITED, -1 a byte > 9, -3 a push past
// max_depth <= 81), for a grid of `waves` waves.  max_tasks 0: the default of
// that grid.  info: rounds, lines donated, lane parks, the most passes a lane
// ran in one round, total, listed.  Returns 0, or -2 for arguments the entry
// refuses.
extern "C" int enum_host_batch(const uint8_t *in, int64_t n, uint8_t *grids, int32_t *owner, int64_t capacity,
                               int64_t limit, int64_t *count, int32_t *status, int waves, int32_t slice,
                               int max_rounds, int64_t max_tasks, uint32_t max_depth, int64_t *info)
{
    if (n == 0) return 0;
    if (n < 0 || waves < 1 || slice < 1 || max_rounds < 1 || max_tasks < 0 || !in || !count || !status) return -2;
    if (capacity < 0 || capacity > INT32_MAX || limit < 0 || (capacity > 0 && (!grids || !owner))) return -2;
    if (max_depth > (uint32_t)plane::COUNT_MAX_DEPTH) max_depth = plane::COUNT_MAX_DEPTH;
    const uint64_t lanes = 64ull * (uint64_t)waves;
    const uint64_t cap = plane::exact_ring_lines(lanes, (uint64_t)max_tasks);
    std::vector<uint32_t> ring(cap * plane::STACK_LINE_WORDS);
    std::vector<host::LineStack> lines(lanes);
    std::vector<Park> park(lanes, Park{0u, 0u});
    std::vector<int32_t> open((size_t)n, 1);
    uint64_t head[plane::XH_WORDS] = {0};
    head[plane::XH_OPEN] = (uint64_t)n;
    for (int64_t i = 0; i < n; ++i) {
        count[i] = 0;
        status[i] = 0;
    }
    const Out out = {count, head, grids, owner};
    uint64_t head0 = 0, ring_limit = 0;
    uint32_t slot0 = 0;
    int rounds = 0;
    while (rounds < max_rounds && head[plane::XH_OPEN] != 0) {
        head[plane::XH_CLAIM] = 0;
        const Shared sh = {head, ring.data(), cap, head0, ring_limit, plane::exact_fill_target(lanes, cap), slot0};
        for (int w = 0; w < waves; ++w) {
            Lane L[64];
            int64_t dopen = 0;
            uint64_t donated = 0, parks = 0;
            for (int l = 0; l < 64; ++l) {
                Park &pk = park[(size_t)w * 64 + l];
                L[l].active = L[l].resume = pk.depth != 0;
                L[l].depth = pk.depth;
                L[l].board = pk.board;
                L[l].found = L[l].passes = 0;
                pk.depth = 0;
            }
            bool tasks_out = false, boards_out = false;
            for (;;) {
                int nwant = 0, nactive = 0;
                for (int l = 0; l < 64; ++l) {
                    nactive += L[l].active;
                    nwant += !L[l].active && L[l].passes < (uint32_t)slice;
                }
                const bool queue_out = tasks_out && boards_out;
                if (nactive == 0 && (nwant == 0 || queue_out)) break;
                if (!queue_out && (nwant >= plane::EXACT_REFILL || (nactive == 0 && nwant > 0))) {
                    uint64_t ntask = 0, tbase = 0, bbase = (uint64_t)n;
                    if (!tasks_out) {
                        const uint64_t h = head[plane::XH_CLAIM];
                        head[plane::XH_CLAIM] += (uint64_t)nwant;
                        const uint64_t len = ring_limit - head0;
                        ntask = h >= len ? 0 : len - h < (uint64_t)nwant ? len - h : (uint64_t)nwant;
                        tbase = head0 + h;
                        tasks_out = h + (uint64_t)nwant >= len;
                    }
                    if (ntask < (uint64_t)nwant && !boards_out) {
                        const uint64_t k = (uint64_t)nwant - ntask;
                        bbase = head[plane::XH_BOARDS];
                        head[plane::XH_BOARDS] += k;
                        boards_out = bbase + k >= (uint64_t)n;
                    }
                    uint64_t r = 0;
                    for (int l = 0; l < 64; ++l) {
                        Lane &a = L[l];
                        if (a.active || a.passes >= (uint32_t)slice) continue;
                        const uint64_t rank = r++;
                        const plane::WordStack<host::LineStack> stk = {lines[(size_t)w * 64 + l]};
                        if (rank < ntask) {
                            const uint32_t e = sh.get(tbase + rank, a.B, a.und, a.board);
                            stk.push(0, a.B, a.und, e);
                            a.depth = 1;
                            a.active = a.resume = true;
                        } else if (bbase + (rank - ntask) < (uint64_t)n) {
                            a.board = (uint32_t)(bbase + (rank - ntask));
                            uint32_t x[21], given[3];
                            host::words_of(in + (int64_t)a.board * 81, x);
                            bool clash = false;
                            if (!plane::load_words(a.B, x, clash, given)) {
                                status[a.board] = -1;
                                open[a.board]--;
                                dopen--;
                            } else if (clash) {
                                open[a.board]--;  // an exact zero
                                dopen--;
                            } else {
                                a.active = true;
                                a.resume = false;
                                a.depth = 0;
                                for (int b = 0; b < 3; ++b) {
                                    a.nd[b] = given[b];
                                    a.und[b] = plane::andn(plane::ROWS, given[b]);
                                }
                            }
                        }
                    }
                }
                for (int l = 0; l < 64; ++l) {
                    Lane &a = L[l];
                    if (!a.active) continue;
                    const plane::WordStack<host::LineStack> stk = {lines[(size_t)w * 64 + l]};
                    int k = plane::X_DONE;
                    if (!plane::enum_dropped(a.resume, (uint64_t)count[a.board], (uint64_t)limit))
                        k = plane::enum_iter(a.B, a.und, a.nd, a.depth, a.passes, a.resume, (uint32_t)slice, stk,
                                             max_depth, [&](const plane::Board &S) {
                                                 return plane::enum_emit(S, a.board, a.found, (uint64_t)limit,
                                                                         (uint64_t)capacity, out);
                                             });
                    if (k == plane::X_CONT) continue;
                    a.active = false;
                    if (k == plane::X_FAULT) {
                        status[a.board] = plane::COUNT_FAULT;
                        a.found = 0;
                    }
                    count[a.board] += a.found;
                    a.found = 0;
                    if (k != plane::X_STOP) {
                        open[a.board]--;
                        dopen--;
                    } else if (plane::exact_donate(a.B, a.und, a.depth, a.board, stk, sh)) {
                        open[a.board] += (int32_t)a.depth - 1;
                        dopen += (int64_t)a.depth - 1;
                        donated += a.depth;
                    } else {
                        park[(size_t)w * 64 + l] = Park{a.depth, a.board};
                        parks++;
                    }
                }
            }
            uint64_t most = 0;
            for (int l = 0; l < 64; ++l)
                if (L[l].passes > most) most = L[l].passes;
            head[plane::XH_OPEN] += (uint64_t)dopen;
            head[plane::XH_DONATED] += donated;
            head[plane::XH_PARKS] += parks;
            if (most > head[plane::XH_MAXPASS]) head[plane::XH_MAXPASS] = most;
        }
        rounds++;
        plane::exact_advance(head[plane::XH_CLAIM], head[plane::XH_TAIL], cap, head0, slot0, ring_limit);
    }
    for (int64_t i = 0; i < n; ++i) {
        uint64_t c = (uint64_t)count[i];
        plane::enum_final(c, status[i], open[i], (uint64_t)limit);
        count[i] = (int64_t)c;
    }
    if (info) {
        info[0] = rounds;
        info[1] = (int64_t)head[plane::XH_DONATED];
        info[2] = (int64_t)head[plane::XH_PARKS];
        info[3] = (int64_t)head[plane::XH_MAXPASS];
        info[4] = (int64_t)head[plane::XH_TOTAL];
        info[5] = (int64_t)plane::enum_listed(head[plane::XH_TOTAL], (uint64_t)capacity);
    }
    return 0;
}

#ifdef ENUM_HOST_MAIN
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

// rows [0, listed) of board `b`: valid grids that keep `g`'s givens, distinct
static int check_rows(const uint8_t *g, int b, const std::vector<uint8_t> &grids, const std::vector<int32_t> &owner,
                      int64_t listed, int64_t want)
{
    std::set<std::string> seen;
    for (int64_t k = 0; k < listed; ++k) {
        if (owner[(size_t)k] != b) continue;
        const uint8_t *r = &grids[(size_t)k * 81];
        for (int c = 0; c < 81; ++c)
            if (r[c] < 1 || r[c] > 9 || (g[c] && g[c] != r[c])) return 1;
        for (int u = 0; u < 9; ++u) {
            int row = 0, col = 0, box = 0;
            for (int j = 0; j < 9; ++j) {
                row |= 1 << r[9 * u + j];
                col |= 1 << r[9 * j + u];
                box |= 1 << r[27 * (u / 3) + 3 * (u % 3) + 9 * (j / 3) + j % 3];
            }
            if (row != 0x3FE || col != 0x3FE || box != 0x3FE) return 2;
        }
        if (!seen.insert(std::string((const char *)r, 81)).second) return 3;
    }
    return (int64_t)seen.size() == want ? 0 : 4;
}

int main()
{
    static const char *full = "897124635531679284642385179154293867289716453376458912923867541765941328418532796";
    uint8_t in[4 * 81];
    for (int b = 0; b < 4; ++b)
        for (int c = 0; c < 81; ++c) in[81 * b + c] = (uint8_t)(full[c] - '0');
    for (int c = 0; c < 81; ++c) {
        if (c % 2 == 0 || c < 27) in[81 + c] = 0;  // many completions
        if (c % 3 != 1 && c >= 27) in[162 + c] = 0;  // others
    }
    in[243] = in[244];  // clashing givens
    int bad = 0;
    const int64_t caps[] = {0, 5, 1 << 16};
    int64_t exact[4] = {0, 0, 0, 0};
    for (int waves = 1; waves <= 3; waves += 2)
        for (int64_t limit : {(int64_t)0, (int64_t)7})
            for (int64_t cap : caps)
                for (int slice : {1, 8, 256}) {
                    std::vector<uint8_t> grids((size_t)cap * 81 + 1, 0xA5);
                    std::vector<int32_t> owner((size_t)cap + 1, -7);
                    int64_t count[4], info[6];
                    int32_t status[4];
                    const int rc = enum_host_batch(in, 4, grids.data(), owner.data(), cap, limit, count, status, waves,
                                                   slice, 1 << 20, slice == 8 ? 64 : 0, 81, info);
                    if (rc != 0) return 10;
                    if (limit == 0 && cap == 0 && slice == 1 && waves == 1) memcpy(exact, count, sizeof exact);
                    if (grids.back() != 0xA5 || owner.back() != -7) bad |= 1;
                    if (info[5] != (info[4] < cap ? info[4] : cap)) bad |= 2;
                    int64_t sum = 0;
                    for (int b = 0; b < 4; ++b) {
                        const int64_t want = limit && exact[b] >= limit ? limit : exact[b];
                        if (count[b] != want || status[b] != (limit && exact[b] >= limit ? 3 : 1)) bad |= 4;
                        sum += want;
                        if (info[4] <= cap && check_rows(in + 81 * b, b, grids, owner, info[5], want)) bad |= 8;
                    }
                    if (info[4] != sum) bad |= 16;
                }
    printf("counts %lld %lld %lld %lld, failed checks 0x%x\n", (long long)exact[0], (long long)exact[1],
           (long long)exact[2], (long long)exact[3], bad);
    return bad;
}
#endif
