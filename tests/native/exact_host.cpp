// Host model of the exact completion count (csrc/plane_exact.h, what
// exact_kernel's lanes run) for the CPU test-suite (tests/test_exact_host.py):
// W simulated waves of 64 lanes, stepped serially, wave after wave, round
// after round, with the kernel's take / stop / donate / park / flush rules,
// the same ring (plane::exact_slot, exact_advance, exact_reserve: the code that
// ships) and the same counters; and exact_ring_sweep, which drives the ring's
// arithmetic alone (tests/test_exact_props_host.py).  Not a product path.
#include <vector>

#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"
#include "../../sudoku_solver_distributed_amd/csrc/plane_exact.h"

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

struct Lane {
    plane::Board B;
    uint32_t und[3], nd[3], depth, found, board, passes;
    bool active, resume;
};

struct Park {
    uint32_t depth, board;
};

}  // namespace

// count[i] / status[i] as sdk_count_exact_batch documents them (status 1
// DONE, 2 PARTIAL, -1 a byte > 9, -3 a push past max_depth <= 81), for a grid
// of `waves` waves.  max_tasks 0: the default of that grid.  stats: rounds,
// lines donated, lane parks, the most passes a lane ran in one round.
// Returns 0, or -2 for arguments the entry refuses.
extern "C" int exact_host_batch(const uint8_t *in, int64_t *count, int32_t *status, int64_t n, int waves,
                                int32_t slice, int max_rounds, int64_t max_tasks, uint32_t max_depth, int64_t *stats)
{
    if (n == 0) return 0;
    if (n < 0 || waves < 1 || slice < 1 || max_rounds < 1 || max_tasks < 0 || !in || !count || !status) return -2;
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
    uint64_t head0 = 0, limit = 0;
    uint32_t slot0 = 0;
    int rounds = 0;
    while (rounds < max_rounds && head[plane::XH_OPEN] != 0) {
        head[plane::XH_CLAIM] = 0;
        const Shared sh = {head, ring.data(), cap, head0, limit, plane::exact_fill_target(lanes, cap), slot0};
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
                        const uint64_t len = limit - head0;
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
                    const int k = plane::exact_iter(a.B, a.und, a.nd, a.depth, a.found, a.passes, a.resume,
                                                    (uint32_t)slice, stk, max_depth);
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
        plane::exact_advance(head[plane::XH_CLAIM], head[plane::XH_TAIL], cap, head0, slot0, limit);
    }
    for (int64_t i = 0; i < n; ++i) {
        if (status[i] == 0) status[i] = open[i] == 0 ? 1 : 2;
        else count[i] = 0;
    }
    if (stats) {
        stats[0] = rounds;
        stats[1] = (int64_t)head[plane::XH_DONATED];
        stats[2] = (int64_t)head[plane::XH_PARKS];
        stats[3] = (int64_t)head[plane::XH_MAXPASS];
    }
    return 0;
}

// The ring's arithmetic as it ships (plane::exact_slot, exact_advance,
// exact_reserve), `rounds` seeded rounds for every cap in [cap_lo, cap_hi]:
// a round claims a random number of lines (up to twice the queue's length, so
// claims overshoot as the kernel's fetch-add does) and appends random runs of
// 1..81 lines through exact_reserve until one finds no room or a random stop.
// Checked every round: head0 <= limit <= tail <= head0 + cap; slot0 ==
// head0 % cap; the slot of every position in [head0, head0 + cap) is pos %
// cap; no position of [head0, limit) shares a slot with one of [limit, tail);
// a reservation succeeds exactly when tail + k - head0 <= cap and returns the
// old tail.  Returns 0, or 1000 * cap + the number of the check that failed.
extern "C" int64_t exact_ring_sweep(uint64_t seed, int rounds, uint32_t cap_lo, uint32_t cap_hi)
{
    uint64_t x = seed;
    auto rnd = [&x](uint64_t below) {  // splitmix64
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return (z ^ (z >> 31)) % below;
    };
    for (uint64_t cap = cap_lo; cap <= cap_hi; ++cap) {
        uint64_t head0 = 0, limit = 0, tail = 0;
        uint32_t slot0 = 0;
        std::vector<int> used(cap);
        for (int r = 0; r < rounds; ++r) {
            // the round's appends
            while (rnd(8) != 0) {
                const uint32_t k = 1 + (uint32_t)rnd(rnd(4) ? (cap < 81 ? cap : 81) : 81);
                const bool room = tail + k - head0 <= cap;
                const uint64_t before = tail;
                const uint64_t got = plane::exact_reserve(Atomics(), &tail, head0, cap, k);
                if (got != (room ? before : plane::X_NO_ROOM) || tail != before + (room ? k : 0)) return 1000 * cap + 1;
            }
            if (!(head0 <= limit && limit <= tail && tail - head0 <= cap)) return 1000 * cap + 2;
            if (slot0 != head0 % cap) return 1000 * cap + 3;
            for (uint64_t pos = head0; pos < head0 + cap; ++pos)
                if (plane::exact_slot(pos, head0, slot0, cap) != pos % cap) return 1000 * cap + 4;
            std::fill(used.begin(), used.end(), 0);
            for (uint64_t pos = head0; pos < limit; ++pos) used[plane::exact_slot(pos, head0, slot0, cap)]++;
            for (uint64_t pos = limit; pos < tail; ++pos)
                if (used[plane::exact_slot(pos, head0, slot0, cap)]++) return 1000 * cap + 5;
            for (uint64_t s = 0; s < cap; ++s)
                if (used[s] > 1) return 1000 * cap + 5;
            // the round's claims, then the host's advance
            const uint64_t len = limit - head0;
            const uint64_t claim = rnd(4) ? rnd(2 * len + 2) : len + rnd(200);
            plane::exact_advance(claim, tail, cap, head0, slot0, limit);
        }
    }
    return 0;
}
