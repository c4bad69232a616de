// rate_kernels.hip -- translation unit of the puzzle rating (rate.h):
// rate_kernel, rate_trial_kernel and their C ABI entries
// (sdk_rate_scratch_bytes, sdk_rate_batch).  A unit of its own: the solve,
// count and canon units, their flags and their workspace are not involved
// (common.h is included for cached_occupancy alone).
//
// rate_kernel: one board per LANE, persistent one-wave workgroups, the queue
// head claimed as count_kernel claims it (SDK_RATE_REFILL idle lanes, one
// agent-scope fetch-add by lane 0).  A lane holds its board's 27 plane words,
// its level and its answer so far, and runs ONE rate::pass per loop iteration
// at its own level (the pass computes every rule's removals and masks those
// its level does not have, so the wave's lanes stay on one instruction
// stream).  A pass that changes nothing ends the level: the lane writes the
// board's answer (dead, solved, or undecided at max_level <= 3), moves one
// level up, or -- still open after level 3 at max_level 4 -- writes open[0..2]
// and appends the board's index to the list in the scratch, the lanes that do
// so in one iteration with one fetch-add between them.
//
// rate_trial_kernel: one WAVE per listed board, persistent one-wave
// workgroups claiming list entries one at a time.  Every lane builds the
// board's level-3 closure for itself (the same instructions on the same
// data: the cost of one lane) and lane 0 puts it into LDS as 27 words, twice:
// S0, the round's state, and S, where the round's removals land.  A round
// numbers the candidates of the cells with two or more by running sums of the
// words' popcounts; lane k of a chunk takes candidate 64 chunk + k, fixes it
// on a copy of S0 in its own registers and closes that at level 3, the lanes
// each at their own pace; a dead trial clears its bit in S with an LDS
// atomic AND.  After a round that cleared a bit the wave reads S back,
// closes it at level 3 and starts over; a round that clears nothing ends the
// board.  (The empty board: 729 candidates, 12 chunks, one round.)
//
// Scratch: [0, 256) the control block -- queue head (word 0), list length
// (byte 64), the trial kernel's list head (byte 128) -- zeroed by the call
// itself in stream order; then, for max_level 4, n int64 list entries.
#include "common.h"
#include "rate.h"

#define RATE_THREADS 64  // one wave per workgroup
#ifndef SDK_RATE_WAVES_PER_EU
#define SDK_RATE_WAVES_PER_EU 4
#endif
#ifndef SDK_RATE_TRIAL_WAVES_PER_EU
#define SDK_RATE_TRIAL_WAVES_PER_EU 4
#endif
// idle lanes before a wave claims boards (results never depend on it)
#ifndef SDK_RATE_REFILL
#define SDK_RATE_REFILL 16
#endif
#define RATE_HEAD_BYTES 256
#define RATE_LIST_COUNT_BYTE 64
#define RATE_LIST_HEAD_BYTE 128

// The 21 words of the board at `src` (any alignment): the 21 aligned dwords
// that hold its 81 bytes (byte 80 lies in dword 20 for every alignment, so
// every dword read holds a byte of the board), funnel-shifted into place.
// Only byte 0 of x[20] is the board's.
__device__ __forceinline__ void rate_load_words(const uint8_t *src, uint32_t (&x)[21])
{
    const uintptr_t a = (uintptr_t)src;
    const uint32_t *d = (const uint32_t *)(a & ~(uintptr_t)3);
    const uint32_t r = ((uint32_t)a & 3u) * 8u;
    uint32_t lo = d[0];
#pragma unroll
    for (int k = 0; k < 20; ++k) {
        const uint32_t hi = d[k + 1];
        x[k] = r ? __builtin_amdgcn_alignbit(hi, lo, r) : lo;
        lo = hi;
    }
    x[20] = lo >> r;
}

__device__ __forceinline__ uint32_t rate_wave_claim(uint32_t *counter, uint32_t k, int lane)
{
    uint32_t h = 0;
    if (lane == 0) h = __hip_atomic_fetch_add(counter, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)h);
}

__global__ __launch_bounds__(RATE_THREADS, SDK_RATE_WAVES_PER_EU) void rate_kernel(
    const uint8_t *__restrict__ boards, int32_t *__restrict__ rating, int32_t *__restrict__ open,
    uint16_t *__restrict__ marks, int64_t n, int max_level, unsigned long long *__restrict__ head,
    uint32_t *__restrict__ list_count, int64_t *__restrict__ list)
{
    const int lane = threadIdx.x;
    plane::Board B;
    rate::Result R;
    rate::start(R);
    int level = 1;
    int64_t p = 0;  // this lane's board
    bool active = false, queue_out = false;
    for (;;) {
        // what this iteration finishes: 1 the answer in R (marks under `keep`), 2 a board for the list
        int fin = 0;
        uint32_t keep = 0u;
        const uint64_t idle = __builtin_amdgcn_ballot_w64(!active);
        const int nidle = __builtin_popcountll(idle);
        if (queue_out && nidle == 64) break;
        if (!queue_out && nidle >= SDK_RATE_REFILL) {
            unsigned long long h = 0;
            if (lane == 0)
                h = __hip_atomic_fetch_add(head, (unsigned long long)nidle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t base = (int64_t)(((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(h >> 32)) << 32) |
                                           __builtin_amdgcn_readfirstlane((uint32_t)h));
            queue_out = base + nidle >= n;  // the batch's end is handed out: no further claim
            const int64_t q = base + (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            if (!active && q < n) {
                p = q;
                uint32_t x[21];
                rate_load_words(boards + p * 81, x);
                if (rate::load(B, x)) {
                    active = true;
                    level = 1;
                    rate::start(R);
                } else {
                    rate::invalid(R);
                    fin = 1;
                }
            }
        }
        if (active) {
            int op;
            const int r = rate::pass(B, level, op);
            if (r != rate::R_OPEN) {
                if (rate::settle(R, level, r, op, max_level)) {
                    fin = 1;
                    keep = r == rate::R_DEAD ? 0u : 0x1FFu;
                } else if (level == 3) {
                    fin = 2;
                } else {
                    level++;
                }
            }
            if (fin) active = false;
        }
        if (fin == 1) {
            rating[p] = R.rating;
            if (open) {
#pragma unroll
                for (int k = 0; k < 4; ++k) open[p * 4 + k] = R.open[k];
            }
            if (marks) {
                uint16_t *m = marks + p * 81;
                rate::store_marks(B, keep, [&](int c, uint32_t v) { m[c] = (uint16_t)v; });
            }
        }
        // the boards level 4 has to look at: one claim for the wave's lanes
        const uint64_t listing = __builtin_amdgcn_ballot_w64(fin == 2);
        if (listing) {
            const uint32_t at = rate_wave_claim(list_count, (uint32_t)__builtin_popcountll(listing), lane);
            if (fin == 2) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(listing >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)listing, 0u));
                list[at + rank] = p;
                if (open) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) open[p * 4 + k] = R.open[k];
                }
            }
        }
    }
}

__global__ __launch_bounds__(RATE_THREADS, SDK_RATE_TRIAL_WAVES_PER_EU) void rate_trial_kernel(
    const uint8_t *__restrict__ boards, int32_t *__restrict__ rating, int32_t *__restrict__ open,
    uint16_t *__restrict__ marks, const uint32_t *__restrict__ list_count, const int64_t *__restrict__ list,
    uint32_t *__restrict__ list_head)
{
    // the board's 27 plane words, word 3 d + b = P[d][b]; S0[27..29]: its cells with one candidate
    __shared__ uint32_t S[32], S0[32];
    const int lane = threadIdx.x;
    const uint32_t listed = *list_count;
    for (;;) {
        const uint32_t at = rate_wave_claim(list_head, 1u, lane);
        if (at >= listed) break;
        const int64_t p = list[at];
        plane::Board B;  // the same in every lane
        {
            uint32_t x[21];
            rate_load_words(boards + p * 81, x);
            rate::load(B, x);
        }
        int op = 0;
        int r = rate::close<3>(B, op);
        while (r == rate::R_FIX) {
            // the round's state twice in LDS: S0 to number the candidates and to
            // start every trial from, S for the dead trials to clear their bits in
            // (so the board's words need no registers while the trials run)
            uint32_t total = 0;
            {
                uint32_t single[3];
                plane::rule_a(B, single);
#pragma unroll
                for (int w = 0; w < 27; ++w)
                    total += (uint32_t)__builtin_popcount(plane::andn(B.P[w / 3][w % 3], single[w % 3]));
                if (lane == 0) {
#pragma unroll
                    for (int w = 0; w < 27; ++w) S0[w] = S[w] = B.P[w / 3][w % 3];
#pragma unroll
                    for (int b = 0; b < 3; ++b) S0[27 + b] = single[b];
                }
            }
            wave_lds_sync();
            for (uint32_t base = 0; base < total; base += 64u) {
                // this lane's candidate: number base + lane among the places of the
                // cells with two or more candidates, in word order
                plane::Board T;
                uint32_t rem = base + (uint32_t)lane, word = 0u;
                int sd = 0, sb = 0;
                const bool act = rem < total;
                bool found = !act;
#pragma unroll
                for (int w = 0; w < 27; ++w) {
                    // numbered on S0; started from S, which the chunks before have
                    // thinned: every bit gone from it went by the rules, so a trial on
                    // it is a trial on a state between S0 and its closure -- as sound,
                    // and dead sooner
                    T.P[w / 3][w % 3] = S[w];
                    const uint32_t m = plane::andn(S0[w], S0[27 + w % 3]);
                    const uint32_t c = (uint32_t)__builtin_popcount(m);
                    const bool hit = !found && rem < c;
                    word = hit ? m : word;
                    sd = hit ? w / 3 : sd;
                    sb = hit ? w % 3 : sb;
                    found = found || hit;
                    rem = found ? rem : rem - c;
                }
                for (uint32_t j = 0; act && j < rem; ++j) word &= word - 1u;
                const uint32_t bit = word & (0u - word);
                int st = rate::R_FIX;
                if (act) {
                    plane::set_cell(T, sb, __builtin_ctz(bit), 1u << sd);
                    st = rate::R_OPEN;
                }
                while (wany(st == rate::R_OPEN)) {
                    if (st == rate::R_OPEN) {
                        int o;
                        st = rate::pass(T, 3, o);
                    }
                }
                if (act && st == rate::R_DEAD) atomicAnd(&S[3 * sd + sb], ~bit);
            }
            wave_lds_sync();
            uint32_t diff = 0;
#pragma unroll
            for (int w = 0; w < 27; ++w) {
                const uint32_t v = S[w];
                diff |= v ^ S0[w];
                B.P[w / 3][w % 3] = v;
            }
            wave_lds_sync();  // everyone has read the words before lane 0 writes them again
            if (!diff) break;
            r = rate::close<3>(B, op);
        }
        if (lane == 0) {
            rating[p] = r == rate::R_DEAD ? 0 : r == rate::R_SOLVED ? 4 : 5;
            if (open) open[p * 4 + 3] = r == rate::R_DEAD ? -1 : r == rate::R_SOLVED ? 0 : op;
        }
        if (marks) {
            for (int c = lane; c < 81; c += 64) {
                const uint32_t m = plane::cell_cand(B, plane::cell_band(c), plane::cell_pos(c));
                marks[p * 81 + c] = (uint16_t)(r == rate::R_DEAD ? 0u : m);
            }
        }
    }
}

// ==================================================================== C ABI
static std::atomic<int> g_rate_bpc{0}, g_rate_trial_bpc{0};

// waves of a full grid on the current device: every CU at the kernel's occupancy
template <typename K>
static int64_t rate_full_waves(K kernel, int waves_per_eu, std::atomic<int> &cache)
{
    const int per_cu = 4 * waves_per_eu;  // four SIMDs per CU
    return (int64_t)sdk_device_cu_count() * cached_occupancy(kernel, RATE_THREADS, per_cu, per_cu, cache);
}

extern "C" {

size_t sdk_rate_scratch_bytes(int64_t n, int max_level)
{
    if (n < 0 || max_level < 1 || max_level > SDK_RATE_MAX_LEVEL) return 0;
    if (n > (int64_t)0x7FFFFFFF) return 0;  // the list's counters are 32-bit
    return RATE_HEAD_BYTES + (max_level == 4 ? (size_t)n * sizeof(int64_t) : 0);
}

int sdk_rate_batch(const uint8_t *d_boards, int32_t *d_rating, int32_t *d_open, uint16_t *d_marks, int64_t n,
                   int max_level, void *d_scratch, size_t scratch_bytes, void *stream)
{
    if (n < 0 || n > (int64_t)0x7FFFFFFF || max_level < 1 || max_level > SDK_RATE_MAX_LEVEL) return -2;
    if (n == 0) return 0;
    if (!d_boards || !d_rating || !d_scratch || ((uintptr_t)d_marks & 1u) || ((uintptr_t)d_rating & 3u) ||
        ((uintptr_t)d_open & 3u) || ((uintptr_t)d_scratch & 7u) || scratch_bytes < sdk_rate_scratch_bytes(n, max_level))
        return -2;
    hipStream_t st = (hipStream_t)stream;
    // the queue head and the list's counters, re-armed in stream order before the kernels
    if (hipMemsetAsync(d_scratch, 0, RATE_HEAD_BYTES, st) != hipSuccess) return -1;
    uint8_t *sc = (uint8_t *)d_scratch;
    uint32_t *list_count = (uint32_t *)(sc + RATE_LIST_COUNT_BYTE);
    int64_t *list = (int64_t *)(sc + RATE_HEAD_BYTES);
    const int64_t want = (n + 63) / 64, cap = rate_full_waves(rate_kernel, SDK_RATE_WAVES_PER_EU, g_rate_bpc);
    hipLaunchKernelGGL(rate_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(RATE_THREADS), 0, st, d_boards,
                       d_rating, d_open, d_marks, n, max_level, (unsigned long long *)d_scratch, list_count, list);
    if (hipGetLastError() != hipSuccess) return -1;
    if (max_level < 4) return 0;
    // one wave per listed board, at most a full grid: how many are listed is known on the device only
    const int64_t tcap = rate_full_waves(rate_trial_kernel, SDK_RATE_TRIAL_WAVES_PER_EU, g_rate_trial_bpc);
    hipLaunchKernelGGL(rate_trial_kernel, dim3((unsigned)(n < tcap ? n : tcap)), dim3(RATE_THREADS), 0, st, d_boards,
                       d_rating, d_open, d_marks, (const uint32_t *)list_count, (const int64_t *)list,
                       (uint32_t *)(sc + RATE_LIST_HEAD_BYTE));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
