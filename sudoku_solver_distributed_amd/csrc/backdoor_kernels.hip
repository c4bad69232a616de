// backdoor_kernels.hip -- translation unit of the backdoor search
// (backdoor.h): backdoor_root_kernel, backdoor_trial_kernel<K>,
// backdoor_final_kernel and their C ABI entries (sdk_backdoor_scratch_bytes,
// sdk_backdoor_batch).  A unit of its own: the solve workspace and the other
// units' flags are not involved (common.h is included for cached_occupancy
// and the wave helpers alone).  DESIGN.md §23.
//
// backdoor_root_kernel: one (board, grid) per LANE, persistent one-wave
// workgroups that claim 64 items at a time.  A lane validates its pair, closes
// the board at the level at its own pace and answers at once what needs no
// subset: the negative codes and size 0.  An open board gets a RECORD in the
// scratch -- its closure, its open cells with the grid's digits, the zeroed
// tallies -- at a place of the device-side list, the lanes that list in one
// iteration with one fetch-add between them.
//
// backdoor_trial_kernel<K>, launched for K = 1 .. max_size in stream order:
// persistent one-wave workgroups.  The work unit is (listed board, slice of
// its C(open, K) ranks); units are claimed one at a time from one 64-bit
// counter, unit / slices the board and unit % slices the slice, `slices` the
// same for every board (chosen by the entry from K: the ranks of the largest
// board over the chunks a slice holds), so nothing needs a prefix sum; a slice
// past a board's last rank is empty.  A board that a smaller size has
// answered is skipped.  Within a slice the wave stages the record in LDS;
// lane j of a chunk takes rank base + j, unranks it, fixes the subset's cells
// on its own copy of the closure and closes that at its own pace.  The solved
// trials of a slice are tallied in LDS (count by ballot, lowest rank, cover by
// LDS OR) and go to the record with one add, one min and three ORs per wave
// and slice.  Add, min and OR commute: the tallies hold no order.  No wave
// ever waits for another; only the launches are ordered, by the stream.
//
// backdoor_final_kernel: one lane per listed board turns its record into the
// four outputs (unranks the lowest rank into d_first).
//
// Scratch: [0, 256) the control block -- the root's queue head (byte 0), the
// list length (byte 64), the trial kernels' unit heads (bytes 128 + 8 K) --
// zeroed by the call itself in stream order; then n records of 320 bytes.
#include "common.h"
#include "backdoor.h"

#define BD_THREADS 64  // one wave per workgroup
#ifndef SDK_BACKDOOR_WAVES_PER_EU
#define SDK_BACKDOOR_WAVES_PER_EU 4
#endif
#define BD_HEAD_BYTES 256
#define BD_LIST_COUNT_BYTE 64
#define BD_UNIT_HEAD_BYTE 128  // + 8 K, K = 1..4
// a record, in 32-bit words
enum {
    BD_CLOSURE = 0,   // 27 words: word 3 d + b = P[d][b] of closure_L(b)
    BD_NOPEN = 27,    // its open cells
    BD_COUNT = 28,    // solved trials of the size that found some
    BD_FOUND = 29,    // that size, 0 while none
    BD_FIRST = 30,    // their lowest rank
    BD_COVER = 31,    // 3 band words: the cells of their subsets
    BD_BOARD = 34,    // 2 words: the item's index
    BD_ENTRIES = 36,  // 81 uint16: open cell | the grid's digit << 8, in cell order
    BD_WORDS = 80
};
#define BD_RECORD_BYTES (BD_WORDS * 4)
// chunks of 64 ranks a slice holds, by size: a slice is what a wave does
// between two claims, a few thousand passes
__host__ __device__ constexpr uint32_t bd_slice_chunks(int k) { return k == 4 ? 4u : 2u; }

// The 21 words of the 81 bytes at `src` (any alignment): rate_kernels.hip's loader
__device__ __forceinline__ void bd_load_words(const uint8_t *src, uint32_t (&x)[21])
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

// one agent-scope fetch-add by lane 0 of a 64-bit counter, the old value to every lane
__device__ __forceinline__ uint64_t bd_wave_claim64(unsigned long long *counter, unsigned long long k, int lane)
{
    unsigned long long h = 0;
    if (lane == 0) h = __hip_atomic_fetch_add(counter, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(h >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)h);
}

__device__ __forceinline__ void bd_write_code(int32_t *size, int32_t *count, uint8_t *first, uint8_t *cover, int64_t p,
                                              int32_t s, int32_t c)
{
    size[p] = s;
    if (count) count[p] = c;
    if (first) {
#pragma unroll
        for (int j = 0; j < 4; ++j) first[p * 4 + j] = 0xFFu;
    }
    if (cover) {
        for (int c81 = 0; c81 < 81; ++c81) cover[p * 81 + c81] = 0;
    }
}

__global__ __launch_bounds__(BD_THREADS, SDK_BACKDOOR_WAVES_PER_EU) void backdoor_root_kernel(
    const uint8_t *__restrict__ boards, const uint8_t *__restrict__ grids, int32_t *__restrict__ size,
    int32_t *__restrict__ count, uint8_t *__restrict__ first, uint8_t *__restrict__ cover, int64_t n, int level,
    unsigned long long *__restrict__ head, uint32_t *__restrict__ list_count, uint32_t *__restrict__ recs)
{
    const int lane = threadIdx.x;
    for (;;) {
        const int64_t base = (int64_t)bd_wave_claim64(head, 64ull, lane);
        if (base >= n) break;
        const int64_t p = base + lane;
        const bool have = p < n;
        plane::Board B;
        int st = rate::R_DEAD, code = 0;
        if (have) {
            uint32_t xb[21], xg[21];
            bd_load_words(boards + p * 81, xb);
            bd_load_words(grids + p * 81, xg);
            code = backdoor::validate(B, xb, xg);
            if (code == 0) st = rate::R_OPEN;
        }
        while (wany(st == rate::R_OPEN)) {
            if (st == rate::R_OPEN) {
                int o;
                st = rate::pass(B, level, o);
            }
        }
        if (have && st != rate::R_FIX) {
            // (a dead closure never happens: the grid is a completion and the rules are sound)
            if (code == 0 && st == rate::R_DEAD) code = backdoor::MISMATCH;
            bd_write_code(size, count, first, cover, p, code ? code : 0, code ? 0 : 1);
        }
        const bool lists = have && st == rate::R_FIX;
        const uint64_t listing = __builtin_amdgcn_ballot_w64(lists);
        if (listing) {
            uint32_t at = 0;
            if (lane == 0)
                at = __hip_atomic_fetch_add(list_count, (uint32_t)__builtin_popcountll(listing), __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
            at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
            if (lists) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(listing >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)listing, 0u));
                uint32_t *rec = recs + (size_t)(at + rank) * BD_WORDS;
#pragma unroll
                for (int w = 0; w < 27; ++w) rec[BD_CLOSURE + w] = B.P[w / 3][w % 3];
                uint32_t open[3];
                rec[BD_NOPEN] = backdoor::open_cells(B, open);
                rec[BD_COUNT] = 0u;
                rec[BD_FOUND] = 0u;
                rec[BD_FIRST] = 0xFFFFFFFFu;
#pragma unroll
                for (int b = 0; b < 3; ++b) rec[BD_COVER + b] = 0u;
                rec[BD_BOARD] = (uint32_t)p;
                rec[BD_BOARD + 1] = (uint32_t)((uint64_t)p >> 32);
                uint16_t *ent = (uint16_t *)(rec + BD_ENTRIES);
                uint32_t k = 0;
#pragma unroll 1
                for (int c = 0; c < 81; ++c) {
                    const int band = plane::cell_band(c), pos = plane::cell_pos(c);
                    if ((plane::band_word(open, band) >> pos) & 1u)
                        ent[k++] = (uint16_t)backdoor::entry_of(c, (uint32_t)grids[p * 81 + c]);
                }
            }
        }
    }
}

template <int K>
__global__ __launch_bounds__(BD_THREADS, SDK_BACKDOOR_WAVES_PER_EU) void backdoor_trial_kernel(
    uint32_t *__restrict__ recs, const uint32_t *__restrict__ list_count, unsigned long long *__restrict__ unit_head,
    int level, uint32_t slices)
{
    // the record; tallies of the slice: [0] solved trials, [1] their lowest rank, [2..4] cover
    __shared__ uint32_t R[BD_WORDS], acc[8];
    const int lane = threadIdx.x;
    const uint64_t total = (uint64_t)*list_count * slices;
    for (;;) {
        const uint64_t unit = bd_wave_claim64(unit_head, 1ull, lane);
        if (unit >= total) break;
        uint32_t *rec = recs + (size_t)(unit / slices) * BD_WORDS;
        const uint32_t slice = (uint32_t)(unit % slices);
        // (wave-uniform reads; BD_FOUND may be set by this launch's waves meanwhile, then to K)
        const uint32_t found = __hip_atomic_load(rec + BD_FOUND, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (found != 0u && found != (uint32_t)K) continue;  // a smaller size has answered this board
        const uint32_t nopen = rec[BD_NOPEN];
        const uint32_t ranks = backdoor::choose(nopen, K);
        const uint32_t begin = slice * (bd_slice_chunks(K) * 64u);
        if (begin >= ranks) continue;
        const uint32_t end = ranks - begin > bd_slice_chunks(K) * 64u ? begin + bd_slice_chunks(K) * 64u : ranks;
        R[lane] = rec[lane];
        if (lane < BD_WORDS - 64) R[64 + lane] = rec[64 + lane];
        if (lane < 8) acc[lane] = lane == 1 ? 0xFFFFFFFFu : 0u;
        wave_lds_sync();
        const uint16_t *ent = (const uint16_t *)(R + BD_ENTRIES);
        for (uint32_t base = begin; base < end; base += 64u) {
            const uint32_t r = base + (uint32_t)lane;
            const bool act = r < end;
            plane::Board T;
#pragma unroll
            for (int w = 0; w < 27; ++w) T.P[w / 3][w % 3] = R[BD_CLOSURE + w];
            uint32_t cov[3] = {0u, 0u, 0u};
            int st = rate::R_FIX;
            if (act) {
                backdoor::fix_subset<K>(T, r, nopen, [&](uint32_t i) { return (uint32_t)ent[i]; }, cov);
                st = rate::R_OPEN;
            }
            while (wany(st == rate::R_OPEN)) {
                if (st == rate::R_OPEN) {
                    int o;
                    st = rate::pass(T, level, o);
                }
            }
            const bool hit = act && st == rate::R_SOLVED;
            const uint64_t hits = __builtin_amdgcn_ballot_w64(hit);
            if (hits) {
                if (lane == 0) {
                    acc[0] += (uint32_t)__builtin_popcountll(hits);
                    const uint32_t lowest = base + (uint32_t)__builtin_ctzll(hits);  // ranks ascend with the lanes
                    if (lowest < acc[1]) acc[1] = lowest;
                }
                if (hit) {
#pragma unroll
                    for (int b = 0; b < 3; ++b)
                        if (cov[b]) atomicOr(&acc[2 + b], cov[b]);
                }
            }
        }
        wave_lds_sync();
        if (acc[0]) {
            if (lane == 0) {
                __hip_atomic_fetch_add(rec + BD_COUNT, acc[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_min(rec + BD_FIRST, acc[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(rec + BD_FOUND, (uint32_t)K, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (lane < 3 && acc[2 + lane])
                __hip_atomic_fetch_or(rec + BD_COVER + lane, acc[2 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        wave_lds_sync();  // everyone has read the tallies before the next unit stages over them
    }
}

__global__ __launch_bounds__(BD_THREADS) void backdoor_final_kernel(
    const uint32_t *__restrict__ recs, const uint32_t *__restrict__ list_count, int32_t *__restrict__ size,
    int32_t *__restrict__ count, uint8_t *__restrict__ first, uint8_t *__restrict__ cover, int max_size)
{
    const uint32_t listed = *list_count;
    const uint64_t stride = (uint64_t)gridDim.x * BD_THREADS;
    for (uint64_t at = (uint64_t)blockIdx.x * BD_THREADS + threadIdx.x; at < listed; at += stride) {
        const uint32_t *rec = recs + (size_t)at * BD_WORDS;
        const int64_t p = (int64_t)(((uint64_t)rec[BD_BOARD + 1] << 32) | rec[BD_BOARD]);
        const uint32_t found = rec[BD_FOUND];
        size[p] = found ? (int32_t)found : max_size + 1;
        if (count) count[p] = found ? (int32_t)rec[BD_COUNT] : 0;
        if (first) {
            uint32_t idx[backdoor::MAX_SIZE] = {0xFFu, 0xFFu, 0xFFu, 0xFFu};
            if (found) backdoor::unrank_k((int)found, rec[BD_FIRST], rec[BD_NOPEN], idx);
            const uint16_t *ent = (const uint16_t *)(rec + BD_ENTRIES);
#pragma unroll
            for (int j = 0; j < backdoor::MAX_SIZE; ++j) {
                const uint32_t e = ent[(uint32_t)j < found ? idx[j] : 0u];  // (no read past the entries)
                first[p * 4 + j] = (uint32_t)j < found ? (uint8_t)(e & 0xFFu) : (uint8_t)0xFFu;
            }
        }
        if (cover) {
            const uint32_t cv[3] = {rec[BD_COVER], rec[BD_COVER + 1], rec[BD_COVER + 2]};
            for (int c = 0; c < 81; ++c)
                cover[p * 81 + c] = (uint8_t)((plane::band_word(cv, plane::cell_band(c)) >> plane::cell_pos(c)) & 1u);
        }
    }
}

// ==================================================================== C ABI
static std::atomic<int> g_bd_root_bpc{0}, g_bd_trial_bpc[5];

// waves of a full grid on the current device: every CU at the kernel's occupancy
template <typename Kn>
static int64_t bd_full_waves(Kn kernel, std::atomic<int> &cache)
{
    const int per_cu = 4 * SDK_BACKDOOR_WAVES_PER_EU;  // four SIMDs per CU
    return (int64_t)sdk_device_cu_count() * cached_occupancy(kernel, BD_THREADS, per_cu, per_cu, cache);
}

template <int K>
static bool bd_launch_trials(uint32_t *recs, const uint32_t *list_count, uint8_t *sc, int64_t n, int level,
                             int max_waves, hipStream_t st)
{
    // slices: the ranks of a board with every cell open over a slice's ranks
    const uint32_t per = bd_slice_chunks(K) * 64u;
    const uint32_t slices = (backdoor::choose(81u, K) + per - 1u) / per;
    const int64_t cap = max_waves > 0 ? (int64_t)max_waves : bd_full_waves(backdoor_trial_kernel<K>, g_bd_trial_bpc[K]);
    const int64_t units = n * (int64_t)slices;  // (n < 2^31, slices < 2^13)
    hipLaunchKernelGGL(backdoor_trial_kernel<K>, dim3((unsigned)(units < cap ? units : cap)), dim3(BD_THREADS), 0, st,
                       recs, list_count, (unsigned long long *)(sc + BD_UNIT_HEAD_BYTE + 8 * K), level, slices);
    return hipGetLastError() == hipSuccess;
}

extern "C" {

size_t sdk_backdoor_scratch_bytes(int64_t n, int max_size, int max_waves)
{
    if (n < 0 || n > (int64_t)0x7FFFFFFF || max_size < 1 || max_size > SDK_BACKDOOR_MAX_SIZE || max_waves < 0) return 0;
    return BD_HEAD_BYTES + (size_t)n * BD_RECORD_BYTES;
}

int sdk_backdoor_batch(const uint8_t *d_boards, const uint8_t *d_grids, int32_t *d_size, int32_t *d_count,
                       uint8_t *d_first, uint8_t *d_cover, int64_t n, int level, int max_size, void *d_scratch,
                       size_t scratch_bytes, int max_waves, void *stream)
{
    if (n < 0 || n > (int64_t)0x7FFFFFFF || level < 1 || level > SDK_BACKDOOR_MAX_LEVEL || max_size < 1 ||
        max_size > SDK_BACKDOOR_MAX_SIZE || max_waves < 0)
        return -2;
    if (n == 0) return 0;
    if (!d_boards || !d_grids || !d_size || !d_scratch || ((uintptr_t)d_size & 3u) || ((uintptr_t)d_count & 3u) ||
        ((uintptr_t)d_scratch & 7u) || scratch_bytes < sdk_backdoor_scratch_bytes(n, max_size, max_waves))
        return -2;
    hipStream_t st = (hipStream_t)stream;
    // the queue heads and the list length, re-armed in stream order before the kernels
    if (hipMemsetAsync(d_scratch, 0, BD_HEAD_BYTES, st) != hipSuccess) return -1;
    uint8_t *sc = (uint8_t *)d_scratch;
    uint32_t *list_count = (uint32_t *)(sc + BD_LIST_COUNT_BYTE);
    uint32_t *recs = (uint32_t *)(sc + BD_HEAD_BYTES);
    const int64_t cap = max_waves > 0 ? (int64_t)max_waves : bd_full_waves(backdoor_root_kernel, g_bd_root_bpc);
    const int64_t want = n / 64 + (n % 64 != 0);
    const int64_t waves = want < cap ? want : cap;
    hipLaunchKernelGGL(backdoor_root_kernel, dim3((unsigned)waves), dim3(BD_THREADS), 0, st, d_boards, d_grids, d_size,
                       d_count, d_first, d_cover, n, level, (unsigned long long *)d_scratch, list_count, recs);
    if (hipGetLastError() != hipSuccess) return -1;
    // how many boards are listed is known on the device only: every size's launch is queued, a full grid at most
    if (!bd_launch_trials<1>(recs, list_count, sc, n, level, max_waves, st)) return -1;
    if (max_size >= 2 && !bd_launch_trials<2>(recs, list_count, sc, n, level, max_waves, st)) return -1;
    if (max_size >= 3 && !bd_launch_trials<3>(recs, list_count, sc, n, level, max_waves, st)) return -1;
    if (max_size >= 4 && !bd_launch_trials<4>(recs, list_count, sc, n, level, max_waves, st)) return -1;
    hipLaunchKernelGGL(backdoor_final_kernel, dim3((unsigned)waves), dim3(BD_THREADS), 0, st, (const uint32_t *)recs,
                       (const uint32_t *)list_count, d_size, d_count, d_first, d_cover, max_size);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
