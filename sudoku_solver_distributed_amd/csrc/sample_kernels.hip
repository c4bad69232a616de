// sample_kernels.hip -- translation unit of the batched random completion
// (plane_sample.h): sample_kernel and its C ABI entries
// (sdk_sample_scratch_bytes, sdk_sample_batch).  A unit of its own, like
// count_kernels.hip and min_kernels.hip: the other units, their flags and the
// solve workspace are not involved (common.h is included for cached_occupancy
// alone).
//
// sample_kernel: min_kernel's shape.  One ITEM per lane, persistent one-wave
// workgroups.  Item q is board q / per_board under key first_key + q.  A lane
// holds its board's 27 plane words, und[] / nd[] (plane::pass_ahead), its
// stack depth, the item's stream h (two registers), its draw counter t and the
// item's index, and runs one plane::sample_iter per loop iteration.  When
// SDK_SAMPLE_REFILL lanes of a wave are idle (all 64 at the start) lane 0
// claims that many items with ONE agent-scope fetch-add on the queue head;
// idle lane number r takes item head + r.  Once a claim reaches the end of the
// batch the wave claims no more and exits when its last item is finished.  A
// refilled lane reads its board's 81 bytes as 21 aligned dwords, funnel-
// shifted into the words plane::load_words takes; with boards == NULL the
// words are zero and no board byte is read.  The completion goes out with
// plane::store_values at the SOLVED verdict, while the planes hold it; an item
// without one gets its input row back.  Which lane or wave runs an item, the
// grid and the refill threshold never change an answer: a draw is a hash of
// (seed, key, t) alone.
//
// Scratch: [0, 256) the queue head's block (zeroed by the call itself, in
// stream order, before the kernel), then per wave 64 lanes x COUNT_MAX_DEPTH
// (81) lines of 128 bytes: plane_stack.h's PlaneStack.  Each wave addresses
// its own lines through a buffer descriptor that covers exactly them.
#include "common.h"
#include "plane_sample.h"
#include "plane_stack.h"

#define SAMPLE_THREADS 64    // one wave per workgroup
#define SAMPLE_WAVES_PER_EU 4
#define SAMPLE_HEAD_BYTES 256
// idle lanes before a wave claims items (results never depend on it): the
// count's measured choice (count_kernels.hip)
#ifndef SDK_SAMPLE_REFILL
#define SDK_SAMPLE_REFILL 16
#endif
#define SAMPLE_LANE_BYTES ((uint32_t)plane::COUNT_MAX_DEPTH * 128u)
#define SAMPLE_WAVE_BYTES (64u * SAMPLE_LANE_BYTES)
#define SAMPLE_MAX_ITEMS ((int64_t)INT32_MAX)

// The 21 words of the board at `src` (any alignment): the 21 aligned dwords
// that hold its 81 bytes (byte 80 lies in dword 20 for every alignment, so
// every dword read holds a byte of the board), funnel-shifted into place.
// Only byte 0 of x[20] is the board's.
__device__ __forceinline__ void sample_load_words(const uint8_t *src, uint32_t (&x)[21])
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

// seed_mix: plane::sample_mix(seed), the same for every item of the call
__global__ __launch_bounds__(SAMPLE_THREADS, SAMPLE_WAVES_PER_EU) void sample_kernel(
    const uint8_t *__restrict__ boards, uint8_t *__restrict__ out, int32_t *__restrict__ status, int64_t items,
    uint32_t per_board, uint64_t seed_mix, uint64_t first_key, unsigned long long *__restrict__ head,
    uint8_t *__restrict__ stack)
{
    const int lane = threadIdx.x;
    const PlaneStack stk = {__builtin_amdgcn_make_buffer_rsrc(stack + (size_t)blockIdx.x * SAMPLE_WAVE_BYTES, 0,
                                                              (int)SAMPLE_WAVE_BYTES, 0x00020000),
                            (uint32_t)lane * SAMPLE_LANE_BYTES};
    plane::Board B;
    uint32_t und[3] = {0u, 0u, 0u}, nd[3] = {0u, 0u, 0u}, depth = 0, t = 0;
    uint64_t h = 0;  // this lane's stream
    int64_t p = 0;   // this lane's item
    bool active = false, queue_out = false;
    for (;;) {
        const uint64_t idle = __builtin_amdgcn_ballot_w64(!active);
        const int nidle = __builtin_popcountll(idle);
        if (queue_out && nidle == 64) break;
        int32_t res = 1;  // the answer of an item that ends in this iteration without a completion
        bool ended = false;
        if (!queue_out && nidle >= SDK_SAMPLE_REFILL) {
            unsigned long long hd = 0;
            if (lane == 0)
                hd = __hip_atomic_fetch_add(head, (unsigned long long)nidle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t base = (int64_t)(((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(hd >> 32)) << 32) |
                                           __builtin_amdgcn_readfirstlane((uint32_t)hd));
            queue_out = base + nidle >= items;  // the batch's end is handed out: no further claim
            const int64_t q = base + (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            if (!active && q < items) {
                p = q;
                uint32_t x[21], given[3];
                if (boards) {
                    sample_load_words(boards + (int64_t)((uint32_t)p / per_board) * 81, x);  // items < 2^31
                } else {
#pragma unroll
                    for (int k = 0; k < 21; ++k) x[k] = 0u;
                }
                bool clash = false;
                if (!plane::load_words(B, x, clash, given)) {
                    res = SDK_INVALID;
                    ended = true;
                } else if (clash) {
                    res = 0;  // no valid completion; rules B-D are unsound on such givens
                    ended = true;
                } else {
                    active = true;
                    depth = 0;
                    t = 0;
                    h = plane::sample_mix(seed_mix + first_key + (uint64_t)p);
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        nd[b] = given[b];
                        und[b] = plane::andn(plane::ROWS, given[b]);
                    }
                }
            }
        }
        if (active) {
            const int k = plane::sample_iter(B, und, nd, depth, stk, (uint32_t)plane::COUNT_MAX_DEPTH, h, t);
            if (k != plane::P_CONT) {
                active = false;
                if (k == plane::P_FOUND) {
                    uint8_t *dst = out + p * 81;
                    plane::store_values(B, [&](int c, uint32_t v) { dst[c] = (uint8_t)v; });
                    status[p] = 1;
                } else {
                    res = k == plane::P_NONE ? 0 : SDK_FAULT;
                    ended = true;
                }
            }
        }
        if (ended) {  // no completion to show: the input board back, never a partial grid
            status[p] = res;
            uint8_t *dst = out + p * 81;
            if (boards) {
                const uint8_t *src = boards + (int64_t)((uint32_t)p / per_board) * 81;
                for (int i = 0; i < 81; ++i) dst[i] = src[i];
            } else {
                for (int i = 0; i < 81; ++i) dst[i] = 0;
            }
        }
    }
}

// ==================================================================== C ABI
static std::atomic<int> g_sample_bpc{0};

// waves of a full grid on the current device: every CU at the kernel's occupancy
static int64_t sample_full_waves()
{
    const int per_cu = 4 * SAMPLE_WAVES_PER_EU;  // four SIMDs per CU
    return (int64_t)sdk_device_cu_count() *
           cached_occupancy(sample_kernel, SAMPLE_THREADS, per_cu, per_cu, g_sample_bpc);
}

static int64_t sample_waves(int64_t items, int max_waves)
{
    const int64_t cap = max_waves > 0 ? (int64_t)max_waves : sample_full_waves();
    const int64_t want = items / 64 + (items % 64 != 0);  // (items + 63 would overflow at INT64_MAX)
    return want < cap ? want : cap;
}

extern "C" {

size_t sdk_sample_scratch_bytes(int64_t items, int max_waves)
{
    if (items < 0 || max_waves < 0) return 0;
    return SAMPLE_HEAD_BYTES + (size_t)sample_waves(items, max_waves) * SAMPLE_WAVE_BYTES;
}

int sdk_sample_batch(const uint8_t *d_boards, uint8_t *d_out, int32_t *d_status, int64_t n, int per_board, uint64_t seed,
                     uint64_t first_key, void *d_scratch, size_t scratch_bytes, int max_waves, void *stream)
{
    if (n == 0) return 0;
    if (n < 0 || max_waves < 0 || per_board < 1 || n > SAMPLE_MAX_ITEMS / per_board) return -2;
    const int64_t items = n * per_board;
    if (!d_out || d_out == d_boards || !d_status || ((uintptr_t)d_status & 3u) || !d_scratch ||
        ((uintptr_t)d_scratch & 7u) || scratch_bytes < sdk_sample_scratch_bytes(items, max_waves))
        return -2;
    hipStream_t st = (hipStream_t)stream;
    // the queue head, re-armed in stream order before the kernel
    if (hipMemsetAsync(d_scratch, 0, SAMPLE_HEAD_BYTES, st) != hipSuccess) return -1;
    const int64_t waves = sample_waves(items, max_waves);
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)waves), dim3(SAMPLE_THREADS), 0, st, d_boards, d_out, d_status, items,
                       (uint32_t)per_board, plane::sample_mix(seed), first_key, (unsigned long long *)d_scratch,
                       (uint8_t *)d_scratch + SAMPLE_HEAD_BYTES);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
