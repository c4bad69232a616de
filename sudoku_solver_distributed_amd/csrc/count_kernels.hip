// count_kernels.hip -- translation unit of the batched, capped completion
// count (plane_count.h): count_kernel and its C ABI entries
// (sdk_count_scratch_bytes, sdk_count_solutions_batch).  A unit of its own:
// the solve kernels' units, their flags and their workspace are not involved
// (common.h is included for cached_occupancy alone).
//
// count_kernel: one board per LANE, persistent one-wave workgroups.  A lane
// holds its board's 27 plane words, und[] / nd[] (plane::pass_ahead), its
// stack depth, its count so far and the board's index, and runs one
// plane::count_iter per loop iteration.  When SDK_COUNT_REFILL lanes of a wave are
// idle (all 64 at the start) lane 0 claims that many boards with ONE agent-
// scope fetch-add on the queue head; idle lane number r takes board head + r.
// Once a claim reaches the end of the batch the wave claims no more; it exits
// when its last board is finished (lanes idle at the drain: there is no
// wave-wide tail in this version).  A refilled lane reads its 81 bytes as 21
// aligned dwords, funnel-shifted into the 21 words plane::load_words takes.
// A finished lane writes its int32 count; the first completion goes out the
// moment it is found, while the planes hold it.
//
// Scratch: [0, 256) the queue head's block (zeroed by the call itself, in
// stream order, before the kernel), then per wave 64 lanes x COUNT_MAX_DEPTH
// stack lines of 128 bytes, pushed and popped by plane_stack.h's PlaneStack
// (words 0..26 planes, 27 entry, 28..30 und[], 31 unused; level L of a lane
// at lane_off + 128 L).  Each wave addresses its own lines through a buffer
// descriptor that covers exactly them, so a bad level could never reach
// another wave's lines.
#include "common.h"
#include "plane_count.h"
#include "plane_stack.h"

#define COUNT_THREADS 64    // one wave per workgroup
#define COUNT_WAVES_PER_EU 4
#define COUNT_HEAD_BYTES 256
// idle lanes before a wave claims boards (results never depend on it): a
// refill costs the whole wave about a third of a pass (load_words) and one
// atomic on the launch's single queue head.  Measured on 2^20 17-clue boards
// at limit 2: 2.40 ms at 4, 1.54 at 16, 1.58 at 32, 2.72 at 64
#ifndef SDK_COUNT_REFILL
#define SDK_COUNT_REFILL 16
#endif
#define COUNT_LANE_BYTES ((uint32_t)plane::COUNT_MAX_DEPTH * 128u)
#define COUNT_WAVE_BYTES (64u * COUNT_LANE_BYTES)
#define COUNT_NONE INT32_MIN  // a lane with no result to write

// The 21 words of the board at `src` (any alignment): the 21 aligned dwords
// that hold its 81 bytes (byte 80 lies in dword 20 for every alignment, so
// every dword read holds a byte of the board), funnel-shifted into place.
// Only byte 0 of x[20] is the board's (load_words reads no other).
__device__ __forceinline__ void count_load_words(const uint8_t *src, uint32_t (&x)[21])
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

__global__ __launch_bounds__(COUNT_THREADS, COUNT_WAVES_PER_EU) void count_kernel(
    const uint8_t *__restrict__ puzzles, int32_t *__restrict__ count, uint8_t *__restrict__ first, int64_t n,
    int32_t limit, unsigned long long *__restrict__ head, uint8_t *__restrict__ stack)
{
    const int lane = threadIdx.x;
    const PlaneStack stk = {__builtin_amdgcn_make_buffer_rsrc(stack + (size_t)blockIdx.x * COUNT_WAVE_BYTES, 0,
                                                              (int)COUNT_WAVE_BYTES, 0x00020000),
                            (uint32_t)lane * COUNT_LANE_BYTES};
    plane::Board B;
    uint32_t und[3] = {0u, 0u, 0u}, nd[3] = {0u, 0u, 0u}, depth = 0;
    int32_t found = 0;
    int64_t p = 0;  // this lane's board
    bool active = false, queue_out = false;
    for (;;) {
        int32_t res = COUNT_NONE;  // the finished board's answer, written at the end of the iteration
        const uint64_t idle = __builtin_amdgcn_ballot_w64(!active);
        const int nidle = __builtin_popcountll(idle);
        if (queue_out && nidle == 64) break;
        if (!queue_out && nidle >= SDK_COUNT_REFILL) {
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
                uint32_t x[21], given[3];
                count_load_words(puzzles + p * 81, x);
                bool clash = false;
                if (!plane::load_words(B, x, clash, given)) {
                    res = SDK_INVALID;
                } else if (clash) {
                    res = 0;  // no valid completion; rules B-D are unsound on such givens
                } else {
                    active = true;
                    depth = 0;
                    found = 0;
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        nd[b] = given[b];
                        und[b] = plane::andn(plane::ROWS, given[b]);
                    }
                }
            }
        }
        if (active) {
            uint8_t *dst = first ? first + p * 81 : nullptr;
            const bool done = plane::count_iter(B, und, nd, depth, found, limit, stk, (uint32_t)plane::COUNT_MAX_DEPTH,
                                                [&](const plane::Board &S) {
                                                    if (dst)
                                                        plane::store_values(S, [&](int c, uint32_t v) { dst[c] = (uint8_t)v; });
                                                });
            if (done) {
                res = found;
                active = false;
            }
        }
        if (res != COUNT_NONE) {
            count[p] = res;
            if (first && res <= 0) {  // no completion to show: the input board back
                const uint8_t *src = puzzles + p * 81;
                uint8_t *dst = first + p * 81;
                for (int i = 0; i < 81; ++i) dst[i] = src[i];
            }
        }
    }
}

// ==================================================================== C ABI
static std::atomic<int> g_count_bpc{0};

// waves of a full grid on the current device: every CU at the kernel's occupancy
static int64_t count_full_waves()
{
    const int per_cu = 4 * COUNT_WAVES_PER_EU;  // four SIMDs per CU
    return (int64_t)sdk_device_cu_count() * cached_occupancy(count_kernel, COUNT_THREADS, per_cu, per_cu, g_count_bpc);
}

static int64_t count_waves(int64_t n, int max_waves)
{
    const int64_t cap = max_waves > 0 ? (int64_t)max_waves : count_full_waves();
    const int64_t want = n / 64 + (n % 64 != 0);  // (n + 63 would overflow at INT64_MAX)
    return want < cap ? want : cap;
}

extern "C" {

size_t sdk_count_scratch_bytes(int64_t n, int max_waves)
{
    if (n < 0 || max_waves < 0) return 0;
    return COUNT_HEAD_BYTES + (size_t)count_waves(n, max_waves) * COUNT_WAVE_BYTES;
}

int sdk_count_solutions_batch(const uint8_t *d_puzzles, int32_t *d_count, uint8_t *d_first, int64_t n, int limit,
                              void *d_scratch, size_t scratch_bytes, int max_waves, void *stream)
{
    if (n < 0 || max_waves < 0 || limit < 1 || limit > SDK_COUNT_MAX_LIMIT) return -2;
    if (n == 0) return 0;
    if (!d_puzzles || !d_count || !d_scratch || scratch_bytes < sdk_count_scratch_bytes(n, max_waves)) return -2;
    hipStream_t st = (hipStream_t)stream;
    // the queue head, re-armed in stream order before the kernel
    if (hipMemsetAsync(d_scratch, 0, COUNT_HEAD_BYTES, st) != hipSuccess) return -1;
    const int64_t waves = count_waves(n, max_waves);
    hipLaunchKernelGGL(count_kernel, dim3((unsigned)waves), dim3(COUNT_THREADS), 0, st, d_puzzles, d_count, d_first, n,
                       (int32_t)limit, (unsigned long long *)d_scratch, (uint8_t *)d_scratch + COUNT_HEAD_BYTES);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
