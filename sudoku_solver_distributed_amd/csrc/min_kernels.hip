// min_kernels.hip -- translation unit of the batched minimisation
// (plane_min.h): min_kernel and its C ABI entries
// (sdk_minimize_scratch_bytes, sdk_minimize_batch).  A unit of its own, like
// count_kernels.hip and cand_kernels.hip: the other units, their flags and the
// solve workspace are not involved (common.h is included for cached_occupancy
// alone).
//
// min_kernel: cand_kernel's shape.  One board per LANE, persistent one-wave
// workgroups.  A lane holds its board's 27 plane words, und[] / nd[]
// (plane::pass_ahead), its stack depth, its mode word (plane_min.h: the phase,
// the turn, the cell under test, the givens removed) and the board's index,
// and runs one plane::min_iter per loop iteration: every lane, in whatever
// phase or turn, shares the iteration's one pass_ahead; the end of a test and
// the next turn are the divergent block beside it, as count_step is.  When
// SDK_MIN_REFILL lanes of a wave are idle (all 64 at the start) lane 0 claims
// that many boards with ONE agent-scope fetch-add on the queue head; idle lane
// number r takes board head + r.  Once a claim reaches the end of the batch
// the wave claims no more and exits when its last board is finished.  A
// refilled lane reads its 81 bytes as 21 aligned dwords, funnel-shifted into
// the words plane::load_words takes.
//
// The working copy.  A refilled lane copies its board to its row of d_out,
// byte by byte (any alignment); from then on the row is the lane's puzzle P: a
// kept removal is one byte store, the digit under test one byte load of a byte
// the lane itself wrote, the turn's cell one byte load of d_order, and the
// answer needs no conversion at the end -- a finished lane writes its int32
// status (and removed count) at once.  A fault copies the input row again.
//
// Scratch: [0, 256) the queue head's block (zeroed by the call itself, in
// stream order, before the kernel), then per wave 64 lanes x MIN_LEVELS (82)
// lines of 128 bytes: plane_stack.h's PlaneStack, levels 0..80 the search's,
// 81 the puzzle's loaded planes with the given mask in its und[] slot.  Each
// wave addresses its own lines through a buffer descriptor that covers
// exactly them.
#include "common.h"
#include "plane_min.h"
#include "plane_stack.h"

#define MIN_THREADS 64    // one wave per workgroup
#define MIN_WAVES_PER_EU 4
#define MIN_HEAD_BYTES 256
// idle lanes before a wave claims boards (results never depend on it): the
// count's measured choice (count_kernels.hip)
#ifndef SDK_MIN_REFILL
#define SDK_MIN_REFILL 16
#endif
#define MIN_LANE_BYTES ((uint32_t)plane::MIN_LEVELS * 128u)
#define MIN_WAVE_BYTES (64u * MIN_LANE_BYTES)

// The 21 words of the board at `src` (any alignment): the 21 aligned dwords
// that hold its 81 bytes (byte 80 lies in dword 20 for every alignment, so
// every dword read holds a byte of the board), funnel-shifted into place.
// Only byte 0 of x[20] is the board's.
__device__ __forceinline__ void min_load_words(const uint8_t *src, uint32_t (&x)[21])
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

// a lane's view of its board: the turns (NULL: turn t takes cell t) and the
// working copy in d_out
struct MinIo {
    const uint8_t *turns;
    uint8_t *out;
    __device__ __forceinline__ uint32_t order(uint32_t t) const { return turns ? (uint32_t)turns[t] : t; }
    __device__ __forceinline__ uint32_t digit(uint32_t c) const { return out[c]; }
    __device__ __forceinline__ void erase(uint32_t c) const { out[c] = 0; }
};

__global__ __launch_bounds__(MIN_THREADS, MIN_WAVES_PER_EU) void min_kernel(
    const uint8_t *__restrict__ boards, const uint8_t *__restrict__ order, uint8_t *out, int32_t *__restrict__ status,
    int32_t *__restrict__ removed, int64_t n, uint32_t probe, uint32_t max_empty, unsigned long long *__restrict__ head,
    uint8_t *__restrict__ stack)
{
    const int lane = threadIdx.x;
    const PlaneStack stk = {__builtin_amdgcn_make_buffer_rsrc(stack + (size_t)blockIdx.x * MIN_WAVE_BYTES, 0,
                                                              (int)MIN_WAVE_BYTES, 0x00020000),
                            (uint32_t)lane * MIN_LANE_BYTES};
    plane::Board B;
    uint32_t und[3] = {0u, 0u, 0u}, nd[3] = {0u, 0u, 0u}, depth = 0, mode = 0;
    int64_t p = 0;            // this lane's board
    bool active = false, queue_out = false;
    for (;;) {
        const uint64_t idle = __builtin_amdgcn_ballot_w64(!active);
        const int nidle = __builtin_popcountll(idle);
        if (queue_out && nidle == 64) break;
        if (!queue_out && nidle >= SDK_MIN_REFILL) {
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
                min_load_words(boards + p * 81, x);
                uint8_t *dst = out + p * 81;  // the working copy
#pragma unroll
                for (int i = 0; i < 81; ++i) dst[i] = (uint8_t)(x[i >> 2] >> (8 * (i & 3)));
                bool clash = false;
                int32_t s = 0;  // clashing givens: no valid completion; rules B-D are unsound on them
                if (!plane::load_words(B, x, clash, given)) {
                    s = SDK_INVALID;
                } else if (!clash) {
                    active = true;
                    plane::min_start(B, given, und, nd, depth, mode, stk);
                }
                if (!active) {
                    status[p] = s;
                    if (removed) removed[p] = 0;
                }
            }
        }
        if (active) {
            const MinIo io = {order ? order + p * 81 : nullptr, out + p * 81};
            const int k = plane::min_iter(B, und, nd, depth, mode, stk, (uint32_t)plane::COUNT_MAX_DEPTH, probe != 0u,
                                          max_empty, io);
            if (k != plane::N_CONT) {
                active = false;
                const bool fault = k == plane::N_FAULT;
                if (fault) {  // never a partial result: the input row again
                    const uint8_t *src = boards + p * 81;
                    for (int i = 0; i < 81; ++i) io.out[i] = src[i];
                }
                status[p] = fault ? SDK_FAULT : plane::min_status(mode);
                if (removed) removed[p] = fault ? 0 : (int32_t)plane::min_removed(mode);
            }
        }
    }
}

// ==================================================================== C ABI
static std::atomic<int> g_min_bpc{0};

// waves of a full grid on the current device: every CU at the kernel's occupancy
static int64_t min_full_waves()
{
    const int per_cu = 4 * MIN_WAVES_PER_EU;  // four SIMDs per CU
    return (int64_t)sdk_device_cu_count() * cached_occupancy(min_kernel, MIN_THREADS, per_cu, per_cu, g_min_bpc);
}

static int64_t min_waves(int64_t n, int max_waves)
{
    const int64_t cap = max_waves > 0 ? (int64_t)max_waves : min_full_waves();
    const int64_t want = n / 64 + (n % 64 != 0);  // (n + 63 would overflow at INT64_MAX)
    return want < cap ? want : cap;
}

extern "C" {

size_t sdk_minimize_scratch_bytes(int64_t n, int max_waves)
{
    if (n < 0 || max_waves < 0) return 0;
    return MIN_HEAD_BYTES + (size_t)min_waves(n, max_waves) * MIN_WAVE_BYTES;
}

int sdk_minimize_batch(const uint8_t *d_boards, const uint8_t *d_order, uint8_t *d_out, int32_t *d_status,
                       int32_t *d_removed, int64_t n, int mode, int max_empty, void *d_scratch, size_t scratch_bytes,
                       int max_waves, void *stream)
{
    if (n == 0) return 0;
    if (n < 0 || max_waves < 0 || (mode != SDK_MIN_GREEDY && mode != SDK_MIN_PROBE) || max_empty < 0 || max_empty > 81)
        return -2;
    if (!d_boards || !d_out || d_out == d_boards || !d_status || ((uintptr_t)d_status & 3u) ||
        ((uintptr_t)d_removed & 3u) || !d_scratch || ((uintptr_t)d_scratch & 7u) ||
        scratch_bytes < sdk_minimize_scratch_bytes(n, max_waves))
        return -2;
    hipStream_t st = (hipStream_t)stream;
    // the queue head, re-armed in stream order before the kernel
    if (hipMemsetAsync(d_scratch, 0, MIN_HEAD_BYTES, st) != hipSuccess) return -1;
    const int64_t waves = min_waves(n, max_waves);
    const bool probe = mode == SDK_MIN_PROBE;
    hipLaunchKernelGGL(min_kernel, dim3((unsigned)waves), dim3(MIN_THREADS), 0, st, d_boards, probe ? nullptr : d_order,
                       d_out, d_status, d_removed, n, probe ? 1u : 0u, (uint32_t)max_empty, (unsigned long long *)d_scratch,
                       (uint8_t *)d_scratch + MIN_HEAD_BYTES);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
