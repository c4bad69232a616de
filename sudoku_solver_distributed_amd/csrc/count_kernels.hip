// count_kernels.hip -- translation unit of the batched, capped completion
// count (plane_count.h): count_kernel and its C ABI entries
// (sdk_count_scratch_bytes, sdk_count_solutions_batch).  A unit of its own:
// the solve kernels' units, their flags and their workspace are not involved.
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
// stack lines of 128 bytes in the layout plane_kernel.h's PlaneStack
// documents (words 0..26 planes, 27 entry, 28..30 und[], 31 unused).  Each
// wave addresses its own lines through a buffer descriptor that covers
// exactly them, so a bad level could never reach another wave's lines.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/sudoku_hip.h"
#include "plane_count.h"

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

typedef uint32_t cnt_v4u __attribute__((ext_vector_type(4)));

// The lane's stack lines (level L at lane_off + 128 L within the wave's
// descriptor).  A push or pop is 8 dwordx4 accesses to one line.
struct CountStack {
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t lane_off;
    __device__ __forceinline__ int voff(uint32_t level) const { return (int)(lane_off + level * 128u); }
    __device__ __forceinline__ void push(uint32_t level, plane::Board &B, const uint32_t (&und)[3],
                                         uint32_t entry) const
    {
        const int v = voff(level);
        plane::pin_board(B);
#define CQ(a, b, c, d) (cnt_v4u){B.P[a / 3][a % 3], B.P[b / 3][b % 3], B.P[c / 3][c % 3], B.P[d / 3][d % 3]}
        const cnt_v4u q0 = CQ(0, 1, 2, 3), q1 = CQ(4, 5, 6, 7), q2 = CQ(8, 9, 10, 11), q3 = CQ(12, 13, 14, 15),
                      q4 = CQ(16, 17, 18, 19), q5 = CQ(20, 21, 22, 23),
                      q6 = (cnt_v4u){B.P[8][0], B.P[8][1], B.P[8][2], entry},
                      q7 = (cnt_v4u){und[0], und[1], und[2], 0u};
#undef CQ
        __builtin_amdgcn_raw_buffer_store_b128(q0, rsrc, v, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q1, rsrc, v, 16, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q2, rsrc, v, 32, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q3, rsrc, v, 48, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q4, rsrc, v, 64, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q5, rsrc, v, 80, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q6, rsrc, v, 96, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q7, rsrc, v, 112, 0);
        // a dwordx4 store reads its data registers after issue, and hipcc does
        // not always pad a following VALU write of them (PlaneStack::push,
        // scripts/store_hazard_check.py): all eight quads stay live through
        // two wait states
        asm volatile("s_nop 1" ::"v"(q0), "v"(q1), "v"(q2), "v"(q3), "v"(q4), "v"(q5), "v"(q6), "v"(q7));
    }
    __device__ __forceinline__ uint32_t pop(uint32_t level, plane::Board &B, uint32_t (&und)[3]) const
    {
        const int v = voff(level);
        const cnt_v4u q0 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 0, 0);
        const cnt_v4u q1 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 16, 0);
        const cnt_v4u q2 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 32, 0);
        const cnt_v4u q3 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 48, 0);
        const cnt_v4u q4 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 64, 0);
        const cnt_v4u q5 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 80, 0);
        const cnt_v4u t = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 96, 0);
        const cnt_v4u u = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 112, 0);
        und[0] = u.x; und[1] = u.y; und[2] = u.z;
        B.P[0][0] = q0.x; B.P[0][1] = q0.y; B.P[0][2] = q0.z; B.P[1][0] = q0.w;
        B.P[1][1] = q1.x; B.P[1][2] = q1.y; B.P[2][0] = q1.z; B.P[2][1] = q1.w;
        B.P[2][2] = q2.x; B.P[3][0] = q2.y; B.P[3][1] = q2.z; B.P[3][2] = q2.w;
        B.P[4][0] = q3.x; B.P[4][1] = q3.y; B.P[4][2] = q3.z; B.P[5][0] = q3.w;
        B.P[5][1] = q4.x; B.P[5][2] = q4.y; B.P[6][0] = q4.z; B.P[6][1] = q4.w;
        B.P[6][2] = q5.x; B.P[7][0] = q5.y; B.P[7][1] = q5.z; B.P[7][2] = q5.w;
        B.P[8][0] = t.x; B.P[8][1] = t.y; B.P[8][2] = t.z;
        return t.w;
    }
    __device__ __forceinline__ void put_entry(uint32_t level, uint32_t entry) const
    {
        __builtin_amdgcn_raw_buffer_store_b32(entry, rsrc, voff(level), 108, 0);
    }
};

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
    const CountStack stk = {__builtin_amdgcn_make_buffer_rsrc(stack + (size_t)blockIdx.x * COUNT_WAVE_BYTES, 0,
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
    int nb = g_count_bpc.load();
    if (!nb) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, count_kernel, COUNT_THREADS, 0) != hipSuccess || nb <= 0)
            nb = 4 * COUNT_WAVES_PER_EU;
        if (nb > 4 * COUNT_WAVES_PER_EU) nb = 4 * COUNT_WAVES_PER_EU;  // four SIMDs per CU
        g_count_bpc.store(nb);
    }
    return (int64_t)sdk_device_cu_count() * nb;
}

static int64_t count_waves(int64_t n, int max_waves)
{
    const int64_t cap = max_waves > 0 ? (int64_t)max_waves : count_full_waves();
    const int64_t want = (n + 63) / 64;
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
