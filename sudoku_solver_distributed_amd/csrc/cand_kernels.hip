// cand_kernels.hip -- translation unit of the batched exact candidates
// (plane_cand.h): cand_kernel and its C ABI entries
// (sdk_candidates_scratch_bytes, sdk_candidates_batch).  A unit of its own,
// like count_kernels.hip: the other units, their flags and the solve
// workspace are not involved (common.h is included for cached_occupancy alone).
//
// cand_kernel: count_kernel's shape.  One board per LANE, persistent one-wave
// workgroups.  A lane holds its board's 27 plane words, und[] / nd[]
// (plane::pass_ahead), its stack depth, its mode word (plane_cand.h; on an
// idle lane, the answer pending for its board) and the board's index, and
// runs one plane::cand_iter per loop iteration: every lane, in whatever
// phase, shares the iteration's one pass_ahead; the phase changes
// (a completion OR-ed into W, the root saved, the next target picked) are the
// divergent blocks beside it, as count_step is.  When SDK_CAND_REFILL lanes of
// a wave are idle (all 64 at the start) lane 0 claims that many boards with
// ONE agent-scope fetch-add on the queue head; idle lane number r takes board
// head + r.  Once a claim reaches the end of the batch the wave claims no
// more and exits when its last board is finished.  A refilled lane reads its
// 81 bytes as 21 aligned dwords, funnel-shifted into the words
// plane::load_words takes.
//
// Answers.  A finished lane's W already sits in its line, so the lane only
// notes that an answer is pending; the 81-cell conversion (plane::cand_marks:
// 81 16-bit stores and the int32 count) runs at the wave's next refill, or at
// its exit, once for all lanes that finished since -- not in every iteration
// in which some lane finishes (measured: that takes 56 % longer on boards
// with one completion).  A board answered without a search (a byte > 9,
// clashing givens) and a fault go the same way with zero planes.
//
// Scratch: [0, 256) the queue head's block (zeroed by the call itself, in
// stream order, before the kernel), then per wave 64 lanes x CAND_LEVELS (83)
// lines of 128 bytes: plane_stack.h's PlaneStack, levels 0..80 the search's,
// 81 the closed root R with its und[], 82 the witnessed candidates W.  Each
// wave addresses its own lines through a buffer descriptor that covers
// exactly them.
#include "common.h"
#include "plane_cand.h"
#include "plane_stack.h"

#define CAND_THREADS 64    // one wave per workgroup
#define CAND_WAVES_PER_EU 4
#define CAND_HEAD_BYTES 256
// idle lanes before a wave claims boards (results never depend on it): the
// count's measured choice (count_kernels.hip); here a refill also converts
// the answers of the lanes that finished
#ifndef SDK_CAND_REFILL
#define SDK_CAND_REFILL 16
#endif
#define CAND_LANE_BYTES ((uint32_t)plane::CAND_LEVELS * 128u)
#define CAND_WAVE_BYTES (64u * CAND_LANE_BYTES)
// an idle lane's mode word: the answer pending for its board (0: none)
enum : uint32_t { CAND_FROM_W = 1, CAND_ZERO = 2, CAND_BAD_BYTE = 3, CAND_FAULTED = 4 };

// The 21 words of the board at `src` (any alignment): the 21 aligned dwords
// that hold its 81 bytes (byte 80 lies in dword 20 for every alignment, so
// every dword read holds a byte of the board), funnel-shifted into place.
// Only byte 0 of x[20] is the board's (load_words reads no other).
__device__ __forceinline__ void cand_load_words(const uint8_t *src, uint32_t (&x)[21])
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

__global__ __launch_bounds__(CAND_THREADS, CAND_WAVES_PER_EU) void cand_kernel(
    const uint8_t *__restrict__ boards, uint16_t *__restrict__ marks, int32_t *__restrict__ count, int64_t n,
    uint32_t sweep, unsigned long long *__restrict__ head, uint8_t *__restrict__ stack)
{
    const int lane = threadIdx.x;
    const PlaneStack stk = {__builtin_amdgcn_make_buffer_rsrc(stack + (size_t)blockIdx.x * CAND_WAVE_BYTES, 0,
                                                              (int)CAND_WAVE_BYTES, 0x00020000),
                            (uint32_t)lane * CAND_LANE_BYTES};
    plane::Board B;
    uint32_t und[3] = {0u, 0u, 0u}, nd[3] = {0u, 0u, 0u}, depth = 0, mode = 0;
    int64_t p = 0;            // this lane's board
    bool active = false, queue_out = false;
    for (;;) {
        const uint64_t idle = __builtin_amdgcn_ballot_w64(!active);
        const int nidle = __builtin_popcountll(idle);
        const bool leave = queue_out && nidle == 64;
        const bool refill = !queue_out && nidle >= SDK_CAND_REFILL;
        if ((leave || refill) && !active && mode) {
            // the answers of the lanes that finished since the last refill
            // (an idle lane's B is dead: W's planes take its registers)
            uint32_t tu[3];
            if (mode == CAND_FROM_W) {
                stk.pop(plane::cand_level(plane::CAND_WIT_LEVEL), B, tu);
            } else {
#pragma unroll
                for (int d = 0; d < 9; ++d)
#pragma unroll
                    for (int b = 0; b < 3; ++b) B.P[d][b] = 0u;
            }
            uint16_t *dst = marks + p * 81;
            // one 16-bit store per cell, each at an index the optimizer cannot
            // relate to its neighbours': gfx950 stores at any alignment, and
            // adjacent 16-bit stores are otherwise merged into dwordx4 stores
            const int32_t c = plane::cand_marks(B, [&](int cell, uint32_t m) {
                uint32_t at = (uint32_t)cell;
                asm volatile("" : "+v"(at));
                dst[at] = (uint16_t)m;
            });
            if (count) count[p] = mode == CAND_FROM_W ? c : mode == CAND_ZERO ? 0 : mode == CAND_BAD_BYTE ? SDK_INVALID : SDK_FAULT;
            mode = 0;
        }
        if (leave) break;
        if (refill) {
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
                cand_load_words(boards + p * 81, x);
                bool clash = false;
                if (!plane::load_words(B, x, clash, given)) {
                    mode = CAND_BAD_BYTE;
                } else if (clash) {
                    mode = CAND_ZERO;  // no valid completion; rules B-D are unsound on such givens
                } else {
                    active = true;
                    depth = 0;
                    mode = 0;
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        nd[b] = given[b];
                        und[b] = plane::andn(plane::ROWS, given[b]);
                    }
                }
            }
        }
        if (active) {
            const int k = plane::cand_iter(B, und, nd, depth, mode, stk, (uint32_t)plane::COUNT_MAX_DEPTH, sweep);
            if (k != plane::K_CONT) {
                active = false;
                mode = k == plane::K_FAULT ? CAND_FAULTED : (mode & plane::CM_WIT) ? CAND_FROM_W : CAND_ZERO;
            }
        }
    }
}

// ==================================================================== C ABI
static std::atomic<int> g_cand_bpc{0};

// waves of a full grid on the current device: every CU at the kernel's occupancy
static int64_t cand_full_waves()
{
    const int per_cu = 4 * CAND_WAVES_PER_EU;  // four SIMDs per CU
    return (int64_t)sdk_device_cu_count() * cached_occupancy(cand_kernel, CAND_THREADS, per_cu, per_cu, g_cand_bpc);
}

static int64_t cand_waves(int64_t n, int max_waves)
{
    const int64_t cap = max_waves > 0 ? (int64_t)max_waves : cand_full_waves();
    const int64_t want = n / 64 + (n % 64 != 0);  // (n + 63 would overflow at INT64_MAX)
    return want < cap ? want : cap;
}

extern "C" {

size_t sdk_candidates_scratch_bytes(int64_t n, int max_waves)
{
    if (n < 0 || max_waves < 0) return 0;
    return CAND_HEAD_BYTES + (size_t)cand_waves(n, max_waves) * CAND_WAVE_BYTES;
}

int sdk_candidates_batch(const uint8_t *d_boards, uint16_t *d_marks, int32_t *d_count, int64_t n, void *d_scratch,
                         size_t scratch_bytes, int max_waves, void *stream)
{
    if (n < 0 || max_waves < 0) return -2;
    if (n == 0) return 0;
    if (!d_boards || !d_marks || ((uintptr_t)d_marks & 1u) || ((uintptr_t)d_count & 3u) || !d_scratch ||
        ((uintptr_t)d_scratch & 7u) || scratch_bytes < sdk_candidates_scratch_bytes(n, max_waves))
        return -2;
    hipStream_t st = (hipStream_t)stream;
    // the queue head, re-armed in stream order before the kernel
    if (hipMemsetAsync(d_scratch, 0, CAND_HEAD_BYTES, st) != hipSuccess) return -1;
    const int64_t waves = cand_waves(n, max_waves);
    hipLaunchKernelGGL(cand_kernel, dim3((unsigned)waves), dim3(CAND_THREADS), 0, st, d_boards, d_marks, d_count, n,
                       (uint32_t)SDK_CAND_SWEEP, (unsigned long long *)d_scratch, (uint8_t *)d_scratch + CAND_HEAD_BYTES);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
