// uniq_kernels.hip -- translation unit of the batched unique candidates
// (plane_uniq.h): uniq_kernel and its C ABI entries
// (sdk_unique_candidates_scratch_bytes, sdk_unique_candidates_batch).  A unit
// of its own, like cand_kernels.hip: the other units, their flags and the
// solve workspace are not involved (common.h is included for
// cached_occupancy alone).
//
// uniq_kernel: cand_kernel's shape.  One board per LANE, persistent one-wave
// workgroups.  A lane holds its board's 27 plane words, und[] / nd[]
// (plane::pass_ahead), its stack depth, its mode word (plane_uniq.h; on an
// idle lane, the answer pending for its board) and the board's index, and
// runs one plane::uniq_iter per loop iteration: every lane, in whatever
// phase, shares the iteration's one pass_ahead; the phase changes (a
// completion folded into W and V, the root saved, a targeted search settled
// and the next target picked) are the divergent blocks beside it, as
// count_step is.  When SDK_UNIQ_REFILL lanes of a wave are idle (all 64 at the
// start) lane 0 claims that many boards with ONE agent-scope fetch-add on the
// queue head; idle lane number r takes board head + r.  Once a claim reaches
// the end of the batch the wave claims no more and exits when its last board
// is finished.  A refilled lane reads its 81 bytes as 21 aligned dwords,
// funnel-shifted into the words plane::load_words takes.
//
// Answers.  A finished lane's marks already sit in a line and uniq_iter has
// left once = marks & ~V in U's, so the lane only notes which line holds the
// marks, and the count; the 81-cell conversions (plane::cand_marks, once per
// array asked for: 81 16-bit stores each, and the int32 count) run at the
// wave's next refill, or at its exit, once for all lanes that finished since
// (DESIGN.md §15 measured why).  One line is converted at a time: a second
// set of planes beside the one being converted does not fit the register
// budget.  A board answered without a search (a byte >
// 9, clashing givens) and a fault go the same way with zero planes.
//
// Scratch: [0, 256) the queue head's block (zeroed by the call itself, in
// stream order, before the kernel), then per wave 64 lanes x UNIQ_LEVELS (85)
// lines of 128 bytes: plane_stack.h's PlaneStack, levels 0..80 the search's,
// 81 the closed root R with its und[], 82 V, 83 U, 84 W / T (plane_uniq.h).
// Each wave addresses its own lines through a buffer descriptor that covers
// exactly them.
#include "common.h"
#include "plane_uniq.h"
#include "plane_stack.h"

#define UNIQ_THREADS 64    // one wave per workgroup
#define UNIQ_WAVES_PER_EU 4
#define UNIQ_HEAD_BYTES 256
// idle lanes before a wave claims boards (results never depend on it): the
// count's measured choice (count_kernels.hip), as in cand_kernels.hip
#ifndef SDK_UNIQ_REFILL
#define SDK_UNIQ_REFILL 16
#endif
#define UNIQ_LANE_BYTES ((uint32_t)plane::UNIQ_LEVELS * 128u)
#define UNIQ_WAVE_BYTES (64u * UNIQ_LANE_BYTES)
// an idle lane's mode word: the answer pending for its board (0: none) and,
// above it, the count of a board whose answer sits in its lines
enum : uint32_t { UNIQ_FROM_W = 1, UNIQ_FROM_R = 2, UNIQ_ZERO = 3, UNIQ_BAD_BYTE = 4, UNIQ_FAULTED = 5, UNIQ_KIND = 7,
                  UNIQ_COUNT_SHIFT = 4 };

// cand_kernels.hip's loader: the 21 words of the board at `src` (any
// alignment) from the 21 aligned dwords that hold its 81 bytes (byte 80 lies
// in dword 20 for every alignment, so every dword read holds a byte of the
// board), funnel-shifted into place.  Only byte 0 of x[20] is the board's.
__device__ __forceinline__ void uniq_load_words(const uint8_t *src, uint32_t (&x)[21])
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

__global__ __launch_bounds__(UNIQ_THREADS, UNIQ_WAVES_PER_EU) void uniq_kernel(
    const uint8_t *__restrict__ boards, uint16_t *__restrict__ once, uint16_t *__restrict__ marks,
    int32_t *__restrict__ count, int64_t n, uint32_t sweep, unsigned long long *__restrict__ head,
    uint8_t *__restrict__ stack)
{
    const int lane = threadIdx.x;
    const PlaneStack stk = {__builtin_amdgcn_make_buffer_rsrc(stack + (size_t)blockIdx.x * UNIQ_WAVE_BYTES, 0,
                                                              (int)UNIQ_WAVE_BYTES, 0x00020000),
                            (uint32_t)lane * UNIQ_LANE_BYTES};
    plane::Board B;
    uint32_t und[3] = {0u, 0u, 0u}, nd[3] = {0u, 0u, 0u}, depth = 0, mode = 0;
    int64_t p = 0;            // this lane's board
    bool active = false, queue_out = false;
    for (;;) {
        const uint64_t idle = __builtin_amdgcn_ballot_w64(!active);
        const int nidle = __builtin_popcountll(idle);
        const bool leave = queue_out && nidle == 64;
        const bool refill = !queue_out && nidle >= SDK_UNIQ_REFILL;
        if ((leave || refill) && !active && mode) {
            // the answers of the lanes that finished since the last refill
            // (an idle lane's B is dead: the marks' planes take its registers)
            // One line at a time: the marks (if asked for), then once, which
            // uniq_iter left in U's line.  One 16-bit store per cell, each at
            // an index the optimizer cannot relate to its neighbours': gfx950
            // stores at any alignment, and adjacent 16-bit stores are
            // otherwise merged into dwordx4 stores (cand_kernels.hip).
            const uint32_t kind = mode & UNIQ_KIND;
            uint32_t tu[3];
            if (marks) {
                if (kind <= UNIQ_FROM_R) {
                    stk.pop(plane::cand_level(kind == UNIQ_FROM_R ? plane::UNIQ_ROOT_LEVEL : plane::UNIQ_WIT_LEVEL), B, tu);
                } else {
#pragma unroll
                    for (int d = 0; d < 9; ++d)
#pragma unroll
                        for (int b = 0; b < 3; ++b) B.P[d][b] = 0u;
                }
                uint16_t *dst = marks + p * 81;
                plane::cand_marks(B, [&](int cell, uint32_t m) {
                    uint32_t at = (uint32_t)cell;
                    asm volatile("" : "+v"(at));
                    dst[at] = (uint16_t)m;
                });
            }
            if (kind <= UNIQ_FROM_R) {
                stk.pop(plane::cand_level(plane::UNIQ_OPEN_LEVEL), B, tu);
            } else {
#pragma unroll
                for (int d = 0; d < 9; ++d)
#pragma unroll
                    for (int b = 0; b < 3; ++b) B.P[d][b] = 0u;
            }
            uint16_t *dst = once + p * 81;
            plane::cand_marks(B, [&](int cell, uint32_t m) {
                uint32_t at = (uint32_t)cell;
                asm volatile("" : "+v"(at));
                dst[at] = (uint16_t)m;
            });
            if (count)
                count[p] = kind <= UNIQ_FROM_R ? (int32_t)(mode >> UNIQ_COUNT_SHIFT)
                           : kind == UNIQ_ZERO ? 0
                           : kind == UNIQ_BAD_BYTE ? SDK_INVALID
                                                   : SDK_FAULT;
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
                uniq_load_words(boards + p * 81, x);
                bool clash = false;
                if (!plane::load_words(B, x, clash, given)) {
                    mode = UNIQ_BAD_BYTE;
                } else if (clash) {
                    mode = UNIQ_ZERO;  // no valid completion; rules B-D are unsound on such givens
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
            const int k = plane::uniq_iter(B, und, nd, depth, mode, stk, (uint32_t)plane::COUNT_MAX_DEPTH, sweep);
            if (k != plane::K_CONT) {
                active = false;
                const uint32_t c = (uint32_t)plane::uniq_count(mode) << UNIQ_COUNT_SHIFT;
                mode = k == plane::K_FAULT ? UNIQ_FAULTED
                       : (mode & plane::UM_TARGET) ? UNIQ_FROM_R | c
                       : (mode & plane::UM_WIT) ? UNIQ_FROM_W | c
                                                : UNIQ_ZERO;
            }
        }
    }
}

// ==================================================================== C ABI
static std::atomic<int> g_uniq_bpc{0};

// waves of a full grid on the current device: every CU at the kernel's occupancy
static int64_t uniq_full_waves()
{
    const int per_cu = 4 * UNIQ_WAVES_PER_EU;  // four SIMDs per CU
    return (int64_t)sdk_device_cu_count() * cached_occupancy(uniq_kernel, UNIQ_THREADS, per_cu, per_cu, g_uniq_bpc);
}

static int64_t uniq_waves(int64_t n, int max_waves)
{
    const int64_t cap = max_waves > 0 ? (int64_t)max_waves : uniq_full_waves();
    const int64_t want = n / 64 + (n % 64 != 0);  // (n + 63 would overflow at INT64_MAX)
    return want < cap ? want : cap;
}

extern "C" {

size_t sdk_unique_candidates_scratch_bytes(int64_t n, int max_waves)
{
    if (n < 0 || max_waves < 0) return 0;
    return UNIQ_HEAD_BYTES + (size_t)uniq_waves(n, max_waves) * UNIQ_WAVE_BYTES;
}

int sdk_unique_candidates_batch(const uint8_t *d_boards, uint16_t *d_once, uint16_t *d_marks, int32_t *d_count, int64_t n,
                                void *d_scratch, size_t scratch_bytes, int max_waves, void *stream)
{
    if (n < 0 || max_waves < 0) return -2;
    if (n == 0) return 0;
    if (!d_boards || !d_once || ((uintptr_t)d_once & 1u) || ((uintptr_t)d_marks & 1u) || ((uintptr_t)d_count & 3u) ||
        !d_scratch || ((uintptr_t)d_scratch & 7u) || scratch_bytes < sdk_unique_candidates_scratch_bytes(n, max_waves))
        return -2;
    hipStream_t st = (hipStream_t)stream;
    // the queue head, re-armed in stream order before the kernel
    if (hipMemsetAsync(d_scratch, 0, UNIQ_HEAD_BYTES, st) != hipSuccess) return -1;
    const int64_t waves = uniq_waves(n, max_waves);
    hipLaunchKernelGGL(uniq_kernel, dim3((unsigned)waves), dim3(UNIQ_THREADS), 0, st, d_boards, d_once, d_marks, d_count,
                       n, (uint32_t)SDK_UNIQ_SWEEP, (unsigned long long *)d_scratch,
                       (uint8_t *)d_scratch + UNIQ_HEAD_BYTES);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
