// canon_kernels.hip -- translation unit of the canonical form (canon.h):
// canon_kernel, canon_reduce_kernel and their C ABI entries
// (sdk_canonical_scratch_bytes, sdk_canonical_batch).  A unit of its own:
// the solve and count kernels' units, their flags and their workspace are
// not involved (common.h is included for cached_occupancy alone).
//
// canon_kernel: one workgroup of four waves per (board, slice).  Slice s of S
// is the row variants [s*2592/S, (s+1)*2592/S).  The board and its transpose
// lie in LDS (162 bytes); every gather of an image cell is a byte read there.
// The work items are the (super-block, ci) pairs of the super-blocks that meet
// the slice (canon.h: a super-block is the 72 row variants with the same first
// three image rows), 256 a round, one per lane; permutations are decoded from
// their numbers.  A lane computes its item's prefix (canon::prefix: rows 0..2);
// the workgroup shares the smallest 16-cell prefix seen so far through one
// 64-bit LDS word (read once per item, lowered with an LDS atomic min), which
// is what kills most items inside their first image row.  The few items that
// live go into an LDS queue, and once it holds CANON_DRAIN_AT of them (or at
// the last round) the workgroup drains it: task (entry, hb), twelve an entry,
// dealt over all 256 lanes, each canon::complete()ing its six row variants
// against the lane's own best record in registers -- so the long tails run
// on full waves, not on the one lane whose item lived.  At the end: a
// butterfly merge across each wave, the four wave records merged by lane 0
// through LDS, and one 64-byte packed record written to the scratch by
// sixteen lanes.
//
// canon_reduce_kernel: one lane per board merges the board's S records,
// unpacks the canon and writes sym and autos.
//
// Scratch: n * S records of 64 bytes, board-major; every record is written
// by the first kernel before the second reads it, so its contents at the
// call do not matter.
#include "common.h"
#include "canon.h"

#define CANON_THREADS 256
#define CANON_WAVES (CANON_THREADS / 64)
#define CANON_WGS_PER_CU 8    // eight waves per SIMD: the most the hardware holds
#define CANON_REDUCE_THREADS 64
// live prefixes that make a drain worth its while: 22 * 12 tasks fill the 256
// lanes.  The queue holds what was left below that plus one round's 256.
#define CANON_DRAIN_AT 22
#define CANON_QUEUE (CANON_DRAIN_AT - 1 + CANON_THREADS)
// A launch's global size, workgroups times threads, is a 32-bit number: the runtime cuts a larger one to its
// low 32 bits and runs that part of the grid without an error (25 898 boards at 2592 slices ran 16 384 of their
// 67 M workgroups).  So a launch holds at most CANON_MAX_GRID workgroups of CANON_THREADS.
#define CANON_MAX_GLOBAL 0xFFFFFFFFll
#define CANON_MAX_GRID (CANON_MAX_GLOBAL / CANON_THREADS)

// the workgroup's shared prefix
struct LdsKey {
    unsigned long long *p;
    __device__ __forceinline__ uint64_t load() const
    {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ void lower(uint64_t k) const
    {
        __hip_atomic_fetch_min(p, (unsigned long long)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

__device__ __forceinline__ uint64_t canon_xor64(uint64_t v, int mask)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
    return (uint64_t)hi << 32 | lo;
}

__global__ __launch_bounds__(CANON_THREADS) void canon_kernel(const uint8_t *__restrict__ boards,
                                                              uint32_t *__restrict__ records, int64_t first_board,
                                                              int slices)
{
    __shared__ uint8_t bt[176];
    __shared__ unsigned long long key;
    __shared__ uint32_t bad;
    __shared__ uint8_t sblist[canon::SUPER_BLOCKS];
    __shared__ int sbcount;
    __shared__ uint32_t qcount;
    __shared__ canon::Prefix queue[CANON_QUEUE];
    __shared__ uint32_t wrec[CANON_WAVES][canon::RECORD_WORDS];
    const int tid = threadIdx.x;
    const int64_t board = first_board + (int64_t)(blockIdx.x / (unsigned)slices);
    const int s = (int)(blockIdx.x % (unsigned)slices);
    uint32_t *dst = records + (board * slices + s) * canon::RECORD_WORDS;
    const int lo = canon::slice_lo(s, slices), hi = canon::slice_lo(s + 1, slices);
    if (tid == 0) {
        key = ~0ull;
        bad = 0u;
        qcount = 0u;
    }
    if (tid == 64) sbcount = canon::list_super_blocks(lo, hi, sblist);
    __syncthreads();
    if (tid < 81) {
        const uint8_t x = boards[board * 81 + tid];
        bt[tid] = x;
        bt[81 + 9 * (tid % 9) + tid / 9] = x;
        if (x > 9) bad = 1u;
    }
    __syncthreads();
    if (bad) {  // a byte > 9: no search, the record says so
        if (tid < canon::RECORD_WORDS) dst[tid] = tid == 13 ? 1u : 0u;
        return;
    }
    const int items = sbcount * canon::LINE_PERMS;
    canon::Record best;
    canon::clear(best);
    LdsKey k = {&key};
#pragma unroll 1
    for (int base = 0; base < items; base += CANON_THREADS) {  // uniform: every lane runs every round
        const int it = base + tid;
        canon::Prefix p;
        const bool live = it < items && canon::prefix(bt, sblist[it / canon::LINE_PERMS], it % canon::LINE_PERMS, p, k);
        const uint64_t lives = __ballot(live);
        if (lives) {  // one queue claim a wave; qcount < CANON_DRAIN_AT before the round, so slot < CANON_QUEUE
            uint32_t first = 0;
            if ((tid & 63) == __builtin_ctzll(lives))
                first = __hip_atomic_fetch_add(&qcount, (uint32_t)__builtin_popcountll(lives), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
            first = (uint32_t)__shfl((int)first, __builtin_ctzll(lives), 64);
            const uint32_t slot = first + __builtin_amdgcn_mbcnt_hi((uint32_t)(lives >> 32),
                                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)lives, 0u));
            if (live && slot < CANON_QUEUE) queue[slot] = p;
        }
        __syncthreads();
        const uint32_t queued = qcount;
        __syncthreads();  // everyone has read it before the next round's claims
        if (queued >= CANON_DRAIN_AT || base + CANON_THREADS >= items) {
#pragma unroll 1
            for (uint32_t task = tid; task < queued * 12u; task += CANON_THREADS)
                canon::complete(bt, queue[task / 12u], (int)(task % 12u), lo, hi, best, k);
            __syncthreads();  // the entries are read: the queue is free again
            if (tid == 0) qcount = 0u;
            __syncthreads();
        }
    }
    // across the wave: after the butterfly every lane holds the wave's record
#pragma unroll 1
    for (int m = 32; m >= 1; m >>= 1) {
        canon::Record o;
#pragma unroll
        for (int i = 0; i < 9; ++i) o.row[i] = canon_xor64(best.row[i], m);
        o.sym = (uint32_t)__shfl_xor((int)best.sym, m, 64);
        o.ties = (uint32_t)__shfl_xor((int)best.ties, m, 64);
        canon::merge(best, o);
    }
    if ((tid & 63) == 0) {
        uint32_t w[canon::RECORD_WORDS];
        canon::pack(best, w);
#pragma unroll
        for (int i = 0; i < canon::RECORD_WORDS; ++i) wrec[tid >> 6][i] = w[i];
    }
    __syncthreads();
    if (tid == 0) {
        canon::Record all;
        canon::reduce(&wrec[0][0], CANON_WAVES, all);
        uint32_t w[canon::RECORD_WORDS];
        canon::pack(all, w);
#pragma unroll
        for (int i = 0; i < canon::RECORD_WORDS; ++i) wrec[0][i] = w[i];
    }
    __syncthreads();
    if (tid < canon::RECORD_WORDS) dst[tid] = wrec[0][tid];
}

__global__ __launch_bounds__(CANON_REDUCE_THREADS) void canon_reduce_kernel(
    const uint8_t *__restrict__ boards, const uint32_t *__restrict__ records, uint8_t *__restrict__ out,
    int32_t *__restrict__ sym, int32_t *__restrict__ autos, int64_t n, int slices)
{
    const int64_t i = (int64_t)blockIdx.x * CANON_REDUCE_THREADS + threadIdx.x;
    if (i >= n) return;
    uint8_t *o = out + i * 81;
    canon::Record r;
    if (!canon::reduce(records + i * slices * canon::RECORD_WORDS, slices, r)) {
        const uint8_t *src = boards + i * 81;
        for (int c = 0; c < 81; ++c) o[c] = src[c];
        sym[i] = SDK_INVALID;
        if (autos) autos[i] = SDK_INVALID;
        return;
    }
    canon::store_cells(r, [&](int c, uint32_t v) { o[c] = (uint8_t)v; });
    sym[i] = (int32_t)r.sym;
    if (autos) autos[i] = (int32_t)r.ties;
}

// ==================================================================== C ABI
static std::atomic<int> g_canon_wgs{0};

// slices == 0: as many (board, slice) workgroups as the device holds at once,
// and at most CANON_AUTO_MAX_SLICES a board.  Every slice walks the first
// image rows of its super-blocks again and starts with no best of its own, so
// slices cost work: measured on one MI355X (profiles/canon_slices_probe.json)
// one 17-clue board takes 1.48 ms at 2592 slices, 0.44 at 144, 0.33 at 72,
// 0.36 at 36 and 0.55 at 18 (a full grid 1.52 / 0.14 / 0.10 / 0.08 / 0.08); 64
// boards are fastest at 18..36 slices, 1024 and more at 1.
#define CANON_AUTO_MAX_SLICES 36  // 72 row variants: the size of a super-block
static int canon_slices(int64_t n, int slices)
{
    if (slices > 0 || n <= 0) return slices;
    const int per_cu = cached_occupancy(canon_kernel, CANON_THREADS, CANON_WGS_PER_CU, CANON_WGS_PER_CU, g_canon_wgs);
    const int64_t S = (int64_t)sdk_device_cu_count() * per_cu / n;
    return (int)(S < 1 ? 1 : S > CANON_AUTO_MAX_SLICES ? CANON_AUTO_MAX_SLICES : S);
}

extern "C" {

size_t sdk_canonical_scratch_bytes(int64_t n, int slices)
{
    if (n < 0 || slices < 0 || slices > SDK_CANON_MAX_SLICES) return 0;
    const size_t per_board = (size_t)canon_slices(n, slices) * (canon::RECORD_WORDS * sizeof(uint32_t));
    if (per_board && (size_t)n > SIZE_MAX / per_board) return 0;  // the size does not fit: no such batch
    return (size_t)n * per_board;
}

int sdk_canonical_batch(const uint8_t *d_boards, uint8_t *d_canon, int32_t *d_sym, int32_t *d_autos, int64_t n,
                        int slices, void *d_scratch, size_t scratch_bytes, void *stream)
{
    if (n < 0 || slices < 0 || slices > SDK_CANON_MAX_SLICES) return -2;
    if (n == 0) return 0;
    const size_t need = sdk_canonical_scratch_bytes(n, slices);  // 0: a size that does not fit size_t
    if (!d_boards || !d_canon || !d_sym || !d_scratch || d_canon == d_boards || need == 0 || scratch_bytes < need)
        return -2;
    const int64_t rb = (n + CANON_REDUCE_THREADS - 1) / CANON_REDUCE_THREADS;
    if (rb > CANON_MAX_GLOBAL / CANON_REDUCE_THREADS) return -2;
    hipStream_t st = (hipStream_t)stream;
    const int S = canon_slices(n, slices);
    // a launch's grid holds whole boards
    const int64_t per_launch = CANON_MAX_GRID / S;
    for (int64_t first = 0; first < n; first += per_launch) {
        const int64_t m = n - first < per_launch ? n - first : per_launch;
        hipLaunchKernelGGL(canon_kernel, dim3((unsigned)(m * S)), dim3(CANON_THREADS), 0, st, d_boards,
                           (uint32_t *)d_scratch, first, S);
    }
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(canon_reduce_kernel, dim3((unsigned)rb), dim3(CANON_REDUCE_THREADS), 0, st, d_boards,
                       (const uint32_t *)d_scratch, d_canon, d_sym, d_autos, n, S);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
