// hit_kernels.hip -- translation unit of the hitting sets (hit.h):
// hit_validate_kernel, hit_search_kernel, hit_info_kernel and their C ABI
// entries (sdk_hitting_sets_scratch_bytes, sdk_hitting_sets_batch).  A unit of
// its own: the solve workspace and the other units' flags are not involved
// (common.h is included for cached_occupancy alone).  DESIGN.md §25.
//
// hit_validate_kernel: one family per lane.  Writes the family's status and a
// zeroed count.
//
// hit_search_kernel: persistent one-wave workgroups.  The work unit is a task
// (family, first cell), 81 a family, claimed from one 64-bit counter; in a
// batch of at most HIT_FINE_FAMILIES families every task is cut into its 81
// fine tasks (family, first cell, second cell), 6561 a family, most of which
// end at once.  Every LANE runs a task of its own, one node of its walk per
// iteration of the wave's loop; a lane whose task has ended takes the next
// one in the same iteration -- a ballot of the idle lanes, one fetch-add for
// all of them.  A lane's state is the six mask words C and X, its family's
// allowed mask, base and length in registers and, in LDS at [word][lane], its
// stack (four words per level); the family's sets are read from global memory
// by index, so the lanes of a wave may be in different families.  The lanes
// that reach a row in an iteration take their places in the list with one
// fetch-add on the 64-bit cursor between them and each adds one to its
// family's count.  With capacity 0 and no limit (pure count) a lane sums what
// its task finds, leaves' binomials included, and adds it once at the task's
// end.  With a limit a row is listed only when the family's count before it
// was below the limit, and running tasks of a family that has reached it end
// within 64 nodes.  No wave, workgroup or launch ever waits for another.
//
// hit_info_kernel: families at or beyond the limit get count = limit and
// SDK_HIT_LIMITED; one lane writes {total, listed} from the cursor.
//
// Scratch: 64 bytes, the control block -- the task head (byte 0), the row
// cursor (byte 8) -- zeroed by the call itself in stream order.
#include "common.h"
#include "hit.h"

#define HIT_THREADS 64  // one wave per workgroup
#define HIT_FINE_FAMILIES 4096  // batches up to this size run fine tasks
#define HIT_HEAD_BYTES 64
#define HIT_STACK_WORDS (4 * hit::MAX_CLUES)

// a lane's view of its family and its LDS column
struct HitMem {
    const uint4 *fam;  // the family's first set
    uint32_t n;
    uint32_t A[3];
    uint32_t *s;  // [HIT_STACK_WORDS][64], this lane's column
    __device__ __forceinline__ uint32_t nsets() const { return n; }
    __device__ __forceinline__ void load(uint32_t i, uint32_t *u) const
    {
        const uint4 v = fam[i];
        u[0] = v.x, u[1] = v.y, u[2] = v.z;
    }
    __device__ __forceinline__ uint32_t allowed(int w) const { return A[w]; }
    __device__ __forceinline__ uint32_t &stk(int l, int j) { return s[(4 * l + j) * 64]; }
};

__device__ __forceinline__ uint64_t hit_first64(unsigned long long h)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(h >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)h);
}

__device__ __forceinline__ uint32_t hit_rank(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ __launch_bounds__(HIT_THREADS) void hit_validate_kernel(const int64_t *__restrict__ offsets,
                                                                   const uint32_t *__restrict__ allowed,
                                                                   const uint32_t *__restrict__ required, int64_t n,
                                                                   int32_t *__restrict__ status,
                                                                   int64_t *__restrict__ count)
{
    const int64_t stride = (int64_t)gridDim.x * HIT_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * HIT_THREADS + threadIdx.x; i < n; i += stride) {
        const uint32_t A[3] = {allowed[4 * i], allowed[4 * i + 1], allowed[4 * i + 2]};
        const uint32_t R[3] = {required[4 * i], required[4 * i + 1], required[4 * i + 2]};
        const int64_t len = offsets[i + 1] - offsets[i];
        status[i] = len < 0 || len > (int64_t)0x7FFFFFFF ? (int)hit::INVALID : hit::validate(A, R);
        count[i] = 0;
    }
}

__global__ __launch_bounds__(HIT_THREADS) void hit_search_kernel(
    const uint4 *__restrict__ sets, const int64_t *__restrict__ offsets, const uint32_t *__restrict__ allowed,
    const uint32_t *__restrict__ required, const int32_t *__restrict__ status, int64_t n, int k, int64_t limit,
    uint4 *__restrict__ rows, int64_t capacity, unsigned long long *__restrict__ count,
    unsigned long long *__restrict__ head, int fine)
{
    __shared__ uint32_t stack[HIT_STACK_WORDS * 64];
    const int lane = threadIdx.x;
    HitMem mem;
    mem.fam = sets, mem.n = 0u, mem.A[0] = mem.A[1] = mem.A[2] = 0u;
    mem.s = stack + lane;
    hit::State S;
    S.depth = 0;
    int64_t mine = 0;  // this lane's family
    unsigned long long acc = 0;  // pure count: what this lane's task has found
    const int count_only = capacity == 0 && limit == 0;
    const uint32_t per = fine ? hit::FINE : hit::COARSE;  // tasks a family
    const uint64_t total = (uint64_t)n * per;
    bool drained = false;
    for (uint32_t it = 0;; ++it) {
        const bool idle = S.depth == 0;
        if (idle && acc) {
            atomicAdd(count + mine, acc);
            atomicAdd(head + 1, acc);
            acc = 0;
        }
        const uint64_t idles = __builtin_amdgcn_ballot_w64(idle);
        uint64_t add = 0;
        bool started = false;
        if (idles && !drained) {
            const uint32_t want = (uint32_t)__builtin_popcountll(idles);
            unsigned long long h = 0;
            if (lane == 0)
                h = __hip_atomic_fetch_add(head, (unsigned long long)want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t base = hit_first64(h);
            drained = base + want >= total;
            const uint64_t t = base + hit_rank(idles);
            if (idle && t < total) {
                const int64_t f = (int64_t)(t / per);
                const int r = (int)(t % per);
                bool live = status[f] == hit::DONE;
                if (live && limit)
                    live = __hip_atomic_load(count + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <
                           (unsigned long long)limit;
                if (live) {
                    const int64_t lo = offsets[f];
                    mine = f;
                    mem.fam = sets + lo;
                    mem.n = (uint32_t)(offsets[f + 1] - lo);
                    const uint4 a = ((const uint4 *)allowed)[f], q = ((const uint4 *)required)[f];
                    mem.A[0] = a.x, mem.A[1] = a.y, mem.A[2] = a.z;
                    const uint32_t R[3] = {q.x, q.y, q.z};
                    add = hit::start(S, mem, R, k, fine ? r / 81 : r, fine ? r % 81 : -1, count_only);
                    started = true;
                }
            }
        } else if (idles == ~0ull) {
            break;
        }
        if (!started && S.depth) add = hit::step(S, mem);
        if (count_only) {
            acc += add;
            continue;
        }
        bool row = add != 0;
        if (row) {
            const unsigned long long before = atomicAdd(count + mine, 1ull);
            if (limit && before >= (unsigned long long)limit) row = false, S.depth = 0;
        }
        if (limit && (it & 63u) == 63u && S.depth &&
            __hip_atomic_load(count + mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned long long)limit)
            S.depth = 0;
        const uint64_t found = __builtin_amdgcn_ballot_w64(row);
        if (found) {
            unsigned long long h = 0;
            if (lane == 0)
                h = __hip_atomic_fetch_add(head + 1, (unsigned long long)__builtin_popcountll(found), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t slot = hit_first64(h) + hit_rank(found);
            if (row && slot < (uint64_t)capacity) rows[slot] = make_uint4(S.C[0], S.C[1], S.C[2], (uint32_t)mine);
        }
    }
}

__global__ __launch_bounds__(HIT_THREADS) void hit_info_kernel(const unsigned long long *__restrict__ head, int64_t n,
                                                               int64_t limit, int64_t capacity,
                                                               int64_t *__restrict__ count, int32_t *__restrict__ status,
                                                               int64_t *__restrict__ info)
{
    if (limit) {
        const int64_t stride = (int64_t)gridDim.x * HIT_THREADS;
        for (int64_t i = (int64_t)blockIdx.x * HIT_THREADS + threadIdx.x; i < n; i += stride) {
            if (status[i] == hit::DONE && count[i] >= limit) {
                count[i] = limit;
                status[i] = hit::LIMITED;
            }
        }
    }
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int64_t total = (int64_t)head[1];
        info[0] = total;
        info[1] = total < capacity ? total : capacity;
    }
}

// ==================================================================== C ABI
static std::atomic<int> g_hit_search_bpc{0};

static int64_t hit_full_waves()
{
    // the stack's 32 KB of LDS a wave bounds the waves of a CU
    return (int64_t)sdk_device_cu_count() * cached_occupancy(hit_search_kernel, HIT_THREADS, 4, 32, g_hit_search_bpc);
}

extern "C" {

size_t sdk_hitting_sets_scratch_bytes(int64_t n, int max_waves)
{
    if (n < 0 || n > (int64_t)0x7FFFFFFF || max_waves < 0) return 0;
    return HIT_HEAD_BYTES;
}

int sdk_hitting_sets_batch(const uint32_t *d_sets, const int64_t *d_offsets, const uint32_t *d_allowed,
                           const uint32_t *d_required, int64_t n, int k, int64_t limit, uint32_t *d_rows,
                           int64_t capacity, int64_t *d_count, int32_t *d_status, int64_t *d_info, void *d_scratch,
                           size_t scratch_bytes, int max_waves, void *stream)
{
    if (n < 0 || n > (int64_t)0x7FFFFFFF || k < 0 || k > SDK_HIT_MAX_CLUES || limit < 0 || capacity < 0 ||
        capacity > (int64_t)(INT64_MAX / 16) || max_waves < 0)
        return -2;
    if (n == 0) return 0;
    // (d_sets may be NULL: every family may be empty; it is never read then)
    if (!d_offsets || !d_allowed || !d_required || !d_count || !d_status || !d_info || !d_scratch ||
        (capacity > 0 && !d_rows) || ((uintptr_t)d_sets & 15u) || ((uintptr_t)d_offsets & 7u) ||
        ((uintptr_t)d_allowed & 15u) || ((uintptr_t)d_required & 15u) || ((uintptr_t)d_rows & 15u) ||
        ((uintptr_t)d_count & 7u) || ((uintptr_t)d_status & 3u) || ((uintptr_t)d_info & 7u) ||
        ((uintptr_t)d_scratch & 7u) || scratch_bytes < sdk_hitting_sets_scratch_bytes(n, max_waves))
        return -2;
    hipStream_t st = (hipStream_t)stream;
    // the task head and the row cursor, re-armed in stream order before the kernels
    if (hipMemsetAsync(d_scratch, 0, HIT_HEAD_BYTES, st) != hipSuccess) return -1;
    unsigned long long *head = (unsigned long long *)d_scratch;
    const int64_t full = hit_full_waves();
    const int64_t cap = max_waves > 0 ? (int64_t)max_waves : full > 0 ? full : 1;
    const int64_t vwant = n / 64 + (n % 64 != 0);
    const unsigned vgrid = (unsigned)(vwant < cap ? vwant : cap);
    hipLaunchKernelGGL(hit_validate_kernel, dim3(vgrid), dim3(HIT_THREADS), 0, st, d_offsets, d_allowed, d_required, n,
                       d_status, d_count);
    if (hipGetLastError() != hipSuccess) return -1;
    const int fine = n <= HIT_FINE_FAMILIES;
    const int64_t tasks = n * (fine ? hit::FINE : hit::COARSE);  // (n < 2^31: below 2^44)
    const int64_t swant = (tasks + 63) / 64;
    hipLaunchKernelGGL(hit_search_kernel, dim3((unsigned)(swant < cap ? swant : cap)), dim3(HIT_THREADS), 0, st,
                       (const uint4 *)d_sets, d_offsets, d_allowed, d_required, (const int32_t *)d_status, n, k, limit,
                       (uint4 *)d_rows, capacity, (unsigned long long *)d_count, head, fine);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(hit_info_kernel, dim3(limit ? vgrid : 1u), dim3(HIT_THREADS), 0, st,
                       (const unsigned long long *)head, n, limit, capacity, d_count, d_status, d_info);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
