// ua_kernels.hip -- translation unit of the unavoidable sets (ua.h):
// ua_validate_kernel, ua_search_kernel, ua_info_kernel, ua_minimal_kernel and
// their C ABI entries (sdk_unavoidable_scratch_bytes, sdk_unavoidable_batch,
// sdk_unavoidable_minimal_batch).  A unit of its own: the solve workspace and
// the other units' flags are not involved (common.h is included for
// cached_occupancy and the wave helpers alone).  DESIGN.md §24.
//
// ua_validate_kernel: one grid per lane.  Writes the grid's status, a zeroed
// count and, into the scratch, its nine digit masks (27 words).
//
// ua_search_kernel: persistent one-wave workgroups.  The work unit is a task
// (grid, seed cell, seed digit), 648 a grid, claimed from one 64-bit counter
// in cell order; in a batch of at most UA_SPLIT_GRIDS grids every task is cut
// into its eight split tasks (ua::start), 5184 a grid, so that a single grid's
// heaviest tasks, a twentieth of its work each, do not leave the device idle.
// Every LANE runs a task of its own, one node of its walk per iteration of
// the wave's loop; a lane whose task has ended takes the next
// one in the same iteration -- a ballot of the idle lanes, one fetch-add for
// all of them -- so no lane waits for the wave's slowest task (the 64
// heaviest tasks of a grid are nine tenths of its work).  A lane's state is
// six mask words in registers and, in LDS at [word][lane], its grid's digit
// masks and its stack (one word and one 16-bit digit set per level).  The
// lanes that reach a row in an iteration take their places in the list with
// one fetch-add on the 64-bit cursor between them and each adds one to its
// grid's count.  No wave, workgroup or launch ever waits for another.
//
// ua_info_kernel: one lane writes {total, listed} from the cursor.
//
// ua_minimal_kernel: persistent one-wave workgroups over (group, chunk of 64
// rows): lane k of a chunk holds its row, the group's rows pass through LDS
// in tiles of 64 and every lane tests each of them with three AND / compare
// words.  Chunk j of group g belongs to wave (j + g) % waves: nothing to
// claim, nothing to wait for.
//
// Scratch: [0, 64) the control block -- the task head (byte 0), the row
// cursor (byte 8) -- zeroed by the call itself in stream order; then n
// records of 128 bytes, the digit masks.
#include "common.h"
#include "ua.h"

#define UA_THREADS 64  // one wave per workgroup
#ifndef SDK_UA_WAVES_PER_EU
#define SDK_UA_WAVES_PER_EU 3
#endif
#define UA_SPLIT_GRIDS 256  // batches up to this size run split tasks
#define UA_HEAD_BYTES 64
#define UA_REC_WORDS 32
#define UA_REC_BYTES (UA_REC_WORDS * 4)

// a lane's view of its LDS columns
struct UaMem {
    const uint32_t *peers;  // [81][3]
    uint32_t *g;            // [27][64], this lane's column
    uint32_t *s;            // [16][64]
    uint16_t *f;            // [16][64]
    __device__ __forceinline__ uint32_t gm(int k, int w) const { return g[(3 * k + w) * 64]; }
    __device__ __forceinline__ uint32_t peer(int c, int w) const { return peers[3 * c + w]; }
    __device__ __forceinline__ uint32_t &stk(int l) { return s[l * 64]; }
    __device__ __forceinline__ uint16_t &fb(int l) { return f[l * 64]; }
};

__device__ __forceinline__ uint64_t ua_first64(unsigned long long h)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(h >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)h);
}

__device__ __forceinline__ uint32_t ua_rank(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ __launch_bounds__(UA_THREADS) void ua_validate_kernel(const uint8_t *__restrict__ grids, int64_t n,
                                                                 int32_t *__restrict__ status,
                                                                 int32_t *__restrict__ count,
                                                                 uint32_t *__restrict__ recs)
{
    const int64_t stride = (int64_t)gridDim.x * UA_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * UA_THREADS + threadIdx.x; i < n; i += stride) {
        const uint8_t *g = grids + i * 81;
        auto byte_at = [&](int c) { return (uint32_t)g[c]; };
        const int st = ua::validate(byte_at);
        status[i] = st;
        count[i] = 0;
        if (st != ua::DONE) continue;
        uint32_t *rec = recs + i * UA_REC_WORDS;
#pragma unroll 1
        for (int d = 1; d <= 9; ++d) {
#pragma unroll
            for (int w = 0; w < 3; ++w) rec[3 * (d - 1) + w] = ua::digit_word(byte_at, d, w);
        }
    }
}

__global__ __launch_bounds__(UA_THREADS, SDK_UA_WAVES_PER_EU) void ua_search_kernel(
    const uint32_t *__restrict__ recs, const int32_t *__restrict__ status, int64_t n, int max_size,
    uint32_t *__restrict__ rows, int64_t capacity, int32_t *__restrict__ count, unsigned long long *__restrict__ head,
    int split)
{
    __shared__ uint32_t peers[81 * 3];
    __shared__ uint32_t gmask[27 * 64];
    __shared__ uint32_t stack[ua::MAX_SIZE * 64];
    __shared__ uint16_t taken[ua::MAX_SIZE * 64];
    const int lane = threadIdx.x;
    for (int c = lane; c < 81; c += 64) {
        uint32_t p[3];
        ua::peer_mask(c, p);
        peers[3 * c] = p[0];
        peers[3 * c + 1] = p[1];
        peers[3 * c + 2] = p[2];
    }
    wave_lds_sync();
    UaMem mem{peers, gmask + lane, stack + lane, taken + lane};
    ua::State S;
    S.depth = 0;
    int64_t mine = -1;  // the grid whose masks this lane's column holds
    const uint32_t per = split ? ua::TASKS * ua::SPLIT : ua::TASKS;  // tasks a grid
    const uint64_t total = (uint64_t)n * per;
    bool drained = false;
    for (;;) {
        const bool idle = S.depth == 0;
        const uint64_t idles = __builtin_amdgcn_ballot_w64(idle);
        if (idles && !drained) {
            const uint32_t want = (uint32_t)__builtin_popcountll(idles);
            unsigned long long h = 0;
            if (lane == 0)
                h = __hip_atomic_fetch_add(head, (unsigned long long)want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t base = ua_first64(h);
            drained = base + want >= total;
            const uint64_t t = base + ua_rank(idles);
            if (idle && t < total) {
                const int64_t grid = (int64_t)(t / per);
                const int r = (int)(t % per);
                if (status[grid] == ua::DONE) {
                    if (grid != mine) {
                        const uint32_t *rec = recs + grid * UA_REC_WORDS;
#pragma unroll
                        for (int w = 0; w < 27; ++w) gmask[w * 64 + lane] = rec[w];
                        mine = grid;
                    }
                    if (split)
                        ua::start(S, mem, r >> 6, (r >> 3) & 7, r & 7, max_size);
                    else
                        ua::start(S, mem, r >> 3, r & 7, -1, max_size);
                }
            }
        } else if (idles == ~0ull) {
            break;
        }
        int row = 0;
        if (S.depth) row = ua::step(S, mem);
        const uint64_t found = __builtin_amdgcn_ballot_w64(row != 0);
        if (found) {
            unsigned long long h = 0;
            if (lane == 0)
                h = __hip_atomic_fetch_add(head + 1, (unsigned long long)__builtin_popcountll(found), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t slot = ua_first64(h) + ua_rank(found);
            if (row) {
                atomicAdd(count + mine, 1);
                if (slot < (uint64_t)capacity)
                    ((uint4 *)rows)[slot] = make_uint4(S.D[0], S.D[1], S.D[2], (uint32_t)mine);
            }
        }
    }
}

__global__ void ua_info_kernel(const unsigned long long *__restrict__ head, int64_t capacity, int64_t *__restrict__ info)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int64_t total = (int64_t)head[1];
        info[0] = total;
        info[1] = total < capacity ? total : capacity;
    }
}

__global__ __launch_bounds__(UA_THREADS) void ua_minimal_kernel(const uint32_t *__restrict__ rows,
                                                                const int64_t *__restrict__ offsets, int64_t groups,
                                                                uint8_t *__restrict__ keep)
{
    __shared__ uint32_t tile[3 * 64];
    const int lane = threadIdx.x;
    const int64_t waves = gridDim.x;
    for (int64_t g = 0; g < groups; ++g) {
        const int64_t begin = offsets[g], end = offsets[g + 1];
        const int64_t chunks = (end - begin + 63) / 64;
        // this wave's first chunk of the group: the least j >= 0 with (j + g) % waves == blockIdx.x
        int64_t j = ((int64_t)blockIdx.x - g % waves + waves) % waves;
        for (; j < chunks; j += waves) {
            const int64_t k = begin + j * 64 + lane;
            const bool have = k < end;
            uint32_t r[3] = {0u, 0u, 0u};
            if (have) {
                const uint4 v = ((const uint4 *)rows)[k];
                r[0] = v.x, r[1] = v.y, r[2] = v.z;
            }
            bool ok = true;
            for (int64_t at = begin; at < end; at += 64) {
                const int64_t q = at + lane;
                wave_lds_sync();  // the tile before has been read
                if (q < end) {
                    const uint4 v = ((const uint4 *)rows)[q];
                    tile[lane] = v.x, tile[64 + lane] = v.y, tile[128 + lane] = v.z;
                }
                wave_lds_sync();
                const int fill = end - at < 64 ? (int)(end - at) : 64;
                for (int i = 0; i < fill; ++i) {
                    const uint32_t o[3] = {tile[i], tile[64 + i], tile[128 + i]};
                    const bool same = ua::same_cells(o, r);
                    if (same ? at + i < k : ua::subset_of(o, r)) ok = false;
                }
            }
            if (have) keep[k] = ok ? 1 : 0;
        }
    }
}

// ==================================================================== C ABI
static std::atomic<int> g_ua_search_bpc{0};

static int64_t ua_full_waves()
{
    const int per_cu = 4 * SDK_UA_WAVES_PER_EU;  // four SIMDs per CU
    return (int64_t)sdk_device_cu_count() * cached_occupancy(ua_search_kernel, UA_THREADS, per_cu, per_cu, g_ua_search_bpc);
}

extern "C" {

size_t sdk_unavoidable_scratch_bytes(int64_t n, int max_waves)
{
    if (n < 0 || n > (int64_t)0x7FFFFFFF || max_waves < 0) return 0;
    return UA_HEAD_BYTES + (size_t)n * UA_REC_BYTES;
}

int sdk_unavoidable_batch(const uint8_t *d_grids, int64_t n, int max_size, uint32_t *d_rows, int64_t capacity,
                          int32_t *d_count, int32_t *d_status, int64_t *d_info, void *d_scratch, size_t scratch_bytes,
                          int max_waves, void *stream)
{
    if (n < 0 || n > (int64_t)0x7FFFFFFF || max_size < ua::MIN_SIZE || max_size > SDK_UA_MAX_SIZE || capacity < 0 ||
        capacity > (int64_t)(INT64_MAX / 16) || max_waves < 0)
        return -2;
    if (n == 0) return 0;
    if (!d_grids || !d_count || !d_status || !d_info || !d_scratch || (capacity > 0 && !d_rows) ||
        ((uintptr_t)d_rows & 15u) || ((uintptr_t)d_count & 3u) || ((uintptr_t)d_status & 3u) || ((uintptr_t)d_info & 7u) ||
        ((uintptr_t)d_scratch & 7u) || scratch_bytes < sdk_unavoidable_scratch_bytes(n, max_waves))
        return -2;
    hipStream_t st = (hipStream_t)stream;
    // the task head and the row cursor, re-armed in stream order before the kernels
    if (hipMemsetAsync(d_scratch, 0, UA_HEAD_BYTES, st) != hipSuccess) return -1;
    unsigned long long *head = (unsigned long long *)d_scratch;
    uint32_t *recs = (uint32_t *)((uint8_t *)d_scratch + UA_HEAD_BYTES);
    const int64_t full = ua_full_waves();
    const int64_t cap = max_waves > 0 ? (int64_t)max_waves : full > 0 ? full : 1;
    const int64_t vwant = n / 64 + (n % 64 != 0);
    hipLaunchKernelGGL(ua_validate_kernel, dim3((unsigned)(vwant < cap ? vwant : cap)), dim3(UA_THREADS), 0, st, d_grids,
                       n, d_status, d_count, recs);
    if (hipGetLastError() != hipSuccess) return -1;
    const int split = n <= UA_SPLIT_GRIDS;
    const int64_t tasks = n * (split ? ua::TASKS * ua::SPLIT : ua::TASKS);  // (n < 2^31: below 2^41)
    const int64_t swant = (tasks + 63) / 64;
    hipLaunchKernelGGL(ua_search_kernel, dim3((unsigned)(swant < cap ? swant : cap)), dim3(UA_THREADS), 0, st,
                       (const uint32_t *)recs, (const int32_t *)d_status, n, max_size, d_rows, capacity, d_count, head,
                       split);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(ua_info_kernel, dim3(1), dim3(UA_THREADS), 0, st, (const unsigned long long *)head, capacity,
                       d_info);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int sdk_unavoidable_minimal_batch(const uint32_t *d_rows, const int64_t *d_offsets, int64_t groups, uint8_t *d_keep,
                                  int max_waves, void *stream)
{
    if (groups < 0 || groups > (int64_t)0x7FFFFFFF || max_waves < 0) return -2;
    if (groups == 0) return 0;
    if (!d_rows || !d_offsets || !d_keep || ((uintptr_t)d_rows & 15u) || ((uintptr_t)d_offsets & 7u)) return -2;
    const int64_t full = (int64_t)sdk_device_cu_count() * 8;
    const int64_t waves = max_waves > 0 ? (int64_t)max_waves : full;
    hipLaunchKernelGGL(ua_minimal_kernel, dim3((unsigned)(waves > 0 ? waves : 1)), dim3(UA_THREADS), 0,
                       (hipStream_t)stream, d_rows, d_offsets, groups, d_keep);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
