// enum_kernels.hip -- translation unit of the completion list (plane_enum.h):
// enum_kernel, its two small companions and the C ABI entries
// (sdk_enumerate_scratch_bytes, sdk_enumerate_batch).  A unit of its own, like
// exact_kernels.hip, whose round it repeats: the other units, their flags and
// the solve workspace are not involved (common.h is included for
// cached_occupancy alone), and exact_kernel's code generation stays as it is.
//
// enum_kernel is one ROUND in exact_kernel's shape: one task per LANE,
// persistent one-wave workgroups, the same grid in every round of a call, a
// park word per lane, the claim on ring lines and then on boards with one
// fetch-add of lane 0 each, plane::enum_iter per loop iteration, donate or
// park at the stop.  What it adds is the emission (plane::enum_emit): at a
// SOLVED verdict, while the planes hold the grid, the lane takes a slot from
// the head block's 64-bit cursor with one agent-scope fetch-add of 1 (the
// compiler turns the adds of the lanes that solved in the same iteration
// into one add of their number by lane 0 and a prefix count: the slots stay
// dense either way), writes the grid with plane::store_values and the owner
// with a vector store when the slot is below the capacity; and the per-board
// limit, for which the board's count is a ticket drawn per completion.  No
// lane or wave waits for another and nothing is polled.
//
// Scratch: exact_kernels.hip's layout -- [0, 256) the head block (plane_exact.h's
// XH_ words and plane_enum.h's XH_TOTAL), then per wave 64 lanes x
// COUNT_MAX_DEPTH stack lines of 128 bytes, the ring's lines, 8 bytes a lane
// of park words, 4 bytes a board of open-task counters.  Nothing of the list
// is initialised: rows at or beyond `listed` are never written.
#include <mutex>

#include "common.h"
#include "plane_enum.h"
#include "plane_stack.h"

#define ENUM_THREADS 64    // one wave per workgroup
#define ENUM_WAVES_PER_EU 4
#define ENUM_HEAD_BYTES 256
#define ENUM_LANE_BYTES ((uint32_t)plane::COUNT_MAX_DEPTH * 128u)
#define ENUM_WAVE_BYTES (64u * ENUM_LANE_BYTES)
#define ENUM_MAX_BOARDS ((int64_t)INT32_MAX)
#define ENUM_MAX_TASKS ((int64_t)INT32_MAX)
#define ENUM_MAX_ROWS ((int64_t)INT32_MAX)
static_assert(plane::XH_WORDS * 8 == ENUM_HEAD_BYTES, "head block");
static_assert(plane::XH_TOTAL < 8, "the cursor lies in the 64 bytes read back after a round");
static_assert(plane::ENUM_DONE == SDK_ENUM_DONE && plane::ENUM_PARTIAL == SDK_ENUM_PARTIAL &&
                  plane::ENUM_LIMITED == SDK_ENUM_LIMITED,
              "statuses");

// The 21 words of the board at `src` (any alignment): the 21 aligned dwords
// that hold its 81 bytes, funnel-shifted into place (exact_load_words).
__device__ __forceinline__ void enum_load_words(const uint8_t *src, uint32_t (&x)[21])
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

struct EnumAtomics {
    __device__ __forceinline__ uint64_t load(const uint64_t *p) const
    {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ bool cas(uint64_t *p, uint64_t &expected, uint64_t desired) const
    {
        return __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
    }
};

// what a round's lanes share: the head block and the ring (plane_exact.h)
struct EnumShared {
    uint64_t *head;
    uint32_t *ring;
    uint64_t cap, head0, limit, target;
    uint32_t slot0;  // head0's slot
    __device__ __forceinline__ bool wants() const { return EnumAtomics().load(&head[plane::XH_TAIL]) - limit < target; }
    __device__ __forceinline__ uint64_t reserve(uint32_t k) const
    {
        return plane::exact_reserve(EnumAtomics(), &head[plane::XH_TAIL], head0, cap, k);
    }
    // the line of a position in [head0, head0 + cap)
    __device__ __forceinline__ sdk_v4u *line(uint64_t pos) const
    {
        return (sdk_v4u *)(ring + plane::exact_slot(pos, head0, slot0, cap) * plane::STACK_LINE_WORDS);
    }
    __device__ __forceinline__ void put(uint64_t pos, plane::Board &B, const uint32_t (&und)[3], uint32_t entry,
                                        uint32_t board) const
    {
        sdk_v4u *w = line(pos);
        plane::pin_board(B);
#define XQ(a, b, c, d) (sdk_v4u){B.P[a / 3][a % 3], B.P[b / 3][b % 3], B.P[c / 3][c % 3], B.P[d / 3][d % 3]}
        w[0] = XQ(0, 1, 2, 3);
        w[1] = XQ(4, 5, 6, 7);
        w[2] = XQ(8, 9, 10, 11);
        w[3] = XQ(12, 13, 14, 15);
        w[4] = XQ(16, 17, 18, 19);
        w[5] = XQ(20, 21, 22, 23);
#undef XQ
        w[6] = (sdk_v4u){B.P[8][0], B.P[8][1], B.P[8][2], entry};
        w[7] = (sdk_v4u){und[0], und[1], und[2], board};
    }
    __device__ __forceinline__ uint32_t get(uint64_t pos, plane::Board &B, uint32_t (&und)[3], uint32_t &board) const
    {
        const sdk_v4u *w = line(pos);
        const sdk_v4u q0 = w[0], q1 = w[1], q2 = w[2], q3 = w[3], q4 = w[4], q5 = w[5], t = w[6], u = w[7];
        PlaneStack::unpack(B, q0, q1, q2, q3, q4, q5, t);
        und[0] = u.x; und[1] = u.y; und[2] = u.z;
        board = u.w;
        plane::pin_board(B);
        return t.w;
    }
};

// the list, as plane::enum_emit reaches it
struct EnumOut {
    unsigned long long *count;
    uint64_t *head;
    uint8_t *grids;
    int32_t *owner;
    __device__ __forceinline__ uint64_t ticket(uint32_t board) const
    {
        return __hip_atomic_fetch_add(&count[board], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ uint64_t slot() const
    {
        return __hip_atomic_fetch_add(&head[plane::XH_TOTAL], (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void write(uint64_t slot, const plane::Board &B, uint32_t board) const
    {
        uint8_t *dst = grids + slot * 81;
        plane::store_values(B, [&](int c, uint32_t v) { dst[c] = (uint8_t)v; });
        owner[slot] = (int32_t)board;
    }
};

struct EnumArgs {
    const uint8_t *puzzles;
    unsigned long long *count;
    int32_t *status, *open;
    uint64_t *head;
    uint32_t *ring;
    uint2 *park;
    uint8_t *stack;
    uint8_t *grids;
    int32_t *owner;
    uint64_t n, cap, head0, limit, target;
    uint64_t capacity, per_board;  // rows of the list; the per-board limit (0: none)
    uint32_t slot0, slice;
};

__device__ __forceinline__ uint64_t enum_first_lane(unsigned long long v)
{
    return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) |
           __builtin_amdgcn_readfirstlane((uint32_t)v);
}

__global__ __launch_bounds__(ENUM_THREADS, ENUM_WAVES_PER_EU) void enum_kernel(const EnumArgs a)
{
    const int lane = threadIdx.x;
    const PlaneStack stk = {__builtin_amdgcn_make_buffer_rsrc(a.stack + (size_t)blockIdx.x * ENUM_WAVE_BYTES, 0,
                                                              (int)ENUM_WAVE_BYTES, 0x00020000),
                            (uint32_t)lane * ENUM_LANE_BYTES};
    const EnumShared sh = {a.head, a.ring, a.cap, a.head0, a.limit, a.target, a.slot0};
    const EnumOut out = {a.count, a.head, a.grids, a.owner};
    const uint32_t slice = a.slice;
    const uint64_t per_board = a.per_board, capacity = a.capacity;
    uint2 *const mypark = a.park + (size_t)blockIdx.x * 64 + lane;
    plane::Board B;
    uint32_t und[3] = {0u, 0u, 0u}, nd[3] = {0u, 0u, 0u}, found = 0, passes = 0;
    // a stack parked in the round before: the search goes on at its deepest level
    const uint2 pk = *mypark;
    uint32_t depth = pk.x, board = pk.y;
    bool active = depth != 0, resume = active;
    if (active) *mypark = make_uint2(0u, 0u);
    int32_t dopen = 0;
    uint32_t donated = 0, parks = 0;
    bool tasks_out = false, boards_out = false;
    for (;;) {
        const bool want = !active && passes < slice;
        const uint64_t wantm = __builtin_amdgcn_ballot_w64(want);
        const int nwant = __builtin_popcountll(wantm);
        const bool none_active = __builtin_amdgcn_ballot_w64(active) == 0;
        const bool queue_out = tasks_out && boards_out;
        if (none_active && (nwant == 0 || queue_out)) break;
        if (!queue_out && nwant > 0 && (nwant >= plane::EXACT_REFILL || none_active)) {
            uint64_t ntask = 0, tbase = 0, bbase = a.n;
            if (!tasks_out) {
                unsigned long long h = 0;
                if (lane == 0)
                    h = __hip_atomic_fetch_add(&a.head[plane::XH_CLAIM], (uint64_t)nwant, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                tbase = enum_first_lane(h);
                const uint64_t len = a.limit - a.head0;
                ntask = tbase >= len ? 0 : len - tbase < (uint64_t)nwant ? len - tbase : (uint64_t)nwant;
                tasks_out = tbase + (uint64_t)nwant >= len;  // the readable part is handed out: no further claim
            }
            if (ntask < (uint64_t)nwant && !boards_out) {
                const uint64_t k = (uint64_t)nwant - ntask;
                unsigned long long h = 0;
                if (lane == 0)
                    h = __hip_atomic_fetch_add(&a.head[plane::XH_BOARDS], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                bbase = enum_first_lane(h);
                boards_out = bbase + k >= a.n;
            }
            const uint64_t rank =
                __builtin_amdgcn_mbcnt_hi((uint32_t)(wantm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)wantm, 0u));
            if (want && rank < ntask) {
                // a task line: level 0 of this lane's stack, then as from a DEAD verdict
                const uint32_t e = sh.get(a.head0 + tbase + rank, B, und, board);
                stk.push(0, B, und, e);
                depth = 1;
                active = resume = true;
            } else if (want && bbase + (rank - ntask) < a.n) {
                board = (uint32_t)(bbase + (rank - ntask));
                uint32_t x[21], given[3];
                enum_load_words(a.puzzles + (size_t)board * 81, x);
                bool clash = false;
                if (!plane::load_words(B, x, clash, given)) {
                    a.status[board] = SDK_INVALID;
                    a.open[board] = 0;  // (the board's only task: nobody else touches its counter)
                    dopen--;
                } else if (clash) {
                    a.open[board] = 0;  // no valid completion, an exact zero
                    dopen--;
                } else {
                    active = true;
                    resume = false;
                    depth = 0;
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        nd[b] = given[b];
                        und[b] = plane::andn(plane::ROWS, given[b]);
                    }
                }
            }
        }
        if (active) {
            int k = plane::X_DONE;
            // a line or a parked stack of a board that has reached its limit is dropped
            if (!(per_board && resume &&
                  plane::enum_dropped(resume, EnumAtomics().load((const uint64_t *)&a.count[board]), per_board)))
                k = plane::enum_iter(B, und, nd, depth, passes, resume, slice, stk, (uint32_t)plane::COUNT_MAX_DEPTH,
                                     [&](const plane::Board &S) {
                                         return plane::enum_emit(S, board, found, per_board, capacity, out);
                                     });
            if (k != plane::X_CONT) {
                active = false;
                if (k == plane::X_FAULT) {
                    a.status[board] = SDK_FAULT;
                    found = 0;
                }
                if (found)
                    __hip_atomic_fetch_add(&a.count[board], (unsigned long long)found, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                found = 0;
                if (k != plane::X_STOP) {  // the task's end
                    __hip_atomic_fetch_add(&a.open[board], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    dopen--;
                } else if (plane::exact_donate(B, und, depth, board, stk, sh)) {
                    if (depth > 1)
                        __hip_atomic_fetch_add(&a.open[board], (int32_t)depth - 1, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                    dopen += (int32_t)depth - 1;
                    donated += depth;
                } else {
                    *mypark = make_uint2(depth, board);
                    parks++;
                }
            }
        }
    }
    // the wave's share of the call's counters: one atomic each
    uint32_t most = passes;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        dopen += __shfl_xor(dopen, s, 64);
        donated += __shfl_xor(donated, s, 64);
        parks += __shfl_xor(parks, s, 64);
        const uint32_t o = __shfl_xor(most, s, 64);
        most = o > most ? o : most;
    }
    if (lane == 0) {
        if (dopen)
            __hip_atomic_fetch_add(&a.head[plane::XH_OPEN], (uint64_t)(int64_t)dopen, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        if (donated)
            __hip_atomic_fetch_add(&a.head[plane::XH_DONATED], (uint64_t)donated, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        if (parks)
            __hip_atomic_fetch_add(&a.head[plane::XH_PARKS], (uint64_t)parks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (most)
            __hip_atomic_fetch_max(&a.head[plane::XH_MAXPASS], (uint64_t)most, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
}

// a call's start: every board is one open task, nothing counted, nobody
// parked, the cursor at row 0
__global__ __launch_bounds__(256) void enum_init_kernel(unsigned long long *__restrict__ count,
                                                         int32_t *__restrict__ status, int32_t *__restrict__ open,
                                                         uint64_t n, uint2 *__restrict__ park, uint64_t lanes,
                                                         uint64_t *__restrict__ head)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = t; i < n; i += stride) {
        count[i] = 0;
        status[i] = 0;
        open[i] = 1;
    }
    for (uint64_t i = t; i < lanes; i += stride) park[i] = make_uint2(0u, 0u);
    if (t < plane::XH_WORDS) head[t] = t == plane::XH_OPEN ? n : 0;
}

// a call's end: DONE / LIMITED / PARTIAL and the clamped count (plane::enum_final)
__global__ __launch_bounds__(256) void enum_final_kernel(unsigned long long *__restrict__ count,
                                                          int32_t *__restrict__ status,
                                                          const int32_t *__restrict__ open, uint64_t n, uint64_t per_board)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t c = count[i];
        int32_t s = status[i];
        plane::enum_final(c, s, open[i], per_board);
        count[i] = c;
        status[i] = s;
    }
}

// ==================================================================== C ABI
static std::atomic<int> g_enum_bpc{0};
static std::mutex g_enum_mu;  // one launch sequence at a time

// waves of a full grid on the current device: every CU at the kernel's occupancy
static int64_t enum_full_waves()
{
    const int per_cu = 4 * ENUM_WAVES_PER_EU;  // four SIMDs per CU
    return (int64_t)sdk_device_cu_count() * cached_occupancy(enum_kernel, ENUM_THREADS, per_cu, per_cu, g_enum_bpc);
}

// the grid of a call: the same in every round, whatever n
static int64_t enum_waves(int max_waves) { return max_waves > 0 ? (int64_t)max_waves : enum_full_waves(); }

struct EnumLayout {
    size_t stack, ring, park, open, bytes;
    uint64_t waves, cap;
};

static EnumLayout enum_layout(int64_t n, int max_waves, int64_t max_tasks)
{
    EnumLayout l;
    l.waves = (uint64_t)enum_waves(max_waves);
    l.cap = plane::exact_ring_lines(64 * l.waves, (uint64_t)max_tasks);
    l.stack = ENUM_HEAD_BYTES;
    l.ring = l.stack + (size_t)l.waves * ENUM_WAVE_BYTES;
    l.park = l.ring + (size_t)l.cap * 128;
    l.open = l.park + (size_t)l.waves * 64 * 8;
    l.bytes = l.open + (((size_t)n * 4 + 15) & ~(size_t)15);
    return l;
}

extern "C" {

size_t sdk_enumerate_scratch_bytes(int64_t n, int max_waves, int64_t max_tasks)
{
    if (n < 0 || n > ENUM_MAX_BOARDS || max_waves < 0 || max_tasks < 0 || max_tasks > ENUM_MAX_TASKS) return 0;
    return enum_layout(n, max_waves, max_tasks).bytes;
}

int sdk_enumerate_batch(const uint8_t *d_boards, int64_t n, uint8_t *d_grids, int32_t *d_owner, int64_t capacity,
                        int64_t limit, int64_t *d_count, int32_t *d_status, int slice, int max_rounds,
                        int64_t max_tasks, void *d_scratch, size_t scratch_bytes, int max_waves, void *stream,
                        int64_t *info)
{
    if (n == 0) return 0;
    if (n < 0 || n > ENUM_MAX_BOARDS || max_waves < 0 || slice < 1 || max_rounds < 1 || max_tasks < 0 ||
        max_tasks > ENUM_MAX_TASKS)
        return -2;
    if (capacity < 0 || capacity > ENUM_MAX_ROWS || limit < 0) return -2;
    if (capacity > 0 && (!d_grids || !d_owner || ((uintptr_t)d_owner & 3u))) return -2;
    if (!d_boards || !d_count || ((uintptr_t)d_count & 7u) || !d_status || ((uintptr_t)d_status & 3u) || !d_scratch ||
        ((uintptr_t)d_scratch & 15u))
        return -2;
    const EnumLayout l = enum_layout(n, max_waves, max_tasks);
    if (scratch_bytes < l.bytes) return -2;
    // every completion costs a pass: a pass budget below 2^63 keeps d_count and the cursor from overflowing
    if ((unsigned __int128)max_rounds * ((uint64_t)slice + plane::EXACT_RUN_MAX) * (64 * l.waves) >> 63) return -2;
    std::lock_guard<std::mutex> lk(g_enum_mu);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *sc = (uint8_t *)d_scratch;
    EnumArgs a;
    a.puzzles = d_boards;
    a.count = (unsigned long long *)d_count;
    a.status = d_status;
    a.open = (int32_t *)(sc + l.open);
    a.head = (uint64_t *)sc;
    a.ring = (uint32_t *)(sc + l.ring);
    a.park = (uint2 *)(sc + l.park);
    a.stack = sc + l.stack;
    a.grids = d_grids;
    a.owner = d_owner;
    a.n = (uint64_t)n;
    a.cap = l.cap;
    a.head0 = a.limit = 0;
    a.target = plane::exact_fill_target(64 * l.waves, l.cap);
    a.capacity = (uint64_t)capacity;
    a.per_board = (uint64_t)limit;
    a.slot0 = 0;
    a.slice = (uint32_t)slice;
    const uint64_t most = (uint64_t)n > 64 * l.waves ? (uint64_t)n : 64 * l.waves;
    const unsigned small = (unsigned)((most + 255) / 256 < 1024 ? (most + 255) / 256 : 1024);
    hipLaunchKernelGGL(enum_init_kernel, dim3(small), dim3(256), 0, st, a.count, a.status, a.open, a.n, a.park,
                       64 * l.waves, a.head);
    if (hipGetLastError() != hipSuccess) return -1;
    uint64_t h[8] = {0};
    int rounds = 0;
    for (;;) {
        // the round's claim counter, re-armed in stream order before the kernel
        if (rounds && hipMemsetAsync(&a.head[plane::XH_CLAIM], 0, 8, st) != hipSuccess) return -1;
        hipLaunchKernelGGL(enum_kernel, dim3((unsigned)l.waves), dim3(ENUM_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess) return -1;
        if (hipMemcpyAsync(h, a.head, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
        if (hipStreamSynchronize(st) != hipSuccess) return -1;
        rounds++;
        if (h[plane::XH_OPEN] == 0 || rounds >= max_rounds) break;
        // lines claimed leave the queue; what the round appended joins it
        plane::exact_advance(h[plane::XH_CLAIM], h[plane::XH_TAIL], l.cap, a.head0, a.slot0, a.limit);
    }
    const unsigned fin = (unsigned)(((uint64_t)n + 255) / 256 < 1024 ? ((uint64_t)n + 255) / 256 : 1024);
    hipLaunchKernelGGL(enum_final_kernel, dim3(fin), dim3(256), 0, st, a.count, a.status, a.open, a.n, a.per_board);
    if (hipGetLastError() != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;
    if (info) {
        info[0] = rounds;
        info[1] = (int64_t)h[plane::XH_DONATED];
        info[2] = (int64_t)h[plane::XH_PARKS];
        info[3] = (int64_t)h[plane::XH_MAXPASS];
        info[4] = (int64_t)h[plane::XH_TOTAL];
        info[5] = (int64_t)plane::enum_listed(h[plane::XH_TOTAL], (uint64_t)capacity);
    }
    return 0;
}

}  // extern "C"
