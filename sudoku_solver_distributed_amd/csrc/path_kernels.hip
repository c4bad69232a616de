// path_kernels.hip -- translation unit of the solving path (path.h):
// path_wave_kernel, path_info_kernel and their C ABI entries
// (sdk_path_scratch_bytes, sdk_path_batch).  A unit of its own, LLVM's default
// flags: the solve workspace, the logic unit and the other units' flags are
// not involved (common.h is included for cached_occupancy and the wave helpers
// alone).  DESIGN.md §27.
//
// path_wave_kernel: one WAVE per board, persistent one-wave workgroups
// claiming boards one at a time from a 64-bit head.  The lanes read the
// board's 81 cells and their pencil marks, a cell a lane, and 27 lanes gather
// the state's 27 words into LDS twice -- S0, the round's start state, which
// every enumeration reads, and S, where a class's removals land.  Per round
// the lanes build the 72 matrices of logic.h from S0 into their own columns
// of two LDS arrays (lane l matrix l, lanes 0..7 matrix 64 + l as well; nine
// words 64 apart, no two lanes share a bank) and keep them for the whole
// round.  Dead and solved are read off them; then,
// class by class in ascending order:
//   pass A  every lane enumerates the class on its matrices (rule L: lane l
//           the (digit, box) pairs l and 64 + l), clears what an effective
//           firing removes in S with LDS atomic ANDs and counts its firings;
//           the lanes' counts meet in one LDS fetch-add each, whose return is
//           the lane's offset among the round's rows.  A class that counts
//           nothing has left S as it was and the next class is tried.
//   pass B  the class fired: `left` is read from S, lane 0 claims the round's
//           rows with one 64-bit fetch-add on the row cursor, and every lane
//           enumerates again on S0, writing each effective firing at its
//           offset -- one 16-byte store a row, none at or past the capacity.
// Then S becomes S0.  No row is staged anywhere; no wave waits for another.
//
// path_info_kernel: one lane writes {total, listed} from the row cursor.
//
// Scratch: 64 bytes, the board head (byte 0) and the row cursor (byte 8),
// zeroed by the call itself in stream order.
#include "common.h"
#include "path.h"

#define PATH_THREADS 64  // one wave per workgroup
#ifndef SDK_PATH_WAVES_PER_EU
#define SDK_PATH_WAVES_PER_EU 3
#endif
#define PATH_HEAD_BYTES 64

// Board p's start state as 27 plane words into S0 and S: the lanes take the
// 81 cells (a given's own digit, else all nine, ANDed with the cell's pencil
// marks) into CELL, then 27 lanes gather a word each.  Byte and 16-bit loads:
// d_boards needs no alignment and no byte outside the board is read.  False
// for a byte > 9 or a mark above 0x1FF.
__device__ __forceinline__ bool path_load(const uint8_t *boards, const uint16_t *start, int64_t p, uint32_t *CELL, uint32_t *S0,
                                          uint32_t *S, int lane)
{
    bool bad = false;
    for (int c = lane; c < 81; c += PATH_THREADS) {
        const uint32_t v = boards ? (uint32_t)boards[p * 81 + c] : 0u;
        const uint32_t s = start ? (uint32_t)start[p * 81 + c] : 0x1FFu;
        bad = bad || v > 9u || (s & ~0x1FFu);
        CELL[c] = (v ? 1u << ((v - 1u) & 15u) : 0x1FFu) & s;
    }
    wave_lds_sync();
    if (lane < 27) {
        const int d = lane / 3, band = lane % 3;
        uint32_t w = 0;
        for (int k = 0; k < 27; ++k) w |= ((CELL[27 * band + k] >> d) & 1u) << (10 * (k / 9) + k % 9);
        S0[lane] = S[lane] = w;
    }
    wave_lds_sync();
    return !wany(bad);
}

__device__ __forceinline__ uint64_t path_first64(unsigned long long h)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(h >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)h);
}

// lane 0 takes k places at *counter; every lane gets the first
__device__ __forceinline__ uint64_t path_claim(unsigned long long *counter, uint32_t k, int lane)
{
    unsigned long long h = 0;
    if (lane == 0) h = __hip_atomic_fetch_add(counter, (unsigned long long)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return path_first64(h);
}

// the least v of the wave through the LDS word *red
__device__ __forceinline__ uint32_t path_wave_min(uint32_t v, uint32_t *red, int lane)
{
    if (lane == 0) *red = 0xFFFFFFFFu;
    wave_lds_sync();
    if (v != 0xFFFFFFFFu) atomicMin(red, v);
    wave_lds_sync();
    const uint32_t m = *red;
    wave_lds_sync();
    return m;
}

// the sum of v over the wave through the LDS word *red; `before`: the sum of
// the lanes that came first
__device__ __forceinline__ uint32_t path_wave_sum(uint32_t v, uint32_t *red, int lane, uint32_t &before)
{
    if (lane == 0) *red = 0u;
    wave_lds_sync();
    before = atomicAdd(red, v);
    wave_lds_sync();
    const uint32_t s = *red;
    wave_lds_sync();
    return s;
}

// Class c on this lane's share of the round's start state: hall(m, M, I, u,
// removed) / lck(d, dir, line, box, t, idx, mask) for every effective firing.
// Returns the lane's smallest violation as m << 18 | I << 9 | u.
template <typename Hall, typename Lck>
__device__ __forceinline__ uint32_t path_class(int c, const uint32_t *S0, const uint32_t *M0, const uint32_t *M1, int lane,
                                               Hall hall, Lck lck)
{
    uint32_t bad = path::NO_VIOLATION;
    if (c == path::C_L) {
        for (int q = lane; q < path::L_PAIRS; q += PATH_THREADS) {
            const int d = q / 9, box = q % 9;
            path::l_pair(S0, d, box, [&](int dir, int line, int t, int idx, uint32_t mask) { lck(d, dir, line, box, t, idx, mask); });
        }
        return bad;
    }
    const int k = path::class_size(c);
    for (int slot = 0; slot < 2; ++slot) {
        const int m = lane + PATH_THREADS * slot;
        if (m >= logic::MATRICES || !path::class_has(c, m)) continue;
        const uint32_t *M = slot ? M1 : M0;
        const uint32_t v = path::hall_class<PATH_THREADS>(M, k, [&](uint32_t I, uint32_t u, int n) { hall(m, M, I, u, n); });
        if (v != path::NO_VIOLATION) {
            const uint32_t key = ((uint32_t)m << 18) | v;
            bad = key < bad ? key : bad;
        }
    }
    return bad;
}

// the call's arguments as one kernel argument: a field is read from the
// kernel-argument segment where it is used (a scalar load) and is not held in
// a scalar register across the rounds
struct PathArgs {
    const uint8_t *boards;
    const uint16_t *start;
    uint32_t *rows;
    int32_t *count, *rounds, *status, *hist;
    uint16_t *marks;
    unsigned long long *head;  // [0] the board head, [1] the row cursor
    int64_t n, capacity;
    uint32_t rules;
    int max_rounds;
};

// The kernel's one argument where it lies, at the start of the kernel-argument
// segment, behind an empty asm: the compiler cannot move the loads of its
// fields out of the board loop and hold them in scalar registers there.
typedef const PathArgs __attribute__((address_space(4))) *PathArgsPtr;
__device__ __forceinline__ PathArgsPtr path_args()
{
    PathArgsPtr a = (PathArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return a;
}

__global__ __launch_bounds__(PATH_THREADS, SDK_PATH_WAVES_PER_EU) void path_wave_kernel(const PathArgs)  // (read through path_args(): it stays the kernel's only argument)
{
    // the state's 27 plane words, word 3 d + b = P[d][b]; a lane's two matrices, nine words 64 apart
    __shared__ uint32_t S[32], S0[32], MM[2 * 9 * PATH_THREADS], CELL[81], HH[path::CLASSES], red[1];
    const int lane = threadIdx.x;
    const uint32_t *M0 = MM + lane, *M1 = MM + 9 * PATH_THREADS + lane;
    for (;;) {
        const uint64_t at = path_claim(path_args()->head, 1u, lane);
        if (at >= (uint64_t)path_args()->n) break;
        const int64_t p = (int64_t)at;
        int st = path::INVALID, r = 0, events = 0;
        if (lane < path::CLASSES) HH[lane] = 0u;  // the board's events per class
        const PathArgsPtr in = path_args();
        const bool valid = path_load(in->boards, in->start, p, CELL, S0, S, lane);
        int left = path::left_of(S0);
        while (valid) {
            const uint32_t rules = path_args()->rules;
            const int max_rounds = path_args()->max_rounds;
            logic::build<PATH_THREADS>(S0, lane, MM + lane);
            if (lane < logic::MATRICES - PATH_THREADS)
                logic::build<PATH_THREADS>(S0, PATH_THREADS + lane, MM + 9 * PATH_THREADS + lane);
            // 1: dead -- the smallest (m, I) among the matrices 18..71 with an empty row
            uint32_t key = path::NO_VIOLATION;
            if (lane >= 18) {
                const uint32_t I = path::empty_row<PATH_THREADS>(M0);
                if (I) key = ((uint32_t)lane << 9) | I;
            }
            if (lane < logic::MATRICES - PATH_THREADS) {
                const uint32_t I = path::empty_row<PATH_THREADS>(M1);
                if (I && key == path::NO_VIOLATION) key = ((uint32_t)(PATH_THREADS + lane) << 9) | I;
            }
            uint32_t w1 = 0, w2 = 0;
            bool contradiction = false;
            if (wany(key != path::NO_VIOLATION)) {
                key = path_wave_min(key, red, lane);
                contradiction = true;
                w1 = path::word1(r + 1, 0, true, 0);
                w2 = path::hall_word((int)(key >> 9), key & 0x1FFu, 0u);
            } else {
                // 2, 3: solved (the nine rows hold every cell), the round limit
                const uint64_t single = __builtin_amdgcn_ballot_w64(lane >= 45 && lane < 54 && path::all_single<PATH_THREADS>(M0));
                if (__builtin_popcountll(single) == 9) {
                    st = path::SOLVED;
                    break;
                }
                if (max_rounds > 0 && r == max_rounds) {
                    st = path::LIMITED;
                    break;
                }
            }
            // 4: the classes in ascending order, pass A
            int fired = -1;
            uint32_t total = 0, before = 0;
            for (int c = 0; c < path::CLASSES && !contradiction; ++c) {
                if (!((rules >> c) & 1u)) continue;
                uint32_t cnt = 0;
                const uint32_t bad = path_class(
                    c, S0, M0, M1, lane,
                    [&](int m, const uint32_t *M, uint32_t I, uint32_t u, int) {
                        ++cnt;
                        path::hall_cells<PATH_THREADS>(m, M, I, u, [&](int d, int band, int pos) { atomicAnd(&S[3 * d + band], ~(1u << pos)); });
                    },
                    [&](int d, int, int, int, int t, int idx, uint32_t mask) {
                        ++cnt;
                        path::unit_cells(t, idx, mask, [&](int band, int pos) { atomicAnd(&S[3 * d + band], ~(1u << pos)); });
                    });
                if (c > path::C_L && wany(bad != path::NO_VIOLATION)) {
                    const uint32_t v = path_wave_min(bad, red, lane);
                    contradiction = true;
                    w1 = path::word1(r + 1, c, true, 0);
                    w2 = path::hall_word((int)(v >> 18), (v >> 9) & 0x1FFu, v & 0x1FFu);
                    break;
                }
                total = path_wave_sum(cnt, red, lane, before);
                if (total) {
                    fired = c;
                    break;
                }
            }
            if (contradiction) {
                // one row, the candidates left before the round
                const PathArgsPtr list = path_args();
                const uint64_t slot = path_claim(list->head + 1, 1u, lane);
                if (lane == 0 && slot < (uint64_t)list->capacity) ((uint4 *)list->rows)[slot] = make_uint4((uint32_t)p, w1, w2, (uint32_t)left);
                ++events;
                st = path::DEAD;
                break;
            }
            if (fired < 0) {
                st = path::STUCK;
                break;
            }
            // 5: the round -- pass B on the same start state
            ++r;
            left = path::left_of(S);
            const PathArgsPtr list = path_args();
            const uint64_t capacity = (uint64_t)list->capacity;
            uint4 *const rows = (uint4 *)list->rows;
            uint64_t slot = path_claim(list->head + 1, total, lane) + before;
            const uint32_t owner = (uint32_t)p, after = (uint32_t)left;
            path_class(
                fired, S0, M0, M1, lane,
                [&](int m, const uint32_t *, uint32_t I, uint32_t u, int removed) {
                    if (slot < capacity)
                        rows[slot] = make_uint4(owner, path::word1(r, fired, false, removed), path::hall_word(m, I, u), after);
                    ++slot;
                },
                [&](int d, int dir, int line, int box, int, int, uint32_t mask) {
                    if (slot < capacity)
                        rows[slot] = make_uint4(owner, path::word1(r, path::C_L, false, __builtin_popcount(mask)),
                                                path::l_word(dir, d, line, box), after);
                    ++slot;
                });
            events += (int)total;
            if (lane == 0) HH[fired] += total;
            wave_lds_sync();  // pass B has read S0
            if (lane < 27) S0[lane] = S[lane];
            wave_lds_sync();
        }
        const PathArgsPtr out = path_args();
        if (lane == 0) {
            out->count[p] = events;
            out->rounds[p] = r;
            out->status[p] = st;
        }
        if (out->hist && lane < path::CLASSES) out->hist[p * 9 + lane] = (int32_t)HH[lane];
        if (out->marks) {
            const bool keep = st != path::INVALID && st != path::DEAD;
            for (int c = lane; c < 81; c += PATH_THREADS) {
                const int band = plane::cell_band(c), pos = plane::cell_pos(c);
                uint32_t m = 0;
                for (int d = 0; d < 9; ++d) m |= ((S0[3 * d + band] >> pos) & 1u) << d;
                out->marks[p * 81 + c] = (uint16_t)(keep ? m : 0u);
            }
        }
        wave_lds_sync();  // the marks have been read before the next board's state is written
    }
}

__global__ void path_info_kernel(const unsigned long long *__restrict__ head, int64_t capacity, int64_t *__restrict__ info)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int64_t total = (int64_t)head[1];
        info[0] = total;
        info[1] = total < capacity ? total : capacity;
    }
}

// ==================================================================== C ABI
static std::atomic<int> g_path_bpc{0};

static int64_t path_full_waves()
{
    const int per_cu = 4 * SDK_PATH_WAVES_PER_EU;  // four SIMDs per CU
    return (int64_t)sdk_device_cu_count() * cached_occupancy(path_wave_kernel, PATH_THREADS, per_cu, per_cu, g_path_bpc);
}

extern "C" {

size_t sdk_path_scratch_bytes(int64_t n, int max_waves)
{
    if (n < 0 || n > (int64_t)0x7FFFFFFF || max_waves < 0) return 0;
    return PATH_HEAD_BYTES;
}

int sdk_path_batch(const uint8_t *d_boards, const uint16_t *d_start, uint32_t rules, int max_rounds, int64_t n, uint32_t *d_rows,
                   int64_t capacity, int32_t *d_count, int32_t *d_rounds, int32_t *d_status, int32_t *d_hist, uint16_t *d_marks,
                   int64_t *d_info, void *d_scratch, size_t scratch_bytes, int max_waves, void *stream)
{
    if (n < 0 || n > (int64_t)0x7FFFFFFF || (rules & ~(uint32_t)logic::ALL) || !(rules & logic::N) || max_rounds < 0 ||
        capacity < 0 || capacity > (int64_t)(INT64_MAX / 16) || max_waves < 0)
        return -2;
    if (n == 0) return 0;
    if ((!d_boards && !d_start) || !d_count || !d_rounds || !d_status || !d_info || !d_scratch || (capacity > 0 && !d_rows) ||
        ((uintptr_t)d_start & 1u) || ((uintptr_t)d_marks & 1u) || ((uintptr_t)d_rows & 15u) || ((uintptr_t)d_count & 3u) ||
        ((uintptr_t)d_rounds & 3u) || ((uintptr_t)d_status & 3u) || ((uintptr_t)d_hist & 3u) || ((uintptr_t)d_info & 7u) ||
        ((uintptr_t)d_scratch & 7u) || scratch_bytes < sdk_path_scratch_bytes(n, max_waves))
        return -2;
    hipStream_t st = (hipStream_t)stream;
    // the board head and the row cursor, re-armed in stream order before the kernels
    if (hipMemsetAsync(d_scratch, 0, PATH_HEAD_BYTES, st) != hipSuccess) return -1;
    unsigned long long *head = (unsigned long long *)d_scratch;
    const int64_t full = path_full_waves();
    const int64_t cap = max_waves > 0 ? (int64_t)max_waves : full > 0 ? full : 1;
    const PathArgs args{d_boards, d_start, d_rows, d_count, d_rounds, d_status, d_hist, d_marks, head, n, capacity, rules, max_rounds};
    hipLaunchKernelGGL(path_wave_kernel, dim3((unsigned)(n < cap ? n : cap)), dim3(PATH_THREADS), 0, st, args);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(path_info_kernel, dim3(1), dim3(PATH_THREADS), 0, st, (const unsigned long long *)head, capacity, d_info);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
