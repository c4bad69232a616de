// logic_kernels.hip -- translation unit of the named techniques (logic.h):
// logic_kernel, logic_wave_kernel and their C ABI entries
// (sdk_logic_scratch_bytes, sdk_logic_batch).  A unit of its own, LLVM's
// default flags: the solve, count, canon and rate units, their flags and their
// workspace are not involved (common.h is included for cached_occupancy and
// the wave helpers alone).
//
// Phase one, logic_kernel: rate_kernel's lane-per-board loop over the
// ladder's leading steps that are levels of rate.h (N, N|H, N|H|L: `lead` of
// them, their levels packed four bits a step).  One board per LANE,
// persistent one-wave workgroups, the queue head claimed as rate_kernel
// claims it.  A lane builds its start state (the board's, ANDed with its
// pencil marks), runs ONE rate::pass per iteration at its own step's level,
// and at a fixpoint writes the board's answer (dead, solved, or undecided at
// the last step), moves a step up, or -- open after the last leading step --
// writes what it has of open and left and appends the board's index to the
// list in the scratch, the lanes that do so in one iteration with one
// fetch-add between them.  With lead == 0 every valid board is listed.
//
// Phase two, logic_wave_kernel: one WAVE per listed board, persistent
// one-wave workgroups claiming list entries one at a time.  Every lane builds
// the board's state for itself (the same instructions on the same data: the
// cost of one lane), closes it under the last leading step's rules again and
// then runs the remaining steps.  A step's closure: N, H and L to their
// fixpoint in every lane's registers; then lane 0 puts the 27 words into LDS
// twice -- S0, the sweep's state, and S, where the sweep's removals land --
// and the lanes take the 72 matrices of logic.h, lane l matrix l and lanes
// 0..7 matrix 64 + l as well (the naked matrices of boxes 1..8: 72 over 64
// lanes, two rounds, the second with eight lanes).  A lane builds its matrix
// from S0 into its own column of an LDS array (nine words, 64 apart: no two
// lanes share a bank), enumerates the subsets of the sizes the step holds
// with their unions built up in registers, and clears what leaves in S with
// LDS atomic ANDs.  After a sweep the wave reads S back; a sweep that cleared
// a bit is followed by N, H and L again, one that cleared nothing ends the
// step.  A lane that finds fewer than k elements in k rows ends the board:
// dead.
//
// Scratch: [0, 256) the control block -- queue head (word 0), list length
// (byte 64), the wave kernel's list head (byte 128) -- zeroed by the call
// itself in stream order; then n int64 list entries.
#include "common.h"
#include "logic.h"

#define LOGIC_THREADS 64  // one wave per workgroup
// (three waves a SIMD: at four, 128 VGPRs, logic_kernel spills 37 registers and logic_wave_kernel 8)
#ifndef SDK_LOGIC_WAVES_PER_EU
#define SDK_LOGIC_WAVES_PER_EU 3
#endif
#ifndef SDK_LOGIC_WAVE_WAVES_PER_EU
#define SDK_LOGIC_WAVE_WAVES_PER_EU 3
#endif
// idle lanes before a wave claims boards (results never depend on it)
#ifndef SDK_LOGIC_REFILL
#define SDK_LOGIC_REFILL 16
#endif
#define LOGIC_HEAD_BYTES 256
#define LOGIC_LIST_COUNT_BYTE 64
#define LOGIC_LIST_HEAD_BYTE 128

struct LogicLadder {
    uint32_t m[logic::MAX_STEPS];
};

// step j's rule set (j wave-uniform: a chain of scalar selects, no indexed kernel argument)
__device__ __forceinline__ uint32_t logic_rules_at(const LogicLadder &lad, int j)
{
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < logic::MAX_STEPS; ++k) v = k == j ? lad.m[k] : v;
    return v;
}

// The 21 words of the board at `src` (any alignment): the 21 aligned dwords
// that hold its 81 bytes (byte 80 lies in dword 20 for every alignment, so
// every dword read holds a byte of the board), funnel-shifted into place.
// Only byte 0 of x[20] is the board's.
__device__ __forceinline__ void logic_load_words(const uint8_t *src, uint32_t (&x)[21])
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

// board p's start state; false for a byte > 9 or a mark above 0x1FF
__device__ __forceinline__ bool logic_load(plane::Board &B, const uint8_t *boards, const uint16_t *start, int64_t p)
{
    bool ok = true;
    if (boards) {
        uint32_t x[21];
        logic_load_words(boards + p * 81, x);
        ok = rate::load(B, x);
    } else {
        logic::empty_board(B);
    }
    if (start) {
        const uint16_t *s = start + p * 81;
        ok = logic::and_marks(B, [&](int c) { return (uint32_t)s[c]; }) && ok;
    }
    return ok;
}

__device__ __forceinline__ uint32_t logic_wave_claim(uint32_t *counter, uint32_t k, int lane)
{
    uint32_t h = 0;
    if (lane == 0) h = __hip_atomic_fetch_add(counter, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)h);
}

__global__ __launch_bounds__(LOGIC_THREADS, SDK_LOGIC_WAVES_PER_EU) void logic_kernel(
    const uint8_t *__restrict__ boards, const uint16_t *__restrict__ start, int32_t *__restrict__ step,
    int32_t *__restrict__ open, int32_t *__restrict__ left, uint16_t *__restrict__ marks, int64_t n, int steps, int lead,
    uint32_t levels, unsigned long long *__restrict__ head, uint32_t *__restrict__ list_count, int64_t *__restrict__ list)
{
    const int lane = threadIdx.x;
    plane::Board B;
    logic::Result R;
    logic::start(R);
    int j = 0;      // this lane's step, 0-based
    int64_t p = 0;  // this lane's board
    bool active = false, queue_out = false;
    for (;;) {
        // what this iteration finishes: 1 the answer in R (marks under `keep`), 2 a board for the list
        int fin = 0;
        uint32_t keep = 0u;
        const uint64_t idle = __builtin_amdgcn_ballot_w64(!active);
        const int nidle = __builtin_popcountll(idle);
        if (queue_out && nidle == 64) break;
        if (!queue_out && nidle >= SDK_LOGIC_REFILL) {
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
                j = 0;
                if (logic_load(B, boards, start, p)) {
                    logic::start(R);
                    if (lead > 0) active = true;
                    else fin = 2;
                } else {
                    logic::invalid(R);
                    fin = 1;
                }
            }
        }
        if (active) {
            int op;
            const int r = rate::pass(B, (int)((levels >> (4 * j)) & 15u), op);
            if (r != rate::R_OPEN) {
                if (logic::settle(R, j, r, op, logic::candidates_left(B), steps)) {
                    fin = 1;
                    keep = r == rate::R_DEAD ? 0u : 0x1FFu;
                } else if (++j == lead) {
                    fin = 2;
                }
            }
            if (fin) active = false;
        }
        if (fin) {
            if (fin == 1) step[p] = R.step;
            if (open) {
#pragma unroll
                for (int k = 0; k < logic::MAX_STEPS; ++k) open[p * 8 + k] = R.open[k];
            }
            if (left) {
#pragma unroll
                for (int k = 0; k < logic::MAX_STEPS; ++k) left[p * 8 + k] = R.left[k];
            }
            if (fin == 1 && marks) {
                uint16_t *m = marks + p * 81;
                rate::store_marks(B, keep, [&](int c, uint32_t v) { m[c] = (uint16_t)v; });
            }
        }
        // the boards the wave kernel has to look at: one claim for the wave's lanes
        const uint64_t listing = __builtin_amdgcn_ballot_w64(fin == 2);
        if (listing) {
            const uint32_t at = logic_wave_claim(list_count, (uint32_t)__builtin_popcountll(listing), lane);
            if (fin == 2) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(listing >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)listing, 0u));
                list[at + rank] = p;
            }
        }
    }
}

// The closure of B (the same in every lane) under `rules`, the Hall steps
// spread over the wave.  S, S0: 32 words each; MM, CC: 9 x 64 words each.
__device__ __forceinline__ int logic_wave_close(plane::Board &B, uint32_t rules, int &op, uint32_t *S, uint32_t *S0,
                                                uint32_t *MM, uint32_t *CC, int lane)
{
    for (;;) {
        const int r = logic::close_nhl(B, rules, op);
        if (r != rate::R_FIX || !(rules & logic::HALL)) return r;
        if (lane == 0) {
#pragma unroll
            for (int w = 0; w < 27; ++w) S0[w] = S[w] = B.P[w / 3][w % 3];
        }
        wave_lds_sync();
        bool dead = false;
        for (int m = lane; m < logic::MATRICES; m += LOGIC_THREADS) {
            const uint32_t ks = logic::sizes(m, rules);
            if (!ks) continue;
            uint32_t *M = MM + lane, *C = CC + lane;
            logic::build<LOGIC_THREADS>(S0, m, M);
            for (int i = 0; i < 9; ++i) C[i * LOGIC_THREADS] = 0u;
            if (logic::hall<LOGIC_THREADS>(M, C, ks)) {
                dead = true;
                break;
            }
            logic::apply<LOGIC_THREADS>(m, M, C, [&](int d, int band, int pos) { atomicAnd(&S[3 * d + band], ~(1u << pos)); });
        }
        wave_lds_sync();
        uint32_t diff = 0;
#pragma unroll
        for (int w = 0; w < 27; ++w) {
            const uint32_t v = S[w];
            diff |= v ^ S0[w];
            B.P[w / 3][w % 3] = v;
        }
        wave_lds_sync();  // everyone has read the words before lane 0 writes them again
        if (wany(dead)) return rate::R_DEAD;
        if (!diff) return rate::R_FIX;
    }
}

__global__ __launch_bounds__(LOGIC_THREADS, SDK_LOGIC_WAVE_WAVES_PER_EU) void logic_wave_kernel(
    const uint8_t *__restrict__ boards, const uint16_t *__restrict__ start, int32_t *__restrict__ step,
    int32_t *__restrict__ open, int32_t *__restrict__ left, uint16_t *__restrict__ marks,
    const uint32_t *__restrict__ list_count, const int64_t *__restrict__ list, uint32_t *__restrict__ list_head,
    LogicLadder lad, int steps, int lead)
{
    // the board's 27 plane words, word 3 d + b = P[d][b]; a lane's matrix and its removals, nine words 64 apart
    __shared__ uint32_t S[32], S0[32], MM[9 * LOGIC_THREADS], CC[9 * LOGIC_THREADS];
    const int lane = threadIdx.x;
    const uint32_t listed = *list_count;
    for (;;) {
        const uint32_t at = logic_wave_claim(list_head, 1u, lane);
        if (at >= listed) break;
        const int64_t p = list[at];
        plane::Board B;  // the same in every lane
        logic_load(B, boards, start, p);
        logic::Result R;
        logic::start(R);
        int op = 0, r = rate::R_FIX;
        // (step lead - 1 again, unsettled: phase one's last fixpoint, the state step `lead` starts from)
        for (int j = lead > 0 ? lead - 1 : 0; j < steps; ++j) {
            r = logic_wave_close(B, logic_rules_at(lad, j), op, S, S0, MM, CC, lane);
            if (j >= lead && logic::settle(R, j, r, op, logic::candidates_left(B), steps)) break;
        }
        if (lane == 0) {
            step[p] = R.step;
#pragma unroll
            for (int k = 0; k < logic::MAX_STEPS; ++k) {
                if (k < lead) continue;
                if (open) open[p * 8 + k] = R.open[k];
                if (left) left[p * 8 + k] = R.left[k];
            }
        }
        if (marks) {
            for (int c = lane; c < 81; c += 64) {
                const uint32_t m = plane::cell_cand(B, plane::cell_band(c), plane::cell_pos(c));
                marks[p * 81 + c] = (uint16_t)(r == rate::R_DEAD ? 0u : m);
            }
        }
    }
}

// ==================================================================== C ABI
static std::atomic<int> g_logic_bpc{0}, g_logic_wave_bpc{0};

// waves of a full grid on the current device: every CU at the kernel's occupancy
template <typename K>
static int64_t logic_full_waves(K kernel, int waves_per_eu, std::atomic<int> &cache)
{
    const int per_cu = 4 * waves_per_eu;  // four SIMDs per CU
    return (int64_t)sdk_device_cu_count() * cached_occupancy(kernel, LOGIC_THREADS, per_cu, per_cu, cache);
}

extern "C" {

size_t sdk_logic_scratch_bytes(int64_t n, int steps)
{
    if (n < 0 || steps < 1 || steps > SDK_LOGIC_MAX_STEPS) return 0;
    if (n > (int64_t)0x7FFFFFFF) return 0;  // the list's counters are 32-bit
    return LOGIC_HEAD_BYTES + (size_t)n * sizeof(int64_t);
}

int sdk_logic_batch(const uint8_t *d_boards, const uint16_t *d_start, const uint32_t *ladder, int steps, int32_t *d_step,
                    int32_t *d_open, int32_t *d_left, uint16_t *d_marks, int64_t n, void *d_scratch, size_t scratch_bytes,
                    void *stream)
{
    if (n < 0 || n > (int64_t)0x7FFFFFFF || !logic::ladder_ok(ladder, steps)) return -2;
    if (n == 0) return 0;
    if ((!d_boards && !d_start) || !d_step || !d_scratch || ((uintptr_t)d_start & 1u) || ((uintptr_t)d_marks & 1u) ||
        ((uintptr_t)d_step & 3u) || ((uintptr_t)d_open & 3u) || ((uintptr_t)d_left & 3u) || ((uintptr_t)d_scratch & 7u) ||
        scratch_bytes < sdk_logic_scratch_bytes(n, steps))
        return -2;
    LogicLadder lad;
    int lead = 0;
    uint32_t levels = 0;
    for (int j = 0; j < logic::MAX_STEPS; ++j) lad.m[j] = j < steps ? ladder[j] : 0u;
    while (lead < steps && logic::rate_level(lad.m[lead])) {
        levels |= (uint32_t)logic::rate_level(lad.m[lead]) << (4 * lead);
        ++lead;
    }
    hipStream_t st = (hipStream_t)stream;
    // the queue head and the list's counters, re-armed in stream order before the kernels
    if (hipMemsetAsync(d_scratch, 0, LOGIC_HEAD_BYTES, st) != hipSuccess) return -1;
    uint8_t *sc = (uint8_t *)d_scratch;
    uint32_t *list_count = (uint32_t *)(sc + LOGIC_LIST_COUNT_BYTE);
    int64_t *list = (int64_t *)(sc + LOGIC_HEAD_BYTES);
    const int64_t want = (n + 63) / 64, cap = logic_full_waves(logic_kernel, SDK_LOGIC_WAVES_PER_EU, g_logic_bpc);
    hipLaunchKernelGGL(logic_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(LOGIC_THREADS), 0, st, d_boards, d_start,
                       d_step, d_open, d_left, d_marks, n, steps, lead, levels, (unsigned long long *)d_scratch, list_count,
                       list);
    if (hipGetLastError() != hipSuccess) return -1;
    if (lead == steps) return 0;
    // one wave per listed board, at most a full grid: how many are listed is known on the device only
    const int64_t tcap = logic_full_waves(logic_wave_kernel, SDK_LOGIC_WAVE_WAVES_PER_EU, g_logic_wave_bpc);
    hipLaunchKernelGGL(logic_wave_kernel, dim3((unsigned)(n < tcap ? n : tcap)), dim3(LOGIC_THREADS), 0, st, d_boards, d_start,
                       d_step, d_open, d_left, d_marks, (const uint32_t *)list_count, (const int64_t *)list,
                       (uint32_t *)(sc + LOGIC_LIST_HEAD_BYTE), lad, steps, lead);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"
