// plane_stack.h -- the 128-byte stack line of the lane solvers on the device:
// one level of one lane's depth-first search, in the workspace of the plane
// kernel (plane_kernel.h) and in the scratch of the count kernel
// (count_kernels.hip).  Both address their lines through a buffer descriptor.
#ifndef SDK_PLANE_STACK_H
#define SDK_PLANE_STACK_H

#include "plane_solver.h"

#ifndef SDK_PLANE_PUSH_PAD
#define SDK_PLANE_PUSH_PAD 1
#endif
static_assert(plane::STACK_ENTRY == 27, "stack layout");
typedef uint32_t sdk_v4u __attribute__((ext_vector_type(4)));

// Per-lane DFS stack in the workspace: level L of lane g is one 128-byte
// line at byte (g * PLANE_MAX_DEPTH + L) * 128, words 0..26 = the 27 planes
// (word 3d+b = P[d][b]), word 27 = the branch entry, words 28..30 = the
// level's undetermined cells (plane::pass_ahead's und[]; the lanes' own: the
// wave-wide solver and the pool records never read them), 31 unused.  A push
// or pop is 8 buffer dwordx4 accesses to ONE line (guesses are lane-
// divergent: a lane-interleaved layout made every push touch 28 lines).
struct PlaneStack {
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t lane_off;  // g * PLANE_MAX_DEPTH * 128 (count_kernel: lane * COUNT_MAX_DEPTH * 128 in its wave's lines)
    __device__ __forceinline__ uint32_t voff(uint32_t level) const { return lane_off + level * 128u; }
    // a value the optimizer cannot trace back to the board's memory layout:
    // four consecutive board words gathered into a vector are otherwise
    // turned into one vector load, which keeps the whole board in scratch
    static __device__ __forceinline__ uint32_t opaque(uint32_t x)
    {
        asm("" : "+v"(x));
        return x;
    }
    __device__ __forceinline__ void push(uint32_t level, plane::Board &B, const uint32_t (&und)[3],
                                         uint32_t entry) const
    {
        const int v = (int)voff(level);
        plane::pin_board(B);
#define PQ(a, b, c, d) (sdk_v4u){B.P[a / 3][a % 3], B.P[b / 3][b % 3], B.P[c / 3][c % 3], B.P[d / 3][d % 3]}
        const sdk_v4u q0 = PQ(0, 1, 2, 3), q1 = PQ(4, 5, 6, 7), q2 = PQ(8, 9, 10, 11), q3 = PQ(12, 13, 14, 15),
                      q4 = PQ(16, 17, 18, 19), q5 = PQ(20, 21, 22, 23),
                      q6 = (sdk_v4u){B.P[8][0], B.P[8][1], B.P[8][2], entry},
                      q7 = (sdk_v4u){und[0], und[1], und[2], 0u};
#undef PQ
        __builtin_amdgcn_raw_buffer_store_b128(q0, rsrc, v, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q1, rsrc, v, 16, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q2, rsrc, v, 32, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q3, rsrc, v, 48, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q4, rsrc, v, 64, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q5, rsrc, v, 80, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q6, rsrc, v, 96, 0);
        __builtin_amdgcn_raw_buffer_store_b128(q7, rsrc, v, 112, 0);
#if SDK_PLANE_PUSH_PAD
        // a dwordx4 store reads its data registers after issue; hipcc pads a
        // following VALU write of them only when soffset is an inline constant,
        // and with a register soffset (offsets past 64) it has reused them at
        // once.  Keeping all eight quads live through a 2-state pad makes
        // every store read its data before any of them is overwritten.
        asm volatile("s_nop 1" ::"v"(q0), "v"(q1), "v"(q2), "v"(q3), "v"(q4), "v"(q5), "v"(q6), "v"(q7));
#endif
    }
    // the 27 planes out of a line's first seven quads (t: the last of them)
    static __device__ __forceinline__ void unpack(plane::Board &B, const sdk_v4u &q0, const sdk_v4u &q1,
                                                  const sdk_v4u &q2, const sdk_v4u &q3, const sdk_v4u &q4,
                                                  const sdk_v4u &q5, const sdk_v4u &t)
    {
        B.P[0][0] = q0.x; B.P[0][1] = q0.y; B.P[0][2] = q0.z; B.P[1][0] = q0.w;
        B.P[1][1] = q1.x; B.P[1][2] = q1.y; B.P[2][0] = q1.z; B.P[2][1] = q1.w;
        B.P[2][2] = q2.x; B.P[3][0] = q2.y; B.P[3][1] = q2.z; B.P[3][2] = q2.w;
        B.P[4][0] = q3.x; B.P[4][1] = q3.y; B.P[4][2] = q3.z; B.P[5][0] = q3.w;
        B.P[5][1] = q4.x; B.P[5][2] = q4.y; B.P[6][0] = q4.z; B.P[6][1] = q4.w;
        B.P[6][2] = q5.x; B.P[7][0] = q5.y; B.P[7][1] = q5.z; B.P[7][2] = q5.w;
        B.P[8][0] = t.x; B.P[8][1] = t.y; B.P[8][2] = t.z;
    }
    // the last quad: planes 24..26 and the branch entry
    __device__ __forceinline__ sdk_v4u top(uint32_t level) const
    {
        return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff(level), 96, 0);
    }
    // the whole line in one round trip: the entry (last quad) decides whether
    // the level still has a digit; if not (rare), the planes go unused
    __device__ __forceinline__ uint32_t pop(uint32_t level, plane::Board &B, uint32_t (&und)[3]) const
    {
        return pop_line(level, B, und)[3];
    }
    __device__ __forceinline__ sdk_v4u pop_line(uint32_t level, plane::Board &B, uint32_t (&und)[3]) const
    {
        const int v = (int)voff(level);
        const sdk_v4u q0 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 0, 0);
        const sdk_v4u q1 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 16, 0);
        const sdk_v4u q2 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 32, 0);
        const sdk_v4u q3 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 48, 0);
        const sdk_v4u q4 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 64, 0);
        const sdk_v4u q5 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 80, 0);
        const sdk_v4u t = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 96, 0);
        const sdk_v4u u = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 112, 0);
        und[0] = u.x; und[1] = u.y; und[2] = u.z;
        unpack(B, q0, q1, q2, q3, q4, q5, t);
        // all eight loads issued before the caller's branch on the entry
        plane::pin_board(B);
        return t;
    }
    __device__ __forceinline__ void restore(uint32_t level, plane::Board &B, const sdk_v4u &t) const
    {
        const int v = (int)voff(level);
        const sdk_v4u q0 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 0, 0);
        const sdk_v4u q1 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 16, 0);
        const sdk_v4u q2 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 32, 0);
        const sdk_v4u q3 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 48, 0);
        const sdk_v4u q4 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 64, 0);
        const sdk_v4u q5 = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v, 80, 0);
        unpack(B, q0, q1, q2, q3, q4, q5, t);
    }
    __device__ __forceinline__ void put_entry(uint32_t level, uint32_t entry) const
    {
        __builtin_amdgcn_raw_buffer_store_b32(entry, rsrc, (int)voff(level), 108, 0);
    }
};

#endif  // SDK_PLANE_STACK_H
