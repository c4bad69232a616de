// flush_count.hip -- plane_flush_outbox alone (csrc/plane_kernel.h), for a
// static instruction count of the store path (scripts/isa_flush_count.py
// compiles it to assembly with SDK_PLANE_ROOTFULL=0 and =1; it is never run).
// Diagnostic, not product code.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../sudoku_solver_distributed_amd/csrc/common.h"
#include "../../sudoku_solver_distributed_amd/csrc/plane_kernel.h"

__global__ __launch_bounds__(64) void flush_only(const uint32_t *records, uint32_t count, const uint8_t *in, uint8_t *out,
                                                 int32_t *status, int64_t n, unsigned long long *ws, int64_t *defer_list,
                                                 uint32_t *counts)
{
    __shared__ __attribute__((aligned(16))) uint32_t outbox[PLANE_OUTBOX * PLANE_OB_WORDS];
    const int lane = threadIdx.x;
    for (int w = 0; w < PLANE_OB_WORDS; ++w) outbox[PLANE_OB_WORDS * lane + w] = records[PLANE_OB_WORDS * lane + w];
    __syncthreads();
    const PlaneIO1 io = {in, out, status, n};
    uint32_t solved = 0, fin = 0, deferred = 0;
    plane_flush_outbox(outbox, count, lane, io, ws, defer_list, solved, fin, deferred);
    counts[lane] = solved + fin + deferred;
}
