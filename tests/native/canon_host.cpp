// Host build of sudoku_solver_distributed_amd/csrc/canon.h (the canonical
// form's search: search_block, merge, pack / unpack, reduce -- what
// canon_kernel's lanes and canon_reduce_kernel run) for the CPU test-suite
// (tests/test_canon_host.py).  Not a product path.
#include <stddef.h>
#include <stdint.h>

#include "../../sudoku_solver_distributed_amd/csrc/canon.h"

// the packed 64-byte record of row variants [lo, hi) of one board, as a
// workgroup of canon_kernel leaves it in the scratch
extern "C" void canon_host_slice(const uint8_t *g, int lo, int hi, uint32_t *words)
{
    canon::Record r;
    const bool ok = canon::canon_board(g, lo, hi, r);
    uint32_t w[canon::RECORD_WORDS];
    canon::pack(r, w);
    if (!ok) w[13] = 1u;
    for (int k = 0; k < canon::RECORD_WORDS; ++k) words[k] = w[k];
}

// canon_reduce_kernel's lane: S records -> canon, sym, autos
extern "C" void canon_host_reduce(const uint8_t *g, const uint32_t *words, int S, uint8_t *out, int32_t *sym,
                                  int32_t *autos)
{
    canon::Record r;
    if (!canon::reduce(words, S, r)) {
        for (int i = 0; i < 81; ++i) out[i] = g[i];
        *sym = *autos = -1;
        return;
    }
    canon::store_cells(r, [&](int cell, uint32_t v) { out[cell] = (uint8_t)v; });
    *sym = (int32_t)r.sym;
    *autos = (int32_t)r.ties;
}

// n boards, each cut into S slices and reduced
extern "C" void canon_host_batch(const uint8_t *in, uint8_t *out, int32_t *sym, int32_t *autos, int64_t n, int S)
{
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t i = 0; i < n; ++i) {
        uint32_t *w = new uint32_t[(size_t)S * canon::RECORD_WORDS];
        for (int s = 0; s < S; ++s)
            canon_host_slice(in + 81 * i, canon::slice_lo(s, S), canon::slice_lo(s + 1, S), w + s * canon::RECORD_WORDS);
        canon_host_reduce(in + 81 * i, w, S, out + 81 * i, sym + i, autos + i);
        delete[] w;
    }
}
