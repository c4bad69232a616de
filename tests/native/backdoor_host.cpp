// Host build of sudoku_solver_distributed_amd/csrc/backdoor.h (the smallest
// backdoors of a puzzle: validation, the level closure, the ranking of the
// subsets and the trials, as backdoor_kernels.hip runs them) for the CPU
// test-suite (tests/test_backdoor_host.py), checked against the fixture
// tests/golden/backdoor_cases.json, which rate_host.cpp alone produced.  Not a
// product path.
//
// With -DBACKDOOR_HOST_MAIN the file is a stand-alone program (the sanitizer
// build: g++ -fsanitize=address,undefined -DBACKDOOR_HOST_MAIN): its standard
// input holds lines "board grid level max_size", 81 digits each.
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"
#include "../../sudoku_solver_distributed_amd/csrc/backdoor.h"

// size[i], count[i] (may be NULL), first[4 i ..] (may be NULL), cover[81 i ..]
// (may be NULL) of (boards[i], grids[i]), as sdk_backdoor_batch documents
// them.  Items are independent: an OpenMP build spreads them over the threads.
extern "C" void backdoor_host_batch(const uint8_t *boards, const uint8_t *grids, int32_t *size, int32_t *count,
                                    uint8_t *first, uint8_t *cover, int64_t n, int level, int max_size)
{
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t i = 0; i < n; ++i) {
        uint32_t xb[21], xg[21];
        host::words_of(boards + i * 81, xb);
        host::words_of(grids + i * 81, xg);
        backdoor::Answer A;
        backdoor::host_board(xb, xg, grids + i * 81, level, max_size, A);
        size[i] = A.size;
        if (count) count[i] = A.count;
        if (first) memcpy(first + 4 * i, A.first, 4);
        if (cover) memcpy(cover + 81 * i, A.cover, 81);
    }
}

extern "C" uint32_t backdoor_host_choose(uint32_t n, int j) { return backdoor::choose(n, j); }

// the j-subset of 0..n-1 with lexicographic rank r, 0xFF in the unused places
extern "C" void backdoor_host_unrank(uint32_t n, int j, uint32_t r, uint8_t *out)
{
    uint32_t idx[backdoor::MAX_SIZE];
    backdoor::unrank_k(j, r, n, idx);
    for (int k = 0; k < backdoor::MAX_SIZE; ++k) out[k] = (uint8_t)idx[k];
}

#ifdef BACKDOOR_HOST_MAIN
#include <stdio.h>
int main()
{
    char line[512];
    int64_t items = 0;
    while (fgets(line, sizeof line, stdin)) {
        uint8_t v[162];
        int k = 0;
        const char *p = line;
        for (; *p && k < 162; ++p)
            if (*p >= '0' && *p <= '9') v[k++] = (uint8_t)(*p - '0');
        int level = 0, max_size = 0;
        if (k != 162 || sscanf(p, "%d %d", &level, &max_size) != 2) continue;
        int32_t size, count;
        uint8_t first[4], cover[81];
        backdoor_host_batch(v, v + 81, &size, &count, first, cover, 1, level, max_size);
        int covered = 0;
        for (int c = 0; c < 81; ++c) covered += cover[c];
        printf("%d %d %d,%d,%d,%d %d\n", size, count, first[0], first[1], first[2], first[3], covered);
        ++items;
    }
    return items ? 0 : 1;
}
#endif
