// Host build of sudoku_solver_distributed_amd/csrc/rate.h (the puzzle
// rating: the level closures rate_kernel's lanes run and the trial level) for
// the CPU test-suite (tests/test_rate_host.py), checked against the definition
// in tests/rate_cases.py.  Not a product path.
//
// With -DRATE_HOST_MAIN the file is a stand-alone program (the sanitizer build:
// g++ -fsanitize=address,undefined -DRATE_HOST_MAIN): it rates the 81-digit
// boards on its standard input, one per line, at every max_level.
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"
#include "../../sudoku_solver_distributed_amd/csrc/rate.h"

// rating[i], open[4 i ..] (may be NULL), marks[81 i ..] (may be NULL) of board
// i at max_level 1..4, as sdk_rate_batch documents them.  Boards are
// independent: an OpenMP build spreads them over the threads.
extern "C" void rate_host_batch(const uint8_t *in, int32_t *rating, int32_t *open, uint16_t *marks, int64_t n,
                                int max_level)
{
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t i = 0; i < n; ++i) {
        uint32_t x[21];
        host::words_of(in + i * 81, x);
        plane::Board B;
        rate::Result R;
        const bool ok = rate::load(B, x);
        if (ok) rate::rate_board(B, max_level, R);
        else rate::invalid(R);
        rating[i] = R.rating;
        if (open)
            for (int k = 0; k < 4; ++k) open[4 * i + k] = R.open[k];
        if (marks)
            rate::store_marks(B, ok && R.rating != 0 ? 0x1FFu : 0u,
                              [&](int cell, uint32_t m) { marks[81 * i + cell] = (uint16_t)m; });
    }
}

#ifdef RATE_HOST_MAIN
#include <stdio.h>
int main()
{
    char line[256];
    int64_t boards = 0;
    while (fgets(line, sizeof line, stdin)) {
        uint8_t b[81];
        int k = 0;
        for (const char *p = line; *p && k < 81; ++p)
            if (*p >= '0' && *p <= '9') b[k++] = (uint8_t)(*p - '0');
            else if (*p == '.') b[k++] = 0;
        if (k != 81) continue;
        for (int m = 1; m <= 4; ++m) {
            int32_t rating, open[4];
            uint16_t marks[81];
            rate_host_batch(b, &rating, open, marks, 1, m);
            printf("%d:%d[%d %d %d %d] ", m, rating, open[0], open[1], open[2], open[3]);
        }
        printf("\n");
        ++boards;
    }
    return boards ? 0 : 1;
}
#endif
