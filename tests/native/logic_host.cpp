// Host build of sudoku_solver_distributed_amd/csrc/logic.h (the named
// techniques: the ladder's closures as logic_kernel's lanes and
// logic_wave_kernel's waves compute them) for the CPU test-suite
// (tests/test_logic_host.py), checked against the definition in
// tests/logic_cases.py.  Not a product path.
//
// With -DLOGIC_HOST_MAIN the file is a stand-alone program (the sanitizer
// build: g++ -fsanitize=address,undefined -DLOGIC_HOST_MAIN): it runs the
// states on its standard input, one per line, at the default ladder: an
// 81-digit board, or "s" and 243 hex digits (three per cell: pencil marks on
// the empty board).
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"
#include "../../sudoku_solver_distributed_amd/csrc/logic.h"

// step[i], open[8 i ..], left[8 i ..], marks[81 i ..] (each of the three may be
// NULL) of board i (in NULL: empty boards) with pencil marks start[81 i ..]
// (NULL: all nine digits) under the ladder, as sdk_logic_batch documents them.
// Returns -2 for a bad ladder or both inputs NULL.  Boards are independent: an
// OpenMP build spreads them over the threads.
extern "C" int logic_host_batch(const uint8_t *in, const uint16_t *start, const uint32_t *ladder, int steps, int32_t *step,
                                int32_t *open, int32_t *left, uint16_t *marks, int64_t n)
{
    if (!logic::ladder_ok(ladder, steps) || (!in && !start)) return -2;
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t i = 0; i < n; ++i) {
        plane::Board B;
        logic::Result R;
        bool ok = true;
        if (in) {
            uint32_t x[21];
            host::words_of(in + i * 81, x);
            ok = rate::load(B, x);
        } else {
            logic::empty_board(B);
        }
        if (start) ok = logic::and_marks(B, [&](int cell) { return (uint32_t)start[81 * i + cell]; }) && ok;
        if (ok) logic::run_board(B, ladder, steps, R);
        else logic::invalid(R);
        step[i] = R.step;
        for (int k = 0; k < 8; ++k) {
            if (open) open[8 * i + k] = R.open[k];
            if (left) left[8 * i + k] = R.left[k];
        }
        if (marks)
            rate::store_marks(B, ok && R.step != 0 ? 0x1FFu : 0u,
                              [&](int cell, uint32_t m) { marks[81 * i + cell] = (uint16_t)m; });
    }
    return 0;
}

#ifdef LOGIC_HOST_MAIN
#include <stdio.h>
static int hex(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }
int main()
{
    static const uint32_t ladder[7] = {1, 3, 7, 15, 63, 127, 511};
    char line[512];
    int64_t states = 0;
    while (fgets(line, sizeof line, stdin)) {
        uint8_t b[81];
        uint16_t s[81];
        bool marks = line[0] == 's';
        int k = 0;
        if (marks) {
            int v = 0, digits = 0;
            for (const char *p = line + 1; *p && k < 81; ++p) {
                if (hex(*p) < 0) continue;
                v = 16 * v + hex(*p);
                if (++digits == 3) s[k++] = (uint16_t)v, v = 0, digits = 0;
            }
        } else {
            for (const char *p = line; *p && k < 81; ++p)
                if (*p >= '0' && *p <= '9') b[k++] = (uint8_t)(*p - '0');
                else if (*p == '.') b[k++] = 0;
        }
        if (k != 81) continue;
        int32_t step, open[8], left[8];
        uint16_t out[81];
        if (logic_host_batch(marks ? nullptr : b, marks ? s : nullptr, ladder, 7, &step, open, left, out, 1)) return 2;
        printf("%d", step);
        for (int j = 0; j < 8; ++j) printf(" %d/%d", open[j], left[j]);
        printf("\n");
        ++states;
    }
    return states ? 0 : 1;
}
#endif
