// Host build of sudoku_solver_distributed_amd/csrc/path.h (the solving path:
// the schedule path_wave_kernel's waves run, one board at a time) for the CPU
// test-suite (tests/test_path_host.py), checked against the definition in
// tests/path_cases.py.  Not a product path.
//
// With -DPATH_HOST_MAIN the file is a stand-alone program (the sanitizer
// build: g++ -fsanitize=address,undefined -DPATH_HOST_MAIN): it runs the
// states on its standard input, one per line, under the rule mask and
// max_rounds of its two arguments: an 81-digit board, or "s" and 243 hex
// digits (three per cell: pencil marks on the empty board).
#include "../../sudoku_solver_distributed_amd/csrc/host_model.h"
#include "../../sudoku_solver_distributed_amd/csrc/path.h"

static bool path_host_load(plane::Board &B, const uint8_t *in, const uint16_t *start, int64_t i)
{
    bool ok = true;
    if (in) {
        uint32_t x[21];
        host::words_of(in + i * 81, x);
        ok = rate::load(B, x);
    } else {
        logic::empty_board(B);
    }
    if (start) ok = logic::and_marks(B, [&](int cell) { return (uint32_t)start[81 * i + cell]; }) && ok;
    return ok;
}

// sdk_path_batch on host memory: rows (capacity * 4 words, NULL ok iff
// capacity == 0), count, rounds, status (n each), hist (n * 9, NULL ok), marks
// (n * 81, NULL ok), info {total, listed}.  Returns -2 for a bad mask, both
// inputs NULL or a NULL row list with a capacity.  Boards are independent: an
// OpenMP build spreads them over the threads.
extern "C" int path_host_batch(const uint8_t *in, const uint16_t *start, uint32_t rules, int max_rounds, int64_t n,
                               uint32_t *rows, int64_t capacity, int32_t *count, int32_t *rounds, int32_t *status,
                               int32_t *hist, uint16_t *marks, int64_t *info)
{
    if ((rules & ~(uint32_t)logic::ALL) || !(rules & logic::N) || max_rounds < 0 || (!in && !start) || capacity < 0 ||
        (capacity > 0 && !rows))
        return -2;
    int64_t cursor = 0;
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t i = 0; i < n; ++i) {
        plane::Board B;
        path::Out O;
        O.count = O.rounds = 0;
        O.status = path::INVALID;
        for (int c = 0; c < path::CLASSES; ++c) O.hist[c] = 0;
        uint32_t W[27];
        if (path_host_load(B, in, start, i)) {
            logic::words_of(B, W);
            path::run_board(W, rules, max_rounds, O, [&](uint32_t w1, uint32_t w2, uint32_t w3) {
                int64_t at;
#pragma omp atomic capture
                at = cursor++;
                if (at < capacity) {
                    uint32_t *r = rows + 4 * at;
                    r[0] = (uint32_t)i, r[1] = w1, r[2] = w2, r[3] = w3;
                }
            });
        }
        count[i] = O.count;
        rounds[i] = O.rounds;
        status[i] = O.status;
        if (hist)
            for (int c = 0; c < path::CLASSES; ++c) hist[9 * i + c] = O.hist[c];
        if (marks) {
            const bool keep = O.status != path::INVALID && O.status != path::DEAD;
            for (int w = 0; w < 27; ++w) B.P[w / 3][w % 3] = keep ? W[w] : 0u;
            rate::store_marks(B, 0x1FFu, [&](int cell, uint32_t m) { marks[81 * i + cell] = (uint16_t)m; });
        }
    }
    if (info) info[0] = cursor, info[1] = cursor < capacity ? cursor : capacity;
    return 0;
}

// Rule L alone on every state: marks_l[81 i ..] = the state minus the union of
// the removals of its L firings, marks_p[81 i ..] = the state after
// logic::pass_l.  Returns how many firings there were in all.
extern "C" int64_t path_host_rule_l(const uint8_t *in, const uint16_t *start, int64_t n, uint16_t *marks_l, uint16_t *marks_p)
{
    int64_t firings = 0;
    for (int64_t i = 0; i < n; ++i) {
        plane::Board B;
        path_host_load(B, in, start, i);
        uint32_t W[27];
        logic::words_of(B, W);
        plane::Board A = B;
        for (int q = 0; q < path::L_PAIRS; ++q)
            path::l_pair(W, q / 9, q % 9, [&](int, int, int t, int idx, uint32_t mask) {
                ++firings;
                path::unit_cells(t, idx, mask, [&](int band, int pos) { A.P[q / 9][band] &= ~(1u << pos); });
            });
        logic::pass_l(B);
        rate::store_marks(A, 0x1FFu, [&](int cell, uint32_t m) { marks_l[81 * i + cell] = (uint16_t)m; });
        rate::store_marks(B, 0x1FFu, [&](int cell, uint32_t m) { marks_p[81 * i + cell] = (uint16_t)m; });
    }
    return firings;
}

#ifdef PATH_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <vector>
static int hex(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }
int main(int argc, char **argv)
{
    const uint32_t rules = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 0) : 0x1FFu;
    const int max_rounds = argc > 2 ? atoi(argv[2]) : 0;
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
        int32_t count, rounds, status, hist[9];
        int64_t info[2];
        uint16_t out[81];
        // a counting call, then the list at its exact size
        if (path_host_batch(marks ? nullptr : b, marks ? s : nullptr, rules, max_rounds, 1, nullptr, 0, &count, &rounds, &status,
                            hist, out, info))
            return 2;
        std::vector<uint32_t> rows(4 * (size_t)info[0] + 4, 0xA5A5A5A5u);
        if (path_host_batch(marks ? nullptr : b, marks ? s : nullptr, rules, max_rounds, 1, rows.data(), info[0], &count, &rounds,
                            &status, hist, out, info))
            return 2;
        if (rows[4 * (size_t)info[0]] != 0xA5A5A5A5u) return 3;
        printf("%d %d %d", status, rounds, count);
        for (int64_t r = 0; r < info[1]; ++r) printf(" %x:%x:%x", rows[4 * r + 1], rows[4 * r + 2], rows[4 * r + 3]);
        printf("\n");
        ++states;
    }
    return states ? 0 : 1;
}
#endif
