// Host build of sudoku_solver_distributed_amd/csrc/ua.h (the unavoidable sets
// of a solution grid: validation, the repair search task by task, and the
// minimal filter by its definition, as ua_kernels.hip runs them) for the CPU
// test-suite (tests/test_ua_host.py), checked against the fixture
// tests/golden/ua_cases.json, which ua.h had no part in.  Not a product path.
//
// With -DUA_HOST_MAIN the file is a stand-alone program (the sanitizer build:
// g++ -fsanitize=address,undefined -DUA_HOST_MAIN): its standard input holds
// lines "grid max_size", the grid as 81 hex digits.
#include <string.h>

#include <vector>

#include "../../sudoku_solver_distributed_amd/csrc/ua.h"

// sdk_unavoidable_batch on the host: rows[4 k ..] = {m0, m1, m2, owner} for
// k < min(total, capacity), count[i], status[i], info = {total, listed},
// nodes[i] (may be NULL) the nodes of grid i's walk.  Grids are independent:
// an OpenMP build spreads them over the threads (the row order then varies).
// split != 0: every task as its eight split tasks, as the kernel runs a small batch.
extern "C" int ua_host_batch_split(const uint8_t *grids, int64_t n, int max_size, uint32_t *rows, int64_t capacity,
                                   int32_t *count, int32_t *status, int64_t *info, uint64_t *nodes, int split)
{
    if (n < 0 || max_size < ua::MIN_SIZE || max_size > ua::MAX_SIZE || capacity < 0) return -2;
    int64_t total = 0;
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t *g = grids + i * 81;
        status[i] = ua::validate([&](int c) { return (uint32_t)g[c]; });
        count[i] = 0;
        if (nodes) nodes[i] = 0;
        if (status[i] != ua::DONE) continue;
        std::vector<uint32_t> mine;
        const uint64_t walked = ua::host_grid(g, max_size, [&](const uint32_t *D) {
            mine.insert(mine.end(), {D[0], D[1], D[2], (uint32_t)i});
        }, split != 0);
        if (nodes) nodes[i] = walked;
        count[i] = (int32_t)(mine.size() / 4);
#pragma omp critical
        {
            for (size_t k = 0; k < mine.size(); k += 4, ++total)
                if (total < capacity) memcpy(rows + 4 * total, &mine[k], 16);
        }
    }
    info[0] = total;
    info[1] = total < capacity ? total : capacity;
    return 0;
}

extern "C" int ua_host_batch(const uint8_t *grids, int64_t n, int max_size, uint32_t *rows, int64_t capacity,
                             int32_t *count, int32_t *status, int64_t *info, uint64_t *nodes)
{
    return ua_host_batch_split(grids, n, max_size, rows, capacity, count, status, info, nodes, 0);
}

// sdk_unavoidable_minimal_batch on the host, by the definition
extern "C" void ua_host_minimal(const uint32_t *rows, const int64_t *offsets, int64_t groups, uint8_t *keep)
{
    for (int64_t g = 0; g < groups; ++g) {
        for (int64_t k = offsets[g]; k < offsets[g + 1]; ++k) {
            bool ok = true;
            for (int64_t j = offsets[g]; j < offsets[g + 1] && ok; ++j) {
                const bool same = ua::same_cells(rows + 4 * j, rows + 4 * k);
                if (same ? j < k : ua::subset_of(rows + 4 * j, rows + 4 * k)) ok = false;
            }
            keep[k] = ok;
        }
    }
}

#ifdef UA_HOST_MAIN
#include <stdio.h>
int main()
{
    char line[256];
    int64_t items = 0;
    while (fgets(line, sizeof line, stdin)) {
        uint8_t g[81];
        int k = 0;
        const char *p = line;
        for (; *p && k < 81; ++p) {
            if (*p >= '0' && *p <= '9') g[k++] = (uint8_t)(*p - '0');
            else if (*p >= 'a' && *p <= 'f') g[k++] = (uint8_t)(*p - 'a' + 10);
        }
        int max_size = 0;
        if (k != 81 || sscanf(p, "%d", &max_size) != 1) continue;
        int32_t count, status;
        int64_t info[2];
        uint64_t nodes;
        std::vector<uint32_t> rows(4 * 4096);
        if (ua_host_batch(g, 1, max_size, rows.data(), 4096, &count, &status, info, &nodes)) return 2;
        std::vector<int64_t> off = {0, info[1]};
        std::vector<uint8_t> keep(info[1] ? info[1] : 1);
        ua_host_minimal(rows.data(), off.data(), 1, keep.data());
        int64_t kept = 0;
        for (int64_t r = 0; r < info[1]; ++r) kept += keep[r];
        printf("%d %d %lld %lld\n", status, count, (long long)info[0], (long long)kept);
        ++items;
    }
    return items ? 0 : 1;
}
#endif
