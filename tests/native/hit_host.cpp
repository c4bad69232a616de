// Host build of sudoku_solver_distributed_amd/csrc/hit.h (the k-cell hitting
// sets of a family of cell sets: validation and the search task by task, as
// hit_kernels.hip runs them) for the CPU test-suite (tests/test_hit_host.py),
// checked against the fixture tests/golden/hit_cases.json, which hit.h had no
// part in.  Not a product path.  -DSDK_HIT_PRUNE=0 builds it without the
// packing prune.
//
// With -DHIT_HOST_MAIN the file is a stand-alone program (the sanitizer build:
// g++ -fsanitize=address,undefined -DHIT_HOST_MAIN): its standard input holds
// one family a line, "k limit A R set set ...", every mask as hex digits.
#include <string.h>

#include <vector>

#include "../../sudoku_solver_distributed_amd/csrc/hit.h"

// sdk_hitting_sets_batch on the host: rows[4 j ..] = {m0, m1, m2, owner} for
// j < min(total, capacity), count[i], status[i], info = {total, listed},
// nodes[i] (may be NULL) the nodes of family i's walk.  mode bit 0: the fine
// task cut; bit 1: count only (leaves add their binomials; capacity must be 0
// and limit 0).  Families are independent: an OpenMP build spreads them over
// the threads (the row order then varies).
extern "C" int hit_host_batch(const uint32_t *sets, const int64_t *offsets, const uint32_t *allowed,
                              const uint32_t *required, int64_t n, int k, int64_t limit, uint32_t *rows,
                              int64_t capacity, int64_t *count, int32_t *status, int64_t *info, uint64_t *nodes, int mode)
{
    if (n < 0 || k < 0 || k > hit::MAX_CLUES || limit < 0 || capacity < 0) return -2;
    if ((mode & 2) && (capacity != 0 || limit != 0)) return -2;
    int64_t total = 0;
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t *A = allowed + 4 * i, *R = required + 4 * i;
        const int64_t len = offsets[i + 1] - offsets[i];
        status[i] = len < 0 || len > (int64_t)0x7FFFFFFF ? (int)hit::INVALID : hit::validate(A, R);
        count[i] = 0;
        if (nodes) nodes[i] = 0;
        if (status[i] != hit::DONE) continue;
        std::vector<uint32_t> mine;
        int64_t found = 0;
        const uint64_t walked = hit::host_family(sets + 4 * offsets[i], len, A, R, k, (mode & 1) != 0, (mode & 2) != 0, limit,
                                                 [&](const uint32_t *C, uint64_t add) {
                                                     found += (int64_t)add;
                                                     if (!(mode & 2)) mine.insert(mine.end(), {C[0], C[1], C[2], (uint32_t)i});
                                                 });
        if (nodes) nodes[i] = walked;
        count[i] = found;
        if (limit > 0 && found >= limit) status[i] = hit::LIMITED;
#pragma omp critical
        {
            if (mode & 2) total += found;
            for (size_t j = 0; j < mine.size(); j += 4, ++total)
                if (total < capacity) memcpy(rows + 4 * total, &mine[j], 16);
        }
    }
    info[0] = total;
    info[1] = total < capacity ? total : capacity;
    return 0;
}

#ifdef HIT_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>
// an 81-bit mask of up to 24 hex digits, most significant first, into three words and a zero
static void parse_mask(const char *s, uint32_t *out)
{
    out[0] = out[1] = out[2] = out[3] = 0u;
    for (; *s; ++s) {
        const uint32_t v = *s >= 'a' ? (uint32_t)(*s - 'a' + 10) : (uint32_t)(*s - '0');
        out[2] = out[2] << 4 | out[1] >> 28;
        out[1] = out[1] << 4 | out[0] >> 28;
        out[0] = out[0] << 4 | v;
    }
}

int main()
{
    static char line[1 << 20];
    int64_t items = 0;
    while (fgets(line, sizeof line, stdin)) {
        std::vector<uint32_t> words;
        int k = -1;
        long long limit = -1;
        int field = 0;
        for (char *tok = strtok(line, " \n"); tok; tok = strtok(NULL, " \n"), ++field) {
            if (field == 0) k = atoi(tok);
            else if (field == 1) limit = atoll(tok);
            else {
                uint32_t m[4];
                parse_mask(tok, m);
                words.insert(words.end(), m, m + 4);
            }
        }
        if (field < 4) continue;
        const int64_t nsets = (int64_t)words.size() / 4 - 2;
        const int64_t off[2] = {0, nsets};
        int64_t count, info[2];
        int32_t status;
        uint64_t nodes;
        std::vector<uint32_t> rows(4 * 4096);
        for (int mode = 0; mode < 2; ++mode) {
            if (hit_host_batch(words.data() + 8, off, words.data(), words.data() + 4, 1, k, limit, rows.data(), 4096, &count,
                               &status, info, &nodes, mode))
                return 2;
            printf("%d %lld %lld %lld%s", status, (long long)count, (long long)info[0], (long long)info[1], mode ? "\n" : " ");
        }
        ++items;
    }
    return items ? 0 : 1;
}
#endif
