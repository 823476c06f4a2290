// The constrained decoder's scratch layout (vitx_layout, gretel_amd/csrc/scratch_layout.hpp: the function the library itself calls)
// against its sizes and order written out by hand, and against the exact decoder's first reservation, which shares the block: the
// vit_out must lie at offset 0 under both.  Per constraint set the back-pointer block must start on a four-byte boundary (the trace
// copies whole words) and no set's last word may reach into the next set's block -- with state counts such as 3 and 9 and an odd
// N + 1 that is what the stride is rounded up for.  Host only; built with -fsanitize=address,undefined by tests/test_masked_host.py.
#include "scratch_layout.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
            failures++;                                   \
        }                                                 \
    } while (0)

static size_t up(size_t x) { return (x + 255) & ~(size_t)255; }

static void check_masked(int N, int L, int ns, int sets)
{
    char what[80];
    snprintf(what, sizeof what, "masked N=%d L=%d states=%d sets=%d", N, L, ns, sets);
    const size_t n1 = (size_t)N + 1, m = (size_t)sets;
    const size_t table_doubles = (size_t)N * (30 * L + 6);
    const size_t row = n1 * ns, bps = (row + 3) / 4 * 4;
    // in order: vit_out, the table ONCE, the sets' back-pointer blocks, their end scores, their end flags, their vit_outs, their
    // path rows, their compacted masks
    const size_t bytes[8] = {24, table_doubles * 8, m * bps, m * ns * 8, m * ns, m * 24, m * n1, m * n1};
    size_t off[9] = {0};
    for (int q = 0; q < 8; q++) off[q + 1] = off[q] + up(bytes[q]);
    const size_t need = off[8];
    CHECK(ns <= GH_VITERBI_MAX_STATES && sets <= GH_MASKED_MAX_SETS, "%s: not a shape the decoder serves", what);
    const vitx_bufs z = vitx_layout(nullptr, N, table_doubles, ns, sets);
    CHECK(z.total == need, "%s: sizing pass %zu, by hand %zu", what, z.total, need);
    CHECK(!z.out && !z.Gb && !z.bp && !z.vend && !z.okend && !z.outs && !z.paths && !z.a5, "%s: the sizing pass hands out parts", what);
    std::vector<char> block(need);
    const vit_bufs first = vit_layout(block.data(), N, 0, 0);     // what vit_open reserves before U is known
    const vitx_bufs b = vitx_layout(block.data(), N, table_doubles, ns, sets);
    CHECK((const char *)first.out == block.data() && (const char *)b.out == block.data(), "%s: vit_out is not at offset 0", what);
    CHECK(b.total == need && b.bps == bps, "%s: total %zu (by hand %zu), stride %zu (by hand %zu)", what, b.total, need, b.bps, bps);
    const void *parts[8] = {b.out, b.Gb, b.bp, b.vend, b.okend, b.outs, b.paths, b.a5};
    for (int q = 0; q < 8; q++) {
        const size_t at = (size_t)((const char *)parts[q] - block.data());
        CHECK(at == off[q], "%s: part %d at %zu, by hand %zu", what, q, at, off[q]);
        CHECK(at % 256 == 0 && at + bytes[q] <= off[q + 1], "%s: part %d (%zu + %zu) is misaligned or runs into what follows", what, q, at, bytes[q]);
        memset(block.data() + at, q, bytes[q]);                   // every byte its user touches lies inside the block
    }
    // per set: the block word-aligned, the last back-pointer the walk stores inside it, the last whole word the trace copies inside
    // it too, and so disjoint from the next set's
    for (int s = 0; s < sets; s++) {
        const size_t at = (size_t)((const char *)b.bp - block.data()) + (size_t)s * b.bps;
        CHECK(at % 4 == 0, "%s: set %d's back-pointers begin mid-word (%zu)", what, s, at);
        CHECK((size_t)N * ns + ns - 1 < b.bps, "%s: set %d's last back-pointer lies outside its block", what, s);
        CHECK((row + 3) / 4 * 4 <= b.bps, "%s: set %d's last whole word reaches into the next block", what, s);
        CHECK(at + b.bps <= off[3], "%s: set %d's block runs into the end rows", what, s);
    }
}

int main()
{
    CHECK(sizeof(vit_out) == 24, "vit_out is %zu bytes", sizeof(vit_out));
    for (int N : {1, 2, 8, 60, 700}) {                            // N + 1 odd and even
        for (int sets : {1, 2, 5, 256}) {
            check_masked(N, 1, 3, sets);
            check_masked(N, 2, 9, sets);
            check_masked(N, 3, 64, sets);
            check_masked(N, 4, 1, sets);                          // one state
            check_masked(N, 3, 27, sets);
        }
        for (int sets : {1, 3}) {
            check_masked(N, 6, 4096, sets);                       // the cap
            check_masked(N, 5, 3125, sets);
        }
    }
    check_masked(8, 6, 4096, 256);
    if (failures) {
        printf("vitx_layout: %d check(s) failed\n", failures);
        return 1;
    }
    printf("vitx_layout done\n");
    return 0;
}
