// The k-best decoder's scratch layout (vitk_layout, gretel_amd/csrc/scratch_layout.hpp: the function the library itself calls)
// against its sizes and order written out by hand, and against the exact decoder's first reservation, which shares the block: the
// vit_out must lie at offset 0 under both.  Host only; built with -fsanitize=address,undefined by tests/test_kbest_host.py.
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

static void check_kbest(int N, int L, int ns, int k)
{
    char what[80];
    snprintf(what, sizeof what, "kbest N=%d L=%d states=%d k=%d", N, L, ns, k);
    const size_t n1 = (size_t)N + 1, slots = (size_t)ns * k;
    const size_t table_doubles = (size_t)N * (30 * L + 6);
    // in order: vit_out, the table, a back-pointer byte per position and slot (and a word), the end scores, the end counts, k
    // path rows, k scores, the n_out word
    const size_t bytes[8] = {24, table_doubles * 8, n1 * slots + 4, slots * 8, (size_t)ns, (size_t)k * n1, (size_t)k * 8, 4};
    size_t off[9] = {0};
    for (int q = 0; q < 8; q++) off[q + 1] = off[q] + up(bytes[q]);
    const size_t need = off[8];
    CHECK(slots <= GH_VITERBI_MAX_STATES && k <= GH_KBEST_MAX, "%s: not a shape the decoder serves", what);
    const vitk_bufs z = vitk_layout(nullptr, N, table_doubles, ns, k);
    CHECK(z.total == need, "%s: sizing pass %zu, by hand %zu", what, z.total, need);
    CHECK(!z.out && !z.Gb && !z.bp && !z.vend && !z.cend && !z.paths && !z.ll && !z.n_out, "%s: the sizing pass hands out parts", what);
    std::vector<char> block(need);
    const vit_bufs first = vit_layout(block.data(), N, 0, 0);     // what vit_open reserves before U is known
    const vitk_bufs b = vitk_layout(block.data(), N, table_doubles, ns, k);
    CHECK((const char *)first.out == block.data() && (const char *)b.out == block.data(), "%s: vit_out is not at offset 0", what);
    CHECK(b.total == need, "%s: total %zu, by hand %zu", what, b.total, need);
    const void *parts[8] = {b.out, b.Gb, b.bp, b.vend, b.cend, b.paths, b.ll, b.n_out};
    for (int q = 0; q < 8; q++) {
        const size_t at = (size_t)((const char *)parts[q] - block.data());
        CHECK(at == off[q], "%s: part %d at %zu, by hand %zu", what, q, at, off[q]);
        CHECK(at % 256 == 0 && at + bytes[q] <= off[q + 1], "%s: part %d (%zu + %zu) is misaligned or runs into what follows", what, q, at, bytes[q]);
        memset(block.data() + at, q, bytes[q]);                   // every byte its user touches lies inside the block
    }
    // the last back-pointer the walk stores and the last word the trace copies
    CHECK(((size_t)N * ns + ns - 1) * k + k - 1 < n1 * slots, "%s: the last back-pointer lies outside its part", what);
    CHECK(((n1 * slots + 3) / 4) * 4 <= bytes[2], "%s: the trace's last whole word lies outside the part", what);
}

int main()
{
    CHECK(sizeof(vit_out) == 24, "vit_out is %zu bytes", sizeof(vit_out));
    for (int N : {1, 60, 700}) {
        check_kbest(N, 1, 5, 32);
        check_kbest(N, 3, 125, 32);      // 4000 slots
        check_kbest(N, 5, 1024, 4);      // the cap
        check_kbest(N, 5, 3125, 1);
        check_kbest(N, 12, 4096, 1);
        check_kbest(N, 4, 1, 7);         // one state, an odd k
        check_kbest(N, 3, 27, 3);        // 81 slots: no multiple of four
    }
    if (failures) {
        printf("vitk_layout: %d check(s) failed\n", failures);
        return 1;
    }
    printf("vitk_layout done\n");
    return 0;
}
