// The max-marginals' layout of the exact decoder's block (vitm_layout, gretel_amd/csrc/scratch_layout.hpp: the function the library
// itself calls) against its size and order written out by hand: the vit_out, the table, one stored row of `states` doubles per
// position, the candidate bytes over the compact indices, mm, the candidate bytes over the symbols.  Host only; built with
// -fsanitize=address,undefined by tests/test_maxmarg_host.py.
#include "scratch_layout.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static_assert(sizeof(vit_out) == 24, "U, hole_at, end_state, pad, ll");

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

static void check(int N, int L, int states)
{
    const size_t n1 = (size_t)N + 1, table_doubles = (size_t)N * (30 * (size_t)L + 6);
    const size_t out_b = up(24), gb_b = up(table_doubles * 8), fb_b = up((size_t)N * states * 8), c5_b = up(n1), mm_b = up(n1 * 7 * 8), cm_b = up(n1);
    const size_t need = out_b + gb_b + fb_b + c5_b + mm_b + cm_b;
    const vitm_bufs z = vitm_layout(nullptr, N, table_doubles, states);
    CHECK(!z.out && !z.Gb && !z.fb && !z.cm5 && !z.mm && !z.cm, "N=%d: the sizing pass hands out parts", N);
    CHECK(z.total == need, "N=%d L=%d states=%d: sizing pass %zu, by hand %zu", N, L, states, z.total, need);
    std::vector<char> block(need);
    // the first reservation of a call is vit_layout's: the vit_out alone, where this layout has it too -- at offset 0
    const vit_bufs first = vit_layout(block.data(), N, 0, 0);
    const vitm_bufs b = vitm_layout(block.data(), N, table_doubles, states);
    CHECK((char *)first.out == block.data() && (char *)b.out == block.data(), "N=%d: vit_out is not at offset 0 under both layouts", N);
    CHECK(vitm_layout(nullptr, N, 0, 0).total == first.total, "N=%d: the two first reservations differ", N);
    size_t at = out_b;
    CHECK((char *)b.Gb == block.data() + at, "N=%d: Gb", N);
    at += gb_b;
    CHECK((char *)b.fb == block.data() + at, "N=%d: fb", N);
    at += fb_b;
    CHECK((char *)b.cm5 == block.data() + at, "N=%d: cm5", N);
    at += c5_b;
    CHECK((char *)b.mm == block.data() + at, "N=%d: mm", N);
    at += mm_b;
    CHECK((char *)b.cm == block.data() + at, "N=%d: cm", N);
    CHECK(at + cm_b == b.total, "N=%d: total %zu, by hand %zu", N, b.total, at + cm_b);
    // every byte its users touch lies inside (the sanitizer watches the block's ends)
    memset(b.out, 1, 24);
    memset(b.Gb, 2, table_doubles * 8);
    memset(b.fb, 3, (size_t)N * states * 8);
    memset(b.cm5, 4, n1);
    memset(b.mm, 5, n1 * 7 * 8);
    memset(b.cm, 6, n1);
    CHECK(((char *)b.fb)[(size_t)N * states * 8 - 1] == 3 && ((char *)b.mm)[n1 * 56 - 1] == 5 && ((char *)b.cm5)[n1 - 1] == 4, "N=%d: parts overlap", N);
}

int main()
{
    const int shapes[][3] = {{1, 1, 2}, {2, 2, 4}, {6, 6, 4096}, {16, 12, 4096}, {60, 5, 3125}, {255, 3, 64}, {256, 3, 125}, {1000, 3, 64}, {1001, 1, 1}};
    for (const auto &s : shapes) check(s[0], s[1], s[2]);
    if (failures) {
        printf("vitm_layout: %d check(s) failed\n", failures);
        return 1;
    }
    printf("vitm_layout done\n");
    return 0;
}
