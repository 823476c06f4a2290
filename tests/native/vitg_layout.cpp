// The grid decoder's layout of the exact decoder's block (vitg_layout, gretel_amd/csrc/scratch_layout.hpp: the function the library
// itself calls) against its size and order written out by hand: the vit_out, the candidate bytes over the compact indices and over
// the symbols, the table, one back-pointer byte per position and state, two score rows, the end rule's partial scores and states
// (one per 4096 states), the path row.  One row is far beyond what can be had here (10 000 SNPs at 2^24 states): its offsets are
// checked as numbers, in 64 bits.  Host only; built with -fsanitize=address,undefined by tests/test_viterbi_grid_host.py.
#include "scratch_layout.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static_assert(sizeof(vit_out) == 24, "U, hole_at, end_state, pad, ll");
static_assert(GH_VITERBI_GRID_MAX_STATES == 16777216 && GH_VITG_END_CHUNK == 4096, "2^24 states, 4096 of them a partial");

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

// the parts' offsets by hand: out, cm5, cm, Gb, bp, rows, pv, pj, path, and the total behind them
struct by_hand {
    size_t at[9], total, parts;
};

static by_hand hand(int N, int L, size_t states)
{
    const size_t n1 = (size_t)N + 1, parts = (states + 4095) / 4096;
    const size_t sizes[9] = {up(24), up(n1), up(n1), up((size_t)N * (30 * (size_t)L + 6) * 8), up(n1 * states), up(2 * states * 8),
                             up(parts * 8), up(parts * 4), up(n1)};
    by_hand h;
    size_t at = 0;
    for (int q = 0; q < 9; q++) {
        h.at[q] = at;
        at += sizes[q];
    }
    h.total = at;
    h.parts = parts;
    return h;
}

static void offsets(const vitg_bufs &b, const char *base, const by_hand &h, int N)
{
    const void *got[9] = {b.out, b.cm5, b.cm, b.Gb, b.bp, b.rows, b.pv, b.pj, b.path};
    static const char *names[9] = {"out", "cm5", "cm", "Gb", "bp", "rows", "pv", "pj", "path"};
    for (int q = 0; q < 9; q++)
        CHECK((size_t)((const char *)got[q] - base) == h.at[q], "N=%d: %s at %zu, by hand %zu", N, names[q], (size_t)((const char *)got[q] - base), h.at[q]);
    CHECK(b.total == h.total && b.parts == h.parts, "N=%d: total %zu (by hand %zu), parts %zu (by hand %zu)", N, b.total, h.total, b.parts, h.parts);
}

static void check(int N, int L, size_t states)
{
    const size_t n1 = (size_t)N + 1, table_doubles = (size_t)N * (30 * (size_t)L + 6);
    const by_hand h = hand(N, L, states);
    const vitg_bufs z = vitg_layout(nullptr, N, table_doubles, states);
    CHECK(!z.out && !z.cm5 && !z.cm && !z.Gb && !z.bp && !z.rows && !z.pv && !z.pj && !z.path, "N=%d: the sizing pass hands out parts", N);
    CHECK(z.total == h.total, "N=%d L=%d states=%zu: sizing pass %zu, by hand %zu", N, L, states, z.total, h.total);
    std::vector<char> block(h.total);
    // the first reservation of a call: the vit_out and the candidate bytes alone, where the full layout has them too
    const vitg_bufs first = vitg_layout(block.data(), N, 0, 0);
    const vitg_bufs b = vitg_layout(block.data(), N, table_doubles, states);
    CHECK((char *)first.out == block.data() && first.out == b.out && first.cm5 == b.cm5 && first.cm == b.cm, "N=%d: the first reservation's parts move", N);
    CHECK(first.total == up(24) + 2 * up(n1) && !first.Gb && !first.bp && !first.rows && !first.path, "N=%d: the first reservation", N);
    CHECK((char *)vit_layout(block.data(), N, 0, 0).out == block.data(), "N=%d: vit_out is not at offset 0 under the decoder's own layout", N);
    offsets(b, block.data(), h, N);
    // every byte its users touch lies inside (the sanitizer watches the block's ends)
    memset(b.out, 1, 24);
    memset(b.cm5, 2, n1);
    memset(b.cm, 3, n1);
    memset(b.Gb, 4, table_doubles * 8);
    memset(b.bp, 5, n1 * states);
    memset(b.rows, 6, 2 * states * 8);
    memset(b.pv, 7, h.parts * 8);
    memset(b.pj, 8, h.parts * 4);
    memset(b.path, 9, n1);
    CHECK(((char *)b.cm)[n1 - 1] == 3 && ((char *)b.bp)[n1 * states - 1] == 5 && ((char *)b.rows)[16 * states - 1] == 6 &&
          ((char *)b.pv)[h.parts * 8 - 1] == 7 && ((char *)b.pj)[h.parts * 4 - 1] == 8 && ((char *)b.Gb)[table_doubles * 8 - 1] == 4, "N=%d: parts overlap", N);
}

int main()
{
    const size_t shapes[][3] = {{1, 1, 2}, {2, 2, 4}, {6, 6, 4096}, {16, 13, 8192}, {14, 6, 15625}, {12, 9, 19683}, {60, 5, 3125},
                                {255, 3, 64}, {1000, 3, 64}, {1001, 1, 1}, {21, 20, 1048576}};
    for (const auto &s : shapes) check((int)s[0], (int)s[1], s[2]);

    // 10 000 SNPs at the cap: nothing is touched, the offsets are numbers.  The back-pointers alone are 10 001 * 2^24 bytes.
    const int N = 10000, L = 12;
    const size_t states = 16777216, table_doubles = (size_t)N * (30 * L + 6);
    const by_hand h = hand(N, L, states);
    CHECK(h.at[5] - h.at[4] == 167788937216ull, "the back-pointer part by hand is %zu bytes", h.at[5] - h.at[4]);
    CHECK(h.at[4] == 256 + 2 * 10240 + 29280000 && h.at[6] - h.at[5] == 268435456 && h.parts == 4096 && h.at[7] - h.at[6] == 32768 &&
          h.at[8] - h.at[7] == 16384 && h.total == h.at[8] + 10240, "the large row by hand");
    CHECK(vitg_layout(nullptr, N, table_doubles, states).total == h.total, "N=10000 at the cap: sizing pass %zu, by hand %zu",
          vitg_layout(nullptr, N, table_doubles, states).total, h.total);
    char *fake = reinterpret_cast<char *>((size_t)1 << 20);   // never dereferenced
    offsets(vitg_layout(fake, N, table_doubles, states), fake, h, N);

    if (failures) {
        printf("vitg_layout: %d check(s) failed\n", failures);
        return 1;
    }
    printf("vitg_layout done\n");
    return 0;
}
