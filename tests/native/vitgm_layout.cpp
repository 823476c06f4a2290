// The layout of the max-marginals on the grid (vitgm_layout, gretel_amd/csrc/scratch_layout.hpp: the function the library itself
// calls) against its size and order written out by hand: the vit_out and the two rows of candidate bytes exactly where vitg_layout
// has them (the call opens as the grid decoder does), the table, one kept row of F per position with the +0.0 of position 0
// behind the last, two rows of B, five partial maxima per position and 512 states, mm, cm.  No two parts overlap.  One row is far
// beyond what can be had here (10 000 SNPs at 2^24 states): its offsets are checked as numbers, in 64 bits.  Host only; built
// with -fsanitize=address,undefined by tests/test_viterbi_grid_marg_host.py.
#include "scratch_layout.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static_assert(sizeof(vit_out) == 24, "U, hole_at, end_state, pad, ll");
static_assert(GH_VITERBI_GRID_MAX_STATES == 16777216 && GH_VITGM_THREADS == 256 && GH_NSYM == 7, "2^24 states, 256 threads, seven symbols");

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

// the parts' offsets by hand: out, cm5, cm0, Gb, F, B, part, mm, cm, and the total behind them
struct by_hand {
    size_t at[9], size[9], total, wgs;
};

static by_hand hand(int N, int L, size_t states)
{
    const size_t n1 = (size_t)N + 1, wgs = (states + 511) / 512;
    const size_t sizes[9] = {24, n1, n1, (size_t)N * (30 * (size_t)L + 6) * 8, ((size_t)N * states + 1) * 8, 2 * states * 8, (size_t)N * wgs * 5 * 8,
                             n1 * 7 * 8, n1};
    by_hand h;
    size_t at = 0;
    for (int q = 0; q < 9; q++) {
        h.at[q] = at;
        h.size[q] = sizes[q];
        at += up(sizes[q]);
    }
    h.total = at;
    h.wgs = wgs;
    return h;
}

static void offsets(const vitgm_bufs &b, const char *base, const by_hand &h, int N)
{
    const void *got[9] = {b.out, b.cm5, b.cm0, b.Gb, b.F, b.B, b.part, b.mm, b.cm};
    static const char *names[9] = {"out", "cm5", "cm0", "Gb", "F", "B", "part", "mm", "cm"};
    for (int q = 0; q < 9; q++) {
        const size_t at = (size_t)((const char *)got[q] - base);
        CHECK(at == h.at[q], "N=%d: %s at %zu, by hand %zu", N, names[q], at, h.at[q]);
        // no two parts overlap: a part ends where the next begins, or before
        CHECK(at + h.size[q] <= (q < 8 ? h.at[q + 1] : h.total), "N=%d: %s runs into the next part", N, names[q]);
    }
    CHECK(b.total == h.total && b.wgs == h.wgs, "N=%d: total %zu (by hand %zu), workgroups %zu (by hand %zu)", N, b.total, h.total, b.wgs, h.wgs);
}

static void check(int N, int L, size_t states)
{
    const size_t n1 = (size_t)N + 1, table_doubles = (size_t)N * (30 * (size_t)L + 6);
    const by_hand h = hand(N, L, states);
    const vitgm_bufs z = vitgm_layout(nullptr, N, table_doubles, states);
    CHECK(!z.out && !z.cm5 && !z.cm0 && !z.Gb && !z.F && !z.B && !z.part && !z.mm && !z.cm, "N=%d: the sizing pass hands out parts", N);
    CHECK(z.total == h.total, "N=%d L=%d states=%zu: sizing pass %zu, by hand %zu", N, L, states, z.total, h.total);
    std::vector<char> block(h.total);
    // the first reservation of a call is the grid decoder's: the vit_out and the candidate bytes, where the full layout has them too
    const vitg_bufs first = vitg_layout(block.data(), N, 0, 0);
    const vitgm_bufs small = vitgm_layout(block.data(), N, 0, 0);
    const vitgm_bufs b = vitgm_layout(block.data(), N, table_doubles, states);
    CHECK((char *)first.out == block.data() && first.out == b.out && first.cm5 == b.cm5 && first.cm == b.cm0, "N=%d: the first reservation's parts move", N);
    CHECK(small.out == b.out && small.cm5 == b.cm5 && small.cm0 == b.cm0 && small.total == first.total && first.total == up(24) + 2 * up(n1) &&
          !small.Gb && !small.F && !small.B && !small.part && !small.mm && !small.cm, "N=%d: the first reservation", N);
    offsets(b, block.data(), h, N);
    // every byte its users touch lies inside (the sanitizer watches the block's ends), and a part's last byte survives its neighbours
    memset(b.out, 1, 24);
    memset(b.cm5, 2, n1);
    memset(b.cm0, 3, n1);
    memset(b.Gb, 4, table_doubles * 8);
    memset(b.F, 5, ((size_t)N * states + 1) * 8);
    memset(b.B, 6, 2 * states * 8);
    memset(b.part, 7, (size_t)N * h.wgs * 5 * 8);
    memset(b.mm, 8, n1 * 7 * 8);
    memset(b.cm, 9, n1);
    CHECK(((char *)b.out)[23] == 1 && ((char *)b.cm5)[n1 - 1] == 2 && ((char *)b.cm0)[n1 - 1] == 3 && ((char *)b.Gb)[table_doubles * 8 - 1] == 4 &&
          ((char *)b.F)[((size_t)N * states + 1) * 8 - 1] == 5 && ((char *)b.B)[16 * states - 1] == 6 && ((char *)b.part)[(size_t)N * h.wgs * 40 - 1] == 7 &&
          ((char *)b.mm)[n1 * 56 - 1] == 8 && ((char *)b.cm)[n1 - 1] == 9 && ((char *)b.Gb)[0] == 4 && ((char *)b.F)[0] == 5 && ((char *)b.B)[0] == 6 &&
          ((char *)b.part)[0] == 7 && ((char *)b.mm)[0] == 8 && ((char *)b.cm)[0] == 9, "N=%d: parts overlap", N);
    // the backward step's workgroups (a thread per S consecutive states) fit the partials under every S the state count can have
    for (size_t S = 2; S <= 5; S++) CHECK((states / S + 255) / 256 <= b.wgs, "N=%d: S=%zu makes more workgroups than the partials hold", N, S);
    CHECK(b.wgs >= 1, "N=%d: one state, one workgroup", N);
}

int main()
{
    const size_t shapes[][3] = {{1, 1, 1}, {1, 1, 2}, {2, 2, 4}, {6, 6, 4096}, {16, 13, 8192}, {14, 6, 15625}, {12, 9, 19683}, {60, 5, 3125},
                                {255, 3, 64}, {1000, 3, 64}, {34, 30, 1}, {3, 10, 1048576}};
    for (const auto &s : shapes) check((int)s[0], (int)s[1], s[2]);

    char *fake = reinterpret_cast<char *>((size_t)1 << 20);   // never dereferenced
    // 60 SNPs at the fill's own L = 10, without and with deletion columns: the sums of tests/test_viterbi_grid_marg_host.py
    {
        const by_hand h = hand(60, 10, 1048576);
        CHECK(h.total == 525160704ull && h.wgs == 2048 && h.at[4] == 768 + 146944 && h.at[5] - h.at[4] == 503316736ull &&
              h.at[6] - h.at[5] == 16777216 && h.at[7] - h.at[6] == 4915200 && h.at[8] - h.at[7] == 3584, "60 SNPs at 4^10 by hand: %zu", h.total);
        CHECK(vitgm_layout(nullptr, 60, 60 * 306, 1048576).total == h.total, "60 SNPs at 4^10: the sizing pass");
        offsets(vitgm_layout(fake, 60, 60 * 306, 1048576), fake, h, 60);
    }
    {
        const by_hand h = hand(60, 10, 9765625);
        CHECK(h.total == 4889679360ull && h.wgs == 19074 && h.at[5] - h.at[4] == 4687500032ull && h.at[6] - h.at[5] == 156250112 &&
              h.at[7] - h.at[6] == 45777664, "60 SNPs at 5^10 by hand: %zu", h.total);
        CHECK(vitgm_layout(nullptr, 60, 60 * 306, 9765625).total == h.total, "60 SNPs at 5^10: the sizing pass");
        offsets(vitgm_layout(fake, 60, 60 * 306, 9765625), fake, h, 60);
    }
    // 10 000 SNPs at the cap: nothing is touched, the offsets are numbers.  The kept rows alone are 10 000 * 2^24 * 8 bytes.
    {
        const int N = 10000, L = 12;
        const size_t states = 16777216, table_doubles = (size_t)N * (30 * L + 6);
        const by_hand h = hand(N, L, states);
        CHECK(h.at[5] - h.at[4] == 1342177280256ull, "the kept rows by hand are %zu bytes", h.at[5] - h.at[4]);
        CHECK(h.at[4] == 256 + 2 * 10240 + 29280000 && h.at[6] - h.at[5] == 268435456 && h.wgs == 32768 && h.at[7] - h.at[6] == 13107200000ull &&
              h.at[8] - h.at[7] == 560128 && h.total == h.at[8] + 10240 && h.total == 1355582786816ull, "the large row by hand");
        CHECK(vitgm_layout(nullptr, N, table_doubles, states).total == h.total, "N=10000 at the cap: sizing pass %zu, by hand %zu",
              vitgm_layout(nullptr, N, table_doubles, states).total, h.total);
        offsets(vitgm_layout(fake, N, table_doubles, states), fake, h, N);
    }

    if (failures) {
        printf("vitgm_layout: %d check(s) failed\n", failures);
        return 1;
    }
    printf("vitgm_layout done\n");
    return 0;
}
