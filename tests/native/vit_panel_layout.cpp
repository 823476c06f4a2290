// The panel decoder's block of the batch (vit_panel_layout, gretel_amd/csrc/scratch_layout.hpp: the function the library itself
// calls) against its size and order written out by hand: n descriptors, n vit_outs, the gathered path rows.  Host only; built with
// -fsanitize=address,undefined by tests/test_panel_exact_host.py.  The descriptor itself holds device types and stands in
// viterbi_panel.hpp, which asserts its size to be WIN_BYTES: a stand-in of that size takes its place here.
#include "scratch_layout.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

#define WIN_BYTES 104
struct win_standin {
    void *p[7];
    int64_t home;
    int v[6];
    uint32_t U;
    uint32_t sm[2];
};
static_assert(sizeof(win_standin) == WIN_BYTES, "seven pointers, a 64-bit offset, six ints, U and two map words, padded to eight");
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

static void check(int n, size_t path_bytes)
{
    const size_t wd_b = up((size_t)n * WIN_BYTES), out_b = up((size_t)n * 24), path_b = up(path_bytes);
    const size_t need = wd_b + out_b + path_b;
    const vit_panel_bufs<win_standin> z = vit_panel_layout<win_standin>(nullptr, n, path_bytes);
    CHECK(!z.wd && !z.outs && !z.paths, "n=%d: the sizing pass hands out parts", n);
    CHECK(z.total == need, "n=%d paths=%zu: sizing pass %zu, by hand %zu", n, path_bytes, z.total, need);
    std::vector<char> block(need);
    const vit_panel_bufs<win_standin> b = vit_panel_layout<win_standin>(block.data(), n, path_bytes);
    CHECK(b.total == need, "n=%d: total %zu, by hand %zu", n, b.total, need);
    CHECK((char *)b.wd == block.data(), "n=%d: the descriptors do not lead", n);
    CHECK((char *)b.outs == block.data() + wd_b, "n=%d: outs at %zu, by hand %zu", n, (size_t)((char *)b.outs - block.data()), wd_b);
    CHECK((char *)b.paths == block.data() + wd_b + out_b, "n=%d: paths at %zu, by hand %zu", n, (size_t)((char *)b.paths - block.data()), wd_b + out_b);
    // every byte its users touch lies inside (the sanitizer watches the block's ends)
    memset(b.wd, 1, (size_t)n * WIN_BYTES);
    memset(b.outs, 2, (size_t)n * 24);
    if (path_bytes) memset(b.paths, 3, path_bytes);
    CHECK(n == 0 || ((char *)b.wd)[(size_t)n * WIN_BYTES - 1] == 1, "n=%d: the outs overwrote the descriptors", n);
    CHECK(n == 0 || ((char *)b.outs)[(size_t)n * 24 - 1] == 2, "n=%d: the paths overwrote the outs", n);
}

int main()
{
    const int ns[] = {1, 2, 3, 16, 40, 64, 255, 256, 257, 1000};
    const size_t pb[] = {2, 255, 256, 257, 10001, 64 * 10001};
    for (int n : ns)
        for (size_t p : pb) check(n, p);
    if (failures) {
        printf("vit_panel_layout: %d check(s) failed\n", failures);
        return 1;
    }
    printf("vit_panel_layout done\n");
    return 0;
}
