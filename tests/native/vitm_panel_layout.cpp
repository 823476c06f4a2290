// The panel max-marginals' block of the batch (vitm_panel_layout, gretel_amd/csrc/scratch_layout.hpp: the function the library
// itself calls) against its sizes and order written out by hand: n descriptors, 2 n list entries, n vit_outs, the gathered mm
// ([positions][7] doubles) and cm ([positions] bytes), every part on a 256-byte boundary.  Host only; built with
// -fsanitize=address,undefined by tests/test_panel_maxmarg_host.py.  The descriptor itself holds device types and stands in
// viterbi_marg_panel.hpp, which asserts its size to be WIN_BYTES: a stand-in of that size takes its place here.
#include "scratch_layout.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

#define WIN_BYTES 104
struct win_standin {
    void *p[7];            // Gb, minfo, out, fb, cm5, mm, cm
    int64_t home;
    int v[6];              // N, Le, S, states, pw, marginal_term
    uint32_t U;
    uint32_t sm[2];
};
static_assert(sizeof(win_standin) == WIN_BYTES, "seven pointers, a 64-bit offset, six ints, U and two map words, padded to eight");
static_assert(sizeof(vit_out) == 24, "U, hole_at, end_state, pad, ll");
static_assert(GH_NSYM == 7, "mm has seven columns");

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

static size_t off_of(const void *p, const char *base) { return (size_t)((const char *)p - base); }

// `pos[w]` = N_w + 1; `hole[w]`: the window's ranges stay unwritten (the layout reserves them all the same)
static void check(const std::vector<int> &pos, const std::vector<int> &hole, size_t wd_b, size_t list_b, size_t out_b, size_t mm_b, size_t cm_b)
{
    const int n = (int)pos.size();
    size_t positions = 0;
    std::vector<size_t> home;
    for (int p : pos) { home.push_back(positions); positions += (size_t)p; }
    const size_t need = wd_b + list_b + out_b + mm_b + cm_b;
    const vitm_panel_bufs<win_standin> z = vitm_panel_layout<win_standin>(nullptr, n, positions);
    CHECK(!z.wd && !z.list && !z.outs && !z.mm && !z.cm, "n=%d: the sizing pass hands out parts", n);
    CHECK(z.total == need, "n=%d positions=%zu: sizing pass %zu, by hand %zu", n, positions, z.total, need);
    // (operator new gives 16-byte alignment: the parts' alignment is checked as offsets, and against a base on a 256-byte boundary)
    std::vector<char> store(need + 256);
    char *block = store.data() + (256 - (reinterpret_cast<uintptr_t>(store.data()) & 255)) % 256;
    const vitm_panel_bufs<win_standin> b = vitm_panel_layout<win_standin>(block, n, positions);
    CHECK(b.total == need, "n=%d: total %zu, by hand %zu", n, b.total, need);
    CHECK(off_of(b.wd, block) == 0, "n=%d: the descriptors do not lead", n);
    CHECK(off_of(b.list, block) == wd_b, "n=%d: list at %zu, by hand %zu", n, off_of(b.list, block), wd_b);
    CHECK(off_of(b.outs, block) == wd_b + list_b, "n=%d: outs at %zu, by hand %zu", n, off_of(b.outs, block), wd_b + list_b);
    CHECK(off_of(b.mm, block) == wd_b + list_b + out_b, "n=%d: mm at %zu, by hand %zu", n, off_of(b.mm, block), wd_b + list_b + out_b);
    CHECK(off_of(b.cm, block) == wd_b + list_b + out_b + mm_b, "n=%d: cm at %zu, by hand %zu", n, off_of(b.cm, block), wd_b + list_b + out_b + mm_b);
    const void *parts[] = {b.wd, b.list, b.outs, b.mm, b.cm};
    for (const void *p : parts) CHECK((reinterpret_cast<uintptr_t>(p) & 255) == 0, "n=%d: a part at offset %zu is not on a 256-byte boundary", n, off_of(p, block));
    // every byte its users touch lies inside, and no part reaches into the next: the descriptors and the lists whole, each
    // window's outs, and the mm and cm ranges of the windows without a hole at their homes
    memset(b.wd, 1, (size_t)n * WIN_BYTES);
    memset(b.list, 2, (size_t)n * 2 * sizeof(int32_t));
    memset(b.outs, 3, (size_t)n * 24);
    for (int w = 0; w < n; w++) {
        if (hole[w]) continue;
        for (size_t q = 0; q < (size_t)pos[w] * 7; q++) b.mm[home[w] * 7 + q] = (double)w;
        memset(b.cm + home[w], 5 + w % 3, (size_t)pos[w]);
    }
    CHECK(((char *)b.wd)[(size_t)n * WIN_BYTES - 1] == 1, "n=%d: the lists overwrote the descriptors", n);
    CHECK(((char *)b.list)[(size_t)n * 8 - 1] == 2, "n=%d: the outs overwrote the lists", n);
    CHECK(((char *)b.outs)[(size_t)n * 24 - 1] == 3, "n=%d: the mm overwrote the outs", n);
    for (int w = 0; w < n; w++) {
        if (hole[w]) continue;
        CHECK(b.mm[home[w] * 7] == (double)w && b.mm[(home[w] + pos[w]) * 7 - 1] == (double)w, "n=%d: window %d's mm was overwritten", n, w);
        CHECK(b.cm[home[w]] == 5 + w % 3 && b.cm[home[w] + pos[w] - 1] == 5 + w % 3, "n=%d: window %d's cm was overwritten", n, w);
    }
    CHECK((char *)(b.cm + positions) <= block + need, "n=%d: cm ends %zu bytes past the block", n, off_of(b.cm + positions, block) - need);
}

int main()
{
    // one window of one position (N = 0 never occurs; N = 1 gives 2): every part is its own 256 bytes
    check({2}, {0}, 256, 256, 256, 256, 256);
    // one window of 1001 positions: mm 1001 * 56 = 56056 -> 56064, cm 1001 -> 1024
    check({1001}, {0}, 256, 256, 256, 56064, 1024);
    // three ragged windows, the middle one with a hole: 2 + 17 + 1001 = 1020 positions; 3 * 104 = 312 -> 512; 24 -> 256; 72 -> 256;
    // mm 1020 * 56 = 57120 -> 57344 (224 * 256); cm 1020 -> 1024
    check({2, 17, 1001}, {0, 1, 0}, 512, 256, 256, 57344, 1024);
    check({2, 17, 1001}, {1, 0, 1}, 512, 256, 256, 57344, 1024);
    // 256 windows, position counts 31 + (w mod 7) * 5, every fifth with a hole: 256 * 104 = 26624 (104 * 256); lists 2048; outs 6144;
    // positions = 256 * 31 + 5 * (36 * 21 + (0 + 1 + 2 + 3)) = 7936 + 5 * 762 = 11746; mm 11746 * 56 = 657776 -> 657920 (2570 * 256);
    // cm 11746 -> 11776 (46 * 256)
    {
        std::vector<int> pos, hole;
        for (int w = 0; w < 256; w++) { pos.push_back(31 + (w % 7) * 5); hole.push_back(w % 5 == 4); }
        check(pos, hole, 26624, 2048, 6144, 657920, 11776);
    }
    // 256 windows of 10 001 positions: 2 560 256 positions; mm 143 374 336 bytes (a multiple of 256); cm 2 560 256 (10001 * 256)
    {
        const vitm_panel_bufs<win_standin> z = vitm_panel_layout<win_standin>(nullptr, 256, (size_t)256 * 10001);
        CHECK(z.total == (size_t)26624 + 2048 + 6144 + 143374336 + 2560256, "256 x 10001: %zu", z.total);
    }
    if (failures) {
        printf("vitm_panel_layout: %d check(s) failed\n", failures);
        return 1;
    }
    printf("vitm_panel_layout done\n");
    return 0;
}
