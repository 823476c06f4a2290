// The panel k-best decoder's block of the batch (vitk_panel_layout, gretel_amd/csrc/scratch_layout.hpp: the function the library
// itself calls) against its sizes and order written out by hand: n descriptors, n list entries, n vit_outs, the gathered path
// rows (the sum of k_w * (N_w + 1) bytes) and scores (the sum of k_w doubles), every part on a 256-byte boundary.  Host only; built
// with -fsanitize=address,undefined by tests/test_panel_kbest_host.py.  The descriptor itself holds device types and stands in
// viterbi_kbest_panel.hpp, which asserts its size to be WIN_BYTES: a stand-in of that size takes its place here.
#include "scratch_layout.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

#define WIN_BYTES 128
struct win_standin {
    void *p[9];            // Gb, minfo, out, bp, vend, cend, paths, ll, n_out
    int64_t row_home, ll_home;
    int v[7];              // N, Le, S, states, K, marginal_term, chunk
    uint32_t U;
    uint32_t sm[2];
};
static_assert(sizeof(win_standin) == WIN_BYTES, "nine pointers, two 64-bit offsets, seven ints, U and two map words");
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

static size_t off_of(const void *p, const char *base) { return (size_t)((const char *)p - base); }

// `pos[w]` = N_w + 1, `k[w]` the rows asked for, `got[w]` the rows the window has (0: a hole -- the layout reserves k all the same)
static void check(const std::vector<int> &pos, const std::vector<int> &k, const std::vector<int> &got, size_t wd_b, size_t list_b, size_t out_b,
                  size_t rows_b, size_t ll_b)
{
    const int n = (int)pos.size();
    size_t path_bytes = 0, scores = 0;
    std::vector<size_t> rhome, lhome;
    for (int w = 0; w < n; w++) {
        rhome.push_back(path_bytes);
        lhome.push_back(scores);
        path_bytes += (size_t)k[w] * (size_t)pos[w];
        scores += (size_t)k[w];
    }
    const size_t need = wd_b + list_b + out_b + rows_b + ll_b;
    const vitk_panel_bufs<win_standin> z = vitk_panel_layout<win_standin>(nullptr, n, path_bytes, scores);
    CHECK(!z.wd && !z.list && !z.outs && !z.paths && !z.ll, "n=%d: the sizing pass hands out parts", n);
    CHECK(z.total == need, "n=%d path_bytes=%zu scores=%zu: sizing pass %zu, by hand %zu", n, path_bytes, scores, z.total, need);
    // (operator new gives 16-byte alignment: the parts' alignment is checked as offsets, and against a base on a 256-byte boundary)
    std::vector<char> store(need + 256);
    char *block = store.data() + (256 - (reinterpret_cast<uintptr_t>(store.data()) & 255)) % 256;
    const vitk_panel_bufs<win_standin> b = vitk_panel_layout<win_standin>(block, n, path_bytes, scores);
    CHECK(b.total == need, "n=%d: total %zu, by hand %zu", n, b.total, need);
    CHECK(off_of(b.wd, block) == 0, "n=%d: the descriptors do not lead", n);
    CHECK(off_of(b.list, block) == wd_b, "n=%d: list at %zu, by hand %zu", n, off_of(b.list, block), wd_b);
    CHECK(off_of(b.outs, block) == wd_b + list_b, "n=%d: outs at %zu, by hand %zu", n, off_of(b.outs, block), wd_b + list_b);
    CHECK(off_of(b.paths, block) == wd_b + list_b + out_b, "n=%d: rows at %zu, by hand %zu", n, off_of(b.paths, block), wd_b + list_b + out_b);
    CHECK(off_of(b.ll, block) == wd_b + list_b + out_b + rows_b, "n=%d: scores at %zu, by hand %zu", n, off_of(b.ll, block),
          wd_b + list_b + out_b + rows_b);
    const void *parts[] = {b.wd, b.list, b.outs, b.paths, b.ll};
    for (const void *p : parts) CHECK((reinterpret_cast<uintptr_t>(p) & 255) == 0, "n=%d: a part at offset %zu is not on a 256-byte boundary", n, off_of(p, block));
    // every byte its users touch lies inside, and no part reaches into the next: the descriptors, the list and the outs whole
    // (the union launch's 104-byte descriptors stand in the first part too), and the rows and scores each window has, at its homes
    memset(b.wd, 1, (size_t)n * WIN_BYTES);
    memset(b.list, 2, (size_t)n * sizeof(int32_t));
    memset(b.outs, 3, (size_t)n * 24);
    for (int w = 0; w < n; w++) {
        if (!got[w]) continue;
        memset(b.paths + rhome[w], 5 + w % 3, (size_t)got[w] * (size_t)pos[w]);
        for (int q = 0; q < got[w]; q++) b.ll[lhome[w] + q] = (double)w;
    }
    CHECK(((char *)b.wd)[(size_t)n * WIN_BYTES - 1] == 1, "n=%d: the list overwrote the descriptors", n);
    CHECK(((char *)b.list)[(size_t)n * 4 - 1] == 2, "n=%d: the outs overwrote the list", n);
    CHECK(((char *)b.outs)[(size_t)n * 24 - 1] == 3, "n=%d: the rows overwrote the outs", n);
    for (int w = 0; w < n; w++) {
        if (!got[w]) continue;
        CHECK(b.paths[rhome[w]] == 5 + w % 3 && b.paths[rhome[w] + (size_t)got[w] * pos[w] - 1] == 5 + w % 3, "n=%d: window %d's rows were overwritten", n, w);
        CHECK(b.ll[lhome[w]] == (double)w && b.ll[lhome[w] + got[w] - 1] == (double)w, "n=%d: window %d's scores were overwritten", n, w);
    }
    CHECK((char *)(b.paths + path_bytes) <= (char *)b.ll, "n=%d: the rows end %zu bytes into the scores", n, off_of(b.paths + path_bytes, block) - off_of(b.ll, block));
    CHECK((char *)(b.ll + scores) <= block + need, "n=%d: the scores end %zu bytes past the block", n, off_of(b.ll + scores, block) - need);
}

int main()
{
    // one window of two positions (N = 0 never occurs; N = 1 gives 2), k = 1: every part is its own 256 bytes
    check({2}, {1}, {1}, 256, 256, 256, 256, 256);
    // one window of 1001 positions, k = 32: rows 32 032 -> 32 256 (126 * 256); scores 256 bytes exactly
    check({1001}, {32}, {32}, 256, 256, 256, 32256, 256);
    // ... and k = 4, two rows found: rows 4004 -> 4096; scores 32 -> 256
    check({1001}, {4}, {2}, 256, 256, 256, 4096, 256);
    // three ragged windows, the middle one with a hole: 3 * 128 = 384 -> 512; list 12 -> 256; outs 72 -> 256;
    // rows 8 * 2 + 4 * 17 + 32 * 1001 = 16 + 68 + 32 032 = 32 116 -> 32 256; scores 44 * 8 = 352 -> 512
    check({2, 17, 1001}, {8, 4, 32}, {2, 0, 32}, 512, 256, 256, 32256, 512);
    check({2, 17, 1001}, {8, 4, 32}, {0, 4, 0}, 512, 256, 256, 32256, 512);
    // 256 windows, position counts 31 + (w mod 7) * 5, k = 1 + w mod 8, every fifth with a hole: 256 * 128 = 32 768; list 1024;
    // outs 6144.  k sums to 32 * 36 = 1152: scores 9216 (36 * 256).  Rows: the sum of (1 + w mod 8) * (31 + 5 * (w mod 7)) =
    // 31 * 1152 + 5 * sum((1 + w mod 8) * (w mod 7)).  w = 56 q + r: over a block of 56, (w mod 8, w mod 7) takes every pair once,
    // sum = 36 * 21 = 756; four blocks 3024; the last 32 (w = 224 .. 255, r = 0 .. 31): the sum over r of (1 + r mod 8) * (r mod 7)
    // = 398 (r 0-7: 0+2+6+12+20+30+42+0 = 112; r 8-15, r mod 7 = 1,2,3,4,5,6,0,1: 1+4+9+16+25+36+0+8 = 99; r 16-23, 2,3,4,5,6,0,1,2:
    // 2+6+12+20+30+0+7+16 = 93; r 24-31, 3,4,5,6,0,1,2,3: 3+8+15+24+0+6+14+24 = 94).
    // Rows = 35 712 + 5 * (3024 + 398) = 35 712 + 17 110 = 52 822 -> 52 992 (207 * 256)
    {
        std::vector<int> pos, k, got;
        for (int w = 0; w < 256; w++) { pos.push_back(31 + (w % 7) * 5); k.push_back(1 + w % 8); got.push_back(w % 5 == 4 ? 0 : 1 + w % 8); }
        check(pos, k, got, 32768, 1024, 6144, 52992, 9216);
    }
    // 256 windows of 1001 positions at k = 32: rows 256 * 32 032 = 8 200 192 (a multiple of 256); scores 65 536
    {
        const vitk_panel_bufs<win_standin> z = vitk_panel_layout<win_standin>(nullptr, 256, (size_t)256 * 32 * 1001, (size_t)256 * 32);
        CHECK(z.total == (size_t)32768 + 1024 + 6144 + 8200192 + 65536, "256 x 1001 x 32: %zu", z.total);
    }
    if (failures) {
        printf("vitk_panel_layout: %d check(s) failed\n", failures);
        return 1;
    }
    printf("vitk_panel_layout done\n");
    return 0;
}
