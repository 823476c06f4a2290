// The four scratch layouts of gretel_amd/csrc/scratch_layout.hpp (the functions the library itself calls) against their sizes and
// orders written out by hand, as the four users spelled them before the header existed.  Host only; built with
// -fsanitize=address,undefined by tests/test_scratch_layout.py.
#include "scratch_layout.hpp"

#include <cstdio>
#include <cstdlib>
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

struct part {
    const void *p;
    size_t off, bytes;     // where it must lie, how many bytes its user touches
};

// the parts in order: each where the hand-written sum puts it, 256-byte aligned, ending before the next begins and inside `total`
static void check_parts(const char *what, const char *base, size_t total, size_t want_total, const std::vector<part> &parts)
{
    CHECK(total == want_total, "%s: total %zu, by hand %zu", what, total, want_total);
    for (size_t k = 0; k < parts.size(); k++) {
        const size_t off = (size_t)((const char *)parts[k].p - base);
        CHECK(off == parts[k].off, "%s: part %zu at %zu, by hand %zu", what, k, off, parts[k].off);
        CHECK(off % 256 == 0, "%s: part %zu at %zu is not 256-byte aligned", what, k, off);
        const size_t end = k + 1 < parts.size() ? (size_t)((const char *)parts[k + 1].p - base) : total;
        CHECK(off + parts[k].bytes <= end, "%s: part %zu (%zu + %zu) runs into what follows at %zu", what, k, off, parts[k].bytes, end);
    }
}

static void check_assign(int n_paths, int N, int64_t n_reads, bool per_read)
{
    char what[96];
    snprintf(what, sizeof what, "assign n_paths=%d N=%d n_reads=%lld per_read=%d", n_paths, N, (long long)n_reads, (int)per_read);
    const size_t nw = ((size_t)n_paths + 63) / 64, path_bytes = (size_t)n_paths * (size_t)(N + 1);
    const size_t cnt_b = up((size_t)3 * n_paths * 8 + 8 * 8);
    const size_t path_b = up(path_bytes);
    const size_t mask_b = up(nw * (size_t)(N + 1) * 5 * 8);
    const size_t read_b = per_read ? up((size_t)n_reads * 3 * 4) : 0;
    const size_t need = cnt_b + path_b + mask_b + read_b;
    const assign_bufs z = assign_layout(nullptr, n_paths, N, n_reads, per_read);
    CHECK(!z.cnt && !z.paths && !z.mask && !z.read, "%s: the sizing pass hands out parts", what);
    CHECK(z.total == need, "%s: sizing pass %zu, by hand %zu", what, z.total, need);
    std::vector<char> block(need);
    const assign_bufs b = assign_layout(block.data(), n_paths, N, n_reads, per_read);
    std::vector<part> parts = {{b.cnt, 0, (size_t)3 * n_paths * 8 + 8 * 8}, {b.paths, cnt_b, path_bytes},
                               {b.mask, cnt_b + path_b, nw * (size_t)(N + 1) * 5 * 8}};
    if (per_read) parts.push_back({b.read, cnt_b + path_b + mask_b, (size_t)n_reads * 3 * 4});
    else CHECK(b.read == nullptr, "%s: per-read results nobody asked for", what);
    check_parts(what, block.data(), b.total, need, parts);
}

static void check_score(int slab, size_t n1)
{
    char what[64];
    snprintf(what, sizeof what, "score slab=%d n1=%zu", slab, n1);
    const size_t path_b = up((size_t)slab * n1), rec_b = up((size_t)slab * sizeof(gh_score_rec)), dbl_b = up((size_t)slab * n1 * 8);
    const size_t need = 2 * path_b + rec_b + 2 * dbl_b;
    CHECK(score_layout(nullptr, slab, n1).total == need, "%s: sizing pass, by hand %zu", what, need);
    std::vector<char> block(need);
    const score_bufs b = score_layout(block.data(), slab, n1);
    check_parts(what, block.data(), b.total, need,
                {{b.weight, 0, (size_t)slab * n1 * 8}, {b.margin, dbl_b, (size_t)slab * n1 * 8}, {b.recs, 2 * dbl_b, (size_t)slab * sizeof(gh_score_rec)},
                 {b.paths, 2 * dbl_b + rec_b, (size_t)slab * n1}, {b.pick, 2 * dbl_b + rec_b + path_b, (size_t)slab * n1}});
}

static void check_beam(int N, int L, int width)
{
    char what[64];
    snprintf(what, sizeof what, "beam N=%d L=%d width=%d", N, L, width);
    const int bps = (width + 3) & ~3;
    const size_t n1 = (size_t)N + 1;
    const size_t gb_b = up((size_t)N * (30 * L + 6) * 8), bp_b = up(n1 * bps), path_b = up(n1 * 32);
    const size_t need = gb_b + bp_b + path_b + up(32 * 8) + up(16);
    const size_t table_doubles = (size_t)N * (30 * L + 6);
    CHECK(beam_layout(nullptr, N, table_doubles, width).total == need, "%s: sizing pass, by hand %zu", what, need);
    std::vector<char> block(need);
    const beam_bufs b = beam_layout(block.data(), N, table_doubles, width);
    CHECK(b.bps == bps, "%s: bps %d, by hand %d", what, b.bps, bps);
    CHECK(sizeof(beam_out) == 16, "beam_out is %zu bytes", sizeof(beam_out));
    check_parts(what, block.data(), b.total, need,
                {{b.Gb, 0, table_doubles * 8}, {b.bp, gb_b, n1 * bps}, {b.paths, gb_b + bp_b, n1 * 32}, {b.ll, gb_b + bp_b + path_b, 32 * 8},
                 {b.out, gb_b + bp_b + path_b + up(32 * 8), 16}});
}

static void check_exact(int N, int L, int ns)
{
    char what[64];
    snprintf(what, sizeof what, "exact N=%d L=%d states=%d", N, L, ns);
    const size_t n1 = (size_t)N + 1;
    const size_t out_b = up(24), gb_b = up((size_t)N * (30 * L + 6) * 8), bp_b = up(n1 * ns + 4);
    const size_t ve_b = up((size_t)ns * 8), ok_b = up((size_t)ns), path_b = up(n1);
    const size_t need = out_b + gb_b + bp_b + ve_b + ok_b + path_b;
    const size_t table_doubles = (size_t)N * (30 * L + 6);
    CHECK(sizeof(vit_out) == 24, "vit_out is %zu bytes", sizeof(vit_out));
    CHECK(vit_layout(nullptr, N, table_doubles, ns).total == need, "%s: sizing pass, by hand %zu", what, need);
    std::vector<char> block(need);
    // the first reservation of a call: k_vit_union's word alone, where the full layout has it too -- at offset 0
    const vit_bufs first = vit_layout(block.data(), N, 0, 0);
    CHECK(first.total == up(24), "%s: the first reservation is %zu bytes, by hand %zu", what, first.total, up(24));
    CHECK((const char *)first.out == block.data(), "%s: vit_out of the first reservation is not at offset 0", what);
    const vit_bufs b = vit_layout(block.data(), N, table_doubles, ns);
    CHECK((const char *)b.out == block.data(), "%s: vit_out is not at offset 0", what);
    check_parts(what, block.data(), b.total, need,
                {{b.out, 0, 24}, {b.Gb, out_b, table_doubles * 8}, {b.bp, out_b + gb_b, n1 * ns + 4}, {b.vend, out_b + gb_b + bp_b, (size_t)ns * 8},
                 {b.okend, out_b + gb_b + bp_b + ve_b, (size_t)ns}, {b.path, out_b + gb_b + bp_b + ve_b + ok_b, n1}});
}

int main()
{
    for (int per_read = 0; per_read < 2; per_read++) {
        check_assign(5, 60, 800, per_read);
        check_assign(130, 300, 6000, per_read);      // three mask words
        check_assign(0, 60, 0, per_read);            // nothing to count, nothing to report
    }
    check_score(15279, 61);                          // one full slab at N = 60
    check_score(1, 2);
    for (int width : {1, 32}) {
        check_beam(60, 3, width);
        check_beam(300, 16, width);
        check_beam(1, 1, width);
    }
    for (int N : {1, 300}) {
        check_exact(N, 4, 1);
        check_exact(N, 3, 64);
        check_exact(N, 6, 4096);
    }
    if (failures) {
        printf("scratch_layout: %d check(s) failed\n", failures);
        return 1;
    }
    printf("scratch_layout done\n");
    return 0;
}
