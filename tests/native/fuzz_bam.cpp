// fuzz_bam.cpp -- malformed-BAM fuzz of the native decoder (gretel_amd/csrc/bam_support.cpp), built by
// tests/test_bam_fuzz.py with -fsanitize=address,undefined on the CPU: every mutated file must come back as a status
// code (0 or a negative error), never as an out-of-bounds access.  Every variant is decoded with pysam's default depth cap and
// with each of the caps given (default 1,3,40: the sequential pass of the cap, the batches set aside in front of it and their
// replay run under the sanitizers too).
//   fuzz_bam <valid.bam> <contig> <end_pos> <iterations> <seed> <scratch.bam> [cap,cap,...]
#include <climits>
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gretel_io.h"

static std::vector<uint8_t> slurp(const char *p)
{
    std::vector<uint8_t> d;
    FILE *f = fopen(p, "rb");
    if (!f) return d;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
    fclose(f);
    return d;
}

static std::vector<uint8_t> gunzip_all(const std::vector<uint8_t> &in)
{
    std::vector<uint8_t> out;
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    inflateInit2(&zs, 15 + 32);
    zs.next_in = const_cast<uint8_t *>(in.data());
    zs.avail_in = (uInt)in.size();
    std::vector<uint8_t> chunk(1 << 16);
    for (;;) {
        zs.next_out = chunk.data();
        zs.avail_out = (uInt)chunk.size();
        int rc = inflate(&zs, Z_NO_FLUSH);
        out.insert(out.end(), chunk.data(), chunk.data() + (chunk.size() - zs.avail_out));
        if (rc == Z_STREAM_END) {
            if (zs.avail_in == 0) break;
            inflateReset(&zs);
        } else if (rc != Z_OK) break;
    }
    inflateEnd(&zs);
    return out;
}

static void bgzf_write(const char *path, const std::vector<uint8_t> &data, size_t payload)
{
    FILE *f = fopen(path, "wb");
    for (size_t o = 0; o <= data.size(); o += payload) {
        const size_t n = o < data.size() ? std::min(payload, data.size() - o) : 0;
        std::vector<uint8_t> c(n + 1024);
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        deflateInit2(&zs, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
        zs.next_in = const_cast<uint8_t *>(data.data() + o);
        zs.avail_in = (uInt)n;
        zs.next_out = c.data();
        zs.avail_out = (uInt)c.size();
        deflate(&zs, Z_FINISH);
        const size_t cl = c.size() - zs.avail_out;
        deflateEnd(&zs);
        const uint16_t bsize = (uint16_t)(cl + 25);
        uint8_t head[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 255), (uint8_t)(bsize >> 8)};
        fwrite(head, 1, 18, f);
        fwrite(c.data(), 1, cl, f);
        const uint32_t crc = (uint32_t)crc32(0, data.data() + o, (uInt)n), isz = (uint32_t)n;
        fwrite(&crc, 4, 1, f);
        fwrite(&isz, 4, 1, f);
        if (n == 0) break;
    }
    fclose(f);
}

// where every record of an inflated BAM starts (its block_size field); empty when the header does not parse
static std::vector<size_t> record_offsets(const std::vector<uint8_t> &d)
{
    std::vector<size_t> out;
    auto i32 = [&](size_t o) { int32_t v; memcpy(&v, &d[o], 4); return v; };
    if (d.size() < 12 || memcmp(d.data(), "BAM\1", 4) != 0) return out;
    size_t o = 8 + (size_t)i32(4);
    if (o + 4 > d.size()) return out;
    const int32_t n_ref = i32(o);
    o += 4;
    for (int32_t r = 0; r < n_ref; r++) {
        if (o + 4 > d.size()) return out;
        o += 8 + (size_t)i32(o);
    }
    while (o + 36 <= d.size()) {
        const int32_t bs = i32(o);
        if (bs < 32 || o + 4 + (size_t)bs > d.size()) break;
        out.push_back(o);
        o += 4 + (size_t)bs;
    }
    return out;
}

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    std::vector<int32_t> caps;
    for (const char *c = argc > 7 ? argv[7] : "1,3,40"; *c; c += strspn(c, ",")) { caps.push_back(atoi(c)); c += strcspn(c, ","); }
    const char *contig = argv[2];
    const int end_pos = atoi(argv[3]), iters = atoi(argv[4]);
    std::mt19937 rng((unsigned)atoi(argv[5]));
    const char *scratch = argv[6];
    const std::vector<uint8_t> raw = gunzip_all(slurp(argv[1]));
    if (raw.size() < 64) return 3;
    const std::vector<size_t> recs = record_offsets(raw);
    if (recs.empty()) return 3;
    std::vector<uint8_t> region((size_t)end_pos + 1, 1);
    std::vector<int32_t> counts((size_t)4 * (end_pos + 1));
    int ok = 0, err = 0;
    auto decode_capped = [&](int stepper_all) {
        gio_table t;
        for (int32_t cap : caps) {
            if (gio_support_table_from_bam_depth(scratch, contig, 1, end_pos, region.data(), stepper_all, cap, &t) == 0) { ok++; gio_table_free(&t); } else err++;
        }
    };
    // a mapped record in front of position 0 as the first of a file whose other records lie at 0, or buckets behind it
    for (int shift : {0, 40, 5000})
        for (int32_t first : {-1, -3, INT_MIN}) {
            std::vector<uint8_t> d = raw;
            for (size_t r = 0; r < recs.size(); r++) {
                int32_t pos;
                memcpy(&pos, &d[recs[r] + 8], 4);
                pos = r ? pos + shift : first;
                memcpy(&d[recs[r] + 8], &pos, 4);
            }
            bgzf_write(scratch, d, 0xff00);
            gio_table t;
            if (gio_support_table_from_bam(scratch, contig, 1, end_pos, region.data(), 0, &t) == 0) { ok++; gio_table_free(&t); } else err++;
            decode_capped(0);
        }
    for (int it = 0; it < iters; it++) {
        std::vector<uint8_t> d = raw;
        const int kind = (int)(rng() % 6);
        if (kind == 0) d.resize(rng() % d.size());                                    // truncation
        else if (kind == 1) for (int q = 0; q < 1 + (int)(rng() % 8); q++) d[rng() % d.size()] = (uint8_t)rng();       // byte noise
        else if (kind == 2) {                                                          // a length field blown up
            size_t o = 12 + (rng() % (d.size() - 16));
            uint32_t v = (rng() % 2) ? 0x7fffffffu : (uint32_t)rng();
            memcpy(&d[o & ~(size_t)3], &v, 4);
        } else if (kind == 3) {                                                        // name without terminator / huge n_cigar
            for (size_t o = 0; o + 40 < d.size(); o++)
                if (d[o] == 'r' && rng() % 7 == 0) { d[o + 1 + rng() % 6] = 0xff; break; }
        } else if (kind == 4) d.insert(d.begin() + (ptrdiff_t)(rng() % d.size()), (size_t)(rng() % 64), (uint8_t)rng());   // shifted tail
        else {
            // a record's pos (what indexes the cap's start histogram and its histogram of ends): earlier, far later, negative,
            // at and beyond end_pos and the reference's length -- of single records (the file is then out of order) or of every
            // record from one on (it stays in order)
            for (int q = 0; q < 1 + (int)(rng() % 3); q++) {
                const size_t r0 = rng() % recs.size();
                const size_t r1 = (rng() % 3) ? r0 + 1 : recs.size();
                const int how = (int)(rng() % 7);
                const int64_t delta = how == 0 ? -(int64_t)(1 + rng() % 200) : how == 1 ? (int64_t)(1 + rng() % 40) : (int64_t)(70000 + rng() % 100000);
                const int32_t fixed[4] = {-1, -2 - (int32_t)(rng() % 1000), INT_MIN, INT_MAX};
                for (size_t r = r0; r < r1; r++) {
                    int32_t pos;
                    memcpy(&pos, &d[recs[r] + 8], 4);
                    int64_t v = how < 3 ? (int64_t)pos + delta : how == 3 ? (int64_t)end_pos - 2 + (int64_t)(rng() % 5) : fixed[how - 4 + (how == 6 ? (int)(rng() % 2) : 0)];
                    if (v > INT_MAX) v = INT_MAX;
                    if (v < INT_MIN) v = INT_MIN;
                    pos = (int32_t)v;
                    memcpy(&d[recs[r] + 8], &pos, 4);
                }
            }
        }
        bgzf_write(scratch, d, 0xff00 >> (rng() % 6));
        gio_table t;
        const int rc = gio_support_table_from_bam(scratch, contig, 1, end_pos, region.data(), (int)(rng() % 2), &t);
        if (rc == 0) { ok++; gio_table_free(&t); } else err++;
        decode_capped((int)(rng() % 2));
        if (gio_count_coverage(scratch, contig, 0, end_pos, counts.data()) == 0) ok++; else err++;
        int64_t len;
        gio_ref_len(scratch, contig, &len);
    }
    // compressed-stream damage as well
    std::vector<uint8_t> comp = slurp(argv[1]);
    for (int it = 0; it < iters; it++) {
        std::vector<uint8_t> d = comp;
        if (rng() % 2) d.resize(rng() % d.size());
        else for (int q = 0; q < 1 + (int)(rng() % 4); q++) d[rng() % d.size()] ^= (uint8_t)(1u << (rng() % 8));
        FILE *f = fopen(scratch, "wb");
        fwrite(d.data(), 1, d.size(), f);
        fclose(f);
        gio_table t;
        if (gio_support_table_from_bam(scratch, contig, 1, end_pos, region.data(), 0, &t) == 0) { ok++; gio_table_free(&t); } else err++;
    }
    printf("fuzz_bam done: %d ok, %d rejected\n", ok, err);
    return 0;
}
