// assign.hpp -- read assignment: which recovered haplotype every read of the support table supports (gh_assign_reads,
// include/gretel_hip.h; the definition: INTEGRATION.md "Read assignment").  No reference counterpart: Gretel reports the
// haplotypes and their likelihoods only.  Everything here is an integer, so the results do not depend on the order of the
// atomics.
//
//   k_assign_masks  the paths as match masks: bit h % 64 of mask[w][s][c] is set when paths[w * 64 + h][s] is symbol c,
//                   c over the five informative symbols A C G T - (40 bytes per SNP per 64 haplotypes)
//   k_assign        one lane per read, grid-stride.  Per word of 64 haplotypes the masks of the read's informative columns
//                   are added into NP bit-sliced counters (plane p holds bit p of every haplotype's match count, ripple
//                   carry); scanning the planes from the top leaves the best count of the word and its tie set.  The words
//                   are folded into the running best, its lowest haplotype and the tie count; an ambiguous read walks the
//                   words once more to count every haplotype of its tie set.  Per-haplotype counters are summed in LDS
//                   and added to the global int64 counters with one atomic per non-zero entry and workgroup.
//
// Nothing depends on the table being sorted by rank.  Columns past SNP N (or before SNP 1) are skipped, never read.
// ---------------------------------------------------------------------------------------------

#define ASSIGN_BLOCK 256
#define ASSIGN_LDS_MAX_H 4096      /* per-haplotype counters in LDS up to here (16 bytes each: 64 KB); global atomics beyond */

// slot of a support byte among the informative symbols A C G T - (0..4); 5: N or _ (skipped); -1: not a symbol at all
__device__ __forceinline__ int assign_slot(int c)
{
    switch (c) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    case '-': return 4;
    case 'N': case '_': return 5;
    default: return -1;
    }
}

// one thread per (SNP s, word w): rows s = 0 .. N of word w (row 0, the sentinel, stays empty)
__global__ void __launch_bounds__(ASSIGN_BLOCK)
k_assign_masks(const uint8_t *__restrict__ paths, int n_paths, int N, unsigned long long *__restrict__ mask)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const int w = blockIdx.y;
    if (s > N) return;
    unsigned long long m[5] = {0, 0, 0, 0, 0};
    const int h_end = min(n_paths - w * 64, 64);
    if (s > 0) {
        for (int b = 0; b < h_end; b++) {
            const int sym = paths[(size_t)(w * 64 + b) * (size_t)(N + 1) + s];     // lanes: consecutive s of one path row
            const unsigned long long bit = 1ull << b;
            if (sym < 4) m[sym] |= bit;
            else if (sym == 5) m[4] |= bit;
        }
    }
    unsigned long long *o = mask + ((size_t)w * (size_t)(N + 1) + (size_t)s) * 5;
#pragma unroll
    for (int c = 0; c < 5; c++) o[c] = m[c];
}

// the match counts of one word: planes P[0..NP) after adding the masks of every informative column of the read.  Returns
// the best count of the word's valid haplotypes; *ties = the haplotypes that reach it.
template <int NP>
__device__ __forceinline__ int assign_word(const unsigned long long *__restrict__ mw, const uint8_t *__restrict__ s, int k, int snp0,
                                           unsigned long long valid, unsigned long long *ties)
{
    // (s[0 .. k) are the read's columns at SNPs snp0 .. snp0 + k - 1, all inside 1 .. N)
    unsigned long long P[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) P[p] = 0;
    for (int j = 0; j < k; j++) {
        const int slot = assign_slot(s[j]);
        if (slot < 0 || slot > 4) continue;
        unsigned long long carry = mw[(size_t)(snp0 + j) * 5 + slot];
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const unsigned long long t = P[p] & carry;
            P[p] ^= carry;
            carry = t;
        }
    }
    unsigned long long cand = valid;
    int v = 0;
#pragma unroll
    for (int p = NP - 1; p >= 0; p--) {
        const unsigned long long t = cand & P[p];
        if (t) { cand = t; v |= 1 << p; }
    }
    *ties = cand;
    return v;
}

// LDS: per-haplotype counters of the workgroup, unique / shared (uint32) and mismatches (uint64)
template <int NP, bool LDS>
__global__ void __launch_bounds__(ASSIGN_BLOCK)
k_assign(const int32_t *__restrict__ rank, const int64_t *__restrict__ off, const uint8_t *__restrict__ bases, int64_t n_reads,
         const unsigned long long *__restrict__ mask, int n_paths, int N, int min_snps, int max_mismatch,
         unsigned long long *__restrict__ g_unique, unsigned long long *__restrict__ g_shared, unsigned long long *__restrict__ g_mis,
         int32_t *__restrict__ read_hap, int32_t *__restrict__ read_best, int32_t *__restrict__ read_inf,
         unsigned long long *__restrict__ g_tot)
{
    extern __shared__ unsigned long long s_dyn[];
    __shared__ unsigned long long s_tot[5];      // informative, unique, ambiguous, unexplained, reads with a byte outside ACGTN-_
    unsigned long long *s_mis = s_dyn;
    unsigned *s_uni = (unsigned *)(s_dyn + (LDS ? n_paths : 0));
    unsigned *s_sha = s_uni + (LDS ? n_paths : 0);
    if (LDS)
        for (int q = threadIdx.x; q < n_paths; q += blockDim.x) { s_mis[q] = 0; s_uni[q] = 0; s_sha[q] = 0; }
    if (threadIdx.x < 5) s_tot[threadIdx.x] = 0;
    __syncthreads();

    const int nw = (n_paths + 63) / 64;
    const unsigned long long last_valid = (n_paths & 63) ? (1ull << (n_paths & 63)) - 1 : ~0ull;
    unsigned long long n_inf = 0, n_uni = 0, n_amb = 0, n_unx = 0, n_bad = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o0 = off[r];
        const int k = (int)(off[r + 1] - o0);
        const uint8_t *s = bases + o0;
        const int64_t s0 = (int64_t)rank[r] + 1;                       // column j lies at SNP s0 + j
        int I = 0;
        bool bad = false;
        for (int j = 0; j < k; j++) {
            const int slot = assign_slot(s[j]);
            const int64_t snp = s0 + j;
            if (slot < 0) bad = true;
            else if (slot < 5 && snp >= 1 && snp <= N) I++;
        }
        if (bad) n_bad++;
        // the columns inside SNPs 1 .. N: j in [jlo, jhi)
        const int jlo = (int)max((int64_t)0, min((int64_t)k, 1 - s0));
        const int jhi = (int)max((int64_t)jlo, min((int64_t)k, (int64_t)N + 1 - s0));
        const uint8_t *sv = s + jlo;
        const int kv = jhi - jlo, snp0 = (int)(s0 + jlo);
        int best = -1, lo = -1, nties = 0;
        for (int w = 0; w < nw; w++) {
            unsigned long long ties;
            const int v = assign_word<NP>(mask + (size_t)w * (size_t)(N + 1) * 5, sv, kv, snp0, w + 1 < nw ? ~0ull : last_valid, &ties);
            if (v > best) { best = v; lo = w * 64 + __builtin_ctzll(ties); nties = __popcll(ties); }
            else if (v == best) nties += __popcll(ties);
        }
        int hap;
        if (I < min_snps) hap = -1;
        else if (n_paths == 0 || (max_mismatch >= 0 && I - best > max_mismatch)) hap = -3;
        else if (nties > 1) hap = -2;
        else hap = lo;
        if (best < 0) best = 0;                                        // (no haplotype)
        if (I >= min_snps) n_inf++;
        if (hap >= 0) {
            n_uni++;
            if (LDS) { atomicAdd(&s_uni[hap], 1u); atomicAdd(&s_mis[hap], (unsigned long long)(I - best)); }
            else { atomicAdd(&g_unique[hap], 1ull); if (I > best) atomicAdd(&g_mis[hap], (unsigned long long)(I - best)); }
        } else if (hap == -2) {
            n_amb++;
            for (int w = 0; w < nw; w++) {
                unsigned long long ties;
                const int v = assign_word<NP>(mask + (size_t)w * (size_t)(N + 1) * 5, sv, kv, snp0, w + 1 < nw ? ~0ull : last_valid, &ties);
                if (v != best) continue;
                while (ties) {
                    const int h = w * 64 + __builtin_ctzll(ties);
                    ties &= ties - 1;
                    if (LDS) atomicAdd(&s_sha[h], 1u);
                    else atomicAdd(&g_shared[h], 1ull);
                }
            }
        } else if (hap == -3) n_unx++;
        if (read_hap) { read_hap[r] = hap; read_best[r] = best; read_inf[r] = I; }      // (three arrays of one device block)
    }
    if (n_inf) atomicAdd(&s_tot[0], n_inf);
    if (n_uni) atomicAdd(&s_tot[1], n_uni);
    if (n_amb) atomicAdd(&s_tot[2], n_amb);
    if (n_unx) atomicAdd(&s_tot[3], n_unx);
    if (n_bad) atomicAdd(&s_tot[4], n_bad);
    __syncthreads();
    if (threadIdx.x < 5 && s_tot[threadIdx.x]) atomicAdd(&g_tot[threadIdx.x], s_tot[threadIdx.x]);
    if (LDS)
        for (int q = threadIdx.x; q < n_paths; q += blockDim.x) {
            if (s_uni[q]) atomicAdd(&g_unique[q], (unsigned long long)s_uni[q]);
            if (s_sha[q]) atomicAdd(&g_shared[q], (unsigned long long)s_sha[q]);
            if (s_mis[q]) atomicAdd(&g_mis[q], s_mis[q]);
        }
}

// host ----------------------------------------------------------------------------------------
template <int NP>
static void assign_launch(hipStream_t st, unsigned grid, const gh_reads *r, const unsigned long long *mask, int n_paths, int N,
                          int min_snps, int max_mismatch, unsigned long long *cnt, int32_t *rd, unsigned long long *tot)
{
    const int64_t n = r->n_reads;
    int32_t *rh = rd, *rb = rd ? rd + n : nullptr, *ri = rd ? rd + 2 * n : nullptr;
    if (n_paths <= ASSIGN_LDS_MAX_H) {
        const size_t lds = (size_t)n_paths * 16;
        if (lds > 32768) hipFuncSetAttribute((const void *)k_assign<NP, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((k_assign<NP, true>), dim3(grid), dim3(ASSIGN_BLOCK), lds, st, r->rank, r->off, r->bases, n, mask, n_paths, N,
                           min_snps, max_mismatch, cnt, cnt + n_paths, cnt + 2 * (size_t)n_paths, rh, rb, ri, tot);
    } else {
        hipLaunchKernelGGL((k_assign<NP, false>), dim3(grid), dim3(ASSIGN_BLOCK), 0, st, r->rank, r->off, r->bases, n, mask, n_paths, N,
                           min_snps, max_mismatch, cnt, cnt + n_paths, cnt + 2 * (size_t)n_paths, rh, rb, ri, tot);
    }
}

extern "C" int gh_assign_reads(gh_t *h, const gh_reads_t *r, const uint8_t *paths, int n_paths, int min_snps, int max_mismatch,
                               int64_t *unique, int64_t *shared, int64_t *mismatches,
                               int32_t *read_hap, int32_t *read_best, int32_t *read_informative, gh_assign_stats *stats)
{
    if (!h || !r || !stats) return fail(GH_ERR_ARG, "null argument");
    if (n_paths < 0) return fail(GH_ERR_ARG, "n_paths must be >= 0 (got %d)", n_paths);
    if (min_snps < 1) return fail(GH_ERR_ARG, "min_snps must be >= 1 (got %d)", min_snps);
    if (max_mismatch < -1) return fail(GH_ERR_ARG, "max_mismatch must be >= -1 (got %d)", max_mismatch);
    if (n_paths > 0 && (!paths || !unique || !shared || !mismatches)) return fail(GH_ERR_ARG, "null argument");
    const bool per_read = read_hap || read_best || read_informative;
    if (r->dev != h->dev) return fail(GH_ERR_ARG, "reads live on device %d, handle on %d", r->dev, h->dev);
    const int N = h->N;
    const size_t path_bytes = (size_t)n_paths * (size_t)(N + 1);
    int rc = check_symbol_rows(paths, n_paths, (size_t)N + 1, GH_ERR_ARG);
    if (rc) return rc;
    // planes of the bit-sliced counters: enough for the longest read's column count
    int np = 1;
    while (np < 31 && (1ll << np) <= (long long)r->max_k) np++;
    const int NP = np <= 2 ? 2 : np <= 3 ? 3 : np <= 4 ? 4 : np <= 6 ? 6 : np <= 8 ? 8 : np <= 12 ? 12 : np <= 16 ? 16 : 32;
    if (set_dev(h)) return GH_ERR_HIP;

    // one device block, kept on the handle: counters [3][n_paths], totals [8], paths, masks [nw][N+1][5], per-read [3][n_reads]
    // (assign_layout)
    const int nw = (n_paths + 63) / 64;
    if (nw > 65535) return fail(GH_ERR_ARG, "n_paths %d: at most %d", n_paths, 65535 * 64);
    const size_t need = assign_layout(nullptr, n_paths, N, r->n_reads, per_read).total;
    if ((rc = scratch_reserve(h, &h->asg, need, "gh_assign_reads: the scratch of the paths' counters and masks and the per-read results"))) return rc;
    const assign_bufs d = assign_layout(h->asg.buf, n_paths, N, r->n_reads, per_read);
    unsigned long long *cnt = d.cnt, *tot = cnt + 3 * (size_t)n_paths, *mask = d.mask;

    HIPCHK(hipMemsetAsync(cnt, 0, (size_t)3 * n_paths * 8 + 8 * 8, h->stream));
    if (n_paths > 0) {
        HIPCHK(hipMemcpyAsync(d.paths, paths, path_bytes, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_assign_masks, dim3((unsigned)((N + 1 + ASSIGN_BLOCK - 1) / ASSIGN_BLOCK), (unsigned)nw), dim3(ASSIGN_BLOCK), 0,
                           h->stream, d.paths, n_paths, N, mask);
        if ((rc = post_launch(h, "k_assign_masks"))) return rc;
    }
    if (r->n_reads > 0) {
        // eight workgroups of 256 lanes per CU at most; the per-haplotype counters leave each workgroup once
        const unsigned grid = (unsigned)std::min<int64_t>((r->n_reads + ASSIGN_BLOCK - 1) / ASSIGN_BLOCK, 2048);
#define ASSIGN_NP(K_) assign_launch<K_>(h->stream, grid, r, mask, n_paths, N, min_snps, max_mismatch, cnt, d.read, tot)
        switch (NP) {
        case 2: ASSIGN_NP(2); break;
        case 3: ASSIGN_NP(3); break;
        case 4: ASSIGN_NP(4); break;
        case 6: ASSIGN_NP(6); break;
        case 8: ASSIGN_NP(8); break;
        case 12: ASSIGN_NP(12); break;
        case 16: ASSIGN_NP(16); break;
        default: ASSIGN_NP(32); break;
        }
#undef ASSIGN_NP
        if ((rc = post_launch(h, "k_assign"))) return rc;
    }
    unsigned long long htot[8];
    HIPCHK(hipMemcpyAsync(htot, tot, sizeof htot, hipMemcpyDeviceToHost, h->stream));
    if (n_paths > 0) {
        HIPCHK(hipMemcpyAsync(unique, cnt, (size_t)n_paths * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(shared, cnt + n_paths, (size_t)n_paths * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(mismatches, cnt + 2 * (size_t)n_paths, (size_t)n_paths * 8, hipMemcpyDeviceToHost, h->stream));
    }
    if (per_read && r->n_reads > 0) {
        const size_t b = (size_t)r->n_reads * 4;
        if (read_hap) HIPCHK(hipMemcpyAsync(read_hap, d.read, b, hipMemcpyDeviceToHost, h->stream));
        if (read_best) HIPCHK(hipMemcpyAsync(read_best, d.read + r->n_reads, b, hipMemcpyDeviceToHost, h->stream));
        if (read_informative) HIPCHK(hipMemcpyAsync(read_informative, d.read + 2 * r->n_reads, b, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (htot[4]) return fail(GH_ERR_SYMBOL, "gh_assign_reads: %llu read(s) carry a byte outside \"ACGTN-_\"", htot[4]);
    stats->n_reads = r->n_reads;
    stats->n_informative = (int64_t)htot[0];
    stats->n_unique = (int64_t)htot[1];
    stats->n_ambiguous = (int64_t)htot[2];
    stats->n_unexplained = (int64_t)htot[3];
    return GH_OK;
}
