/*
 * gretel_hip.h -- C ABI of libgretel_hip.so, the MI355X (gfx950) implementation of
 * Gretel's hot path: the Hansel SNP-pair co-observation tensor and the three
 * loops that run over it (BAM->Hansel fill, L'th-order Markov path extension,
 * per-path reweighting).
 *
 * The reference has no FFI for this path: its seam is the Python object protocol
 * of `hansel.Hansel` (third-party hanselx==0.0.92, reference setup.py:8) plus
 * two functions of gretel/gretel.py.  Each entry point below names the
 * reference interface it replaces (file:line relative to the reference tree);
 * gretel_amd/hansel.py, gretel_amd/gretel.py and gretel_amd/util.py bind them
 * with ctypes and re-expose the reference's Python names.
 *
 * Conventions
 *   - every function returns GH_OK (0) or a negative gh_status; the message of
 *     the last failure on the calling thread is gh_last_error().
 *   - "no branch at SNP k" (reference gretel/gretel.py:176-180 returns a None
 *     triple) is a VALUE (hole_at >= 1), not an error.
 *   - symbols are indices in the reference's order (gretel/util.py:83):
 *       A=0 C=1 G=2 T=3 N=4 -=5 _=6 ; unsymbols are N and _.
 *   - positions are 0..n_snps+1 (0 and n_snps+1 are the sentinels).
 *   - a handle owns its device buffers and one HIP stream; it is not
 *     thread-safe; one handle per (contig,start,end) window.
 *   - all output buffers are caller-allocated host memory unless stated.
 */
#ifndef GRETEL_HIP_H
#define GRETEL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gh_handle gh_t;          /* one Hansel tensor resident in HBM */
typedef struct gh_reads gh_reads_t;     /* one support table resident in HBM */

typedef enum {
    GH_OK = 0,
    GH_ERR_ARG = -1,        /* bad argument */
    GH_ERR_HIP = -2,        /* HIP runtime failure (no device, launch error, ...) */
    GH_ERR_BAND = -3,       /* observation with pos_to-pos_from outside [1, band] */
    GH_ERR_SYMBOL = -4,     /* byte that is not one of "ACGTN-_" in a support_seq */
    GH_ERR_NOMEM = -5,
    GH_ERR_STATE = -6       /* call order (e.g. generate_path before any fill) */
} gh_status;

#define GH_NSYM 7
#define GH_STORAGE_F32 0
#define GH_STORAGE_F64 1
#define GH_COND_A 0   /* (1+H[a,b,i,j]) / (V(j) + sum_x H[a,x,i,j])   frozen default */
#define GH_COND_B 1   /* (1+H[a,b,i,j]) / (V(i) + c_a(i))                            */
#define GH_COND_C 2   /* (1+H[a,b,i,j]) / (V(i) + sum_x H[x,b,i,j])                  */
#define GH_COND_D 3   /* (1+H[a,b,i,j]) / (V(i) + sum_x H[a,x,i,j])   the reading of gretel.py:10's TODO with V at pos_from */
#define GH_COND_E 4   /* (1+H[a,b,i,j]) / (V(j) + sum_x H[x,b,i,j])   C with the "unique variants" term at pos_to       */
/* (C and E read a cell as P(a at i | b at j): the earlier variant given the candidate -- the naive-Bayes form of the
 * published method, reference README.md:79-94; A and D read it as P(b at j | a at i); B conditions on c_a(i).) */

typedef struct {
    int32_t n_snps;         /* N: number of SNPs of the window (VCF_h["N"], gretel/util.py:409) */
    int32_t band;           /* W: largest pos_to-pos_from stored (= max SNPs on a read - 1, >= 1) */
    int32_t storage;        /* GH_STORAGE_F32 | GH_STORAGE_F64 */
    int32_t cond_mode;      /* GH_COND_*  */
    int32_t marginal_term;  /* 1: edge weight also adds log10(marginal) (App. A-7) */
    int32_t device;         /* HIP device ordinal, -1 = current */
    int32_t offer_zero;     /* 1: get_edge_weights_at offers every valid symbol, also those with a zero count at the position (App. A-4/5) */
    uint8_t cand_order[8];  /* [0..4]: the order the candidates are offered in = dict insertion order of get_edge_weights_at =
                             * the tie-break of gretel/gretel.py:166-174 (first key wins); a permutation of the valid symbol
                             * indices {0,1,2,3,5}.  All zero = the default A C G T - (symbol index order). */
} gh_config;

typedef struct {
    int64_t n_slices;       /* reads with >1 SNP            gretel/util.py:233,329 */
    int64_t n_crumbs;       /* pair observations            gretel/util.py:268,276,281,330 */
    int64_t covered_snps;   /* informative SNPs on them     gretel/util.py:239 */
    int32_t L;              /* ceil(covered/slices)         gretel/util.py:333 */
    int32_t _pad;
} gh_fill_stats;

typedef struct {
    double hp_current;      /* gretel/gretel.py:185,189 */
    double hp_original;     /* gretel/gretel.py:186,189 */
    double ratio;           /* min marginal after the 1% clamp, gretel/cmd.py:157-160 */
    double magnitude;       /* reweight_hansel_from_path return, gretel/cmd.py:161 */
    double min_marginal;    /* generate_path's third return value before the clamp (the "%.10f too small" note, cmd.py:158-160) */
} gh_path_rec;

const char *gh_last_error(void);
int gh_device_count(int *n);
/* peak shader clock of a device in kHz (bench.py prices its instruction-issue floors with it) */
int gh_device_clock_khz(int device, int *khz);

/* log10 as every kernel evaluates it: include/gh_detlog.h, glibc's log10 restated so that the arg-max of
 * gretel/gretel.py:159-174 and the sums of gretel/gretel.py:185-186 see the very doubles math.log10 (gretel/gretel.py:2)
 * gives the reference.  gh_log10_device runs it on the GPU over an array, gh_log10_host is the same source compiled
 * for the host (touches no device): the tests hold both to the running libm. */
int gh_log10_device(int device, const double *x, double *y, int64_t n);
int gh_log10_host(const double *x, double *y, int64_t n);

/* Hansel.init_matrix(['A','C','G','T','N','-','_'], ['N','_'], N) -- gretel/util.py:83.
 * Allocates the zeroed banded tensor [(N+2)][band][7][7] in HBM. */
int gh_create(const gh_config *cfg, gh_t **out);
int gh_destroy(gh_t *h);
/* hansel.copy() -- gretel/cmd.py:79 (deep copy incl. L, n_slices, n_crumbs). */
int gh_copy(const gh_t *src, gh_t **out);
/* zero the tensor and the fill counters (re-use a handle for another window of the same shape) */
int gh_clear(gh_t *h);
int gh_sync(gh_t *h);

/* hansel.L / n_slices / n_crumbs attributes -- gretel/util.py:329-333, gretel/cmd.py:227-229 */
int gh_set_L(gh_t *h, int32_t L);
int gh_get_L(const gh_t *h, int32_t *L);
int gh_get_fill_stats(const gh_t *h, gh_fill_stats *out);
int gh_set_fill_stats(gh_t *h, const gh_fill_stats *in);

/* Support table (per read: rank of gretel/util.py:198, support_seq of util.py:238 as ASCII)
 * copied to HBM once; off has n_reads+1 entries.  The arrays may lie in page-locked memory (gh_host_alloc): they are then read
 * by DMA instead of through a staging copy.  GH_ERR_ARG when off[] runs backwards somewhere. */
int gh_reads_upload(const gh_t *h, const int32_t *rank, const int64_t *off, const uint8_t *bases,
                    int64_t n_reads, gh_reads_t **out);
int gh_reads_free(gh_reads_t *r);
/* the longest read of an uploaded table (max of off[q + 1] - off[q]; found on the device behind the upload): a matrix needs a band
 * of at least max_k - 1 to take it */
int gh_reads_max_k(const gh_reads_t *r, int32_t *max_k);
/* What the upload found out about the table (for the tests; the fills choose their kernel and their counter width by it):
 * info[0] longest read, [1] 1 when the ranks ascend, [2] the widest run of positions a block of 2048 reads covers + longest read + 1,
 * [3] the most reads whose ranks fall into 128 consecutive positions, [4] entries of first_at (0: none); the last three are 0 for
 * a table whose ranks do not ascend.  first_at (may be NULL): room for info[4] entries, first_at[p] = the first read whose
 * rank is >= p -- call once with NULL for the count. */
int gh_reads_info(const gh_reads_t *r, int64_t info[5], int64_t *first_at);

/* The per-read pair loop of load_from_bam -- gretel/util.py:226-286 -- and the
 * counters/L of util.py:329-333, over a device-resident support table.
 * Accumulates into the tensor (call gh_clear first for a fresh fill). */
int gh_fill(gh_t *h, const gh_reads_t *reads, int use_end_sentinels, gh_fill_stats *out);

/* hansel.add_observation / get_observation / reweight_observation --
 * gretel/util.py:266-286, tests/test_test.py:41-52, gretel/gretel.py:84,96.
 * One-cell compatibility API (a host round trip each): not the fast path. */
int gh_add(gh_t *h, int a, int b, int i, int j);
int gh_add_batch(gh_t *h, const uint8_t *a, const uint8_t *b, const int32_t *i, const int32_t *j, int64_t n);
int gh_get(gh_t *h, int a, int b, int i, int j, double *out);
int gh_reweight_obs(gh_t *h, int a, int b, int i, int j, double ratio, double *removed);

/* hansel.get_counts_at(p) -- gretel/cmd.py:86,127: out[s] = c_s(p), out[7] = total. */
int gh_counts_at(gh_t *h, int p, double out[8]);
/* hansel.get_marginal_of_at(s, p) -- gretel/gretel.py:182,186 */
int gh_marginal_of_at(gh_t *h, int s, int p, double *out);
/* hansel.get_edge_weights_at(p, current_path) -- gretel/gretel.py:155.
 * path[0..p-1] are the selected symbol indices (path[0] = '_'); w[s] is set for
 * the candidate symbols, *cand_mask has bit s set for each candidate. */
int gh_edge_weights_at(gh_t *h, int p, const uint8_t *path, double w[GH_NSYM], int *cand_mask);
/* the gap check of gretel/cmd.py:85-118: first position in [0,N] whose total is 0, else -1 */
int gh_gap_check(gh_t *h, int *first_gap);

/* candidate bitmask per position (bit s set <=> valid symbol s has c_s(p) > 0), out[0..N] */
int gh_export_cmask(gh_t *h, uint32_t *out);

/* Freeze the current marginals as the "original" ones: what gretel/cmd.py:79's
 * hansel.copy() is used for at gretel/gretel.py:186 (M0[p][s] replaces a second tensor). */
int gh_snapshot_original(gh_t *h);

/* gretel.generate_path(n_snps, hansel, original_hansel) -- gretel/gretel.py:102-189.
 * `original` may be NULL (then h's snapshot, or h itself if none was taken).
 * path_out: N+1 symbol indices, path_out[0] = '_'.  *hole_at = 0 on success, else the
 * SNP at which no branch could be selected (gretel.py:176-180); then path_out[0..hole_at-1]
 * holds the prefix walked so far and the three doubles are not written. */
int gh_generate_path(gh_t *h, const gh_t *original, uint8_t *path_out,
                     double *hp_current, double *hp_original, double *min_marginal, int *hole_at);

/* gretel.reweight_hansel_from_path(hansel, path, ratio) -- gretel/gretel.py:79-98. */
int gh_reweight_path(gh_t *h, const uint8_t *path, double ratio, double *removed);

/* The spin loop of gretel/cmd.py:148-179 without host round trips: up to max_paths x
 * { generate_path, clamp ratio to >= min_remove (cmd.py:157-160), reweight }.
 * Stops at the first hole (cmd.py:153).  paths_out: [max_paths][N+1]. */
int gh_spin(gh_t *h, int max_paths, double min_remove, uint8_t *paths_out, gh_path_rec *recs,
            int *n_out, int *hole_at);

/* Batched recovery: the spin loop of gretel/cmd.py:148-179 over MANY windows of one shape (same n_snps, band, storage,
 * modes, device and L).  From two dozen windows on and at 2..10 lags -- under every conditional, with or without the marginal
 * term -- every window is carried through ALL its paths by one persistent workgroup (gretel_amd/csrc/wpipe.hpp):
 * the reweight of path s-1 (gretel/gretel.py:79-98) sweeps through the tensor a few chunks ahead of the walk of path s
 * (gretel/gretel.py:143-189), one launch per batch, 256 windows at a time on one MI355X.  Otherwise (and for windows the
 * pipeline cannot carry: a position with five candidates, a hole) every kernel of a path is launched over all windows --
 * one path-extension workgroup per window.  The handles stay usable on their own; fill them first.
 * paths_out: [n][max_paths][N+1], recs: [n][max_paths], n_out/hole_at: [n]. */
/* Page-locked host memory for result buffers (paths_out / recs of gh_spin and gh_batch_spin accept any host memory; into pinned
 * memory the copies run at the link's rate and without a staging pass -- 256 windows x 100 paths are 256 MB).  No reference
 * counterpart: the reference keeps its paths in Python lists (gretel/cmd.py:148-179). */
int gh_host_alloc(size_t bytes, void **out);
int gh_host_free(void *p);

typedef struct gh_batch gh_batch_t;
int gh_batch_create(gh_t **handles, int n, gh_batch_t **out);
int gh_batch_destroy(gh_batch_t *b);
int gh_batch_spin(gh_batch_t *b, int max_paths, double min_remove, uint8_t *paths_out, gh_path_rec *recs,
                  int *n_out, int *hole_at);
/* HIP-event timing of the batched kernels (bench.py's roofline of the throughput mode): every = k > 0 brackets the batched
 * launches of every k-th path of the FIRST window group on its stream (0 = off); the pipeline's one launch is bracketed as
 * a whole and reported under GH_K_WALK (bytes: extension + reweight of all its paths).  gh_batch_profile_get: kernel GH_K_WALK
 * (the batched serial extension) or GH_K_REWEIGHT (the fused reweight k_marg<T,true>) of the last gh_batch_spin --
 * milliseconds summed over the sampled launches, their number, the windows one such launch covers, and the algorithmic
 * bytes per launch (per window x windows; the definitions of DESIGN.md section 3). */
/* the last gh_batch_spin: out[0] = windows the pipeline carried, out[1] = of those, windows it handed back to gh_spin before
 * their last path (a candidate mask moved under a reweight), out[2] = threads per pipeline workgroup, out[3] = positions per
 * chunk of its walker tables (0, 0 when it did not run) */
int gh_batch_pipe_info(gh_batch_t *b, int32_t out[4]);
int gh_batch_profile_enable(gh_batch_t *b, int every);
int gh_batch_profile_get(gh_batch_t *b, int kernel, double *total_ms, int64_t *launches, int32_t *windows, double *bytes_per_launch);

/* Panels: a batch whose windows may differ in n_snps, band and L -- one region (gene) per window.  gh_panel_create makes the
 * checks of gh_batch_create except for n_snps and band.  gh_panel_spin runs the windows in one group per L: every group the window
 * pipeline can carry (as gh_batch_spin decides it, over the group's own windows) is carried by it, up to four groups at a time on
 * the batch's streams; whatever it does not carry is finished by gh_spin window by window.  Each window's results are those of
 * gh_spin on that window alone, bit for bit.  Window w's paths are [max_paths][N_w + 1] at paths_out + paths_off[w];
 * recs: [n][max_paths], n_out / hole_at: [n] as in gh_batch_spin.  gh_batch_destroy, gh_batch_pipe_info (windows summed over the
 * groups; threads and chunk of the largest launch) and gh_batch_profile_* take a panel; gh_batch_spin refuses one. */
int gh_panel_create(gh_t **handles, int n, gh_batch_t **out);
int gh_panel_spin(gh_batch_t *b, int max_paths, double min_remove, uint8_t *paths_out, const int64_t *paths_off,
                  gh_path_rec *recs, int *n_out, int *hole_at);

/* Read assignment (no reference counterpart: Gretel reports haplotypes and likelihoods only; INTEGRATION.md "Read assignment").
 * Every read of an uploaded support table against n_paths >= 0 haplotypes, paths = [n_paths][N + 1] symbol indices (rows of
 * gh_spin's paths_out; index 0, the '_' sentinel, is ignored).  Column j of read r lies at SNP rank[r] + j + 1; it is informative
 * when its symbol is one of A C G T - and the SNP lies in 1..N (N, '_' and columns outside are skipped).  I = informative columns,
 * m_h = those where paths[h] carries the read's symbol, best = max_h m_h (0 when n_paths = 0), T = {h : m_h = best}.  In this order:
 * I < min_snps: uninformative (hap -1); max_mismatch >= 0 and I - best > max_mismatch, or n_paths = 0: unexplained (-3);
 * |T| > 1: ambiguous (-2, shared[h] += 1 for every h in T); else unique (hap = h, unique[h] += 1, mismatches[h] += I - best).
 * unique / shared / mismatches: [n_paths]; read_hap / read_best / read_informative: [n_reads] each, each may be NULL.
 * GH_ERR_ARG for n_paths < 0, min_snps < 1, max_mismatch < -1, a path byte above 6, or reads on another device than h;
 * GH_ERR_SYMBOL when a read holds a byte outside "ACGTN-_"; GH_ERR_NOMEM when the device scratch cannot be had (the message
 * names its size).  Reads the table and the paths only: the tensor, L, the fill
 * statistics and the snapshot stay as they are.  All integers: the results do not depend on the order of the device's atomics. */
typedef struct {
    int64_t n_reads;        /* reads in the table */
    int64_t n_informative;  /* I >= min_snps */
    int64_t n_unique;
    int64_t n_ambiguous;
    int64_t n_unexplained;
} gh_assign_stats;
int gh_assign_reads(gh_t *h, const gh_reads_t *reads, const uint8_t *paths, int n_paths, int min_snps, int max_mismatch,
                    int64_t *unique, int64_t *shared, int64_t *mismatches,
                    int32_t *read_hap, int32_t *read_best, int32_t *read_informative,
                    gh_assign_stats *stats);

/* Scoring given haplotypes (gretel/gretel.py:11 "TODO Util to parse known input and return SNP seq" is as far as the reference
 * goes; INTEGRATION.md "Scoring haplotypes").  paths = [n_paths][N + 1] symbol indices, rows as gh_spin writes them (index 0,
 * the '_' sentinel, is ignored: the history reads '_' there).  With L, the conditional, the marginal term, the candidate order and
 * offer_zero of the handle, at every position p = 1..N of a path x: cm(p) and w_p[s] are what gh_edge_weights_at(h, p, x, ...)
 * returns -- the history is x's own, any symbol 0..6 may sit in it; pick(p) is the candidate gh_generate_path would take (the
 * first of cand_order, replaced only by a strictly larger weight; 255 when cm(p) is empty).  p is ON when x[p] is in cm(p): then
 * weight(p) = w_p[x[p]] and margin(p) = weight(p) - max of the other candidates' weights (+inf when there is none; > 0: the walk
 * follows the path here, < 0: it leaves it, 0: a tie, which cand_order decides).  OFF (x[p] is N, '_', an allele not offered
 * at p, or p is a hole): weight(p) = margin(p) = -inf.  Per path, over the ON positions only, in ascending p, as sequential
 * binary64 additions from 0.0 (the order of gretel/gretel.py:185-186): ll_chain = sum of weight(p) -- the quantity the walk
 * maximises step by step; hp_current = sum of log10 marginal(x[p], p); hp_original = the same under the snapshot of
 * gh_snapshot_original (the current marginals when none was taken); min_marginal = the smallest current marginal (+inf when
 * nothing is on); min_margin / argmin_margin = the smallest margin and the first position that has it (+inf / 0 when nothing is
 * on); n_on; n_greedy = on positions with x[p] == pick(p); first_off = the first off position
 * (0: none).  Scoring the path of gh_generate_path on the tensor it came from gives n_greedy == n_on == N, every margin >= 0 and
 * its hp_current, hp_original and min_marginal bit for bit.
 * recs: [n_paths]; weight / margin / pick: [n_paths][N + 1], each may be NULL; pick[.][0] = 6, weight[.][0] = margin[.][0] = 0.
 * GH_ERR_ARG for a null h, paths or recs or n_paths < 0; n_paths == 0 returns GH_OK and writes nothing; GH_ERR_SYMBOL for a path
 * byte above 6; GH_ERR_STATE before any fill, add or import; GH_ERR_NOMEM when the device scratch cannot be had (the message
 * names its size).  Reads the tensor only: the band, L, the fill statistics, the
 * snapshot and the results of a following gh_spin stay as they are.  The device scratch is bounded whatever n_paths is (the paths
 * go through in slabs). */
typedef struct {
    double ll_chain, hp_current, hp_original, min_marginal, min_margin;
    int32_t n_on, n_greedy, first_off, argmin_margin;
} gh_score_rec;
int gh_score_paths(gh_t *h, const uint8_t *paths, int n_paths, gh_score_rec *recs,
                   double *weight, double *margin, uint8_t *pick);

/* Beam search over the chain likelihood (no reference counterpart; INTEGRATION.md "Beam search").  gh_generate_path keeps, at
 * each SNP, the one candidate of largest edge weight; a beam of width B, 1 <= B <= GH_BEAM_MAX, keeps the B best path prefixes by
 * their summed weight -- the ll_chain of gh_score_paths -- over the same weights.  An opt-in search and a diagnostic (is there a
 * path of higher chain likelihood that the greedy walk missed?), not a better default.  With the handle's L, conditional, marginal
 * term and candidate order:
 *   A hypothesis is a path prefix x[0..p], x[0] = '_', and a score.  At p = 0 there is one, of score +0.0.
 *   Step p = 1..N: cm(p) is the candidate set of p (it does not depend on the history).  Empty: the search stops, hole_at = p
 *   (below).  Otherwise every hypothesis of rank k = 0..n-1 spawns one child per c in cm(p), of weight w = w_p[c | x_k] -- what
 *   gh_edge_weights_at(h, p, x_k, ...) returns for c bit for bit: the marginal term first, then lags 1, 2, ... in that order --
 *   and score score_k + w, one binary64 addition.
 *   The children are put in a total order by (1) score descending, (2) parent rank ascending, (3) w descending, (4) index of c in
 *   cand_order ascending; comparisons are plain IEEE > and ==, so equal -inf scores tie.  The first min(B, #children) become
 *   the hypotheses of ranks 0, 1, ... at step p.  (For one parent this is "the first of cand_order, replaced only by a
 *   strictly larger weight": fl(s + .) is monotone, and equal sums fall back to w, then to the order.  Hence B = 1 is
 *   gh_generate_path.)
 *   Result: the n_out hypotheses alive at p = N in rank order: their paths [n_out][N + 1] (index 0 = 6, '_') and scores
 *   ll_chain[n_out], each the sequential sum from 0.0 in ascending p, so equal to gh_score_paths(...).ll_chain of that path bit
 *   for bit, with n_on == N.  Distinct hypotheses are distinct paths; hypotheses that share their last L symbols are NOT merged.
 *   Hole: n_out = 0, hole_at = p, ll_chain is not written; row 0 of paths_out, indices [0..p-1], holds the prefix of the rank-0
 *   hypothesis at step p - 1 (at B = 1 what gh_generate_path leaves).
 * GH_ERR_ARG for a null h, paths_out, n_out or hole_at (gh_beam_spin: recs too), a width outside 1..GH_BEAM_MAX, max_paths < 0,
 * min(L, N) > 2048 (the histories live in on-chip memory), or a handle created with offer_zero: a zero-count candidate can weigh
 * NaN (-inf + +inf), which no order ranks.  GH_ERR_STATE before any fill, add or import.  GH_ERR_NOMEM when the scratch cannot be
 * had: the beam builds its own conditional table in a block of the handle that GROWS WITH N * L -- N * (30 L + 6) * 8 bytes (12 MB
 * at 10k SNPs and L = 5, 134 MB at 50k and L = 11), kept until gh_destroy.
 * gh_beam_paths only reads the tensor: the band, L, the fill statistics, the snapshot, the handle's conditional tables and the
 * results of a following gh_spin stay as they are, bit for bit.
 * gh_beam_spin is the recovery loop of gretel/cmd.py:148-179 with the beam's rank-0 path in place of generate_path: per path, run
 * the beam; hp_current, hp_original (under the snapshot, taken now if there is none) and min_marginal of that path as
 * gh_score_paths gives them on the tensor at that moment; ratio = max(min_marginal, min_remove); magnitude = the removed mass of
 * gh_reweight_path; it stops at the first hole, as gh_spin does.  ll_chain[s] = the beam score of path s.  A host loop over
 * those pieces, one beam launch sequence and two host round trips per path: NOT the throughput path (that is gh_spin).  At
 * width 1 its results are gh_spin's.
 * gh_beam_info, the last beam run on the handle: out[0] = 1 if the table slice was staged through on-chip memory (LDS), 0 if it
 * was read from global memory (L >= 19); out[1] = source positions the LDS ring holds (it is refilled one position per step;
 * 0 if not staged); out[2] = threads of the walk workgroup; out[3] = bytes of the beam's device scratch. */
#define GH_BEAM_MAX 32
int gh_beam_paths(gh_t *h, int width, uint8_t *paths_out /*[width][N+1]*/, double *ll_chain /*[width], may be NULL*/,
                  int *n_out, int *hole_at);
int gh_beam_spin(gh_t *h, int width, int max_paths, double min_remove, uint8_t *paths_out /*[max_paths][N+1]*/,
                 gh_path_rec *recs, double *ll_chain /*[max_paths], may be NULL*/, int *n_out, int *hole_at);
int gh_beam_info(const gh_t *h, int64_t out[4]);

/* Exact decoding of the chain likelihood (no reference counterpart; INTEGRATION.md "Exact decoding").  The beam can only say that a
 * better path than the greedy one exists; this says what the best one is.  Notation as above: cm(p) the candidate set at SNP p,
 * w_p(c | x) the weight gh_edge_weights_at(h, p, x, ...) returns for c (the marginal term first, then lags 1, 2, ... in that
 * order), q(c) the index of c in the handle's cand_order, Le = min(L, N).
 *   A full path x has x[0] = '_' and x[p] in cm(p) for p = 1..N.  score(x) is the sequential binary64 sum of w_p(x[p] | x) in
 *   ascending p from +0.0: exactly the ll_chain of gh_score_paths(x).
 *   Result: ll = the maximum of score(x) over all full paths, attained exactly: a weight depends on the last Le picks only, so the
 *   chain likelihood is a Markov score of order Le, and fl(a + w) is monotone in a -- keeping the best prefix per state (the last
 *   Le picks) loses nothing.
 *   Tie rule: the path returned is the one this procedure keeps.  After step p two prefixes compete when they agree on positions
 *   p-Le+1..p.  For p > Le they then differ at position p-Le: they are taken in ascending q(x[p-Le]); the first stays and is
 *   replaced only by a strictly larger score (plain IEEE >; the arg-max rule of gretel/gretel.py:159-174).  For p <= Le nothing
 *   competes.  At p = N the surviving prefixes are taken in ascending lexicographic order of (q(x[N]), q(x[N-1]), ...,
 *   q(x[N-Le+1])); the first stays unless strictly beaten.
 *   Hole: at the first p with empty cm(p), hole_at = p and neither path nor score is written.  Otherwise hole_at = 0.
 *   State space: U = the union over p = 1..N of the candidate symbols offered, S = |U| (4 in a window without deletion columns);
 *   the states number S^Le.  The decoder serves S^Le <= GH_VITERBI_MAX_STATES: L <= 6 without deletion columns, L <= 5 with them,
 *   L <= 12 in biallelic windows -- 4096 is the largest power of four whose two score rows (64 KB) leave the table ring room in
 *   on-chip memory.  Beyond it the call is refused; the beam remains the tool for larger L.
 * GH_ERR_ARG for a null argument (ll_chain of gh_viterbi_spin may be NULL), max_paths < 0, a handle created with offer_zero (a
 * zero-count candidate can weigh NaN, which no order ranks) or S^Le > GH_VITERBI_MAX_STATES (the message names S, Le and the
 * count).  GH_ERR_STATE before any fill, add or import.  GH_ERR_NOMEM when the scratch cannot be had: a block of the handle of
 * its own, kept until gh_destroy -- the beam's table, N * (30 Le + 6) * 8 bytes, and one back-pointer byte per position and
 * state, (N + 1) * S^Le bytes (10 MB at 10k SNPs and 1024 states, 41 MB at 4096).
 * gh_viterbi_path only reads the tensor: the band, L, the fill statistics, the snapshot, the handle's conditional tables and the
 * results of a following gh_spin stay as they are, bit for bit.
 * gh_viterbi_spin is gh_beam_spin with the exact path in place of the beam's rank-0 path: per path, decode; hp_current,
 * hp_original (under the snapshot, taken now if there is none) and min_marginal as gh_score_paths gives them on the tensor at
 * that moment; ratio = max(min_marginal, min_remove); magnitude = the removed mass of gh_reweight_path; it stops at the first
 * hole.  ll_chain[s] = the exact maximum when path s was found.  A host loop, NOT the throughput path.
 * gh_viterbi_info, the last decoding on the handle: out[0] = S, out[1] = Le, out[2] = states = S^Le, out[3] = bytes of the
 * decoder's device scratch (all 0 before the first). */
#define GH_VITERBI_MAX_STATES 4096
int gh_viterbi_path(gh_t *h, uint8_t *path_out /*[N+1]*/, double *ll_chain, int *hole_at);
int gh_viterbi_spin(gh_t *h, int max_paths, double min_remove, uint8_t *paths_out /*[max_paths][N+1]*/,
                    gh_path_rec *recs, double *ll_chain /*[max_paths], may be NULL*/, int *n_out, int *hole_at);
int gh_viterbi_info(const gh_t *h, int64_t out[4]);
/* S, Le and S^Le (saturating at INT64_MAX) of the tensor as it stands, without decoding: out[0..2].  The refusals are those of
 * gh_viterbi_path short of the cap (a null argument, offer_zero, no fill yet); the count comes back GH_OK however large it is, so
 * a caller can tell beforehand which windows the decoder serves.  Only the handle's marginal tables are brought up to date. */
int gh_viterbi_states(gh_t *h, int64_t out[3]);

/* Exact decoding on the grid (INTEGRATION.md "Exact decoding on the grid"): the decoder above keeps its two score rows in the
 * on-chip memory of one workgroup, hence its cap; the fill's own L = ceil(mean SNPs per read) is often beyond it (L = 10 on a
 * window of 60 SNPs: 4^10 or 5^10 states).  The grid decoder is a second exact decoder under the SAME definition -- score, tie
 * rule during the walk, tie rule at the end, hole rule, the refusal of offer_zero, every addition in the same order -- with the
 * score rows in device memory and one kernel launch per SNP, each a grid over the states.  No workgroup waits for another; the
 * launch boundary is the only synchronisation.  It serves S^Le <= GH_VITERBI_GRID_MAX_STATES = 2^24 = 4^12 (5^10 lies below it;
 * with S >= 2 that bounds Le at 24).
 *   Where both serve a window, path, ll_chain and hole_at of gh_viterbi_path_grid equal gh_viterbi_path's bit for bit, under every
 *   spec and candidate order, also where every path scores +inf (conditionals C and D) or -inf.  The grid calls always run the
 *   grid kernels, also on a window of 64 states (where the launch per SNP costs more than the other decoder's whole step).
 *   gh_viterbi_spin_grid is gh_viterbi_spin with the grid decoding per path.
 * The refusals are gh_viterbi_path's with this cap in place of that one: GH_ERR_ARG for a null argument (ll_chain of the spin may
 * be NULL), max_paths < 0, offer_zero, or S^Le > GH_VITERBI_GRID_MAX_STATES (the message names S, Le, the count and the cap, and
 * points to the beam; nothing is allocated for such a window).  GH_ERR_STATE before any fill.  GH_ERR_NOMEM names the bytes.  The
 * scratch is the exact decoder's block of the handle, kept until gh_destroy: the table, N * (30 Le + 6) * 8 bytes, one
 * back-pointer byte per position and state, (N + 1) * S^Le bytes, and two score rows, 16 * S^Le bytes -- 0.08 GB at 60 SNPs and
 * 4^10 states, 0.75 GB at 5^10, 168 GB at 10k SNPs and the cap: ask gh_viterbi_states first.  A hole is found on the host, from
 * the candidate bits, before any of that is reserved.
 * The calls only read the tensor (the spin reweights it as gh_viterbi_spin does); gh_viterbi_info is not touched.
 * gh_viterbi_grid_info, the last grid call on the handle: out[0] = S, out[1] = Le, out[2] = states = S^Le, out[3] = bytes of
 * the scratch it reserved (all 0 before the first). */
#define GH_VITERBI_GRID_MAX_STATES 16777216
int gh_viterbi_path_grid(gh_t *h, uint8_t *path_out /*[N+1]*/, double *ll_chain, int *hole_at);
int gh_viterbi_spin_grid(gh_t *h, int max_paths, double min_remove, uint8_t *paths_out /*[max_paths][N+1]*/,
                         gh_path_rec *recs, double *ll_chain /*[max_paths], may be NULL*/, int *n_out, int *hole_at);
int gh_viterbi_grid_info(const gh_t *h, int64_t out[4]);

/* Max-marginals of the chain likelihood (no reference counterpart; INTEGRATION.md "Max-marginals").  gh_score_paths' margin says
 * what one greedy step would have lost with the history held fixed; this says, for every SNP p and every candidate c, the best
 * chain likelihood of ANY full path that takes c at p -- everything else free to re-optimise around the choice.  Notation as in
 * "Exact decoding" above.  A state at p is the last min(Le, p) picks; it is reachable where each of its picks is offered at its
 * position.
 *   Forward.  F_0(()) = +0.0.  F_p(s) = the maximum over the reachable predecessors s' of  F_{p-1}(s') + w_p(newest(s) | s'):  one
 *   binary64 addition, plain >.  (The scores the exact decoder keeps per state.)
 *   Backward.  B_N(s) = +0.0 for every reachable s.  For p < N, B_p(s) = the maximum over c in cm(p+1) of
 *   w_{p+1}(c | s) + B_{p+1}(s.c):  one addition, the weight on the left, w summed in the definition's order (the marginal term,
 *   then lags 1, 2, ..., Le) before it meets B.
 *   Max-marginal.  For p = 1..N and c in cm(p):  M[p][c] = the maximum of  F_p(s) + B_p(s)  -- one addition -- over the reachable
 *   states s at p whose newest pick is c.  A maximum of doubles does not depend on the order and there are no NaNs (offer_zero is
 *   refused), so there is no tie rule.  -inf is a value like any other.
 *   Exactness.  fl(+) is monotone in each argument, so M[p][c] equals, bit for bit, the maximum over all full paths x with
 *   x[p] = c of fl(fwd_p(x) + bwd_p(x)):  fwd_p the sequential sum of w_1 .. w_p in ascending order from +0.0;  bwd_p from +0.0,
 *   b <- w_t + b for t = N down to p + 1.
 *   Output.  mm[N+1][7] by symbol index: entries of symbols not offered at p are -inf, row 0 is all -inf.  cm[N+1]: the candidate
 *   bits over the seven symbols (bit s = symbol s offered), which tell an offered -inf from "not offered"; cm[0] = 0.  Hole: at
 *   the first p with empty cm(p), hole_at = p and neither mm nor cm is written.  Otherwise hole_at = 0.
 *   Hence  max_c mm[N][c] == gh_viterbi_path's ll_chain  exactly (B_N = +0.0), and every finite entry lies within N * 2^-52 * A of
 *   the sequentially summed maximum gh_score_paths would give over the paths through (p, c), A the largest sum of |w_t| over
 *   full paths (two summation orders of N terms); an entry is -inf exactly where that maximum is.
 * The refusals are gh_viterbi_path's: GH_ERR_ARG for a null argument, offer_zero, or more than GH_VITERBI_MAX_STATES states (the
 * same message); GH_ERR_STATE before any fill.  GH_ERR_NOMEM names the size of the scratch, which is the exact decoder's block of
 * the handle (kept until gh_destroy) and here holds the table, ONE stored row of S^Le doubles per position -- N * S^Le * 8 bytes,
 * 82 MB at 10k SNPs and 1024 states, 328 MB at 4096; it is not bounded by checkpointing -- and mm and cm.  The forward walk stores
 * F there, the backward walk puts F + B over it, a parallel kernel takes the maxima.
 * It only reads the tensor: the band, L, the fill statistics, the snapshot, the handle's conditional tables and the results of a
 * following gh_spin stay as they are, bit for bit.  gh_viterbi_info afterwards describes this call: S, Le, states, scratch bytes. */
int gh_viterbi_marginals(gh_t *h, double *mm /*[N+1][7]*/, uint8_t *cm /*[N+1]*/, int *hole_at);

/* Max-marginals on the grid (INTEGRATION.md "Max-marginals on the grid"): gh_viterbi_marginals under the grid decoder's cap.  The
 * definition is the one above, word for word -- F, B, M, the association of every addition, the output, the hole rule, the
 * exactness paragraph -- so where both calls serve a window mm, cm and hole_at are equal as IEEE values, -inf included, under
 * every spec and candidate order, and  max_c mm[N][c] == gh_viterbi_path_grid's ll_chain  exactly.  What differs is where the
 * dynamic programme lives: one kept row of F per position and two rows of B in device memory, one launch per position each way
 * on the handle's stream, the maxima taken per workgroup inside the backward step and by one launch at the end.  No workgroup
 * waits for another; the launch boundary is the only synchronisation.  Always the grid kernels, also on a window of 64 states.
 * The refusals are gh_viterbi_path_grid's: GH_ERR_ARG for a null argument, offer_zero, or S^Le > GH_VITERBI_GRID_MAX_STATES (the
 * same message: S, Le, the count, the cap; nothing is allocated for such a window).  GH_ERR_STATE before any fill.  GH_ERR_NOMEM
 * names the bytes.  A hole is found on the host, from the candidate bits, before anything large is reserved or any step launched.
 * The scratch is the exact decoder's block of the handle, kept until gh_destroy: the table, N * S^Le * 8 bytes of F (it is not
 * bounded by checkpointing), 16 * S^Le bytes of B, five partial maxima per position and 512 states, mm and cm -- 525 160 704 bytes
 * at 60 SNPs and 4^10 states, 4 889 679 360 at 5^10; 2 558 689 024 and 23 823 391 488 at 300 SNPs: ask gh_viterbi_states first.
 * It only reads the tensor; gh_viterbi_grid_info afterwards describes this call (S, Le, states, bytes reserved); gh_viterbi_info is
 * not touched. */
int gh_viterbi_marginals_grid(gh_t *h, double *mm /*[N+1][7]*/, uint8_t *cm /*[N+1]*/, int *hole_at);

/* K-best exact decoding of the chain likelihood (no reference counterpart; INTEGRATION.md "K-best decoding").  gh_viterbi_path says
 * what the best full path is and gh_viterbi_marginals how much every other choice would cost; this returns the runner-up paths
 * themselves: the k full paths of largest score, exactly.  Notation as in "Exact decoding" above; a state at p is the last
 * min(Le, p) picks.
 *   Per state.  Every state keeps a list of at most k prefixes in rank order 0, 1, ...  At p = 0 there is the empty state with one
 *   prefix of score +0.0.  At step p every kept prefix of rank r in predecessor state s' spawns one child per c in cm(p), of score
 *   score + w_p(c | s'), the additions those of the exact decoder: V + (prefix + T_Le) with prefix the marginal term and then lags
 *   1 .. Le-1, and V + prefix alone for p < Le.
 *   Merge.  For p > Le the children that meet in a state differ at x[p-Le] or in r.  They stand in the total order (1) score
 *   descending, by plain IEEE > and ==; (2) q(x[p-Le]) ascending; (3) r ascending; the first min(k, #children) are kept as ranks
 *   0, 1, ...  For p <= Le a state has one predecessor, whose list carries over in order (and has exactly one entry).
 *   End.  The entries of all states at p = N stand in the order (1) score descending; (2) ascending lexicographic
 *   (q(x[N]), ..., q(x[N-Le+1])); (3) r ascending.  The first n_out = min(k, number of full paths) are returned in that order:
 *   paths_out[i][0] = '_' (6), ll_chain[i] = the path's sequential sum from +0.0 in ascending p.
 *   Exactness.  fl(a + w) is monotone in a, so a child of a prefix outside the k best of its state is preceded by the k children
 *   of those that take the same pick: it is never among the k best of the state it enters.  By induction the k lists at p = N
 *   hold the k largest scores.  Hence:
 *     ll_chain[0..n_out) is, as a list, the n_out largest values of score(x) over all full paths, bit for bit;
 *     ll_chain[i] == gh_score_paths(paths_out[i]).ll_chain with n_on == N;  the paths are pairwise distinct;
 *     k = 1 is gh_viterbi_path, path and score;  max_c mm[N][c] of gh_viterbi_marginals == ll_chain[0];
 *     -inf is a score like any other (reachability is a count per state, never a score).
 *   Hole: at the first p with empty cm(p), hole_at = p, n_out = 0 and nothing else is written.  Otherwise hole_at = 0.
 *   Limits: 1 <= k <= GH_KBEST_MAX (a back-pointer is one byte: the dropped digit in 3 bits, the predecessor's rank in 5) and
 *   k * S^Le <= GH_VITERBI_MAX_STATES: the lists are the exact decoder's two score rows (64 KB on chip).
 * GH_ERR_ARG for a null argument (ll_chain included), k outside 1..GH_KBEST_MAX, offer_zero, more than GH_VITERBI_MAX_STATES
 * states (gh_viterbi_path's message) or k * S^Le beyond it (the message names S, Le, the states and the largest k the window
 * takes, GH_VITERBI_MAX_STATES / states).  GH_ERR_STATE before any fill.  GH_ERR_NOMEM names the size of the scratch: the exact
 * decoder's block of the handle, here the table, (N + 1) * S^Le * k back-pointer bytes (at most (N + 1) * 4096), the end lists
 * and the k path rows.
 * It only reads the tensor: the band, L, the fill statistics, the snapshot, the handle's conditional tables and the results of a
 * following gh_spin stay as they are, bit for bit.  gh_viterbi_info afterwards describes this call: S, Le, states = S^Le, bytes. */
#define GH_KBEST_MAX 32
int gh_viterbi_kbest(gh_t *h, int k, uint8_t *paths_out /*[k][N+1]*/, double *ll_chain /*[k]*/, int *n_out, int *hole_at);

/* Constrained exact decoding of the chain likelihood (no reference counterpart; INTEGRATION.md "Constrained decoding").  The
 * max-marginals say what the best full path through (p, c) scores; this returns that path -- and the best completion of any
 * partly known haplotype: exact decoding under per-position allele masks (pins and bans), many constraint sets over one window in
 * one call.  Notation as in "Exact decoding" above.
 *   A constraint set is allow[0..N], one byte per position: bit s set = symbol s (index order ACGTN-_) is allowed at p.  allow[0]
 *   and the bits of N and '_' are ignored; bit 7 set is an error.  The masked candidate set is cm'(p) = cm(p) & allow[p].  A full
 *   path has x[p] in cm'(p) for p = 1..N; score(x) is unchanged, gh_score_paths' ll_chain.
 *   Result per set: the maximum of score(x) over the full paths of the masked window, attained exactly; the path is the one kept
 *   by gh_viterbi_path's procedure run over cm': the same competition rule for p > Le, the same end rule.
 *   Hole: at the first p with empty cm'(p), hole_at[set] = p, and neither that set's path row nor its score is written; the other
 *   sets run on.  A mask can make a hole where the window has none: that is a value ("infeasible at p"), not an error.
 *   Otherwise hole_at[set] = 0.
 *   State space: U, S and S^Le are those of the UNMASKED window as it stands, for every set: the call serves exactly the windows
 *   gh_viterbi_path serves and refuses the others with the same message.  A mask only removes reachable states; the tie rules are
 *   stated in q(), not in digits, so this choice is invisible in the results.
 *   Hence:
 *     allow all 0x7f gives gh_viterbi_path's path and score, bit for bit;
 *     ll_chain[set] == gh_score_paths(paths[set]).ll_chain with n_on == N, and every x[p] is allowed;
 *     one-hot masks of a full path x at all positions return x and its gh_score_paths score;
 *     one-hot masks of the unmasked best path x* at any subset of positions return x* and its score (fl(a + w) is monotone in a:
 *     a competitor that x*'s prefix strictly beat, or tied with priority, in the full problem can only score lower in the
 *     restricted one);
 *     a pin (N, c) gives ll == mm[N][c] of gh_viterbi_marginals exactly (B_N = +0.0); for any p the maximum over c in cm(p) of the
 *     pinned scores equals gh_viterbi_path's ll_chain exactly; for p < N a pinned score and mm[p][c] differ only by the
 *     summation order, within the bound stated under "Max-marginals".
 * GH_ERR_ARG for a null argument, n_sets outside 0..GH_MASKED_MAX_SETS, an allow byte with bit 7 set, offer_zero, or more than
 * GH_VITERBI_MAX_STATES states (gh_viterbi_path's message); GH_ERR_STATE before any fill.  n_sets == 0 returns GH_OK and writes
 * nothing -- on a window the call serves: the refusals above come first, the cap included.  A window that offers nothing anywhere gives hole_at = 1 for every set.  GH_ERR_NOMEM names the size of the scratch: the
 * exact decoder's block of the handle (kept until gh_destroy), here the table ONCE, and per set (N + 1) * S^Le back-pointer
 * bytes (each set's block on a four-byte boundary), the end row, a path row and the compacted masks.  There is no slab or budget
 * scheme: 256 sets at 10k SNPs and 4096 states are 10.5 GB.
 * It only reads the tensor: the band, L, the fill statistics, the snapshot, the handle's conditional tables and the results of a
 * following gh_spin stay as they are, bit for bit.  gh_viterbi_info afterwards describes this call: S, Le, states, bytes.
 * gh_viterbi_masked_info, the last such call on the handle: out[0] = sets, out[1] = sets that met a hole, out[2] = walk launches,
 * out[3] = scratch bytes (all 0 before the first). */
#define GH_MASKED_MAX_SETS 256
int gh_viterbi_path_masked(gh_t *h, const uint8_t *allow /*[n_sets][N+1]*/, int n_sets,
                           uint8_t *paths_out /*[n_sets][N+1]*/, double *ll_chain /*[n_sets]*/, int *hole_at /*[n_sets]*/);
int gh_viterbi_masked_info(const gh_t *h, int64_t out[4]);

/* gh_viterbi_spin over every window of a batch or panel, the decoders of a round side by side: a window's exact decoder is ONE
 * workgroup, so one launch with a workgroup per window decodes all of them in about the time of the slowest.
 * Window w's paths ([max_paths][N_w + 1] at paths_out + paths_off[w], as gh_panel_spin; for a batch paths_off[w] =
 * w * max_paths * (N + 1)), recs[w][..], ll_chain[w][..] (may be NULL), n_out[w] and hole_at[w] are what gh_viterbi_spin writes for
 * that window alone: paths, ll_chain, hp_current, hp_original, min_marginal, ratio and magnitude bit for bit (the reweight is
 * gh_reweight_path's, window by window).  Afterwards each handle's gh_viterbi_info describes that window's last decoding, and the
 * tensor, snapshot (taken now where there is none), band, L and fill statistics of each window are as the single spin leaves them.
 * Round s, for every window still live (fewer than max_paths paths, no hole yet): the chain table of the tensor as it stands (per
 * window, on its handle's stream); the union, the walk and the trace as one launch each over the live windows (windows that need
 * the walk without the table ring -- one candidate symbol and Le > 12 -- in a walk launch of their own); the vit_outs and paths
 * home in two copies; per window the record and the reweight (gh_score_paths, gh_reweight_path).  A window that meets a hole or
 * its last path drops out; the call ends when no window is live.  No workgroup depends on another: a panel of more windows than
 * the card holds workgroups finishes all the same.
 * Stream order: panel launches and copies run on the batch's stream, a window's own work on its handle's; the batch's stream
 * waits for each handle's by an event, the host waits for the batch's stream before it touches a handle.
 * Refusals are made as a whole, before any window's tensor, snapshot or scratch is touched: GH_ERR_ARG for a null b, paths_out,
 * paths_off, recs, n_out or hole_at, for max_paths < 0, a negative offset, a window with offer_zero or a window with more than
 * GH_VITERBI_MAX_STATES states (gh_viterbi_path's message behind "window <w>: "); GH_ERR_STATE for a window never filled.
 * max_paths == 0 returns GH_OK with every n_out[w] = 0.  GH_ERR_NOMEM names the window whose scratch cannot be had ((N + 1) *
 * states back-pointer bytes and the table, as gh_viterbi_path).  Candidate masks only lose bits under a reweight, so round 0's
 * state count bounds every later round's; the count is checked every round all the same.
 * gh_panel_viterbi_info, the last such call: out[0] = windows, out[1] = rounds run, out[2] = the most windows one walk launch
 * carried, out[3] = walk launches in all.
 * gh_debug_panel_viterbi_phases (measurements only): on != 0 makes every following gh_panel_viterbi_spin of the process wait for
 * the device after each phase and add up host milliseconds; out (may be NULL) receives what has been added up since the last call
 * -- [0] table builds (and the call's preamble), [1] union + walk + trace, [2] gather and copies home, [3] records and reweights
 * -- and the sums start again. */
int gh_panel_viterbi_spin(gh_batch_t *b, int max_paths, double min_remove, uint8_t *paths_out, const int64_t *paths_off,
                          gh_path_rec *recs /*[n][max_paths]*/, double *ll_chain /*[n][max_paths], may be NULL*/,
                          int *n_out /*[n]*/, int *hole_at /*[n]*/);
int gh_panel_viterbi_info(gh_batch_t *b, int64_t out[4]);
int gh_debug_panel_viterbi_phases(int on, double out[4]);

/* gh_viterbi_marginals over every window of a batch or panel, the walks side by side: a window's forward walk and its backward
 * walk are ONE workgroup each, so one launch with a workgroup per window does every window's in about the time of the slowest.
 * Window w's mm ([N_w + 1][7] doubles at mm + 7 * pos_off[w]), cm ([N_w + 1] bytes at cm + pos_off[w]) and hole_at[w] are what
 * gh_viterbi_marginals writes for that handle alone, as IEEE values, -inf included.  pos_off is in positions; the running sum of
 * N_v + 1 packs the windows back to back.  A window that meets a hole has neither of its ranges written; the others run on.
 * Afterwards each handle's gh_viterbi_info is what the single call would have left (S, Le, states, the bytes of that window's
 * block).  The call only reads the tensors: for every window the band, L, the fill statistics, the snapshot, the conditional
 * tables and the results of a following gh_spin / gh_panel_spin stay as they are, bit for bit.
 * Launches: the candidate bits of all windows in one (2-D: y the window); the forward walks in one, and a second for the windows
 * that walk without the table ring (one candidate symbol and Le > 12, or GH_VIT_STAGE=0); the backward walks in one for the
 * windows whose four rows and ring fit 160 KB of LDS and a second for the others (two symbols and Le >= 11, for one) -- the
 * single call's decision, window by window; the maxima in one; a gather of the vit_outs, mm and cm, then one copy home each
 * where the caller's offsets are the running sum and no window met a hole (one more pair per break otherwise).  No workgroup
 * depends on another: a panel of more windows than the card holds workgroups finishes all the same.
 * Scratch: each window's block is its handle's own exact-decoder block under the max-marginals' layout, exactly as the single
 * call reserves it (kept until gh_destroy); all blocks are reserved before the first walk is launched.  There is no wave or budget
 * scheme: the panel asks for the sum over its windows of N * states * 8 bytes plus the tables and the small parts -- 64 windows of
 * 10 000 SNPs at 1 024 states are 6 GB.  GH_ERR_NOMEM names the window that could not be served and that sum.  The descriptors,
 * the launch lists and the gathered results ((N_w + 1) * 57 bytes a window) are a block of the batch, shared with
 * gh_panel_viterbi_spin.
 * Stream order: a window's marginal tables and chain table on its handle's stream, an event per window before the batch's
 * stream, everything panel-wide on the batch's stream; the host waits for the batch's stream before it touches a handle.
 * Refusals are made as a whole, before any window's scratch or gh_viterbi_info is touched: GH_ERR_ARG for a null b, mm, cm,
 * pos_off or hole_at, a negative offset, a window with offer_zero or a window with more than GH_VITERBI_MAX_STATES states
 * (gh_viterbi_path's message behind "window <w>: "); GH_ERR_STATE for a window never filled.
 * gh_panel_viterbi_marginals_info, the last such call: out[0] = windows, out[1] = windows that met a hole, out[2] = walk
 * launches, forward and backward together, out[3] = scratch bytes summed over the handles' blocks.  GH_ERR_ARG for a null
 * argument.
 * Under gh_debug_panel_viterbi_phases (measurements only) this call adds up too: [0] the preamble, the table builds and the
 * candidate bits, [1] the forward walks, [2] the backward walks, [3] the maxima, the gather and the copies home. */
int gh_panel_viterbi_marginals(gh_batch_t *b, double *mm, uint8_t *cm, const int64_t *pos_off /*[n]*/, int *hole_at /*[n]*/);
int gh_panel_viterbi_marginals_info(gh_batch_t *b, int64_t out[4]);

/* gh_viterbi_kbest over every window of a batch or panel, each with its own k (regions of a panel differ in S^Le, so the largest
 * k they take differs), the walks side by side: a window's k-best walk and its trace are ONE workgroup each, so one launch with a
 * workgroup per window does every window's in about the time of the slowest.
 * Window w's n_out[w] path rows ([N_w + 1] bytes each, from paths_out + paths_off[w]; paths_off in bytes), its scores (from
 * ll_chain + ll_off[w]; ll_off in doubles), n_out[w] and hole_at[w] are what gh_viterbi_kbest(h_w, k[w], ...) writes for that handle
 * alone, bit for bit and in the same order, the two tie orders and -inf scores included.  Rows and scores beyond n_out[w] are not
 * written; nothing of a window that met a hole is written (n_out[w] = 0, the others run on).  The running sums of
 * k[w] * (N_w + 1) and of k[w] pack the windows back to back.
 * Afterwards each handle's gh_viterbi_info is what the single call leaves (S, Le, states, the bytes of that window's block).  The
 * call only reads the tensors: for every window the band, L, the fill statistics, the snapshot, the conditional tables and the
 * results of a following gh_spin, gh_panel_spin or gh_panel_viterbi_spin stay as they are, bit for bit.
 * Launches: the walks in one, and a second for the windows that walk without the table ring (one candidate symbol and Le > 12, or
 * GH_VIT_STAGE=0) -- the single call's decision, window by window; K is a run-time value of the walk, so windows of differing k
 * share a launch; the traces in one; a gather of the vit_outs, the rows and the scores in window order, then the vit_outs home
 * (the host learns n_out and the holes) and one copy each of rows and scores per run of neighbouring windows that are full
 * (n_out[w] == k[w], no hole) and whose destinations lie as the gathered ranges do: three copies in all for a packed call with
 * every window full.  No workgroup depends on another: a panel of more windows than the card holds workgroups finishes all the same.
 * Scratch: each window's block is its handle's own exact-decoder block under the k-best layout, exactly as the single call
 * reserves it (kept until gh_destroy); all blocks are reserved before the first walk is launched.  The panel asks for the sum over
 * its windows of (N + 1) * states * k bytes plus the tables and the small parts.  GH_ERR_NOMEM names the window whose block could
 * not be had and that sum.  The descriptors, the launch list and the gathered results are a block of the batch, shared with
 * gh_panel_viterbi_spin and gh_panel_viterbi_marginals.
 * Stream order: a window's marginal tables and chain table on its handle's stream, an event per window before the batch's
 * stream, everything panel-wide on the batch's stream; the host waits for the batch's stream before it touches a handle.
 * Refusals are made as a whole, before any window's scratch or gh_viterbi_info is touched: GH_ERR_ARG for a null argument, a
 * negative offset, a k[w] outside 1..GH_KBEST_MAX, a window with offer_zero, a window with more than GH_VITERBI_MAX_STATES states
 * or one whose k[w] * states is beyond it (gh_viterbi_kbest's messages behind "window <w>: "; the last names the largest k the
 * window takes); GH_ERR_STATE for a window never filled.
 * gh_panel_viterbi_kbest_info, the last such call: out[0] = windows, out[1] = windows that met a hole, out[2] = walk launches,
 * out[3] = scratch bytes summed over the handles' blocks.  GH_ERR_ARG for a null argument.
 * Under gh_debug_panel_viterbi_phases (measurements only) this call adds up too: [0] the preamble and the table builds, [1] the
 * walks, [2] the traces, [3] the gather and the copies home. */
int gh_panel_viterbi_kbest(gh_batch_t *b, const int *k /*[n]*/,
                           uint8_t *paths_out, const int64_t *paths_off /*[n], bytes*/,
                           double *ll_chain,  const int64_t *ll_off    /*[n], doubles*/,
                           int *n_out /*[n]*/, int *hole_at /*[n]*/);
int gh_panel_viterbi_kbest_info(gh_batch_t *b, int64_t out[4]);

/* tensor export/import for --dumpmatrix (gretel/cmd.py:81-82) and tests:
 * band layout [(N+2)][band][7][7] as doubles; dense layout [7][7][N+2][N+2] (gretel/cmd.py:76-77). */
int gh_export_band(gh_t *h, double *out);
int gh_import_band(gh_t *h, const double *in);
int gh_export_dense(gh_t *h, double *out);

/* gretel-snpper's site calling -- gretel/snpper.py:29-50 -- as a GPU histogram: the aligned runs of the BAM (gio_match_runs,
 * include/gretel_io.h: per run its 0-based reference start, bases as codes A0 C1 G2 T3, 4 = other) are counted per
 * position of the window [start0, start0+len) and base; site_out[p] = 1 where more than one base is seen on more than
 * `depth` reads (snpper.py:38-40).  counts_out (optional): int32[4][len], the array pysam's count_coverage returns. */
int gh_coverage_sites(int device, const int32_t *ref_start, const int64_t *off, const uint8_t *codes, int64_t n_runs,
                      int32_t start0, int32_t len, int32_t depth, int32_t *counts_out, uint8_t *site_out);

/* Per-kernel HIP-event timing on the handle's own stream (bench.py's roofline leg).
 * gh_profile_enable(h, k): k = 0 off; k >= 1 brackets every k-th launch of each kernel with a pair of events
 * (an event between two kernels costs the stream a ~10 us bubble, so a timed region samples with k > 1). */
/* GH_K_WALK: the whole path extension of one path (one serial walker launch, or k_seg + k_scan + k_emit);
 * GH_K_SEG: k_seg alone, the largest kernel of the segment-parallel extension (inside gh_spin: the first path only);
 * GH_K_RWSEG: k_rwseg alone -- the reweight of path k-1 and the k_seg of path k in one launch (every later path of a gh_spin) */
enum { GH_K_FILL = 0, GH_K_MARG = 1, GH_K_LT = 2, GH_K_WALK = 3, GH_K_REWEIGHT = 4, GH_K_SEG = 5, GH_K_RWSEG = 6, GH_K_COUNT = 7 };
int gh_profile_enable(gh_t *h, int on);
int gh_profile_reset(gh_t *h);
int gh_profile_get(gh_t *h, int kernel, double *total_ms, int64_t *launches);
/* what a bracket reads beyond its kernel: out[0] = two events back to back, out[1] = around an empty kernel (ms, medians) */
int gh_profile_overhead(gh_t *h, int reps, double out[2]);
/* diagnostics of the last path-extension launch: out[0] = shader cycles (s_memtime) the walker wave spent,
 * out[1] = the same interval in 100 MHz ticks (s_memrealtime), out[2] = steps it executed, out[3] = the variant
 * that ran (2 = depth-2 speculation, 1 = depth 1 without '-' candidates, 0 = depth 1 with them; 3 = segment-parallel
 * walk, which has no single walker wave: then out[0] = how often the last gh_spin rebuilt the conditional table and
 * queued its remaining paths again because a candidate mask moved, out[1] = the state space it enumerated (4: candidate
 * ranks of a window whose positions offer at most four; 5: all symbol histories; 6: mixed radix -- few positions offer five),
 * out[2] = the most states that enter a target as a mixed-radix number (0: not taken); 4 = candidate-pool segments
 * (L = 6..128): out[0] = re-queues of the last gh_spin, out[1] = paths this handle handed to the serial walker so far,
 * out[2] = walk/scan rounds it queued so far) */
int gh_debug_walk_clock(gh_t *h, uint64_t out[4]);
/* diagnostic builds only (-DRWS_STAMPS_ALL): the s_memtime stamps every k_rwseg workgroup of the last launch left at its phase
 * boundaries, 16 doubles per workgroup (scratch/wg_stamps.py) -- which workgroup a launch waits for, and in which phase */
int gh_debug_segment_stamps(gh_t *h, double *out, int n_workgroups);
/* how the candidate-pool extension (gretel/gretel.py:143-189 for 6 <= L <= 128) would cut a window of n_snps positions at lag count
 * L, over candidate ranks (five = 0) or over the symbols A C G T - (five = 1); no handle, no GPU: out[0] = segments, out[1] = positions
 * per segment, out[2] = targets per LDS chunk of the walker, out[3] = bytes of dynamic LDS it is launched with, out[4] = 1 if a state
 * is a packed 64-bit word (k_cwalk), 0 if bytes next to a hash (k_cwalkg), out[5] = threads per workgroup */
int gh_debug_pool_geometry(int32_t n_snps, int32_t L, int32_t five, int64_t out[6]);
/* Which kernels run for every path of a gh_spin is chosen once per spin, as a value.  What the choice depends on: */
typedef struct gh_spin_plan_in {
    int32_t n_snps, band, L, storage, cond_mode, marginal_term, offer_zero;   /* as gh_config and gh_set_L */
    int32_t walk_mode;      /* GH_WALK at creation: 0 seg (default), 1 spec, 2 spec1, 3 src */
    int32_t lt_full;        /* GH_LT_FULL at creation */
    int32_t need_rinfo;     /* marginal term, or GH_FUSE >= 1 at creation */
    int32_t pools_off;      /* the window has shown a position the candidate pools cannot take */
    int32_t ranked;         /* the conditional table's layout: 1 over candidate ranks, 0 over the symbols, -1 not looked at yet */
    int32_t rwseg, rwseg_small, emit_small, fuse, seg6, mixed;   /* GH_RWSEG, GH_RWSEG_SMALL, GH_EMIT_SMALL, GH_FUSE, GH_SEG6, GH_MIXED: the value, -1 = unset */
    int32_t rw_lp16, rw_tband;                                   /* GH_RW_LP16, GH_RW_TBAND (per process): the value, -1 = unset */
} gh_spin_plan_in;
/* ... and the choice.  All zero: outside a spin (a lone gh_generate_path / gh_reweight_path) */
enum { GH_FLOW_NONE = 0,
       GH_FLOW_SERIAL = 1,   /* a serial walker + k_marg<T,true> per path */
       GH_FLOW_SEG = 2,      /* the enumerated states: k_seg, k_scan + k_emit (or k_emit_small alone), k_rw */
       GH_FLOW_RWSEG = 3,    /* ... the reweight of a path inside the k_seg launch of the next: k_rwseg, k_scan + k_emit (or k_emit_small) */
       GH_FLOW_FUSE = 4,     /* ... opt-in (GH_FUSE): k_seg, k_scan, and a k_rw that chains the maps itself */
       GH_FLOW_POOLS = 5 };  /* candidate pools (L >= 6) */
typedef struct gh_spin_plan {
    int32_t flow;           /* GH_FLOW_* */
    int32_t emit_small;     /* every segment map fits one workgroup's LDS: k_emit_small instead of k_scan + k_emit */
    int32_t seg6;           /* L = 6 over a ranked table: the enumerated states (4^6), not pools */
    int32_t stride;         /* doubles between two paths' partial sums of the removed mass */
    int32_t rw_lanes;       /* lanes per position of the reweight kernel the stride is sized for */
    int32_t S;              /* segments the spin sizes for (0: serial) */
    int32_t mixed;          /* the table builds of this spin classify the window for the mixed-radix states (k_classify) */
    int32_t need_layout;    /* the choice depends on `ranked` and the caller has not looked (ranked = -1): look, and plan again */
    int64_t lds;            /* dynamic LDS of the flow's largest launch: k_rwseg's patch offset + the patch, or the fused k_rw's prologue (0 otherwise) */
} gh_spin_plan;
/* the choice for a window described by *in; no handle, no GPU (tests/test_spin_plan_host.py) */
int gh_debug_spin_plan(const gh_spin_plan_in *in, gh_spin_plan *out);
/* the plan the last gh_spin on this handle ran with (all zero: none yet) */
int gh_debug_last_spin_plan(gh_t *h, gh_spin_plan *out);
/* algorithmic bytes of the last launch of each kernel */
int gh_profile_bytes(gh_t *h, int kernel, double *bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* GRETEL_HIP_H */
