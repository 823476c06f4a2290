// gretel_hip.hip -- host side of libgretel_hip.so: the C ABI of include/gretel_hip.h over the gfx950 kernels
// of kernels.hpp (which documents every kernel and table).
//
// Data in HBM per window:
//   band    T[(N+2)][7][W][7]      element (a, b) of cell (i, j=i+d), d in 1..W, at bidx(W, i, d, a, b) = ((i*7+a)*W+(d-1))*7+b ; T = float | double
//   cnt, marg  f64[(N+2)][8]       c_s(p) = sum_t H[s,t,p,p+1] (+ total), c_s/total          (lookup API)
//   nvalid, cmask                  V(p), candidate bitmask
//   minfo   f64[(N+2)][16]         log10 marginal x5, marginal x5, candidate bits, log10 ORIGINAL marginal x5
//   G (lt)  f64[(N+16)][6][L][5]   source-major log10 conditionals, over symbols or over candidate ranks (k_lt)
//
// Launch sequence of one path of a spin (gretel/cmd.py:148-179):  k_lt (full build for the first path, then only a
// check of the candidate-mask flags) -> k_walk_spec -> k_marg<T,true> (reweight + marginals + the table rows the path
// changed); gh_spin reduces the removed mass of all paths with one k_reweight_finish_all at the end, gh_batch_spin
// launches each kernel over all windows (k_reweight_finish per path).
//
// Arithmetic contract (identical to oracle/hansel_ref.py): row/column sums accumulate
// sequentially in the storage dtype, everything else is IEEE binary64 with NO fma
// contraction (build with -ffp-contract=off) and gh_log10 from gh_detlog.h.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "gretel_hip.h"
#include "gh_detlog.h"
#include "scratch_layout.hpp"


// ---------------------------------------------------------------------------------------------
// error handling
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(GH_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),    \
                        __FILE__, __LINE__);                                                  \
    } while (0)

extern "C" const char *gh_last_error(void) { return g_err; }

#include "kernels.hpp"
#include "segwalk.hpp"
#include "cwalk.hpp"
#include "wpipe.hpp"

// ---------------------------------------------------------------------------------------------
// handle
// ---------------------------------------------------------------------------------------------
struct prof_slot {
    std::vector<hipEvent_t> ev;   // start/stop pairs
    size_t used = 0;
    double ms = 0.0;
    int64_t launches = 0;
    double bytes = 0.0;
    int64_t seq = 0;              // launches seen since profiling was switched on
    bool open = false;            // prof_begin recorded a start event for the launch in flight
};

// the GH_* switches: a number (def when unset), and "set to 0"
static int env_int(const char *name, int def)
{
    const char *v = getenv(name);
    return v ? atoi(v) : def;
}
static bool env_off(const char *name) { return env_int(name, 1) == 0; }

// GH_WALK (read when a handle is created): see the walker selection further down
enum { WM_SEG = 0, WM_SPEC = 1, WM_SPEC1 = 2, WM_SRC = 3 };

static int walk_mode_from_env()
{
    const char *m = getenv("GH_WALK");
    if (!m || !*m || !strcmp(m, "seg")) return WM_SEG;
    if (!strcmp(m, "spec1")) return WM_SPEC1;
    if (!strcmp(m, "src")) return WM_SRC;
    return WM_SPEC;
}

struct dev_scratch {       // a device block that grows on demand (scratch_reserve); free_handle frees it
    void *buf;
    size_t cap;
};

// gh_create value-initialises the handle: what is not given a value here starts at zero / null / false
struct gh_handle {
    gh_config cfg;
    int N, W, L = 1;
    int dev;
    hipStream_t stream;
    size_t n_cells;
    void *band;
    double *cnt, *marg, *minfo;
    int32_t *nvalid;
    uint32_t *cmask;
    double *rinfo;                // [(N+2)][8] log10 marginal / marginal by candidate rank (k_marg, k_rw)
    unsigned long long *pipe_pk;  // [N+2] the window pipeline's packed candidate words (wpipe.hpp), allocated by the first batch that takes it
    double *pipe_gp;              // ... and its compact table, (N+LT_PAD) sources of L x 128 bytes (wpipe.hpp: pipe_gp_piece)
    size_t pipe_gp_bytes;
    double *pipe_lm;              // ... and, with the marginal term, the candidates' log-marginals by rank [N+2][4]
    double *pipe_gw;              // ... and, for a window with a few five-candidate positions, their side table + the chunk directory (wpipe.hpp)
    size_t pipe_gw_bytes;
    bool need_rinfo;              // ... kept only where somebody reads it: with the marginal term (k_seg, k_cwalk add it in front of x1) and
                                  // for the three-launch spins (GH_FUSE at creation); nullptr goes to the kernels otherwise (C5: k_rw is bound by its stores)
    symmap sm;                    // compact index <-> symbol (gh_config.cand_order)
    double *lt;
    bool ht_stale;                // an incremental refresh left the depth-2 walker's tables (ht, yt) out: a full rebuild before they are read
    bool lt_baked;                // lt holds the marginal term in its lag-1 entries (built for a serial walker; only with cfg.marginal_term)
    double *ht, *yt;              // depth-2 walker tables derived from lt (k_lt), when walk_depth2_ok(L)
    unsigned long long fill_seen[6];   // host mirror of dstate->fill as last read (the counters only move under this handle's calls)
    uint8_t *spin_paths;          // gh_spin's device results, kept between calls: [spin_cap][N+1]
    gh_path_rec *spin_recs;       // [spin_cap]
    int spin_cap;
    int lt_L;
    bool dirty_marg = true, dirty_lt = true, have_orig;
    const uint8_t *lt_inc_path;   // non-null: the ONLY mutation since G was last built is a path reweight whose fused
                                  // kernel has rewritten the rows it changed (k_lt then only checks the mask flags)
    uint8_t *d_rw_path;           // [N+1] device copy of the path of gh_reweight_path
    dev_state *dstate;
    double *partial;       // reweight block partial sums
    int partial_cap;
    uint8_t *d_path;       // [N+1] scratch path
    gh_path_rec *d_rec;    // 1 scratch record
    // segment-parallel walk (segwalk.hpp), sized for seg_L by alloc_seg
    uint32_t *seg_hist;    // picks of every (segment, entry state)
    uint16_t *seg_maps, *seg_pmaps, *seg_gmaps;
    double *seg_min;       // [CW_MAX_SEG]
    double *seg_smin, *seg_gmin;   // minimum marginal per (segment, entry state) / per (group, entry state)
    size_t seg_smin_bytes;
    uint8_t *cm5snap;      // [N+2] candidate bits as the last k_seg saw them
    bool band_zero = true; // the tensor holds nothing but zeros (gh_create, gh_clear; until something is added): k_fill_own may store instead of add
    void *tband;           // column conditionals, lane groups of 16 / 32: the band once more, TO-major (tband[bidx(W, p, d, b, a)] = band[bidx(W, p, d, a, b)])
    bool lt_inc_seg;       // lt_inc_path was left by a reweight behind a segment-parallel walk (k_rw / k_rwseg keep the table under every conditional)
    uint64_t band_epoch = 1, tband_epoch;  // tband mirrors the band iff equal: everything that writes the band counts, k_rw<.., COL> keeps both
    void *seg_halo;        // k_rwseg: per segment, the band blocks of the L positions in front of it (k_emit's copy)
    size_t seg_halo_bytes;
    double *lmsel1;        // [N+1] selected log-marginals of a lone gh_generate_path
    double *spin_lmsel;    // [spin_cap][N+1] the same for every path of a spin
    int seg_L;
    // candidate-pool segment walk (cwalk.hpp)
    cw_key *cw_keys, *cw_exits, *cw_pend, *cw_pend_exit;
    int32_t *cw_pend_ready;
    uint32_t *cw_phist;
    uint32_t *cw_hist;
    int32_t *cw_npend;
    int32_t *cw_last_hit, *cw_npool, *cw_true;
    uint8_t *cw_walked;
    int8_t *cw_nxt;
    bool cw_ready;         // the pools hold states of this tensor (seeded by a serial walk since the last fill / L change)
    bool cw_off;           // a position with five candidates and more than CW_MAX_L5 lags: serial walkers only
    bool cw_wide;          // the conditional table is over the symbols, not over candidate ranks: k_cwalk<L, 5>
    bool cw_pool_wide;     // ... and what the pools' states are made of
    uint8_t *cw_keys_d, *cw_exits_d, *cw_pend_d;      // k_cwalkg: the states as bytes, [S][CW_K][cw_LD] (cw_pend_d: two sets, as the request lists)
    uint8_t *cw_pend_exit_d;                          // ... and the exit states run-on requests arrive with, two sets
    int cw_LD;
    int cw_rounds = 2;     // walk/scan rounds queued per path (adapts to how often chains stay open)
    int cw_stamp;
    int cw_pp;             // k_cwalk launches so far: which of the two request-list sets this launch appends to (cwalk.hpp)
    size_t cw_S;           // segments the pool buffers are sized for (the second set of request lists lies cw_S entries behind the first)
    int64_t cw_stat[4];    // paths through the pools, paths handed to the serial walker, rounds queued, re-queues
    int force_stale_at = env_int("GH_SEG_FORCE_STALE", -1);   // at creation (tests): path k of every gh_spin finds the table stale once
    uint8_t *stage;        // pinned host staging for the results of a spin
    size_t stage_cap;
    double *ew_buf;        // gh_edge_weights_at: seven weights and the candidate mask
    // four scratch blocks, each grown on demand (scratch_reserve) and laid out by its user's function in scratch_layout.hpp.  Four,
    // not one arena: gh_beam_spin and gh_viterbi_spin call gh_score_paths while the decoder's block still holds the path row
    dev_scratch asg;       // gh_assign_reads (assign.hpp): counters, paths, match masks and per-read results
    dev_scratch score;     // gh_score_paths (score.hpp): one slab's paths, records and per-position values
    dev_scratch beam;      // gh_beam_paths / gh_beam_spin (beam.hpp): its chain table, back-pointers, path rows and scores; grows with N * L
    int64_t beam_last[4];  // gh_beam_info: the last beam run on this handle
    dev_scratch vit;       // gh_viterbi_path / gh_viterbi_spin (viterbi.hpp): its chain table, N * states back-pointer bytes, the end row, the path
    int64_t vit_last[4];   // gh_viterbi_info: the last exact decoding on this handle
    int64_t vitx_last[4];  // gh_viterbi_masked_info: the last constrained decoding on this handle (viterbi_masked.hpp)
    int64_t vitg_last[4];  // gh_viterbi_grid_info: the last decoding on the grid on this handle (viterbi_grid.hpp)
    int cw_round_cap = env_int("GH_CW_ROUND_CAP", 0);   // =k at creation (tests): never more than k rounds per launch, so that chains stay open and the serial fallback runs
    gh_spin_plan last_plan;    // what the last gh_spin ran with (gh_debug_last_spin_plan; nothing else reads it)
    int spin_requeues;     // how often the last gh_spin rebuilt the table and queued the remaining paths again
    gh_fill_stats stats = {0, 0, 0, 1, 0};
    int wmode = walk_mode_from_env();        // WM_*: which path extension (GH_WALK at creation)
    bool lt_full = env_int("GH_LT_FULL", 0) != 0;   // at creation: rebuild the conditional table in full before every path (A/B)
    int prof;                     // 0 = off, k = bracket every k-th launch of each kernel
    prof_slot ps[GH_K_COUNT];
};

struct gh_reads {
    int dev;
    int64_t n_reads, n_bases;
    int32_t *rank;
    int64_t *off;
    uint8_t *bases;
    int max_k;
    bool sorted;      // ranks ascend: k_fill_sorted applies
    int span_pos;     // sorted tables: widest run of positions one workgroup of k_fill_sorted (FILL_RPB reads) covers
    int64_t dens128;  // sorted tables: the most reads whose ranks fall into any 128 consecutive positions (k_fill_own's counter width)
    int64_t *first_at; // sorted tables: [n_first] first_at[p] = the first read whose rank is >= p (first_at[n_first - 1] = n_reads)
    int n_first;
};
#define FILL_RPB 2048     /* reads per workgroup of k_fill_sorted */
#define FILL_PAIRS_MIN_K 10   /* k_fill_pairs (32 lanes per read) from this many SNPs in the longest read */

static inline size_t esize(const gh_handle *h) { return h->cfg.storage == GH_STORAGE_F64 ? 8 : 4; }

// f(T()) with T = the handle's storage type (float / double): one launch site per kernel, instantiated for both
template <typename F> static auto with_storage(const gh_handle *h, F &&f)
{
    return h->cfg.storage == GH_STORAGE_F64 ? f(0.0) : f(0.0f);
}

// raises kernel K's dynamic-LDS limit where this device's last raise was lower: once per instantiation and device, not on
// every launch (gh_batch_spin runs gh_spin on several host threads)
template <auto K> static void lds_limit(size_t lds, int dev)
{
    static std::atomic<size_t> set[64];
    if (lds > set[dev & 63]) {
        hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        set[dev & 63] = lds;
    }
}

// the window's control words to the host: one copy, one wait on its stream
static int read_state(gh_handle *h, dev_state *hs)
{
    hipError_t e = hipMemcpyAsync(hs, h->dstate, sizeof *hs, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(GH_ERR_HIP, "gh_spin failed: %s", hipGetErrorString(e));
    return GH_OK;
}

// algorithmic bytes (gh_profile_bytes, gh_batch_profile_get; bench.py's roofline), es = bytes per element.  The extension of a
// path, SURVEY 8(d): per step the marginal cell + L history cells (49 elements each) + the original marginals (7 x 4 B).  What
// this build's layout needs per step is one table row: N * (L * 40 + 25) bytes.
static double walk_bytes(int N, int L, double es) { return (double)N * ((1.0 + (double)L) * CELL * es + 28.0); }
// the reweight of a path: the reweighted elements (read+write) + the marginal pass (read cell (p,p+1), write the tables)
// (+ rows: one band row read and L x 5 table entries written per (source, lag) when the table rows are rewritten too)
static double reweight_bytes(int N, int W, int L, double es, bool rows)
{
    const int wl = W < L ? W : L;
    return (double)(N + 1) * ((double)W * 2.0 * es + 1.0 + CELL * es + 2 * 64 + 88 + 8) +
           (rows ? (double)N * ((double)wl * 7 * es + (double)L * LT_ROW * 8.0) : 0.0);
}

// k_marg's and k_lt's arguments by name (kernels.hpp takes them in this order); what a launch leaves out is null / 0
struct marg_args {
    void *band = nullptr;
    int N = 0, W = 0;
    double *cnt = nullptr, *marg = nullptr;
    int32_t *nvalid = nullptr;
    uint32_t *cmask = nullptr;
    double *minfo = nullptr;
    dev_state *st = nullptr;
    const win_desc *wd = nullptr;
    const uint8_t *rw_path = nullptr;
    double ratio = 0.0;
    int use_state_ratio = 0;
    double *partial = nullptr;
    int spin = 0;
    double *G = nullptr;            // the batched k_marg<T,true>: any non-null pointer = take G from the descriptor
    int L = 0, cond_mode = 0;
    const double *segmin = nullptr;
    gh_path_rec *seg_rec = nullptr;
    symmap sm{};
    int offer_zero = 0;
    double *rinfo = nullptr;
};
template <bool RW> static void launch_marg(const gh_handle *h, dim3 grid, hipStream_t st, const marg_args &a)
{
    with_storage(h, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL((k_marg<T, RW>), grid, dim3(256), 0, st, (T *)a.band, a.N, a.W, a.cnt, a.marg, a.nvalid, a.cmask, a.minfo,
                           a.st, a.wd, a.rw_path, a.ratio, a.use_state_ratio, a.partial, a.spin, a.G, a.L, a.cond_mode, a.segmin,
                           a.seg_rec, a.sm, a.offer_zero, a.rinfo);
    });
}

// the handle's own tensors and tables (single-window launches)
static marg_args marg_of(const gh_handle *h)
{
    marg_args a;
    a.band = h->band; a.N = h->N; a.W = h->W; a.cnt = h->cnt; a.marg = h->marg; a.nvalid = h->nvalid; a.cmask = h->cmask;
    a.minfo = h->minfo; a.st = h->dstate; a.sm = h->sm; a.offer_zero = h->cfg.offer_zero; a.rinfo = h->need_rinfo ? h->rinfo : nullptr;
    return a;
}

struct lt_args {
    const void *band = nullptr;
    int N = 0, W = 0, L = 0, cond_mode = 0;
    int bake_lm = 0;                // (k_lt's marginal_term)
    const double *cnt = nullptr;
    const int32_t *nvalid = nullptr;
    const uint32_t *cmask = nullptr;
    const double *minfo = nullptr;
    double *G = nullptr;
    dev_state *st = nullptr;
    const uint8_t *inc_path = nullptr;
    const win_desc *wd = nullptr;
    int spin = 0, allow_ranked = 0;
    double *Ht = nullptr, *Yt = nullptr;
    symmap sm{};
    const void *tband = nullptr;
};
static void launch_lt(const gh_handle *h, dim3 grid, hipStream_t st, const lt_args &a)
{
    with_storage(h, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(k_lt<T>, grid, dim3(256), 0, st, (const T *)a.band, a.N, a.W, a.L, a.cond_mode, a.bake_lm, a.cnt, a.nvalid,
                           a.cmask, a.minfo, a.G, a.st, a.inc_path, a.wd, a.spin, a.allow_ranked, a.Ht, a.Yt, a.sm, (const T *)a.tband);
    });
}

static int set_dev(const gh_handle *h)
{
    HIPCHK(hipSetDevice(h->dev));
    return GH_OK;
}

// launch check: GH_DEBUG_SYNC=1 synchronises after every launch so that a fault names its kernel
static int post_launch(gh_handle *h, const char *what)
{
    static const bool dbg = env_int("GH_DEBUG_SYNC", 0) != 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && dbg) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(GH_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return GH_OK;
}

// the to-major copy while it mirrors the band (nullptr otherwise): a column sum is then a contiguous run, same addends in the same order
static const void *tband_current(const gh_handle *h) { return (h->tband && h->tband_epoch == h->band_epoch) ? h->tband : nullptr; }

// a scratch block that holds `need` bytes: kept while it is large enough, otherwise freed and had anew once the stream has drained
// (what it held is gone).  A block that cannot be had is GH_ERR_NOMEM, and not left behind as HIP's last error for the next
// post_launch of this thread to find.
static int scratch_reserve(gh_handle *h, dev_scratch *s, size_t need, const char *what)
{
    if (need <= s->cap) return GH_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    hipFree(s->buf);
    s->buf = nullptr;
    s->cap = 0;
    if (hipMalloc(&s->buf, need) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GH_ERR_NOMEM, "%s cannot be had (%zu bytes)", what, need);
    }
    s->cap = need;
    return GH_OK;
}

// profiling brackets --------------------------------------------------------------------------
static void prof_begin(gh_handle *h, int k)
{
    if (!h->prof) return;
    prof_slot &s = h->ps[k];
    s.open = false;
    // (k_seg samples half a stride away from the bracket around the whole extension it is nested in, so that neither
    // times the other's event bubbles)
    if ((s.seq++ % h->prof) != (k == GH_K_SEG ? h->prof / 2 : 0)) return;
    if (s.used + 2 > s.ev.size()) {
        for (int q = 0; q < 2; q++) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            s.ev.push_back(e);
        }
    }
    hipEventRecord(s.ev[s.used], h->stream);
    s.open = true;
}

static void prof_end(gh_handle *h, int k, double bytes)
{
    if (!h->prof) return;
    prof_slot &s = h->ps[k];
    s.bytes = bytes;
    if (!s.open) return;
    s.open = false;
    hipEventRecord(s.ev[s.used + 1], h->stream);
    s.used += 2;
}

static void prof_collect(gh_handle *h)
{
    for (int k = 0; k < GH_K_COUNT; k++) {
        prof_slot &s = h->ps[k];
        for (size_t q = 0; q + 1 < s.used; q += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, s.ev[q], s.ev[q + 1]) == hipSuccess) {
                s.ms += ms;
                s.launches++;
            }
        }
        s.used = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int init_constants()
{
    int8_t lut[256];
    memset(lut, -1, sizeof lut);
    lut['A'] = 0; lut['C'] = 1; lut['G'] = 2; lut['T'] = 3; lut['N'] = 4; lut['-'] = 5; lut['_'] = 6;
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(c_sym_of_char), lut, sizeof lut));
    return GH_OK;
}

extern "C" int gh_device_count(int *n)
{
    if (!n) return fail(GH_ERR_ARG, "null argument");
    HIPCHK(hipGetDeviceCount(n));
    return GH_OK;
}

extern "C" int gh_device_clock_khz(int device, int *khz)
{
    if (!khz) return fail(GH_ERR_ARG, "null argument");
    if (device < 0) HIPCHK(hipGetDevice(&device));
    HIPCHK(hipDeviceGetAttribute(khz, hipDeviceAttributeClockRate, device));
    return GH_OK;
}

// log10 as the kernels evaluate it (include/gh_detlog.h), over an array: what tests/test_gpu_detlog.py holds to the host's libm
__global__ void k_log10_many(const double *__restrict__ x, double *__restrict__ y, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = gh_log10(x[i]);
}

extern "C" int gh_log10_device(int device, const double *x, double *y, int64_t n)
{
    if (!x || !y || n < 0) return fail(GH_ERR_ARG, "null argument");
    if (n == 0) return GH_OK;
    if (device >= 0) HIPCHK(hipSetDevice(device));
    double *dx = nullptr, *dy = nullptr;
    if (hipMalloc(&dx, n * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return fail(GH_ERR_NOMEM, "hipMalloc of %lld doubles failed", (long long)n); }
    if (hipMalloc(&dy, n * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); hipFree(dx); return fail(GH_ERR_NOMEM, "hipMalloc of %lld doubles failed", (long long)n); }
    int rc = GH_OK;
    if (hipMemcpy(dx, x, n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = fail(GH_ERR_HIP, "hipMemcpy");
    if (rc == GH_OK) {
        k_log10_many<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(dx, dy, n);
        if (hipGetLastError() != hipSuccess || hipMemcpy(y, dy, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(GH_ERR_HIP, "k_log10_many");
    }
    hipFree(dx); hipFree(dy);
    return rc;
}

// the same function compiled for the host (no device touched): the restatement itself against the running libm
extern "C" int gh_log10_host(const double *x, double *y, int64_t n)
{
    if (!x || !y || n < 0) return fail(GH_ERR_ARG, "null argument");
    for (int64_t i = 0; i < n; i++) y[i] = gh_log10(x[i]);
    return GH_OK;
}

static void free_handle(gh_handle *h)
{
    if (!h) return;
    hipSetDevice(h->dev);
    if (h->stream) hipStreamSynchronize(h->stream);
    hipFree(h->band); hipFree(h->tband); hipFree(h->cnt); hipFree(h->marg); hipFree(h->minfo);
    hipFree(h->pipe_pk); hipFree(h->pipe_gp); hipFree(h->pipe_lm); hipFree(h->pipe_gw);
    hipFree(h->nvalid); hipFree(h->cmask); hipFree(h->rinfo); hipFree(h->lt); hipFree(h->ht); hipFree(h->yt); hipFree(h->dstate); hipFree(h->partial);
    hipFree(h->spin_paths); hipFree(h->spin_recs);
    hipFree(h->d_path); hipFree(h->d_rw_path); hipFree(h->d_rec);
    hipFree(h->seg_hist); hipFree(h->seg_maps); hipFree(h->seg_pmaps); hipFree(h->seg_gmaps); hipFree(h->seg_min); hipFree(h->lmsel1); hipFree(h->spin_lmsel);
    hipFree(h->seg_smin); hipFree(h->seg_gmin); hipFree(h->cm5snap); hipFree(h->seg_halo);
    if (h->stage) hipHostFree(h->stage);
    hipFree(h->ew_buf); hipFree(h->asg.buf); hipFree(h->score.buf); hipFree(h->beam.buf); hipFree(h->vit.buf);
    hipFree(h->cw_keys_d); hipFree(h->cw_exits_d); hipFree(h->cw_pend_d); hipFree(h->cw_pend_exit_d);
    hipFree(h->cw_pend_exit); hipFree(h->cw_pend_ready); hipFree(h->cw_phist);
    hipFree(h->cw_keys); hipFree(h->cw_exits); hipFree(h->cw_hist); hipFree(h->cw_last_hit); hipFree(h->cw_npool); hipFree(h->cw_walked); hipFree(h->cw_nxt); hipFree(h->cw_true); hipFree(h->cw_pend); hipFree(h->cw_npend);
    for (int k = 0; k < GH_K_COUNT; k++)
        for (hipEvent_t e : h->ps[k].ev) hipEventDestroy(e);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

extern "C" int gh_create(const gh_config *cfg, gh_t **out)
{
    if (!cfg || !out) return fail(GH_ERR_ARG, "null argument");
    if (cfg->n_snps < 1) return fail(GH_ERR_ARG, "n_snps must be >= 1 (got %d)", cfg->n_snps);
    if (cfg->band < 1) return fail(GH_ERR_ARG, "band must be >= 1 (got %d)", cfg->band);
    if (cfg->storage != GH_STORAGE_F32 && cfg->storage != GH_STORAGE_F64)
        return fail(GH_ERR_ARG, "bad storage %d", cfg->storage);
    if (cfg->cond_mode < 0 || cfg->cond_mode > GH_COND_E) return fail(GH_ERR_ARG, "bad cond_mode %d", cfg->cond_mode);
    uint8_t order[5] = {0, 1, 2, 3, 5};
    {
        bool all_zero = true;
        for (int q = 0; q < 8; q++) all_zero = all_zero && cfg->cand_order[q] == 0;
        if (!all_zero) {
            unsigned seen = 0;
            for (int q = 0; q < 5; q++) {
                if (cfg->cand_order[q] > 5 || cfg->cand_order[q] == 4) return fail(GH_ERR_ARG, "cand_order[%d] = %d is not a valid symbol index", q, cfg->cand_order[q]);
                seen |= 1u << cfg->cand_order[q];
                order[q] = cfg->cand_order[q];
            }
            if (seen != 0x2Fu) return fail(GH_ERR_ARG, "cand_order is not a permutation of the valid symbols {0,1,2,3,5}");
        }
    }
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(GH_ERR_HIP, "no HIP device visible");
    int dev = cfg->device;
    if (dev < 0) HIPCHK(hipGetDevice(&dev));
    if (dev >= ndev) return fail(GH_ERR_ARG, "device %d out of range (%d devices)", dev, ndev);
    HIPCHK(hipSetDevice(dev));
    int rc = init_constants();
    if (rc) return rc;

    gh_handle *h = new (std::nothrow) gh_handle();
    if (!h) return fail(GH_ERR_NOMEM, "host allocation failed");
    h->cfg = *cfg;
    h->cfg.device = dev;
    h->cfg.offer_zero = cfg->offer_zero ? 1 : 0;
    memset(h->cfg.cand_order, 0, sizeof h->cfg.cand_order);
    memcpy(h->cfg.cand_order, order, 5);
    h->sm = make_symmap(order);
    h->need_rinfo = cfg->marginal_term != 0 || env_int("GH_FUSE", 0) >= 1;
    h->dev = dev;
    h->N = cfg->n_snps;
    h->W = cfg->band;
    h->n_cells = (size_t)(h->N + 2) * h->W;
    const size_t np = (size_t)h->N + 2;
#define ALLOC(ptr, bytes)                                                                     \
    do {                                                                                      \
        hipError_t e_ = hipMalloc((void **)&(ptr), (bytes));                                  \
        if (e_ != hipSuccess) {                                                               \
            free_handle(h);                                                                   \
            return fail(GH_ERR_NOMEM, "hipMalloc(%zu) failed: %s", (size_t)(bytes),           \
                        hipGetErrorString(e_));                                               \
        }                                                                                     \
    } while (0)
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        free_handle(h);
        return fail(GH_ERR_HIP, "hipStreamCreate failed");
    }
    ALLOC(h->band, h->n_cells * CELL * esize(h));
    ALLOC(h->cnt, np * 8 * sizeof(double));
    ALLOC(h->marg, np * 8 * sizeof(double));
    ALLOC(h->minfo, np * MINFO * sizeof(double));
    ALLOC(h->nvalid, np * sizeof(int32_t));
    ALLOC(h->cmask, np * sizeof(uint32_t));
    ALLOC(h->rinfo, np * RINFO * sizeof(double));
    ALLOC(h->dstate, sizeof(dev_state));
    ALLOC(h->d_path, np);
    ALLOC(h->d_rw_path, np);
    ALLOC(h->d_rec, sizeof(gh_path_rec));
#undef ALLOC
    hipMemsetAsync(h->band, 0, h->n_cells * CELL * esize(h), h->stream);
    hipMemsetAsync(h->dstate, 0, sizeof(dev_state), h->stream);
    hipMemsetAsync(h->minfo, 0, np * MINFO * sizeof(double), h->stream);
    hipMemsetAsync(h->rinfo, 0, np * RINFO * sizeof(double), h->stream);
    hipMemsetAsync(h->cmask, 0, np * sizeof(uint32_t), h->stream);
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = h;
    return GH_OK;
}

extern "C" int gh_destroy(gh_t *h)
{
    free_handle(h);
    return GH_OK;
}

extern "C" int gh_sync(gh_t *h)
{
    if (!h) return fail(GH_ERR_ARG, "null handle");
    if (set_dev(h)) return GH_ERR_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    return GH_OK;
}

extern "C" int gh_clear(gh_t *h)
{
    if (!h) return fail(GH_ERR_ARG, "null handle");
    if (set_dev(h)) return GH_ERR_HIP;
    HIPCHK(hipMemsetAsync(h->band, 0, h->n_cells * CELL * esize(h), h->stream));
    HIPCHK(hipMemsetAsync(h->dstate, 0, sizeof(dev_state), h->stream));
    memset(h->fill_seen, 0, sizeof h->fill_seen);
    memset(&h->stats, 0, sizeof h->stats);
    h->stats.L = 1;
    h->L = 1;
    h->dirty_marg = h->dirty_lt = true; h->lt_inc_path = nullptr; h->band_zero = true; h->band_epoch++;
    h->have_orig = false;
    h->cw_ready = false; h->cw_off = false;
    return GH_OK;
}

extern "C" int gh_copy(const gh_t *src, gh_t **out)
{
    if (!src || !out) return fail(GH_ERR_ARG, "null argument");
    gh_t *h = nullptr;
    int rc = gh_create(&src->cfg, &h);
    if (rc) return rc;
    hipStreamSynchronize(src->stream);
    // device-to-device copies are asynchronous to the host: order it on the new handle's stream
    hipError_t e = hipMemcpyAsync(h->band, src->band, src->n_cells * CELL * esize(src), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { free_handle(h); return fail(GH_ERR_HIP, "copy failed: %s", hipGetErrorString(e)); }
    h->L = src->L;
    h->stats = src->stats;
    h->band_zero = src->band_zero;
    *out = h;
    return GH_OK;
}

extern "C" int gh_set_L(gh_t *h, int32_t L)
{
    if (!h) return fail(GH_ERR_ARG, "null handle");
    if (L < 1) return fail(GH_ERR_ARG, "L must be >= 1 (got %d)", L);
    if (L > 32767) return fail(GH_ERR_ARG, "L > 32767 unsupported (got %d)", L);
    if (L != h->L) { h->dirty_lt = true; h->cw_ready = false; }
    h->L = L;
    h->stats.L = L;
    return GH_OK;
}

extern "C" int gh_get_L(const gh_t *h, int32_t *L)
{
    if (!h || !L) return fail(GH_ERR_ARG, "null argument");
    *L = h->L;
    return GH_OK;
}

extern "C" int gh_get_fill_stats(const gh_t *h, gh_fill_stats *out)
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    *out = h->stats;
    out->L = h->L;
    return GH_OK;
}

extern "C" int gh_set_fill_stats(gh_t *h, const gh_fill_stats *in)
{
    if (!h || !in) return fail(GH_ERR_ARG, "null argument");
    h->stats.n_slices = in->n_slices;
    h->stats.n_crumbs = in->n_crumbs;
    h->stats.covered_snps = in->covered_snps;
    return GH_OK;
}

// reads ---------------------------------------------------------------------------------------
extern "C" int gh_reads_upload(const gh_t *h, const int32_t *rank, const int64_t *off,
                               const uint8_t *bases, int64_t n_reads, gh_reads_t **out)
{
    if (!h || !out || n_reads < 0 || (n_reads > 0 && (!rank || !off))) return fail(GH_ERR_ARG, "bad argument");
    if (set_dev(h)) return GH_ERR_HIP;
    gh_reads *r = new (std::nothrow) gh_reads();
    if (!r) return fail(GH_ERR_NOMEM, "host allocation failed");
    r->dev = h->dev;
    r->n_reads = n_reads;
    r->n_bases = n_reads ? off[n_reads] : 0;
    r->rank = nullptr; r->off = nullptr; r->bases = nullptr;
    r->max_k = 0;
    r->sorted = true;
    r->span_pos = 0;
    r->dens128 = 0;
    r->first_at = nullptr; r->n_first = 0;
    // The table's properties (longest read, off[] ascending, ranks ascending and then span / density / first_at) are found on the
    // device behind the copies (k_reads_meta): the host looks at the two ends of rank[] only, to size first_at for a table that
    // turns out to be sorted.  Page-locked sources (gh_host_alloc: what gretel_amd.util.load_from_bam decodes into) are read by DMA.
    int64_t top = 0;
    if (n_reads > 0 && rank[0] >= 0 && rank[n_reads - 1] >= rank[0]) {
        top = (int64_t)rank[n_reads - 1] + 2;
        if (top > ((int64_t)1 << 28)) top = 0;
    }
    reads_meta *dm = nullptr;
    reads_meta hm;
    hm.max_k = 0; hm.unsorted = 0; hm.bad_off = 0x7fffffffffffffffll; hm.span = 0; hm.dens128 = 0;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMalloc((void **)&r->rank, (size_t)(n_reads ? n_reads : 1) * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&r->off, (size_t)(n_reads + 1) * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&r->bases, (size_t)(r->n_bases ? r->n_bases : 1));
    if (e == hipSuccess && top > 0) e = hipMalloc((void **)&r->first_at, (size_t)top * 8);
    if (e == hipSuccess && n_reads) e = hipMalloc((void **)&dm, sizeof(reads_meta));
    if (e == hipSuccess && n_reads) e = hipMemcpyAsync(dm, &hm, sizeof hm, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && n_reads) e = hipMemcpyAsync(r->rank, rank, (size_t)n_reads * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && n_reads) e = hipMemcpyAsync(r->off, off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && n_reads) {
        const int grid = (int)std::min<int64_t>((n_reads + 256) / 256, 2048);
        k_reads_meta<<<grid, 256, 0, h->stream>>>(r->rank, r->off, n_reads, dm);
        if (top > 0) k_reads_first_at<<<grid, 256, 0, h->stream>>>(r->rank, n_reads, r->first_at, top, dm);
        k_reads_meta2<<<grid, 256, 0, h->stream>>>(r->rank, n_reads, r->first_at, FILL_RPB, dm);
        e = hipGetLastError();
    }
    if (e == hipSuccess && r->n_bases) e = hipMemcpyAsync(r->bases, bases, (size_t)r->n_bases, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && n_reads) e = hipMemcpyAsync(&hm, dm, sizeof hm, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    hipFree(dm);
    if (e != hipSuccess) {
        hipFree(r->rank); hipFree(r->off); hipFree(r->bases); hipFree(r->first_at);
        delete r;
        return fail(GH_ERR_HIP, "upload failed: %s", hipGetErrorString(e));
    }
    if (hm.bad_off != 0x7fffffffffffffffll) {
        hipFree(r->rank); hipFree(r->off); hipFree(r->bases); hipFree(r->first_at);
        delete r;
        return fail(GH_ERR_ARG, "off[] not monotone at read %lld", hm.bad_off);
    }
    r->max_k = hm.max_k;
    r->sorted = !hm.unsorted;
    if (r->sorted && n_reads > 0) {
        r->span_pos = hm.span + r->max_k + 1;             // the slice k_fill_sorted counts in LDS
        if (r->first_at) { r->n_first = (int)top; r->dens128 = hm.dens128; }
        else {
            // (ranks ascend from a negative one, or reach beyond 2^28: no first_at; the density the slow way)
            int64_t lo = 0;
            for (int64_t q = 0; q < n_reads; q++) {
                while (rank[q] - rank[lo] >= 128) lo++;
                if (q - lo + 1 > r->dens128) r->dens128 = q - lo + 1;
            }
        }
    } else if (r->first_at) {
        hipFree(r->first_at);
        r->first_at = nullptr;
    }
    *out = r;
    return GH_OK;
}

extern "C" int gh_reads_max_k(const gh_reads_t *r, int32_t *max_k)
{
    if (!r || !max_k) return fail(GH_ERR_ARG, "bad argument");
    *max_k = r->max_k;
    return GH_OK;
}

extern "C" int gh_reads_info(const gh_reads_t *r, int64_t info[5], int64_t *first_at)
{
    if (!r || !info) return fail(GH_ERR_ARG, "bad argument");
    info[0] = r->max_k; info[1] = r->sorted ? 1 : 0; info[2] = r->span_pos; info[3] = r->dens128; info[4] = r->first_at ? r->n_first : 0;
    if (first_at && r->first_at) {
        HIPCHK(hipSetDevice(r->dev));
        HIPCHK(hipMemcpy(first_at, r->first_at, (size_t)r->n_first * 8, hipMemcpyDeviceToHost));
    }
    return GH_OK;
}

extern "C" int gh_reads_free(gh_reads_t *r)
{
    if (!r) return GH_OK;
    hipSetDevice(r->dev);
    hipFree(r->rank); hipFree(r->off); hipFree(r->bases); hipFree(r->first_at);
    delete r;
    return GH_OK;
}

static int pull_fill_state(gh_handle *h, const char *what)
{
    dev_state hs;
    HIPCHK(hipMemcpyAsync(&hs, h->dstate, sizeof hs, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    unsigned long long before[6];
    memcpy(before, h->fill_seen, sizeof before);
    memcpy(h->fill_seen, hs.fill, sizeof before);
    h->stats.n_slices += (int64_t)(hs.fill[0] - before[0]);
    h->stats.n_crumbs += (int64_t)(hs.fill[1] - before[1]);
    h->stats.covered_snps += (int64_t)(hs.fill[2] - before[2]);
    if (hs.fill[3] != before[3])
        return fail(GH_ERR_SYMBOL, "%s: %llu item(s) carry a symbol outside \"ACGTN-_\"", what,
                    hs.fill[3] - before[3]);
    if (hs.fill[4] != before[4])
        return fail(GH_ERR_BAND, "%s: %llu observation(s) outside band %d / positions [0,%d]", what,
                    hs.fill[4] - before[4], h->W, h->N + 1);
    return GH_OK;
}

extern "C" int gh_fill(gh_t *h, const gh_reads_t *r, int use_end_sentinels, gh_fill_stats *out)
{
    if (!h || !r) return fail(GH_ERR_ARG, "null argument");
    if (r->dev != h->dev) return fail(GH_ERR_ARG, "reads live on device %d, handle on %d", r->dev, h->dev);
    if (set_dev(h)) return GH_ERR_HIP;
    if (r->n_reads > 0) {
        const int block = 256;
        int64_t nb = (r->n_reads + block - 1) / block;
        if (nb > 256 * 32) nb = 256 * 32;
        const double bytes = 8.0 * 0 + (double)r->n_reads * 12.0 + (double)r->n_bases;   // + 8*adds, added below
        prof_begin(h, GH_K_FILL);
        // sorted tables: LDS-privatised counting when a run of reads stays inside a slice that fits in LDS
        static const bool no_sorted = env_int("GH_FILL_SCATTER", 0) != 0;
        const int rpb = FILL_RPB;                                 // reads per workgroup
        int max_pos = 0;
        if (r->sorted && !no_sorted) {
            // LDS for the widest slice any workgroup needs (known from the upload), at most 96 KB: several
            // workgroups per CU when the slices are narrow; what falls outside a slice goes to global atomics
            const size_t per_pos = (size_t)h->W * CELL * sizeof(unsigned);
            max_pos = (int)((96 * 1024) / per_pos);
            if (max_pos > 1024) max_pos = 1024;
            if (r->span_pos > 0 && r->span_pos < max_pos) max_pos = r->span_pos > r->max_k + 8 ? r->span_pos : r->max_k + 8;
        }
        // rank-sorted tables: the tensor cut by owner (k_fill_own) -- no global atomics -- when a slice of from-positions wide enough
        // to keep the overlap between neighbours small fits the LDS: P positions x W x 49 counters of 2 bytes (4 where a workgroup
        // may see 65 536 reads).  GH_FILL_OWN=0 keeps the older fills (the tests run them against each other).
        int own_P = 0;
        bool own_half = true;
        if (r->sorted && r->first_at && !no_sorted && !env_off("GH_FILL_OWN")) {
            int P = (h->N + 2 + 1023) / 1024;                    // about a thousand workgroups ...
            if (P < 2 * r->max_k) P = 2 * r->max_k;              // ... that visit a read 1.5 times at most
            if (P < 8) P = 8;
            // the reads one workgroup can see: ranks within P + max_k positions
            const int64_t win = (int64_t)((P + r->max_k + 127) / 128 + 1) * r->dens128;
            own_half = win < 65536 && !env_int("GH_FILL_OWN_WIDE", 0);      // (the tests force the 4-byte counters)
            const size_t per_pos = (size_t)h->W * CELL * (own_half ? 2 : 4);
            const int P_lds = (int)((150 * 1024 - FILL_OWN_SYMS) / per_pos);
            if (P > P_lds) P = P_lds;
            if (P >= r->max_k && P >= 8 && r->max_k <= FILL_OWN_SYMS) own_P = P;               // (narrower: every read would be visited by many workgroups)
        }
        with_storage(h, [&](auto z) {
            using T = decltype(z);
            if (own_P > 0) {
                const unsigned gb = (unsigned)((h->N + 2 + own_P - 1) / own_P);
                const size_t sym_off = (((size_t)own_P * h->W * CELL * (own_half ? 2 : 4)) + 15) & ~(size_t)15;
                const size_t lds = sym_off + FILL_OWN_SYMS;
#define FILL_OWN(CT_, Z_, G_) do {                                                                                                       \
                    lds_limit<k_fill_own<T, CT_, Z_, G_>>(lds, h->dev);                                                                  \
                    hipLaunchKernelGGL((k_fill_own<T, CT_, Z_, G_>), dim3(gb), dim3(1024), lds, h->stream, (T *)h->band, h->N, h->W, r->rank, \
                                       r->off, r->bases, r->n_reads, own_P, r->max_k, use_end_sentinels, h->dstate, r->first_at, r->n_first, (int)sym_off); \
                } while (0)
                // lanes per read: one for short reads, four / eight for long ones (a lane takes every G-th from-index of its read)
#define FILL_OWN_G(CT_, Z_) do { if (r->max_k <= 8) FILL_OWN(CT_, Z_, 1); else if (r->max_k <= 32) FILL_OWN(CT_, Z_, 4); else FILL_OWN(CT_, Z_, 8); } while (0)
#define FILL_OWN_Z(CT_) do { if (h->band_zero) FILL_OWN_G(CT_, true); else FILL_OWN_G(CT_, false); } while (0)
                if (own_half) FILL_OWN_Z(uint16_t); else FILL_OWN_Z(uint32_t);
#undef FILL_OWN_G
#undef FILL_OWN_Z
#undef FILL_OWN
            } else if (max_pos >= r->max_k + 8) {
                const unsigned gb = (unsigned)((r->n_reads + rpb - 1) / rpb);
                const size_t lds = (size_t)max_pos * h->W * CELL * sizeof(unsigned);
                lds_limit<k_fill_sorted<T>>(lds, h->dev);
                hipLaunchKernelGGL(k_fill_sorted<T>, dim3(gb), dim3(block), lds, h->stream, (T *)h->band, h->N, h->W,
                                   r->rank, r->off, r->bases, r->n_reads, rpb, max_pos, r->max_k, use_end_sentinels, h->dstate);
            } else if (r->max_k >= FILL_PAIRS_MIN_K && r->max_k <= 32 && !env_off("GH_FILL_PAIRS")) {
                // long reads, sparse tensor: 32 lanes per read (k_fill_pairs)
                int64_t nbp = (r->n_reads * 32 + block - 1) / block;
                if (nbp > 256 * 64) nbp = 256 * 64;
                hipLaunchKernelGGL(k_fill_pairs<T>, dim3((unsigned)nbp), dim3(block), 0, h->stream, (T *)h->band,
                                   h->N, h->W, r->rank, r->off, r->bases, r->n_reads, use_end_sentinels, h->dstate);
            } else
                hipLaunchKernelGGL(k_fill<T>, dim3((unsigned)nb), dim3(block), 0, h->stream, (T *)h->band,
                                   h->N, h->W, r->rank, r->off, r->bases, r->n_reads, use_end_sentinels, h->dstate);
        });
        prof_end(h, GH_K_FILL, bytes);
        { int rc_ = post_launch(h, "k_fill"); if (rc_) return rc_; }
    }
    h->dirty_marg = h->dirty_lt = true; h->lt_inc_path = nullptr; if (r->n_reads > 0) h->band_zero = false; h->band_epoch++;
    h->cw_ready = false; h->cw_off = false;
    int rc = pull_fill_state(h, "gh_fill");
    if (h->stats.n_slices > 0) {                                   // util.py:333
        int L = (int)std::ceil((double)h->stats.covered_snps / (double)h->stats.n_slices);
        if (L < 1) L = 1;
        h->L = L;
        h->stats.L = L;
    }
    if (h->prof) {
        // algorithmic bytes: one 4/8-byte read-modify-write per add_observation + the table itself
        h->ps[GH_K_FILL].bytes = 2.0 * esize(h) * (double)h->stats.n_crumbs * 1.0 + (double)r->n_reads * 12.0 + (double)r->n_bases;
    }
    if (out) { *out = h->stats; out->L = h->L; }
    return rc;
}

// one-cell API --------------------------------------------------------------------------------
static int cell_index(const gh_handle *h, int a, int b, int i, int j, size_t *idx)
{
    if (a < 0 || a >= NSYM || b < 0 || b >= NSYM) return fail(GH_ERR_SYMBOL, "symbol index out of range (%d,%d)", a, b);
    int d = j - i;
    if (i < 0 || j > h->N + 1 || d < 1 || d > h->W) return 1;    // outside the band: a zero cell
    *idx = bidx(h->W, (size_t)i, d, a, b);
    return 0;
}

extern "C" int gh_get(gh_t *h, int a, int b, int i, int j, double *out)
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    if (set_dev(h)) return GH_ERR_HIP;
    size_t idx;
    int rc = cell_index(h, a, b, i, j, &idx);
    if (rc < 0) return rc;
    if (rc == 1) { *out = 0.0; return GH_OK; }
    return with_storage(h, [&](auto z) -> int {
        using T = decltype(z);
        HIPCHK(hipMemcpyAsync(&z, (T *)h->band + idx, sizeof z, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        *out = (double)z;
        return GH_OK;
    });
}

extern "C" int gh_add_batch(gh_t *h, const uint8_t *a, const uint8_t *b, const int32_t *i, const int32_t *j, int64_t n)
{
    if (!h || n < 0 || (n > 0 && (!a || !b || !i || !j))) return fail(GH_ERR_ARG, "bad argument");
    if (n == 0) return GH_OK;
    if (set_dev(h)) return GH_ERR_HIP;
    uint8_t *da = nullptr, *db = nullptr;
    int32_t *di = nullptr, *dj = nullptr;
    hipError_t e = hipMalloc((void **)&da, n);
    if (e == hipSuccess) e = hipMalloc((void **)&db, n);
    if (e == hipSuccess) e = hipMalloc((void **)&di, n * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&dj, n * 4);
    if (e == hipSuccess) e = hipMemcpy(da, a, n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(db, b, n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(di, i, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dj, j, n * 4, hipMemcpyHostToDevice);
    int rc = GH_OK;
    if (e != hipSuccess) rc = fail(GH_ERR_HIP, "gh_add_batch staging failed: %s", hipGetErrorString(e));
    if (rc == GH_OK) {
        const int block = 256;
        const unsigned nb = (unsigned)((n + block - 1) / block);
        with_storage(h, [&](auto z) {
            using T = decltype(z);
            hipLaunchKernelGGL(k_add_batch<T>, dim3(nb), dim3(block), 0, h->stream, (T *)h->band, h->N, h->W, da, db, di, dj, n, h->dstate);
        });
        h->dirty_marg = h->dirty_lt = true; h->lt_inc_path = nullptr; h->band_zero = false; h->band_epoch++;
        int64_t s0 = h->stats.n_slices, c0 = h->stats.n_crumbs, v0 = h->stats.covered_snps;
        rc = pull_fill_state(h, "gh_add_batch");
        h->stats.n_slices = s0; h->stats.n_crumbs = c0; h->stats.covered_snps = v0;
    }
    hipFree(da); hipFree(db); hipFree(di); hipFree(dj);
    return rc;
}

extern "C" int gh_add(gh_t *h, int a, int b, int i, int j)
{
    if (a < 0 || a >= NSYM || b < 0 || b >= NSYM) return fail(GH_ERR_SYMBOL, "symbol index out of range (%d,%d)", a, b);
    uint8_t ua = (uint8_t)a, ub = (uint8_t)b;
    int32_t ii = i, jj = j;
    return gh_add_batch(h, &ua, &ub, &ii, &jj, 1);
}

extern "C" int gh_reweight_obs(gh_t *h, int a, int b, int i, int j, double ratio, double *removed)
{
    if (!h) return fail(GH_ERR_ARG, "null handle");
    if (set_dev(h)) return GH_ERR_HIP;
    size_t idx;
    int rc = cell_index(h, a, b, i, j, &idx);
    if (rc < 0) return rc;
    double rem = 0.0;
    if (rc == 0) {
        double *d_rem = &h->d_rec->magnitude;
        with_storage(h, [&](auto z) {
            using T = decltype(z);
            hipLaunchKernelGGL(k_reweight_one<T>, dim3(1), dim3(1), 0, h->stream, (T *)h->band + idx, ratio, d_rem);
        });
        HIPCHK(hipMemcpyAsync(&rem, d_rem, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->dirty_marg = h->dirty_lt = true; h->lt_inc_path = nullptr; h->band_epoch++;
    }
    if (removed) *removed = rem;
    return GH_OK;
}

// tables --------------------------------------------------------------------------------------
static int ensure_marg(gh_handle *h)
{
    if (!h->dirty_marg) return GH_OK;
    const int threads = (h->N + 1) * 8;
    const int block = 256;
    // re-arm the "first SNP without a candidate" word that k_marg min-reduces into
    HIPCHK(hipMemsetAsync(&h->dstate->first_hole, 0x7f, 4 * sizeof(int), h->stream));   // first_hole, nodel, cm_same, narrow
    prof_begin(h, GH_K_MARG);
    launch_marg<false>(h, dim3((threads + block - 1) / block), h->stream, marg_of(h));
    // algorithmic bytes: read the (p,p+1) cell, write cnt/marg (2x64), minfo (88), nvalid+cmask (8)
    prof_end(h, GH_K_MARG, (double)(h->N + 1) * (CELL * esize(h) + 2 * 64 + 88 + 8));
    { int rc_ = post_launch(h, "k_marg"); if (rc_) return rc_; }
    h->dirty_marg = false;
    return GH_OK;
}

static int alloc_lt(gh_handle *h);
// may the fused reweight keep the conditional table current (k_marg<T,true> rewrites the rows a path changes)?
// k_marg<T,true> (behind the serial walkers, gh_reweight_path): rows only -- conditionals whose denominator is a row sum or a
// marginal count, and no marginal term baked into the table
static bool lt_incremental_ok(const gh_handle *h)
{
    return h->cfg.cond_mode != GH_COND_C && h->cfg.cond_mode != GH_COND_E && !h->cfg.marginal_term && !h->lt_full;
}
// k_rw (behind the segment-parallel walks, which add the marginal term themselves): every conditional -- rows, or columns for C and E
static bool rw_incremental_ok(const gh_handle *h) { return !h->lt_full && !h->lt_baked; }
static bool walk_depth2_ok(int wm, int L);
static bool walk_ranked_ok(int wm, int L);
static bool seg_ok(int wm, int L);

// baked: the table is for a serial walker, which reads whole rows: with the marginal term its lag-1 entries hold lm + x1
// (k_lt); the segment-parallel walks want the bare conditionals and add lm themselves
// derived = false (the candidate pools' looks): the depth-2 serial walker's tables Ht / Yt are left alone -- nobody reads them
// until a serial walk, in front of which the table is rebuilt in full anyway (45 us per look at C5 otherwise)
// the mixed-radix state space (segmix.hpp) for this handle?  L = 5 over the segment-parallel extension; not where every symbol is
// offered everywhere (five candidates at every position: nothing to gain) and not for a spin of the opt-in GH_FUSE flow
// (`enumerated`; false outside spins), whose k_seg / k_scan / k_rw carry the minima over the enumerated states
static bool mixed_ok(bool on, bool enumerated, int L, int wm, int offer_zero) { return on && !enumerated && L == SEGM_L && wm == WM_SEG && !offer_zero; }
static bool mixed_on() { static const bool on = !env_off("GH_MIXED"); return on; }      // (read once per process)
static bool mixed_allowed(const gh_handle *h, bool enumerated) { return mixed_ok(mixed_on(), enumerated, h->L, h->wmode, h->cfg.offer_zero); }

static int ensure_lt(gh_handle *h, bool baked = false, bool derived = true, bool enumerated = false)
{
    int rc = ensure_marg(h);
    if (rc) return rc;
    const bool want_baked = baked && h->cfg.marginal_term;
    const bool need_derived = derived && h->ht_stale;
    if (!h->dirty_lt && h->lt && h->lt_L == h->L && h->lt_baked == want_baked && !need_derived) return GH_OK;
    if ((rc = alloc_lt(h))) return rc;
    // what kept the table current since the last build: k_marg<T,true> behind a serial walker (rows, conditionals A / B without the
    // marginal term), or k_rw / k_rwseg behind a segment-parallel walk (every conditional: rows or columns; the derived tables of the
    // depth-2 serial walker are refreshed by ROWS only, so under a column conditional or the marginal term a caller that wants those
    // gets a full build).  Round 3 rebuilt the whole table at every look of a pool spin under C / E / the marginal term.
    const bool col_or_mt = h->cfg.cond_mode == GH_COND_C || h->cfg.cond_mode == GH_COND_E || h->cfg.marginal_term;
    const bool inc_rule = h->lt_inc_seg ? (rw_incremental_ok(h) && (!col_or_mt || !derived)) : lt_incremental_ok(h);
    const bool inc_ok = h->lt_inc_path && inc_rule && h->lt_baked == want_baked && !need_derived;
    const uint8_t *inc = inc_ok ? h->lt_inc_path : nullptr;
    const size_t total = inc ? (size_t)h->N * 4 : (size_t)(h->N + LT_PAD) * h->L * LT_BLK;
    const int block = 256;
    size_t nb = (total + block - 1) / block;
    if (nb > 256 * 16) nb = 256 * 16;
    // (column conditionals: the to-major copy, while it mirrors the band, makes the column sums contiguous reads)
    const void *tb_lt = tband_current(h);
    lt_args a;
    a.band = h->band; a.N = h->N; a.W = h->W; a.L = h->L; a.cond_mode = h->cfg.cond_mode; a.bake_lm = want_baked ? 1 : 0;
    a.cnt = h->cnt; a.nvalid = h->nvalid; a.cmask = h->cmask; a.minfo = h->minfo; a.G = h->lt; a.st = h->dstate; a.inc_path = inc;
    a.allow_ranked = walk_ranked_ok(h->wmode, h->L);
    a.Ht = derived ? h->ht : nullptr; a.Yt = derived ? h->yt : nullptr; a.sm = h->sm; a.tband = tb_lt;
    prof_begin(h, GH_K_LT);
    launch_lt(h, dim3((unsigned)nb), h->stream, a);
    const int wl = h->W < h->L ? h->W : h->L;
    // algorithmic bytes: full = read the band cells within reach + write G; after a fused reweight = the two flags
    prof_end(h, GH_K_LT, inc ? 8.0
                             : (double)h->N * ((double)wl * CELL * esize(h) + (double)h->L * LT_BLK * 8.0));
    { int rc_ = post_launch(h, "k_lt"); if (rc_) return rc_; }
    // mixed radix for the segment-parallel extension (segmix.hpp): how many states enter a target at most, taken whenever the table
    // may have been rebuilt (k_lt zeroes it then; behind an incremental refresh the old bound stands: candidates only disappear)
    if (mixed_allowed(h, enumerated)) {
        hipLaunchKernelGGL(k_classify, dim3((unsigned)((h->N + 255) / 256)), dim3(256), 0, h->stream, (const uint32_t *)h->cmask, h->N, h->L, h->dstate);
        int rc_ = post_launch(h, "k_classify"); if (rc_) return rc_;
    }
    h->dirty_lt = false;
    h->lt_inc_path = nullptr;
    h->lt_baked = want_baked;
    if (inc && !derived && h->ht) h->ht_stale = true;       // (a full build writes them from the band whatever `derived` says -- k_lt)
    else if (!inc) h->ht_stale = !derived && h->ht != nullptr;
    return GH_OK;
}

extern "C" int gh_counts_at(gh_t *h, int p, double out[8])
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    if (p < 0 || p > h->N) return fail(GH_ERR_ARG, "position %d outside [0,%d]", p, h->N);
    if (set_dev(h)) return GH_ERR_HIP;
    int rc = ensure_marg(h);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, h->cnt + (size_t)p * 8, 64, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GH_OK;
}

extern "C" int gh_marginal_of_at(gh_t *h, int s, int p, double *out)
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    if (s < 0 || s >= NSYM) return fail(GH_ERR_SYMBOL, "symbol index %d out of range", s);
    if (p < 0 || p > h->N) return fail(GH_ERR_ARG, "position %d outside [0,%d]", p, h->N);
    if (set_dev(h)) return GH_ERR_HIP;
    int rc = ensure_marg(h);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, h->marg + (size_t)p * 8 + s, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GH_OK;
}

extern "C" int gh_edge_weights_at(gh_t *h, int p, const uint8_t *path, double w[GH_NSYM], int *cand_mask)
{
    if (!h || !path || !w || !cand_mask) return fail(GH_ERR_ARG, "null argument");
    if (p < 1 || p > h->N) return fail(GH_ERR_ARG, "position %d outside [1,%d]", p, h->N);
    if (set_dev(h)) return GH_ERR_HIP;
    int rc = ensure_marg(h);
    if (rc) return rc;
    const int lmax = h->L < p ? h->L : p;
    std::vector<uint8_t> hist(lmax);
    for (int l = 1; l <= lmax; l++) {
        if (path[p - l] >= NSYM) return fail(GH_ERR_SYMBOL, "path[%d] = %d is not a symbol index", p - l, path[p - l]);
        hist[l - 1] = path[p - l];
    }
    // (the handle's own scratch: the lone-path buffer holds the history, eight doubles the answer -- no allocation per call)
    uint8_t *d_hist = h->d_path;
    if (!h->ew_buf && hipMalloc((void **)&h->ew_buf, 8 * sizeof(double)) != hipSuccess) return fail(GH_ERR_NOMEM, "hipMalloc failed");
    double *d_w = h->ew_buf;
    hipError_t e = hipMemcpyAsync(d_hist, hist.data(), lmax, hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess) return fail(GH_ERR_HIP, "gh_edge_weights_at failed: %s", hipGetErrorString(e));
    with_storage(h, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(k_edge_weights<T>, dim3(1), dim3(64), 0, h->stream, (const T *)h->band, h->W, h->cfg.cond_mode, p, h->L,
                           h->cfg.marginal_term, h->cnt, h->marg, h->nvalid, h->cmask, d_hist, d_w, (int *)(d_w + 7));
    });
    double hw[8];
    e = hipMemcpyAsync(hw, d_w, sizeof hw, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(GH_ERR_HIP, "gh_edge_weights_at failed: %s", hipGetErrorString(e));
    memcpy(w, hw, 7 * sizeof(double));
    memcpy(cand_mask, &hw[7], sizeof(int));
    return GH_OK;
}

extern "C" int gh_gap_check(gh_t *h, int *first_gap)
{
    if (!h || !first_gap) return fail(GH_ERR_ARG, "null argument");
    if (set_dev(h)) return GH_ERR_HIP;
    int rc = ensure_marg(h);
    if (rc) return rc;
    int *d_gap = reinterpret_cast<int *>(&h->dstate->fill[5]);      // (a spare word of the state)
    int big = 0x7fffffff;
    HIPCHK(hipMemcpyAsync(d_gap, &big, 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_gap, dim3((h->N + 1 + 255) / 256), dim3(256), 0, h->stream, h->cnt, h->N, d_gap);
    int g;
    HIPCHK(hipMemcpyAsync(&g, d_gap, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *first_gap = (g == big) ? -1 : g;
    return GH_OK;
}

extern "C" int gh_export_cmask(gh_t *h, uint32_t *out)
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    if (set_dev(h)) return GH_ERR_HIP;
    int rc = ensure_marg(h);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, h->cmask, (size_t)(h->N + 1) * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int p = 0; p <= h->N; p++) out[p] = CM_CAND(out[p]);      // (the device word also carries the symbols seen: kernels.hpp)
    return GH_OK;
}

extern "C" int gh_snapshot_original(gh_t *h)
{
    if (!h) return fail(GH_ERR_ARG, "null handle");
    if (set_dev(h)) return GH_ERR_HIP;
    int rc = ensure_marg(h);
    if (rc) return rc;
    hipLaunchKernelGGL(k_snapshot, dim3(((h->N + 1) * 8 + 255) / 256), dim3(256), 0, h->stream, h->minfo, h->minfo, h->N, (const win_desc *)nullptr);
    { int rc_ = post_launch(h, "k_snapshot"); if (rc_) return rc_; }
    h->have_orig = true;
    return GH_OK;
}

static int alloc_lt(gh_handle *h)
{
    if (h->lt && h->lt_L == h->L) return GH_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->lt) hipFree(h->lt);
    if (h->ht) hipFree(h->ht);
    if (h->yt) hipFree(h->yt);
    h->lt = nullptr; h->ht = nullptr; h->yt = nullptr;
    size_t bytes = (size_t)(h->N + LT_PAD) * h->L * LT_BLK * sizeof(double);
    hipError_t e = hipMalloc((void **)&h->lt, bytes);
    if (e == hipSuccess && walk_depth2_ok(h->wmode, h->L) && !seg_ok(h->wmode, h->L)) {
        // the tables the depth-2 walker's loaders copy (k_lt keeps them in step with lt)
        e = hipMalloc((void **)&h->ht, (size_t)(h->N + WALK_TPAD) * 64 * sizeof(double));
        const size_t ypos = (size_t)16 * deep_nyp(h->L);
        if (e == hipSuccess && ypos) e = hipMalloc((void **)&h->yt, (size_t)(h->N + WALK_TPAD) * ypos * sizeof(double));
    }
    if (e != hipSuccess) return fail(GH_ERR_NOMEM, "hipMalloc(%zu) for the conditional table failed", bytes);
    h->lt_L = h->L;
    h->dirty_lt = true; h->lt_inc_path = nullptr;
    return GH_OK;
}

// path extension / reweight -------------------------------------------------------------------
static int walk_threads()
{
    static const int n = env_int("GH_WALK_THREADS", 512);
    return (n >= 192 && n <= 512 && n % 64 == 0) ? n : 512;
}
#define WALK_THREADS walk_threads()
#define WALK_MAX_LC 16

// Which path extension runs.  GH_WALK pins one for A/B measurements and tests; it is read when a handle is created:
//   unset / "seg"   segment-parallel (segwalk.hpp) for L <= SEG_MAX_L, else the serial walkers below
//   "spec"          k_walk_spec: one wavefront, speculation depth 2 where the window allows it, else depth 1
//   "spec1"         k_walk_spec at depth 1       "src"  k_walk_src (no speculation)
static bool seg_ok(int wm, int L) { return wm == WM_SEG && L >= 1 && L <= SEG_MAX_L; }

// Whether the depth-2 walker can run for this L: then k_lt may build G over candidate ranks (kernels.hpp).
static bool walk_depth2_ok(int wm, int L)
{
    const bool off = wm == WM_SRC || wm == WM_SPEC1;
    return !off && L >= 2 && L <= WALK_MAX_LC && walk_chunk(L, false) > 0 && walk_chunk(L, true) > 0 && WALK_THREADS == 512;
}

// candidate-pool segments (cwalk.hpp) for the lag counts above: spins only, narrow windows only (checked on the device)
static bool cw_ok(int wm, int L) { return wm == WM_SEG && L >= CW_MIN_L && L <= CW_MAX_LG; }
// beyond what a 64-bit state holds (2 bits per pick over ranks, 3 over symbols): states as bytes next to their hash, k_cwalkg
static bool cw_digit_mode(const gh_handle *h) { return h->cw_wide ? h->L > CW_MAX_L5 : h->L > CW_MAX_L; }
// ... of which 33..64 lags over ranks and 22..40 over the symbols are walked by k_cwalk2 (registers and an unrolled block, as
// k_cwalk) instead of k_cwalkg (GH_CWALK2=0: k_cwalkg, for the tests and A/B; read per launch)
static bool cw2_ok(const gh_handle *h)
{
    if (env_off("GH_CWALK2")) return false;
    return h->cw_wide ? (h->L > CW_MAX_L5 && h->L <= CW2_MAX_L5) : (h->L > CW_MAX_L && h->L <= CW2_MAX_L);
}

// single windows: may k_lt build the ranked layout?  (the segment-parallel walk reads either layout)
static bool walk_ranked_ok(int wm, int L) { return seg_ok(wm, L) || cw_ok(wm, L) || walk_depth2_ok(wm, L); }

template <int LC>
static void launch_walk_lc(bool spec, size_t lds, hipStream_t stream, const walk_params &P, int grid, const win_desc *wd, int spin)
{
    if (spec) {
        hipFuncSetAttribute((const void *)k_walk_spec<LC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((k_walk_spec<LC>), dim3(grid), dim3(WALK_THREADS), lds, stream, P, wd, spin);
    } else {
        hipFuncSetAttribute((const void *)k_walk_src<LC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((k_walk_src<LC>), dim3(grid), dim3(WALK_THREADS), lds, stream, P, wd, spin);
    }
}

static void launch_walk_src(int LC, bool spec, size_t lds, hipStream_t stream, const walk_params &P, int grid = 1,
                            const win_desc *wd = nullptr, int spin = 0)
{
#define GH_WALK_CASE(n) case n: launch_walk_lc<n>(spec, lds, stream, P, grid, wd, spin); break;
    switch (LC) {
        GH_WALK_CASE(1) GH_WALK_CASE(2) GH_WALK_CASE(3) GH_WALK_CASE(4)
        GH_WALK_CASE(5) GH_WALK_CASE(6) GH_WALK_CASE(7) GH_WALK_CASE(8)
        GH_WALK_CASE(9) GH_WALK_CASE(10) GH_WALK_CASE(11) GH_WALK_CASE(12)
        GH_WALK_CASE(13) GH_WALK_CASE(14) GH_WALK_CASE(15) GH_WALK_CASE(16)
    }
#undef GH_WALK_CASE
}

// launches the path-extension kernel for `grid` windows (grid == 1: the handle's own buffers in P)
static void launch_walk_any(int wm, int N, int L, walk_params P, hipStream_t stream, int grid, const win_desc *wd, int spin)
{
    const int chunk = L <= WALK_MAX_LC ? walk_chunk(L, false) : 0;
    if (chunk > 0) {
        P.chunk = chunk;                    // k_walk_src; k_walk_spec takes walk_chunk(L, variant) itself
        size_t lds = walk_lds_bytes(L, false);
        if (walk_depth2_ok(wm, L) && walk_lds_bytes(L, true) > lds) lds = walk_lds_bytes(L, true);
        const bool spec = wm != WM_SRC;
        P.depth2 = walk_depth2_ok(wm, L);
        launch_walk_src(L, spec, lds, stream, P, grid, wd, spin);
    } else {
        int hl = 16;
        while (hl <= L) hl <<= 1;
        P.chunk = 0; P.depth2 = 0;
        hipLaunchKernelGGL(k_walk_global, dim3(grid), dim3(64), (size_t)hl, stream, P, hl, wd, spin);
    }
}

// ---- segment-parallel walk ---------------------------------------------------------------------
static size_t max2(size_t a, size_t b) { return a > b ? a : b; }
// the largest value of f(class) over the state spaces a lag count can be walked in: 4 (ranked), 5 (symbols, L <= 5), 6 (mixed radix, L = 5);
// which one applies is decided on the device (seg_class), the host sizes for all
template <typename F> static size_t max_cls(int L, F f)
{
    size_t m = f(4);
    if (seg_radix_ok(5, L)) m = max2(m, f(5));
    if (L == SEGM_L) m = max2(m, f(SEG_CLS_MIXED));
    return m;
}

static int alloc_seg(gh_handle *h)
{
    if (h->seg_hist && h->seg_L == h->L) return GH_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    hipFree(h->seg_hist); hipFree(h->seg_maps); hipFree(h->seg_pmaps); hipFree(h->seg_gmaps); hipFree(h->seg_min); hipFree(h->lmsel1);
    hipFree(h->seg_smin); hipFree(h->seg_gmin); hipFree(h->cm5snap);
    h->seg_hist = nullptr; h->seg_maps = nullptr; h->seg_pmaps = nullptr; h->seg_gmaps = nullptr; h->seg_min = nullptr; h->lmsel1 = nullptr;
    h->seg_smin = nullptr; h->seg_gmin = nullptr; h->cm5snap = nullptr;
    // the layout is decided on the device (st->ranked): size for both (L = 6: ranked tables only, see gh_spin)
    const int N_ = h->N, L_ = h->L;
    const size_t hist_b = max_cls(L_, [&](int R) { const seg_geom g = seg_geometry(N_, L_, R); return (size_t)g.S * g.NW * g.NS; }) * 4;
    const size_t maps_b = max_cls(L_, [&](int R) { const seg_geom g = seg_geometry(N_, L_, R); return (size_t)g.S * g.NS; }) * 2;
    const size_t gmaps_b = max_cls(L_, [&](int R) { const seg_geom g = seg_geometry(N_, L_, R); return (size_t)g.G1 * g.NS; }) * 2;
    hipError_t e = hipMalloc((void **)&h->seg_hist, hist_b);
    if (e == hipSuccess) e = hipMalloc((void **)&h->seg_maps, maps_b);
    if (e == hipSuccess) e = hipMalloc((void **)&h->seg_pmaps, maps_b + 16);        // (+ slack: 16-byte copies in k_rw)
    if (e == hipSuccess) e = hipMalloc((void **)&h->seg_gmaps, gmaps_b + 16);      // (+ slack: k_rw copies the group maps four bytes at a time)
    if (e == hipSuccess) e = hipMalloc((void **)&h->seg_smin, maps_b * 4);          // doubles where the maps hold 2-byte states
    h->seg_smin_bytes = maps_b * 4;
    if (e == hipSuccess) e = hipMalloc((void **)&h->seg_gmin, gmaps_b * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&h->cm5snap, (size_t)h->N + 2);
    // (behind the segment minima: k_rwseg's flag words, one int2 per segment)
    if (e == hipSuccess) e = hipMalloc((void **)&h->seg_min, CW_MAX_SEG * (sizeof(double) + sizeof(int2)));
    if (e == hipSuccess) e = hipMalloc((void **)&h->lmsel1, ((size_t)h->N + 2) * sizeof(double));
    if (e != hipSuccess) return fail(GH_ERR_NOMEM, "hipMalloc for the segment-parallel walk failed: %s", hipGetErrorString(e));
    h->seg_L = h->L;
    return GH_OK;
}

// the segment-parallel walk's parameters for this handle (k_seg_fin reads N, L, st and segmin only)
static seg_params seg_make_params(const gh_handle *h, int rearm, int check_masks, uint8_t *d_path, double *d_lmsel)
{
    seg_params P;
    memset(&P, 0, sizeof P);
    P.N = h->N; P.L = h->L; P.rearm = rearm; P.check_masks = check_masks;
    P.G = h->lt; P.minfo = h->minfo; P.rinfo = h->rinfo; P.mt = h->cfg.marginal_term; P.nanp = h->cfg.marginal_term && h->cfg.offer_zero; P.sm = h->sm; P.st = h->dstate;
    P.hist = h->seg_hist; P.maps = h->seg_maps; P.pmaps = h->seg_pmaps; P.gmaps = h->seg_gmaps; P.segmin = h->seg_min;
    P.smin = h->seg_smin; P.gmin = h->seg_gmin; P.cm5snap = h->cm5snap;
    P.W = h->W; P.esz = (int)esize(h); P.band = h->band;
    P.rwflags = reinterpret_cast<int2 *>(h->seg_min + CW_MAX_SEG);
    P.path_out = d_path; P.lmsel = d_lmsel;
    return P;
}

typedef gh_spin_plan spin_plan;       // which kernels run for every path of a spin (plan_spin); value-initialised: outside a spin

// segments / groups the launches over the enumerated states are cut into
static int seg_S(int N, int L) { return (int)max_cls(L, [&](int R) { return (size_t)seg_geometry(N, L, R).S; }); }
static int seg_G1(int N, int L) { return (int)max_cls(L, [&](int R) { return (size_t)seg_geometry(N, L, R).G1; }); }
// short memories / small windows: every segment map fits the LDS of the emitting workgroup (k_emit_small).  sw: GH_EMIT_SMALL, -1 = unset
static bool emit_small_ok(int N, int L, int sw) { return sw != 0 && max_cls(L, [&](int R) { return emit_small_lds_bytes(N, L, R); }) <= 64 * 1024; }

// what follows the first kernel of a path: k_emit_small alone (behind k_rwseg it takes k_scan's look at what the reweight found as
// well: two launches per path), else k_scan + k_emit
template <int LC>
static void launch_emit_tail(gh_handle *h, const spin_plan &plan, const seg_params &P)
{
    const int N = h->N, S = seg_S(N, LC);
    if (plan.emit_small) {
        const size_t lds_small = max_cls(LC, [&](int R) { return emit_small_lds_bytes(N, LC, R); });
        lds_limit<k_emit_small<LC>>(lds_small, h->dev);
        hipLaunchKernelGGL((k_emit_small<LC>), dim3(S), dim3(SEG_THREADS), lds_small, h->stream, P);
        return;
    }
    const size_t lds_scan = max_cls(LC, [&](int R) { return scan_lds_bytes(N, LC, R); });
    const size_t lds_emit = max_cls(LC, [&](int R) { return emit_lds_bytes(N, LC, R); });
    lds_limit<k_scan<LC, false>>(lds_scan, h->dev);
    lds_limit<k_emit<LC>>(lds_emit, h->dev);
    hipLaunchKernelGGL((k_scan<LC, false>), dim3(seg_G1(N, LC)), dim3(SEG_THREADS), lds_scan, h->stream, P);
    hipLaunchKernelGGL((k_emit<LC>), dim3(S), dim3(SEG_THREADS), lds_emit, h->stream, P);
}

template <int LC, bool TRACK>
static void launch_seg_first(gh_handle *h, const seg_params &P)
{
    const size_t lds_seg = max_cls(LC, [&](int R) { return seg_lds_total(R, LC); });
    lds_limit<k_seg<LC, TRACK>>(lds_seg, h->dev);
    prof_begin(h, GH_K_SEG);
    hipLaunchKernelGGL((k_seg<LC, TRACK>), dim3(seg_S(h->N, LC)), dim3(SEG_THREADS), lds_seg, h->stream, P);
    // algorithmic bytes of k_seg: the conditional lookups of the extension (L history cells per step)
    prof_end(h, GH_K_SEG, (double)h->N * (double)LC * CELL * esize(h));
}

template <int LC>
static void launch_seg_lc(gh_handle *h, const spin_plan &plan, const seg_params &P)
{
    if (plan.flow != GH_FLOW_FUSE) { launch_seg_first<LC, false>(h, P); launch_emit_tail<LC>(h, plan, P); return; }
    // spins without k_emit: k_seg / k_scan also carry the minimum marginals (TRACK), k_rw chains the group maps itself
    const size_t lds_scan = max_cls(LC, [&](int R) { return scan_lds_bytes(h->N, LC, R); });
    lds_limit<k_scan<LC, true>>(lds_scan, h->dev);
    launch_seg_first<LC, true>(h, P);
    hipLaunchKernelGGL((k_scan<LC, true>), dim3(seg_G1(h->N, LC)), dim3(SEG_THREADS), lds_scan, h->stream, P);
}

static int launch_seg_walk(gh_handle *h, const spin_plan &plan, uint8_t *d_path, double *d_lmsel, int rearm, int check_masks)
{
    int rc = alloc_seg(h);
    if (rc) return rc;
    seg_params P = seg_make_params(h, rearm, check_masks, d_path, d_lmsel ? d_lmsel : h->lmsel1);      // (lmsel1 exists only behind alloc_seg)
    P.halo = plan.flow == GH_FLOW_RWSEG ? h->seg_halo : nullptr;
    if (h->L < 1 || h->L > SEG_MAX_L_NARROW) return fail(GH_ERR_STATE, "segment-parallel walk needs L <= %d", SEG_MAX_L_NARROW);
    prof_begin(h, GH_K_WALK);
    switch (h->L) {
#define SEG_CASE(n) case n: launch_seg_lc<n>(h, plan, P); break;
        SEG_CASE(1) SEG_CASE(2) SEG_CASE(3) SEG_CASE(4) SEG_CASE(5) SEG_CASE(6)      // (6: ranked tables only, plan_spin decides)
#undef SEG_CASE
    }
    prof_end(h, GH_K_WALK, walk_bytes(h->N, h->L, esize(h)));
    return post_launch(h, "k_seg/k_scan/k_emit");
}

// ---- k_rwseg: reweight of the path before + this path's k_seg in one launch, then k_scan, k_emit (segwalk.hpp) ----------
// where the patch lies in k_rwseg's dynamic LDS (behind k_seg's regions for either radix and, under the column conditionals,
// behind the staged band blocks of the workgroup's positions); the kernel needs this + sizeof(seg_patch).  es: bytes per element
static size_t rws_patch_off(int N, int W, int LC, bool col, size_t es)
{
    size_t off = max2(max_cls(LC, [&](int R) { return seg_lds_total(R, LC); }), (size_t)SEG_THREADS * 8);      // (the reweight phase's reduction scratch)
    off = (off + 15) & ~(size_t)15;
    if (col) {
        const int longest = (int)max_cls(LC, [&](int R) { return (size_t)seg_geometry(N, LC, R).seglen; });
        const size_t need = (size_t)SEG_THREADS * 8 + (size_t)(longest + LC + 1) * NSYM * W * NSYM * es;
        if (need > off) off = (need + 15) & ~(size_t)15;
    }
    return off;
}
#define RWS_LDS_MAX (160 * 1024 - 3 * 1024 - 512)      /* what a workgroup may have of the CU's 160 KB, less the kernel's static variables */

template <typename T, int LC, bool COL>
static void launch_rwseg_lc(gh_handle *h, const spin_plan &plan, seg_params P, const rws_params &Q)
{
    const size_t lds = (size_t)plan.lds;
    lds_limit<k_rwseg<T, LC, COL>>(lds, h->dev);
    P.patch_off = (int)(lds - sizeof(seg_patch));
    prof_begin(h, GH_K_RWSEG);
    hipLaunchKernelGGL((k_rwseg<T, LC, COL>), dim3(seg_S(h->N, LC)), dim3(SEG_THREADS), lds, h->stream, P, Q);
    // the extension's conditional lookups + what the reweight of a path reads and writes (the figure GH_K_REWEIGHT quotes)
    prof_end(h, GH_K_RWSEG, (double)h->N * (double)LC * CELL * esize(h) + reweight_bytes(h->N, h->W, LC, esize(h), true));
    launch_emit_tail<LC>(h, plan, P);
}

// reweights along d_prev (record d_prev_rec, removed mass into slot prev_slot) and walks the next path into d_path
static int launch_rwseg(gh_handle *h, const spin_plan &plan, const uint8_t *d_prev, gh_path_rec *d_prev_rec, int prev_slot, double min_remove,
                        uint8_t *d_path, double *d_lmsel, int check_masks)
{
    int rc = alloc_seg(h);
    if (rc) return rc;
    seg_params P = seg_make_params(h, 1, check_masks, d_path, d_lmsel);
    P.rws = 1; P.halo = h->seg_halo;
    rws_params Q;
    Q.band = h->band; Q.cnt = h->cnt; Q.marg = h->marg; Q.minfo = h->minfo; Q.rinfo = h->need_rinfo ? h->rinfo : nullptr; Q.G = h->lt;
    Q.nvalid = h->nvalid; Q.cmask = h->cmask; Q.path = d_prev; Q.min_remove = min_remove;
    Q.partial = h->partial + (size_t)prev_slot * plan.stride;
    Q.rec = d_prev_rec; Q.cond_mode = h->cfg.cond_mode; Q.offer_zero = h->cfg.offer_zero;
    if (h->L < 1 || h->L > SEG_MAX_L_NARROW) return fail(GH_ERR_STATE, "k_rwseg needs L <= %d", SEG_MAX_L_NARROW);   // before the bracket opens
    prof_begin(h, GH_K_WALK);
    const bool col = h->cfg.cond_mode == GH_COND_C || h->cfg.cond_mode == GH_COND_E;
    with_storage(h, [&](auto z) {
        using T = decltype(z);
        switch (h->L) {
#define RWS_CASE(n) case n: if (col) launch_rwseg_lc<T, n, true>(h, plan, P, Q); else launch_rwseg_lc<T, n, false>(h, plan, P, Q); break;
            RWS_CASE(1) RWS_CASE(2) RWS_CASE(3) RWS_CASE(4) RWS_CASE(5) RWS_CASE(6)
#undef RWS_CASE
        }
    });
    prof_end(h, GH_K_WALK, walk_bytes(h->N, h->L, esize(h)));
    // (what launch_reweight_marg notes behind a fused reweight: the table is current up to the rows this path's reweight wrote)
    h->lt_inc_path = d_prev;
    h->lt_inc_seg = true;
    h->dirty_lt = true;
    h->dirty_marg = false;
    h->band_epoch++;
    return post_launch(h, "k_rwseg/k_scan/k_emit");
}

// serial walkers: the record is closed by the walker itself.  Segment-parallel: by the k_marg<T,true> that follows
// (spins) or by k_seg_fin (lone gh_generate_path); d_lmsel receives the selected log-marginals for k_hp.
static int launch_walk(gh_handle *h, const spin_plan &plan, uint8_t *d_path, gh_path_rec *d_rec, double min_remove, int rearm,
                       double *d_lmsel = nullptr, int check_masks = 0)
{
    if (seg_ok(h->wmode, h->L) || plan.seg6) return launch_seg_walk(h, plan, d_path, d_lmsel, rearm, check_masks);
    walk_params P;
    P.N = h->N; P.L = h->L; P.chunk = 0; P.rearm = rearm;
    P.G = h->lt; P.Ht = h->ht; P.Yt = h->yt; P.minfo = h->minfo;
    P.path_out = d_path; P.rec = d_rec; P.st = h->dstate; P.min_remove = min_remove; P.sm = h->sm;
    prof_begin(h, GH_K_WALK);
    launch_walk_any(h->wmode, h->N, h->L, P, h->stream, 1, nullptr, 0);
    prof_end(h, GH_K_WALK, walk_bytes(h->N, h->L, esize(h)));
    return post_launch(h, "k_walk");
}

// reweight along d_path AND refresh the marginal tables in one pass (k_marg<T, true>)
// room for `slots` sets of per-block partial sums of the removed mass
static int ensure_partial(gh_handle *h, int nb, int slots)
{
    const size_t need = (size_t)nb * (slots > 0 ? slots : 1);
    if (need > (size_t)h->partial_cap) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->partial) hipFree(h->partial);
        h->partial = nullptr; h->partial_cap = 0;
        HIPCHK(hipMalloc((void **)&h->partial, need * sizeof(double)));
        h->partial_cap = (int)need;
    }
    return GH_OK;
}

// k_rw's lane group: 32 lanes per position where the band or the lag count exceeds 8 (all distances and lags in one
// round), else 8; blocks per path accordingly (also the stride of the per-path partial sums of the removed mass)
// (16: row conditionals with bands up to 32 and at most 16 lags -- the distances beyond 16 take a second round, the table
// entries are dealt out over the group anyway, and the marginals, 7 lanes of every group, cost a wavefront half as much)
// the to-major copy of the band (column conditionals): allocated on first use and converted on `st` when something else wrote the
// band since; the caller marks it in step (tband_epoch) -- at once, or behind the kernel that keeps both
static int ensure_tband(gh_handle *h, hipStream_t st)
{
    const size_t nel = h->n_cells * CELL;
    if (!h->tband && hipMalloc(&h->tband, nel * esize(h)) != hipSuccess) { h->tband = nullptr; return fail(GH_ERR_NOMEM, "hipMalloc for the to-major band failed"); }
    if (h->tband_epoch != h->band_epoch)
        with_storage(h, [&](auto z) {
            using T = decltype(z);
            hipLaunchKernelGGL(k_band_to_major<T>, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, st, (const T *)h->band, (T *)h->tband, nel, h->W);
        });
    return GH_OK;
}

static bool rw_col(const gh_handle *h) { return h->cfg.cond_mode == GH_COND_C || h->cfg.cond_mode == GH_COND_E; }
// column conditionals beyond the 8-lane groups: k_rw reads its columns from a to-major copy of the band (GH_RW_TBAND=0: from the staged block)
static bool rw_tband_on() { static const bool on = !env_off("GH_RW_TBAND"); return on; }      // (both read once per process)
static bool rw_lp16_on() { static const bool on = !env_off("GH_RW_LP16"); return on; }
static bool rw_tband(const gh_handle *h) { return rw_col(h) && (h->W > 8 || h->L > 8) && rw_tband_on(); }
static int rw_lanes_of(int W, int L, bool col, bool lp16, bool tband)
{
    if (!(W > 8 || L > 8)) return 8;
    return (W <= 32 && L <= 16 && lp16 && (!col || tband)) ? 16 : 32;
}
static int rw_lanes(const gh_handle *h) { return rw_lanes_of(h->W, h->L, rw_col(h), rw_lp16_on(), rw_tband_on()); }
static int rw_blocks_of(int N, int lanes) { return (int)(((size_t)(N + 1) * lanes + 255) / 256); }
static int rw_blocks(const gh_handle *h, bool seg) { return rw_blocks_of(h->N, seg ? rw_lanes(h) : 8); }

struct rw_req {
    const uint8_t *path;        // the path to reweight along, and its record
    gh_path_rec *rec;
    double ratio = 0.0;         // what to remove (seg: min_remove)
    int use_state = 1;          // the ratio is the one the walker left in the window's state (0: a lone reweight by `ratio`)
    int slot = -1;              // < 0: reduce the removed mass right behind the pass (k_reweight_finish); >= 0 (gh_spin): this path's partial
                                // sums in their own slot, the caller reduces all paths with one k_reweight_finish_all at the end
    bool seg = false;           // behind a segment-parallel walk: the kernel reduces the minimum marginal itself, clamps it to `ratio`, closes the record
    bool chained = false;       // a spin without k_lt between its paths (below)
    int nseg = 0;               // segments of a candidate-pool walk whose minima the kernel reduces (0: the enumerated states)
    double *lmsel = nullptr;    // the three-launch flow: where k_rw writes the selected log-marginals
};
static int launch_reweight_marg(gh_handle *h, const spin_plan &plan, const rw_req &q)
{
    const int use_state = q.use_state, slot = q.slot, block = 256;
    const bool seg = q.seg;
    const int nb = rw_blocks(h, seg);
    // (a spin strides its per-path partial sums by the widest kernel it may launch: plan_spin)
    const int stride = (slot >= 0 && plan.stride > nb) ? plan.stride : nb;
    // the three-launch flow: behind k_seg + k_scan without a k_emit the kernel finds its picks itself and writes the path to q.path / lmsel
    const bool fused = plan.flow == GH_FLOW_FUSE && q.nseg == 0;
    if (slot < 0) { int rc_ = ensure_partial(h, nb, 1); if (rc_) return rc_; }
    double *partial = h->partial + (slot > 0 ? (size_t)slot * stride : 0);
    if (slot >= 0 && stride > nb && plan.flow != GH_FLOW_RWSEG) HIPCHK(hipMemsetAsync(partial + nb, 0, sizeof(double) * (size_t)(stride - nb), h->stream));
    // in a spin the walker re-armed the flags when it finished; a lone reweight does it here
    if (!use_state) hipLaunchKernelGGL(k_rearm, dim3(1), dim3(64), 0, h->stream, h->dstate, (const win_desc *)nullptr, 0);
    // with a valid conditional table (conditional A or B, no marginal term) the kernel also rewrites the table rows
    // this path changes; k_lt then only has to confirm that no candidate mask moved
    // (chained: a spin without k_lt between its paths -- the table is current up to the rows the previous reweight rewrote, and
    // the k_seg that ran before this reweight has checked the candidate masks)
    const bool lt_ok = (!h->dirty_lt || q.chained) && h->lt && h->lt_L == h->L && (seg ? rw_incremental_ok(h) : lt_incremental_ok(h));
    double *lt_rows = lt_ok ? h->lt : nullptr;
    prof_begin(h, GH_K_REWEIGHT);
    if (seg) {
        // behind a segment-parallel walk (L <= SEG_MAX_L <= 8: one table row per lane): segwalk.hpp's k_rw
        const bool wide = rw_lanes(h) == 32, mid = rw_lanes(h) == 16;
        const bool col = rw_col(h);                         // the table entries a reweighted cell feeds: a column
        // the to-major copy: made (or made again, when something else wrote the band since) right here, kept by the kernel
        const bool use_tb = rw_tband(h) && !fused;
        if (use_tb) { int rc_ = ensure_tband(h, h->stream); if (rc_) return rc_; }
        fuse_params fz;
        memset(&fz, 0, sizeof fz);
        const size_t fuse_lds = fused ? (size_t)plan.lds : 0;
        if (fused) {
            fz.hist = h->seg_hist; fz.pmaps = h->seg_pmaps; fz.gmaps = h->seg_gmaps; fz.gmin = h->seg_gmin; fz.cm5snap = h->cm5snap;
            fz.path_out = const_cast<uint8_t *>(q.path); fz.lmsel = q.lmsel;
        }
        with_storage(h, [&](auto z) {
            using T = decltype(z);
#define GH_RW_LAUNCH(LP, COL, FZ)                                                                                                 \
    do {                                                                                                                          \
        /* COL: the band block of the workgroup's positions staged in LDS when it fits (k_rw) */                                   \
        const size_t blk_b = (size_t)(256 / LP) * NSYM * h->W * NSYM * sizeof(T);                                                 \
        /* | 2: `cnt` holds the row sums of the band as it stands (k_rw takes the rows a reweight does not touch from there) */     \
        const int stage = ((COL && !use_tb && blk_b <= 64 * 1024 && !env_off("GH_RW_STAGE")) ? 1 : 0) |                           \
                          ((!h->dirty_marg && !env_off("GH_RW_CNT")) ? 2 : 0) | ((COL && use_tb) ? 4 : 0);                        \
        const size_t lds_b = fuse_lds + ((stage & 1) ? blk_b : 0);                                                                \
        lds_limit<k_rw<T, LP, COL, FZ>>(lds_b, h->dev);                                                                           \
        hipLaunchKernelGGL((k_rw<T, LP, COL, FZ>), dim3(nb), dim3(block), lds_b, h->stream, (T *)h->band, h->N, h->W, h->cnt, h->marg, h->nvalid, \
                           h->cmask, h->minfo, h->dstate, q.path, q.ratio, partial, lt_rows, h->L, h->cfg.cond_mode,                \
                           (const double *)h->seg_min, q.rec, q.nseg, h->sm, h->cfg.offer_zero, h->need_rinfo ? h->rinfo : nullptr, stage, fz, (int)fuse_lds, \
                           (T *)(use_tb ? h->tband : nullptr));                                                                   \
    } while (0)
#define GH_RW_LAUNCH2(LP) do { if (col) GH_RW_LAUNCH(LP, true, false); else GH_RW_LAUNCH(LP, false, false); } while (0)
            if (fused) {                                    // (three-launch spins: lane groups of 8 only, plan_spin decides)
                if (col) GH_RW_LAUNCH(8, true, true); else GH_RW_LAUNCH(8, false, true);
            } else if (mid) GH_RW_LAUNCH2(16);
            else if (wide) GH_RW_LAUNCH2(32);
            else GH_RW_LAUNCH2(8);
#undef GH_RW_LAUNCH2
#undef GH_RW_LAUNCH
        });
    } else {
        marg_args a = marg_of(h);
        a.rw_path = q.path; a.ratio = q.ratio; a.use_state_ratio = use_state; a.partial = partial; a.G = lt_rows; a.L = h->L;
        a.cond_mode = h->cfg.cond_mode;
        launch_marg<true>(h, dim3(nb), h->stream, a);
    }
    if (slot < 0)
        hipLaunchKernelGGL(k_reweight_finish, dim3(1), dim3(256), 0, h->stream, partial, nb, h->dstate, use_state, q.rec,
                           (const win_desc *)nullptr, 0);
    prof_end(h, GH_K_REWEIGHT, reweight_bytes(h->N, h->W, h->L, esize(h), lt_ok));
    { int rc_ = post_launch(h, "k_marg<reweight>"); if (rc_) return rc_; }
    h->lt_inc_path = lt_ok ? q.path : nullptr;
    h->lt_inc_seg = seg;
    h->dirty_lt = true;
    h->dirty_marg = false;
    h->band_epoch++;
    if (seg && rw_tband(h) && !fused) h->tband_epoch = h->band_epoch;      // (the kernel wrote both)
    return GH_OK;
}

// the control words a spin starts from (stop, hole_at, n_done; lt_stale, cw_unres) and, for k_rwseg, the partial sums of the
// removed mass, in one launch instead of two small copies and a memset with a dispatch gap each
__global__ void k_spin_reset(dev_state *st, double *partial, size_t n)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) partial[q] = 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->stop = 0; st->hole_at = 0; st->n_done = 0; st->lt_stale = 0; st->cw_unres = 0; }
}

static int reset_spin_state(gh_handle *h, double *partial = nullptr, size_t n = 0)
{
    const int blocks = n ? (int)((n + 1023) / 1024 > 256 ? 256 : (n + 1023) / 1024) : 1;
    hipLaunchKernelGGL(k_spin_reset, dim3(blocks), dim3(256), 0, h->stream, h->dstate, partial, n);
    return post_launch(h, "k_spin_reset");
}

// ---- candidate-pool segment walk (cwalk.hpp): L = 6 .. 16, spins -------------------------------
static int alloc_cw(gh_handle *h)
{
    if (h->cw_keys) return GH_OK;
    // sized for whichever geometry a lag count gives this N (h->L can change between spins)
    const cw_geom ga = cw_geometry(h->N, CW_MIN_L), gb = cw_geometry(h->N, CW_MAX_L);
    const size_t S = (size_t)(ga.S > gb.S ? ga.S : gb.S);
    const size_t SNW = (size_t)ga.S * ga.NW5 > (size_t)gb.S * gb.NW5 ? (size_t)ga.S * ga.NW5 : (size_t)gb.S * gb.NW5;      // (8 picks per word is the wider one)
    hipError_t e = hipMalloc((void **)&h->cw_keys, sizeof(cw_key) * S * CW_K);
    if (e == hipSuccess) e = hipMalloc((void **)&h->cw_exits, sizeof(cw_key) * S * CW_K);
    if (e == hipSuccess) e = hipMalloc((void **)&h->cw_last_hit, sizeof(int32_t) * S * CW_K);
    if (e == hipSuccess) e = hipMalloc((void **)&h->cw_hist, sizeof(uint32_t) * SNW * CW_K);
    if (e == hipSuccess) e = hipMalloc((void **)&h->cw_npool, sizeof(int32_t) * S);
    // (the request lists twice: a launch appends to one set and consumes the other, cwalk.hpp)
    h->cw_S = S;
    if (e == hipSuccess) e = hipMalloc((void **)&h->cw_pend, sizeof(cw_key) * 2 * S * CW_K);
    if (e == hipSuccess) e = hipMalloc((void **)&h->cw_pend_exit, sizeof(cw_key) * 2 * S * CW_K);
    if (e == hipSuccess) e = hipMalloc((void **)&h->cw_pend_ready, sizeof(int32_t) * 2 * S * CW_K);
    if (e == hipSuccess) e = hipMemsetAsync(h->cw_pend_ready, 0, sizeof(int32_t) * 2 * S * CW_K, h->stream);
    if (e == hipSuccess) e = hipMalloc((void **)&h->cw_phist, sizeof(uint32_t) * 2 * SNW * CW_K);
    if (e == hipSuccess) e = hipMalloc((void **)&h->cw_npend, sizeof(int32_t) * 2 * S);
    if (e == hipSuccess) e = hipMemsetAsync(h->cw_npend, 0, sizeof(int32_t) * 2 * S, h->stream);
    if (e == hipSuccess) e = hipMalloc((void **)&h->cw_walked, S * CW_K);
    if (e == hipSuccess) e = hipMalloc((void **)&h->cw_nxt, S * CW_K);
    if (e == hipSuccess) e = hipMalloc((void **)&h->cw_true, sizeof(int32_t) * S);
    if (e == hipSuccess) e = hipMemsetAsync(h->cw_npool, 0, sizeof(int32_t) * S, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->cw_walked, 0, S * CW_K, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->cw_nxt, 0xff, S * CW_K, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->cw_last_hit, 0, sizeof(int32_t) * S * CW_K, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->cw_keys, 0, sizeof(cw_key) * S * CW_K, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->cw_exits, 0, sizeof(cw_key) * S * CW_K, h->stream);
    if (e == hipSuccess && !h->seg_min) e = hipMalloc((void **)&h->seg_min, CW_MAX_SEG * sizeof(double));      // (alloc_seg sizes for L <= 5 only)
    if (e != hipSuccess) {
        // all or nothing: a later call must not find cw_keys set next to pool buffers that never came to be
        hipStreamSynchronize(h->stream);
        hipFree(h->cw_pend_exit); hipFree(h->cw_pend_ready); hipFree(h->cw_phist);
        h->cw_pend_exit = nullptr; h->cw_pend_ready = nullptr; h->cw_phist = nullptr;
        hipFree(h->cw_keys); hipFree(h->cw_exits); hipFree(h->cw_last_hit); hipFree(h->cw_hist); hipFree(h->cw_npool); hipFree(h->cw_pend);
        hipFree(h->cw_npend); hipFree(h->cw_walked); hipFree(h->cw_nxt); hipFree(h->cw_true);
        h->cw_keys = nullptr; h->cw_exits = nullptr; h->cw_last_hit = nullptr; h->cw_hist = nullptr; h->cw_npool = nullptr; h->cw_pend = nullptr;
        h->cw_npend = nullptr; h->cw_walked = nullptr; h->cw_nxt = nullptr; h->cw_true = nullptr;
        return fail(GH_ERR_NOMEM, "hipMalloc for the candidate pools failed: %s", hipGetErrorString(e));
    }
    return GH_OK;
}

// the request lists of a launch: the set it appends to (h->cw_pp picks it) and the set it consumes, which the launch before
// appended to (cwalk.hpp); the lists of run-on results only where P.runon says walkers run on
static void cw_pend_sets(const gh_handle *h, const cw_geom &g, cw_params &P)
{
    const size_t nw = (size_t)(h->cw_wide ? g.NW5 : g.NW);
    const size_t a = (size_t)(h->cw_pp & 1), c = a ^ 1;
    P.pend = h->cw_pend + a * h->cw_S * CW_K;            P.pend_c = h->cw_pend + c * h->cw_S * CW_K;
    P.npend = h->cw_npend + a * h->cw_S;                 P.npend_c = h->cw_npend + c * h->cw_S;
    if (P.runon > 0) {
        P.pend_exit = h->cw_pend_exit + a * h->cw_S * CW_K;   P.pend_exit_c = h->cw_pend_exit + c * h->cw_S * CW_K;
        P.pend_ready = h->cw_pend_ready + a * h->cw_S * CW_K; P.pend_ready_c = h->cw_pend_ready + c * h->cw_S * CW_K;
        P.phist = h->cw_phist + a * g.S * nw * CW_K;          P.phist_c = h->cw_phist + c * g.S * nw * CW_K;
    }
    if (cw_digit_mode(h)) {
        const size_t bytes = (size_t)g.S * CW_K * h->cw_LD;
        P.pend_d = h->cw_pend_d + a * bytes;             P.pend_d_c = h->cw_pend_d + c * bytes;
        P.pend_exit_d = h->cw_pend_exit_d + a * bytes;   P.pend_exit_d_c = h->cw_pend_exit_d + c * bytes;
    }
}

// no_reweight: no reweight follows the path (k_cemit leaves the window's flags standing)
static cw_params cw_make_params(gh_handle *h, uint8_t *d_path, double *d_lmsel, bool no_reweight)
{
    cw_params P;
    memset(&P, 0, sizeof P);
    P.N = h->N; P.L = h->L; P.rearm = no_reweight ? 0 : 1; P.stamp = h->cw_stamp;
    P.G = h->lt; P.minfo = h->minfo; P.rinfo = h->rinfo; P.mt = h->cfg.marginal_term; P.sm = h->sm; P.st = h->dstate;
    P.keys = h->cw_keys; P.exits = h->cw_exits; P.last_hit = h->cw_last_hit; P.npool = h->cw_npool; P.walked = h->cw_walked; P.nxt = h->cw_nxt; P.pend = h->cw_pend; P.npend = h->cw_npend;
    P.hist = h->cw_hist; P.true_idx = h->cw_true; P.segmin = h->seg_min; P.path_out = d_path; P.lmsel = d_lmsel;
    // run-on (cwalk.hpp): how far a walker follows a new track beyond its own segment -- some two hundred positions: the launch
    // lasts as long as its longest walker (GH_CW_RUNON=k pins the number of segments, 0 = off; read per launch: the tests switch it)
    const cw_geom ggr = cw_geometry(h->N, h->L);
    int runon = ggr.seglen <= 64 ? 256 / ggr.seglen : 0;      // (C5, 98 positions per segment: 168 us per path without, 175 with two segments of run-on)
    if (runon > CW_RUNON) runon = CW_RUNON;
    // (states as bytes, beyond 32 lags: a step of k_cwalkg costs several times k_cwalk's, and a launch lasts as long as its longest
    // walker -- 736 us per path without run-on at L = 33, 855..897 with one to three segments of it)
    // (33..64 lags over ranks and 22..40 over the symbols go through k_cwalk2 since round 6: k_cwalk's step, and its run-on)
    if (cw_digit_mode(h) && !cw2_ok(h)) runon = 0;
    runon = env_int("GH_CW_RUNON", runon);
    if (runon > CW_RUNON) runon = CW_RUNON;
    P.runon = runon;
    cw_pend_sets(h, ggr, P);
    if (cw_digit_mode(h)) {
        P.keys_d = h->cw_keys_d; P.exits_d = h->cw_exits_d; P.LD = h->cw_LD;
        P.key0 = cw_hash_digits([](int) { return 0u; }, h->L);      // the start state: L zero bytes
    }
    return P;
}

template <int LC, int R>
static void launch_cwalk_lc(const cw_params &P, hipStream_t stream, int S, int dev)
{
    lds_limit<k_cwalk<LC, R>>(cw_lds_bytes(LC, R), dev);
    hipLaunchKernelGGL((k_cwalk<LC, R>), dim3(S), dim3(CW_K * cw_lanes(R)), cw_lds_bytes(LC, R), stream, P);
}

template <int LC, int R = 4>
static void launch_cwalk2_lc(const cw_params &P, hipStream_t stream, int S, int dev)
{
    lds_limit<k_cwalk2<LC, R>>(cw2_lds_bytes(LC, R), dev);
    hipLaunchKernelGGL((k_cwalk2<LC, R>), dim3(S), dim3(CW_K * cw_lanes(R)), cw2_lds_bytes(LC, R), stream, P);
}

template <int R>
static void launch_cwalkg(const cw_params &P, hipStream_t stream, int S, int dev)
{
    const size_t lds = cwg_lds_bytes(P.L, R);
    lds_limit<k_cwalkg<R>>(lds, dev);
    hipLaunchKernelGGL((k_cwalkg<R>), dim3(S), dim3(CW_K * cw_lanes(R)), lds, stream, P);
}

// the kernels of one path: `rounds` x (walk what is new, link + chain), emit
static int launch_cw_path(gh_handle *h, uint8_t *d_path, double *d_lmsel, int rounds, int check_masks, bool no_reweight, bool resume = false)
{
    const cw_geom g = cw_geometry(h->N, h->L);
    cw_params P = cw_make_params(h, d_path, d_lmsel, no_reweight);
    if (h->cw_round_cap > 0 && rounds > h->cw_round_cap) rounds = h->cw_round_cap;
    const bool skip0 = !resume && !env_off("GH_CW_SKIP0");      // (GH_CW_SKIP0=0: A/B, tests)
    if (!cw_digit_mode(h) && (h->L < CW_MIN_L || h->L > CW_MAX_L)) return fail(GH_ERR_STATE, "candidate-pool walk needs %d <= L <= %d", CW_MIN_L, CW_MAX_LG);
    prof_begin(h, GH_K_WALK);
    for (int r = 0; r < rounds; r++) {
        P.round = resume ? r + 1 : r;                       // (a resumed path continues behind the rounds already run)
        P.check_masks = (r == 0 && !resume) ? check_masks : 0;
        P.last_round = r == rounds - 1;
        // every k_cwalk launch appends to the request lists the launch before consumed, and the other way round
        h->cw_pp++;
        cw_pend_sets(h, g, P);
        if (r == 0) prof_begin(h, GH_K_SEG);                // (bench.py: the pool walker alone, first round of a path)
        if (cw_digit_mode(h) && cw2_ok(h) && h->cw_wide) {
            switch (cw2_lc(h->L, 5)) {
                case 24: launch_cwalk2_lc<24, 5>(P, h->stream, g.S, h->dev); break;
                case 28: launch_cwalk2_lc<28, 5>(P, h->stream, g.S, h->dev); break;
                case 32: launch_cwalk2_lc<32, 5>(P, h->stream, g.S, h->dev); break;
                case 36: launch_cwalk2_lc<36, 5>(P, h->stream, g.S, h->dev); break;
                default: launch_cwalk2_lc<40, 5>(P, h->stream, g.S, h->dev); break;
            }
        } else if (cw_digit_mode(h) && cw2_ok(h)) {
            switch (cw2_lc(h->L)) {
                case 36: launch_cwalk2_lc<36>(P, h->stream, g.S, h->dev); break;
                case 40: launch_cwalk2_lc<40>(P, h->stream, g.S, h->dev); break;
                case 44: launch_cwalk2_lc<44>(P, h->stream, g.S, h->dev); break;
                case 48: launch_cwalk2_lc<48>(P, h->stream, g.S, h->dev); break;
                case 52: launch_cwalk2_lc<52>(P, h->stream, g.S, h->dev); break;
                case 56: launch_cwalk2_lc<56>(P, h->stream, g.S, h->dev); break;
                case 60: launch_cwalk2_lc<60>(P, h->stream, g.S, h->dev); break;
                default: launch_cwalk2_lc<64>(P, h->stream, g.S, h->dev); break;
            }
        } else if (cw_digit_mode(h)) {
            if (!h->cw_wide) launch_cwalkg<4>(P, h->stream, g.S, h->dev);
            else launch_cwalkg<5>(P, h->stream, g.S, h->dev);
        } else
        switch (h->L) {
            // (the table over the symbols: 3 bits per pick, CW_MAX_L5 lags in a state)
#define CW_CASE(n) case n: if (!h->cw_wide) launch_cwalk_lc<n, 4>(P, h->stream, g.S, h->dev); else launch_cwalk_lc<(n <= CW_MAX_L5 ? n : CW_MAX_L5), 5>(P, h->stream, g.S, h->dev); break;
            CW_CASE(6) CW_CASE(7) CW_CASE(8) CW_CASE(9) CW_CASE(10) CW_CASE(11) CW_CASE(12) CW_CASE(13) CW_CASE(14) CW_CASE(15) CW_CASE(16)
            CW_CASE(17) CW_CASE(18) CW_CASE(19) CW_CASE(20) CW_CASE(21) CW_CASE(22) CW_CASE(23) CW_CASE(24)
            // (25..32 lags: over ranks only -- cw_digit_mode sends the symbol table beyond CW_MAX_L5 to k_cwalkg)
            CW_CASE(25) CW_CASE(26) CW_CASE(27) CW_CASE(28) CW_CASE(29) CW_CASE(30) CW_CASE(31) CW_CASE(32)
#undef CW_CASE
            default: return fail(GH_ERR_STATE, "candidate-pool walk needs %d <= L <= %d", CW_MIN_L, CW_MAX_LG);
        }
        if (r == 0) prof_end(h, GH_K_SEG, (double)h->N * (double)h->L * CELL * esize(h));
        // (skip0: hardly any chain closes in the round that walks everything -- the states a reweight moved are only found by
        // it -- so its link + scan launches, 15 us of a path, are left out and the chain is first followed behind round 1)
        if (r == 0 && skip0 && rounds >= 2) continue;
        hipLaunchKernelGGL(k_clink, dim3(g.S), dim3(CW_K), 0, h->stream, P);
        hipLaunchKernelGGL(k_cscan, dim3(1), dim3(1024), 0, h->stream, P);
    }
    hipLaunchKernelGGL(k_cemit, dim3(g.S), dim3(256), 0, h->stream, P);
    prof_end(h, GH_K_WALK, walk_bytes(h->N, h->L, esize(h)));
    return post_launch(h, "k_cwalk/k_cscan/k_cemit");
}


// device buffers for the paths, records and selected log-marginals of a spin of max_paths paths
static int ensure_spin_buffers(gh_handle *h, int max_paths)
{
    const size_t n1 = (size_t)h->N + 1;
    if (max_paths > h->spin_cap) {
        // (a handle is sized for the reference's default spin -- 100 paths, gretel/cmd.py:148 -- the first time it spins, however
        // few paths that first call asks for: growing later costs three frees, three allocations and the pinned staging buffer
        // over again, 0.7 ms on the caller's clock -- a fifth of a C3 spin -- unless the window is so long that the floor is real memory)
        const int floor_paths = 128;
        if (max_paths < floor_paths && n1 * 9 * (size_t)floor_paths <= ((size_t)256 << 20)) max_paths = floor_paths;
        HIPCHK(hipStreamSynchronize(h->stream));
        hipFree(h->spin_paths); hipFree(h->spin_recs);
        h->spin_paths = nullptr; h->spin_recs = nullptr; h->spin_cap = 0;
        hipFree(h->spin_lmsel); h->spin_lmsel = nullptr;
        hipError_t ea = hipMalloc((void **)&h->spin_paths, n1 * max_paths);
        if (ea == hipSuccess) ea = hipMalloc((void **)&h->spin_recs, sizeof(gh_path_rec) * max_paths);
        // the selected symbols' log-marginals of every path, for the likelihood sums behind the loop (k_hp)
        if (ea == hipSuccess) ea = hipMalloc((void **)&h->spin_lmsel, sizeof(double) * n1 * max_paths);
        if (ea != hipSuccess) {
            hipFree(h->spin_paths); h->spin_paths = nullptr;
            hipFree(h->spin_recs); h->spin_recs = nullptr;
            return fail(GH_ERR_NOMEM, "hipMalloc failed");
        }
        h->spin_cap = max_paths;
    }
    return GH_OK;
}

struct spin_io {
    int max_paths;
    double min_remove;
    size_t n1;              // bytes per path
    spin_plan plan;         // (all zero: a lone gh_generate_path)
    uint8_t *paths_out;
    gh_path_rec *recs;
    bool no_reweight;       // gh_generate_path: the path is only recovered (its record closed by k_seg_fin), the tensor stays
};
static int spin_candidate_pools(gh_handle *h, const spin_io &io, dev_state &hs, int *first_out, bool *gave_up);

// one path through the serial walker, its boundary states into the pools (merge: keep what is there)
static int cw_serial_path(gh_handle *h, const spin_io &io, uint8_t *d_path, gh_path_rec *d_rec, double *d_lmsel, int slot, int merge)
{
    // the serial depth-2 walker reads tables that k_lt keeps; behind pool paths (no k_lt between them) they are stale
    h->lt_inc_path = nullptr;
    h->dirty_lt = true;
    int rc = ensure_lt(h, true);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(d_lmsel, 0, sizeof(double), h->stream));      // k_hp: the walker sums this path itself
    if ((rc = launch_walk(h, io.plan, d_path, d_rec, io.min_remove, 1, nullptr, 0))) return rc;
    cw_params P = cw_make_params(h, d_path, d_lmsel, io.no_reweight);
    const cw_geom g = cw_geometry(h->N, h->L);
    hipLaunchKernelGGL(k_cseed, dim3((g.S + 255) / 256), dim3(256), 0, h->stream, P, (const uint8_t *)d_path, merge);
    if ((rc = post_launch(h, "k_cseed"))) return rc;
    if (!io.no_reweight) {
        rw_req q;
        q.path = d_path; q.rec = d_rec; q.slot = slot;
        rc = launch_reweight_marg(h, io.plan, q);
    }
    h->cw_stat[1]++;
    return rc;
}

// what gh_generate_path hands back: where a hole stopped the path, else the closed record
static void give_record(const dev_state &hs, const gh_path_rec &rec, double *hp_current, double *hp_original, double *min_marginal, int *hole_at)
{
    *hole_at = hs.stop ? hs.hole_at : 0;
    if (hs.stop) return;
    if (hp_current) *hp_current = rec.hp_current;
    if (hp_original) *hp_original = rec.hp_original;
    if (min_marginal) *min_marginal = rec.min_marginal;
}

extern "C" int gh_generate_path(gh_t *h, const gh_t *original, uint8_t *path_out, double *hp_current,
                                double *hp_original, double *min_marginal, int *hole_at)
{
    if (!h || !path_out || !hole_at) return fail(GH_ERR_ARG, "null argument");
    if (set_dev(h)) return GH_ERR_HIP;
    const bool pools = cw_ok(h->wmode, h->L) && !h->cw_off;
    int rc = ensure_lt(h, !seg_ok(h->wmode, h->L) && !pools);      // (a serial walker wants the marginal term in the table)
    if (rc) return rc;
    const int nb8 = ((h->N + 1) * 8 + 255) / 256;
    if (original && original != h) {
        gh_handle *o = const_cast<gh_handle *>(original);
        if (o->N != h->N) return fail(GH_ERR_ARG, "original has %d SNPs, hansel has %d", o->N, h->N);
        if (o->dev != h->dev) return fail(GH_ERR_ARG, "original lives on another device");
        if ((rc = ensure_marg(o))) return rc;
        HIPCHK(hipStreamSynchronize(o->stream));
        hipLaunchKernelGGL(k_snapshot, dim3(nb8), dim3(256), 0, h->stream, h->minfo, o->minfo, h->N, (const win_desc *)nullptr);
        h->have_orig = true;
    } else if (!h->have_orig) {
        hipLaunchKernelGGL(k_snapshot, dim3(nb8), dim3(256), 0, h->stream, h->minfo, h->minfo, h->N, (const win_desc *)nullptr);
    }
    if ((rc = reset_spin_state(h))) return rc;
    if (pools) {
        // lag counts of the candidate pools: the path comes out of them (one path, no reweight: the tensor stays as it is,
        // the pools keep what they learnt for the next call); only a window they cannot take goes on to the serial walker
        if ((rc = ensure_spin_buffers(h, 1))) return rc;
        gh_path_rec rec1;
        spin_io io{};
        io.max_paths = 1; io.n1 = (size_t)h->N + 1; io.paths_out = path_out; io.recs = &rec1; io.no_reweight = true;
        dev_state hs1;
        memset(&hs1, 0, sizeof hs1);
        int first1 = 0;
        bool gave_up = false;
        if ((rc = spin_candidate_pools(h, io, hs1, &first1, &gave_up))) return rc;
        if (!gave_up) {
            // (a hole: the prefix that was walked -- the reference returns what it has)
            if (hs1.stop) HIPCHK(hipMemcpy(path_out, h->spin_paths, (size_t)h->N + 1, hipMemcpyDeviceToHost));
            give_record(hs1, rec1, hp_current, hp_original, min_marginal, hole_at);
            return GH_OK;
        }
        if ((rc = reset_spin_state(h))) return rc;
        if ((rc = ensure_lt(h, true))) return rc;                   // the pools gave the window up: the serial walker's table
    }
    spin_plan lone{};                                               // outside a spin: only the tail of the segment-parallel walk is chosen
    lone.emit_small = seg_ok(h->wmode, h->L) && emit_small_ok(h->N, h->L, env_int("GH_EMIT_SMALL", -1));
    if ((rc = launch_walk(h, lone, h->d_path, h->d_rec, 0.0, 0))) return rc;
    if (seg_ok(h->wmode, h->L)) {
        // close the record (hole / minimum marginal), then the two likelihood sums
        hipLaunchKernelGGL(k_seg_fin, dim3(1), dim3(256), 0, h->stream, seg_make_params(h, 0, 0, nullptr, nullptr), h->d_rec, 0.0, 0);
        hipLaunchKernelGGL(k_hp, dim3(1, 2), dim3(64), 0, h->stream, (const double *)h->lmsel1, (size_t)0, (const uint8_t *)h->d_path,
                           (size_t)0, (const double *)h->minfo, h->N, (const dev_state *)h->dstate, h->d_rec, h->sm);
        if ((rc = post_launch(h, "k_seg_fin/k_hp"))) return rc;
    }
    dev_state hs;
    gh_path_rec rec;
    HIPCHK(hipMemcpyAsync(&rec, h->d_rec, sizeof rec, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(path_out, h->d_path, (size_t)h->N + 1, hipMemcpyDeviceToHost, h->stream));
    if ((rc = read_state(h, &hs))) return rc;
    give_record(hs, rec, hp_current, hp_original, min_marginal, hole_at);
    return GH_OK;
}

extern "C" int gh_reweight_path(gh_t *h, const uint8_t *path, double ratio, double *removed)
{
    if (!h || !path) return fail(GH_ERR_ARG, "null argument");
    if (set_dev(h)) return GH_ERR_HIP;
    for (int q = 0; q <= h->N; q++)
        if (path[q] >= NSYM) return fail(GH_ERR_SYMBOL, "path[%d] = %d is not a symbol index", q, path[q]);
    HIPCHK(hipMemcpyAsync(h->d_rw_path, path, (size_t)h->N + 1, hipMemcpyHostToDevice, h->stream));
    rw_req q;
    q.path = h->d_rw_path; q.rec = h->d_rec; q.ratio = ratio; q.use_state = 0;
    int rc = launch_reweight_marg(h, spin_plan{}, q);
    if (rc) return rc;
    gh_path_rec rec;
    HIPCHK(hipMemcpyAsync(&rec, h->d_rec, sizeof rec, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (removed) *removed = rec.magnitude;
    return GH_OK;
}

// pinned staging of at least `need` bytes (a new buffer: `cap`); false: no pinned memory to be had
static bool ensure_stage(gh_handle *h, size_t need, size_t cap)
{
    if (need <= h->stage_cap) return true;
    if (h->stage) hipHostFree(h->stage);
    h->stage = nullptr; h->stage_cap = 0;
    if (hipHostMalloc((void **)&h->stage, cap, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h->stage = nullptr; return false; }
    h->stage_cap = cap;
    return true;
}

// results to the caller's (pageable) buffers through pinned staging: one asynchronous copy each at PCIe rate and a
// host memcpy, instead of the runtime's chunked pageable path
static int results_to_host(gh_handle *h, uint8_t *paths_out, const uint8_t *d_paths, size_t path_bytes, gh_path_rec *recs,
                           const gh_path_rec *d_recs, size_t rec_bytes)
{
    const size_t need = path_bytes + rec_bytes;
    if (!ensure_stage(h, need, need + need / 2 + 4096)) {
        // no pinned memory to be had: the plain copies
        HIPCHK(hipMemcpy(paths_out, d_paths, path_bytes, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(recs, d_recs, rec_bytes, hipMemcpyDeviceToHost));
        return GH_OK;
    }
    HIPCHK(hipMemcpyAsync(h->stage, d_paths, path_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->stage + path_bytes, d_recs, rec_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(paths_out, h->stage, path_bytes);
    memcpy(recs, h->stage + path_bytes, rec_bytes);
    return GH_OK;
}

// The end of a spin in ONE wait: the device state and the results of the `launched` paths go to pinned staging together
// (how many of them are complete is only known from the state); deliver_results then hands n_done of them to the caller.
// Returns 1 when there is no pinned memory to be had (the caller takes the two-step way).
static int state_and_results_to_stage(gh_handle *h, dev_state *hs, const uint8_t *d_paths, size_t n1, const gh_path_rec *d_recs, int launched)
{
    const size_t pb = n1 * (size_t)launched, rb = sizeof(gh_path_rec) * (size_t)launched, need = pb + rb + sizeof(dev_state) + 64;
    // (pinned memory is the dearest allocation of a spin: sized once for what the device buffers hold -- ensure_spin_buffers)
    const size_t lc = (size_t)(launched > h->spin_cap ? launched : h->spin_cap);
    if (!ensure_stage(h, need, (n1 + sizeof(gh_path_rec)) * lc + sizeof(dev_state) + 64 + 4096)) return 1;
    const size_t rec_off = (pb + 63) & ~(size_t)63;
    HIPCHK(hipMemcpyAsync(h->stage + rec_off + rb, h->dstate, sizeof(dev_state), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->stage + rec_off, d_recs, rb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->stage, d_paths, pb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(hs, h->stage + rec_off + rb, sizeof(dev_state));
    return GH_OK;
}

// zeroes n control words of the window from *word on (lt_stale and, behind it, cw_unres; cw_need), on the handle's stream
static int clear_flags(gh_handle *h, int *word, int n = 1)
{
    static const int zero[2] = {0, 0};
    const hipError_t e = hipMemcpyAsync(word, zero, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream);
    return e == hipSuccess ? GH_OK : fail(GH_ERR_HIP, "gh_spin failed: %s", hipGetErrorString(e));
}

// The end of a queue of n paths.  hp: the likelihood sums of every path in one launch (strictly sequential additions, one wavefront per
// sum).  lt_baked >= 0: the table in step with the last reweight while its path is still allocated (in full when a candidate mask moved).
// Then the removed mass of every path in one launch, and the state and the results in one wait (*staged: they lie in the pinned buffer)
static int finish_spin(gh_handle *h, const spin_io &io, int n, bool hp, int lt_baked, dev_state &hs, bool *staged)
{
    int rc;
    *staged = false;
    if (n <= 0) return read_state(h, &hs);
    if (hp) {
        hipLaunchKernelGGL(k_hp, dim3(n, 2), dim3(64), 0, h->stream, (const double *)h->spin_lmsel, io.n1, (const uint8_t *)h->spin_paths, io.n1,
                           (const double *)h->minfo, h->N, (const dev_state *)h->dstate, h->spin_recs, h->sm);
        if ((rc = post_launch(h, "k_hp"))) return rc;
    }
    if (lt_baked >= 0 && (rc = ensure_lt(h, lt_baked != 0, true, io.plan.flow == GH_FLOW_FUSE))) return rc;
    if (!io.no_reweight) {
        hipLaunchKernelGGL(k_reweight_finish_all, dim3(n), dim3(256), 0, h->stream, h->partial, io.plan.stride, h->dstate, h->spin_recs);
        if ((rc = post_launch(h, "k_reweight_finish_all"))) return rc;
    }
    const int sr = state_and_results_to_stage(h, &hs, h->spin_paths, io.n1, h->spin_recs, n);
    if (sr < 0) return sr;
    *staged = sr == GH_OK;
    return *staged ? GH_OK : read_state(h, &hs);
}

// the n_done complete paths of the `launched` ones to the caller
static int deliver_results(gh_handle *h, const spin_io &io, const dev_state &hs, int launched, bool staged)
{
    const size_t pb = io.n1 * (size_t)hs.n_done, rb = sizeof(gh_path_rec) * (size_t)hs.n_done;
    if (hs.n_done <= 0) return GH_OK;
    if (!staged || hs.n_done > launched) return results_to_host(h, io.paths_out, h->spin_paths, pb, io.recs, h->spin_recs, rb);
    memcpy(io.paths_out, h->stage, pb);
    memcpy(io.recs, h->stage + ((io.n1 * (size_t)launched + 63) & ~(size_t)63), rb);
    return GH_OK;
}

// The spin of lag counts 6 .. 24: segments walked from candidate pools (cwalk.hpp).  The paths are queued a few at a
// time: a path whose chain stays open after the queued rounds idles the kernels behind it; the host then queues more
// rounds for that one path, and if its chain is still open hands it to the serial walker (whose states join the pools)
// before queueing on.  Returns with *gave_up set when the window turned out to have a position with five candidates:
// paths *first .. go the serial walkers' way (the caller's loop).

static int spin_candidate_pools(gh_handle *h, const spin_io &io, dev_state &hs, int *first_out, bool *gave_up)
{
    const int max_paths = io.max_paths;
    const double min_remove = io.min_remove;
    const size_t n1 = io.n1;
    uint8_t *d_paths = h->spin_paths;
    gh_path_rec *d_recs = h->spin_recs;
    int rc = GH_OK, first = 0;
    bool cw_gave_up = false;
    if ((rc = alloc_cw(h))) return rc;
    const cw_geom cg = cw_geometry(h->N, h->L);
    // what follows the kernels of a path: the fused reweight (which also closes the path's record), or only the closing
    auto finish_path = [&](uint8_t *pth, gh_path_rec *rec, int slot, bool chained) -> int {
        if (!io.no_reweight) {
            rw_req q;
            q.path = pth; q.rec = rec; q.ratio = min_remove; q.slot = slot; q.seg = true; q.chained = chained; q.nseg = cg.S;
            return launch_reweight_marg(h, io.plan, q);
        }
        hipLaunchKernelGGL(k_seg_fin, dim3(1), dim3(256), 0, h->stream, seg_make_params(h, 0, 0, nullptr, nullptr), rec, min_remove, cg.S);
        return post_launch(h, "k_seg_fin");
    };
    if ((rc = clear_flags(h, &h->dstate->lt_stale, 2))) return rc;      // lt_stale, cw_unres
    // which layout did k_lt choose for this tensor?  (ranks when every position has at most four candidates, else symbols:
    // the walker's instantiation, the bits per pick and what a pool entry means follow from it)
    auto look_at_layout = [&](int ranked) {
        h->cw_wide = !ranked;
        if (h->cw_pool_wide != h->cw_wide) { h->cw_ready = false; h->cw_pool_wide = h->cw_wide; }

        if (cw_digit_mode(h) && !h->cw_off) {
            const int LD = (h->L + 3) & ~3;
            if (h->cw_LD != LD) {
                hipStreamSynchronize(h->stream);
                hipFree(h->cw_keys_d); hipFree(h->cw_exits_d); hipFree(h->cw_pend_d); hipFree(h->cw_pend_exit_d);
                h->cw_keys_d = h->cw_exits_d = h->cw_pend_d = h->cw_pend_exit_d = nullptr;
                const cw_geom gg = cw_geometry(h->N, h->L);
                const size_t bytes = (size_t)gg.S * CW_K * LD;
                if (hipMalloc((void **)&h->cw_keys_d, bytes) != hipSuccess || hipMalloc((void **)&h->cw_exits_d, bytes) != hipSuccess ||
                    hipMalloc((void **)&h->cw_pend_d, 2 * bytes) != hipSuccess || hipMalloc((void **)&h->cw_pend_exit_d, 2 * bytes) != hipSuccess) {
                    rc = fail(GH_ERR_NOMEM, "hipMalloc for the candidate pools failed");
                    h->cw_LD = 0;
                    return;
                }
                hipMemsetAsync(h->cw_keys_d, 0, bytes, h->stream); hipMemsetAsync(h->cw_exits_d, 0, bytes, h->stream); hipMemsetAsync(h->cw_pend_d, 0, 2 * bytes, h->stream); hipMemsetAsync(h->cw_pend_exit_d, 0, 2 * bytes, h->stream);
                h->cw_LD = LD;
                h->cw_ready = false;
            }
        }
    };
    {
        dev_state look;
        if ((rc = ensure_lt(h)) || (rc = read_state(h, &look))) return rc;
        look_at_layout(look.ranked);
    }
    int done = 0;
    int CHUNK = 8, clean = 0;        // paths queued between two looks at the device state: grows while every chain closes
    while (rc == GH_OK && done < max_paths) {
        if (h->cw_off) {
            // a position with five candidates: the rest of the spin goes the serial walkers' way (the loop below)
            cw_gave_up = true;
            first = done;
            if (hipMemset2DAsync(h->spin_lmsel + n1 * done, n1 * sizeof(double), 0, sizeof(double), (size_t)(max_paths - done), h->stream) != hipSuccess)
                rc = fail(GH_ERR_HIP, "gh_spin failed: hipMemset2DAsync");
            break;
        }
        if (!h->cw_ready) {
            // no pools yet for this tensor: one entry per pool from the largest marginals (k_cguess), and rounds
            // until closure has brought in what the walk really does (the serial walker costs 20 rounds at L <= 16
            // and 400 beyond: it only takes the path if the chain is still open after CW_BOOT + the resumed rounds)
            h->cw_stamp++;
            if ((rc = ensure_lt(h))) break;
            uint8_t *pth = d_paths + n1 * done;
            cw_params P = cw_make_params(h, pth, h->spin_lmsel + n1 * done, io.no_reweight);
            hipLaunchKernelGGL(k_cguess, dim3((unsigned)((h->N + 256) / 256)), dim3(256), 0, h->stream, P, pth);
            hipLaunchKernelGGL(k_cseed, dim3((cg.S + 255) / 256), dim3(256), 0, h->stream, P, (const uint8_t *)pth, 0);
            if ((rc = post_launch(h, "k_cguess/k_cseed"))) break;
            if ((rc = launch_cw_path(h, pth, h->spin_lmsel + n1 * done, CW_BOOT_ROUNDS, 0, io.no_reweight))) break;
            if ((rc = finish_path(pth, d_recs + done, done, false))) break;
            h->cw_stat[2] += CW_BOOT_ROUNDS;
            h->cw_ready = true;
        } else {
            const int upto = done + CHUNK < max_paths ? done + CHUNK : max_paths;
            // (conditional C / the marginal term: the reweight cannot keep the table current, k_lt rebuilds it in front of
            // every path -- queued like everything else; otherwise once per look, and k_cwalk checks the masks)
            if ((rc = ensure_lt(h, false, false))) break;
            const bool inc = rw_incremental_ok(h);
            for (int s = done; s < upto && rc == GH_OK; s++) {
                h->cw_stamp++;
                if (!inc && s > done && (rc = ensure_lt(h))) break;
                if ((rc = launch_cw_path(h, d_paths + n1 * s, h->spin_lmsel + n1 * s, h->cw_rounds, (inc && s > done) ? 1 : 0, io.no_reweight))) break;
                rc = finish_path(d_paths + n1 * s, d_recs + s, s, s > done);
                h->cw_stat[2] += h->cw_rounds;
            }
            if (rc) break;
        }
        if ((rc = read_state(h, &hs))) break;
        if (getenv("GH_PRINT_STATE"))
            fprintf(stderr, "gh_spin(cw): n_done %d stop %d lt_stale %d cw_unres %d open_at %d rounds %d  closed in round 0/1/2/3/4+: %llu %llu %llu %llu %llu\n", hs.n_done, hs.stop, hs.lt_stale,
                    hs.cw_unres, hs.cw_open_at, h->cw_rounds, hs.dbg8[0], hs.dbg8[1], hs.dbg8[2], hs.dbg8[3], hs.dbg8[4]);
        h->cw_stat[0] += hs.n_done - done;
        done = hs.n_done;
        if (hs.stop) break;
        if (!hs.lt_stale && !hs.cw_unres) {
            // (a look costs ~25 us of idle GPU; an open chain costs the ~37 us of idle launches of every path queued
            // behind it: at one open chain in 50..100 paths the optimum is 8..16 paths per look)
            if (CHUNK < 16) CHUNK *= 2;
            // idle rounds cost three launches each: one fewer when, three looks in a row, no path needed as many as are queued
            if (hs.cw_need > 0 && hs.cw_need < h->cw_rounds) { if (++clean >= 3) { h->cw_rounds--; clean = 0; } }
            else clean = 0;
            if (hs.cw_need > 0 && (rc = clear_flags(h, &h->dstate->cw_need))) break;
        } else { CHUNK = 8; clean = 0; }
        if (hs.lt_stale || hs.cw_unres) {
            if ((rc = clear_flags(h, &h->dstate->lt_stale, 2))) break;
            h->spin_requeues++;
            h->cw_stat[3]++;
            // a moved candidate mask or a window for the serial walkers: the next ensure_lt rebuilds the table in
            // full.  Behind a chain that merely stayed open the table is current: every kernel queued behind it
            // idled, and the reweights that ran kept their rows.
            h->lt_inc_path = nullptr;
            h->dirty_lt = hs.lt_stale != 0;
            // an open chain costs a look, the resumed rounds and the idle launches of everything queued behind it -- far
            // more than an idle round (three empty launches) on every path: queue one round more from now on
            if (hs.cw_unres == 1 && h->cw_rounds < 8) h->cw_rounds++;
            if (hs.cw_unres == 2) look_at_layout(hs.ranked);        // a rebuild changed the table's layout: the other instantiation, new pools
            else if (hs.cw_unres == 1 && done < max_paths) {
                // the queued rounds did not close this path's chain.  Its pools keep what has been walked (the tensor
                // has not changed): more rounds first; if the chain is still open, the serial walker takes the path
                // and its states join the pools.
                bool closed = false;
                if (!hs.lt_stale) {
                    if ((rc = ensure_lt(h))) break;
                    // Every round carries the verified chain at least one segment further (the state it stopped at joins
                    // the next pool and is walked), so S rounds always close it.  Beyond 16 lags the serial walker is
                    // k_walk_global, 3 ms per thousand SNPs: there the rounds go on until the chain is closed; up to 16
                    // lags the depth-2 walker costs about as much as a dozen rounds, and takes over after those.
                    const int more = h->L > 16 ? 48 : 12;
                    const int tries = h->L > 16 ? (cg.S + 16) / more + 1 : 1;
                    for (int a = 0; a < tries && !closed; a++) {
                        if ((rc = launch_cw_path(h, d_paths + n1 * done, h->spin_lmsel + n1 * done, more, 0, io.no_reweight, true))) break;
                        if ((rc = finish_path(d_paths + n1 * done, d_recs + done, done, false))) break;
                        h->cw_stat[2] += more;
                        if ((rc = read_state(h, &hs))) break;
                        closed = !hs.cw_unres && hs.n_done > done;
                        if (hs.cw_unres && (rc = clear_flags(h, &h->dstate->lt_stale, 2))) break;
                        if (hs.stop) break;
                    }
                    if (rc != GH_OK) break;
                }
                if (!closed) {
                    h->cw_stamp++;
                    if ((rc = cw_serial_path(h, io, d_paths + n1 * done, d_recs + done, h->spin_lmsel + n1 * done, done, 1))) break;
                    if ((rc = read_state(h, &hs))) break;
                }
                done = hs.n_done;
                if (hs.stop) break;
            }
        }
    }
    // the serial walkers' tables were not kept between pool paths: rebuild before anybody walks serially again
    // (a lone path without a reweight leaves the tensor, and the table, as they were)
    if (!io.no_reweight) {
        h->lt_inc_path = nullptr;
        h->dirty_lt = true;
    }
    if (rc == GH_OK && done > 0 && !cw_gave_up) {
        bool staged;
        if ((rc = finish_spin(h, io, done, true, -1, hs, &staged)) == GH_OK) rc = deliver_results(h, io, hs, done, staged);
    }
    *first_out = first;
    *gave_up = cw_gave_up;
    return rc;
}

// ---- which kernels run for every path of a spin: chosen once, as a value (DESIGN.md section 4.1 has the table) ----------------
static int sw(int v, int def) { return v < 0 ? def : v; }      // a switch of gh_spin_plan_in: -1 = unset

// Pure: no HIP call, no handle.  in.ranked < 0 and a choice that depends on the table's layout: need_layout, nothing else.
static spin_plan plan_spin(const gh_spin_plan_in &in)
{
    spin_plan p{};
    const int N = in.n_snps, W = in.band, L = in.L, wm = in.walk_mode;
    const bool col = in.cond_mode == GH_COND_C || in.cond_mode == GH_COND_E;
    const int lanes = rw_lanes_of(W, L, col, sw(in.rw_lp16, 1) != 0, sw(in.rw_tband, 1) != 0);
    bool seg = seg_ok(wm, L);
    if (!seg && wm == WM_SEG && L == SEG_MAX_L_NARROW && sw(in.seg6, 1) != 0) {
        // 4^6 states can still be enumerated -- 5^6 cannot: the layout k_lt chose decides (narrow stays narrow: candidates only disappear)
        if (in.ranked < 0) { p.need_layout = 1; return p; }
        p.seg6 = seg = in.ranked != 0;
    }
    p.rw_lanes = (seg || cw_ok(wm, L)) ? lanes : 8;
    p.stride = rw_blocks_of(N, p.rw_lanes);                     // the blocks of the widest reweight kernel this spin may launch
    if (!seg) {
        p.flow = (cw_ok(wm, L) && !in.pools_off) ? GH_FLOW_POOLS : GH_FLOW_SERIAL;
        p.S = p.flow == GH_FLOW_POOLS ? cw_geometry(N, L).S : 0;
        return p;
    }
    p.S = seg_S(N, L);
    // three launches, no k_emit: where the group maps fit k_rw's LDS and the band the halo it resolves; bit-identical but measured
    // slower than four (docs/HISTORY.md, H), so opt-in: GH_FUSE=1 (large windows) or 2 (every window the maps fit; the tests)
    const int fuse = sw(in.fuse, 0);
    if (in.need_rinfo && W <= RW_FUSE_HALO && lanes == 8 && fuse >= 1) {
        if (in.ranked < 0) { p = spin_plan{}; p.need_layout = 1; return p; }
        const int R = in.ranked ? 4 : 5;
        const size_t lds = rw_fuse_lds_bytes(N, L, R, 256 / lanes, W);
        const bool small_r = emit_small_lds_bytes(N, L, R) <= 64 * 1024 && sw(in.emit_small, 1) != 0;
        // (small windows -- by the table's own radix -- keep k_emit_small: three launches too)
        if ((!small_r || fuse == 2) && seg_radix_ok(R, L) && lds <= 64 * 1024) { p.flow = GH_FLOW_FUSE; p.lds = (int64_t)lds; return p; }
    }
    p.flow = GH_FLOW_SEG;
    p.emit_small = emit_small_ok(N, L, in.emit_small);
    p.mixed = mixed_ok(sw(in.mixed, 1) != 0, false, L, wm, in.offer_zero);
    // k_rwseg: the reweight of a path rides in the k_seg launch of the next one.  Lane groups of 8, at most 128 positions per workgroup
    // with the halo, and its LDS must fit (the column conditionals stage the band blocks of all those positions)
    if (!in.lt_full && lanes == 8 && sw(in.rwseg, 1) != 0 && (!p.emit_small || sw(in.rwseg_small, 1) != 0)) {
        const int longest = (int)max_cls(L, [&](int R) { return (size_t)seg_geometry(N, L, R).seglen; });
        const size_t lds = rws_patch_off(N, W, L, col, in.storage == GH_STORAGE_F64 ? 8 : 4) + sizeof(seg_patch);
        if (longest + L + 1 <= SEG_THREADS / 8 && lds <= RWS_LDS_MAX) {
            p.flow = GH_FLOW_RWSEG; p.lds = (int64_t)lds;
            if (p.S > p.stride) p.stride = p.S;                 // k_rwseg leaves one partial sum per segment
        }
    }
    return p;
}

// what the choice depends on for this handle; the layout not looked at
static gh_spin_plan_in plan_inputs(const gh_handle *h)
{
    gh_spin_plan_in in{};
    in.n_snps = h->N; in.band = h->W; in.L = h->L; in.storage = h->cfg.storage; in.cond_mode = h->cfg.cond_mode;
    in.marginal_term = h->cfg.marginal_term; in.offer_zero = h->cfg.offer_zero; in.ranked = -1;
    in.walk_mode = h->wmode; in.lt_full = h->lt_full; in.need_rinfo = h->need_rinfo; in.pools_off = h->cw_off;
    in.rwseg = env_int("GH_RWSEG", -1); in.rwseg_small = env_int("GH_RWSEG_SMALL", -1); in.emit_small = env_int("GH_EMIT_SMALL", -1);
    in.fuse = env_int("GH_FUSE", -1); in.seg6 = env_int("GH_SEG6", -1);
    in.mixed = mixed_on(); in.rw_lp16 = rw_lp16_on(); in.rw_tband = rw_tband_on();      // (per process)
    return in;
}

extern "C" int gh_debug_spin_plan(const gh_spin_plan_in *in, gh_spin_plan *out)
{
    if (!in || !out) return fail(GH_ERR_ARG, "null argument");
    if (in->n_snps < 1 || in->band < 1 || in->L < 1 || (in->storage != GH_STORAGE_F32 && in->storage != GH_STORAGE_F64) ||
        in->cond_mode < GH_COND_A || in->cond_mode > GH_COND_E || in->walk_mode < WM_SEG || in->walk_mode > WM_SRC || in->ranked < -1 || in->ranked > 1)
        return fail(GH_ERR_ARG, "spin plan: n_snps >= 1, band >= 1, L >= 1, a storage, a conditional, a walk mode, ranked in -1..1");
    *out = plan_spin(*in);
    return GH_OK;
}

extern "C" int gh_debug_last_spin_plan(gh_t *h, gh_spin_plan *out)
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    *out = h->last_plan;
    return GH_OK;
}

extern "C" int gh_spin(gh_t *h, int max_paths, double min_remove, uint8_t *paths_out, gh_path_rec *recs,
                       int *n_out, int *hole_at)
{
    if (!h || !paths_out || !recs || !n_out || !hole_at) return fail(GH_ERR_ARG, "null argument");
    if (max_paths < 0) return fail(GH_ERR_ARG, "max_paths < 0");
    if (set_dev(h)) return GH_ERR_HIP;
    *n_out = 0; *hole_at = 0;
    if (max_paths == 0) return GH_OK;
    int rc;
    if (!h->have_orig && (rc = gh_snapshot_original(h))) return rc;
    if ((rc = ensure_spin_buffers(h, max_paths))) return rc;
    spin_io io{};
    io.max_paths = max_paths; io.min_remove = min_remove; io.n1 = (size_t)h->N + 1; io.paths_out = paths_out; io.recs = recs;
    gh_spin_plan_in in = plan_inputs(h);
    io.plan = plan_spin(in);
    if (io.plan.need_layout) {
        // which layout did k_lt choose for this tensor?  One look per spin, only where the choice depends on it
        dev_state look;
        if ((rc = ensure_lt(h)) || (rc = read_state(h, &look))) return rc;
        in.ranked = look.ranked ? 1 : 0;
        io.plan = plan_spin(in);
    }
    const spin_plan &plan = h->last_plan = io.plan;
    const bool rws = plan.flow == GH_FLOW_RWSEG, fused = plan.flow == GH_FLOW_FUSE, seg = rws || fused || plan.flow == GH_FLOW_SEG;
    if ((rws || fused) && (rc = alloc_seg(h))) return rc;
    // (the three-launch flow walks the enumerated states: whatever k_classify found before the flow was chosen does not apply)
    if (fused) HIPCHK(hipMemsetAsync(&h->dstate->maxstates, 0, sizeof(int), h->stream));
    const size_t halo = rws ? (size_t)plan.S * h->L * NSYM * h->W * NSYM * esize(h) : 0;
    if (halo > h->seg_halo_bytes) {
        HIPCHK(hipStreamSynchronize(h->stream));
        hipFree(h->seg_halo); h->seg_halo = nullptr; h->seg_halo_bytes = 0;
        if (hipMalloc(&h->seg_halo, halo) != hipSuccess) return fail(GH_ERR_NOMEM, "hipMalloc failed");
        h->seg_halo_bytes = halo;
    }
    // L only changes through gh_set_L / gh_fill, never inside a spin
    if ((rc = ensure_partial(h, plan.stride, max_paths > h->spin_cap ? max_paths : h->spin_cap))) return rc;
    // (k_rwseg: every slot is summed over the whole stride: what a kernel with fewer workgroups leaves untouched must read 0)
    if ((rc = reset_spin_state(h, rws ? h->partial : nullptr, rws ? (size_t)plan.stride * max_paths : 0))) return rc;
    // no k_lt between two paths over the enumerated states: the reweight keeps the table current, and where a candidate mask moved
    // (rare) the next k_seg marks the table stale and the rest of the queue idles; the host rebuilds and queues the rest again
    const bool optimistic = seg && !h->lt_full;
    dev_state hs;
    memset(&hs, 0, sizeof hs);
    int first = 0;
    bool cw_gave_up = false;
    h->spin_requeues = 0;
    if (plan.flow == GH_FLOW_POOLS && (rc = spin_candidate_pools(h, io, hs, &first, &cw_gave_up))) return rc;
    // (the pools hand paths `first` .. to the serial walkers when the window turns out to have a position with five candidates)
    while (plan.flow != GH_FLOW_POOLS || cw_gave_up) {
        int launched = first;
        for (int s = first; s < max_paths; s++) {
            if ((!optimistic || s == first) && (rc = ensure_lt(h, !seg, true, fused))) return rc;
            const int cmk = !(optimistic && s > first) ? 0 : (s == h->force_stale_at && h->spin_requeues == 0 ? 2 : 1);
            uint8_t *pth = h->spin_paths + io.n1 * s;
            double *lmsel = h->spin_lmsel + io.n1 * s;
            // k_rwseg: path s is walked by the launch that reweights path s - 1; the last path's reweight is a plain k_rw
            if (rws && s > first) rc = launch_rwseg(h, plan, pth - io.n1, h->spin_recs + (s - 1), s - 1, min_remove, pth, lmsel, cmk);
            else rc = launch_walk(h, plan, pth, h->spin_recs + s, min_remove, 1, lmsel, cmk);
            if (rc) return rc;
            if (!rws || s == max_paths - 1) {
                rw_req q;
                q.path = pth; q.rec = h->spin_recs + s; q.ratio = seg ? min_remove : 0.0; q.slot = s; q.seg = seg;
                q.chained = optimistic && s > first; q.lmsel = lmsel;
                if ((rc = launch_reweight_marg(h, plan, q))) return rc;
            }
            launched = s + 1;
        }
        bool staged;
        if ((rc = finish_spin(h, io, launched, seg || cw_gave_up, seg ? 0 : 1, hs, &staged))) return rc;
        if (getenv("GH_PRINT_STATE"))
            fprintf(stderr, "gh_spin: stop %d hole_at %d n_done %d first_hole %d cur_hole %d lt_stale %d cm_same %d narrow %d ranked %d\n", hs.stop, hs.hole_at,
                    hs.n_done, hs.first_hole, hs.cur_hole, hs.lt_stale, hs.cm_same, hs.narrow, hs.ranked);
        if (optimistic && hs.lt_stale && !hs.stop && hs.n_done < max_paths) {
            // paths 0 .. n_done-1 are complete; the table has just been rebuilt (finish_spin): queue the rest again
            if ((rc = clear_flags(h, &h->dstate->lt_stale))) return rc;
            first = hs.n_done;
            h->spin_requeues++;
            continue;
        }
        if ((rc = deliver_results(h, io, hs, launched, staged))) return rc;
        break;
    }
    *n_out = hs.n_done;
    *hole_at = hs.stop ? hs.hole_at : 0;
    return GH_OK;
}

// batched recovery: many windows of one shape, every kernel launched over all of them ---------
struct gh_batch {
    int n, dev, N, W, L;
    std::vector<gh_handle *> hs;
    hipStream_t stream;
    hipStream_t gstream[3];     // window groups of the batched kernels (gh_batch_spin): created on first use
    hipEvent_t gevent[3];
    win_desc *d_wd;
    dev_state *d_states;        // every window's dev_state, gathered by k_batch_states for one copy to the host
    uint8_t *d_paths;           // window w's paths at d_paths + off[w], [max_paths][N_w + 1] back to back (batch_path_offsets)
    gh_path_rec *d_recs;        // [n][max_paths]
    double *d_partial;
    int cap_paths, nb;          // cap_paths: the max_paths d_paths and d_recs hold
    int prof_every;             // gh_batch_profile_enable
    int pipe_windows, pipe_aborted;     // the last spin: windows the pipeline (wpipe.hpp) carried / handed back to gh_spin
    int pinfo_nt, pinfo_c;              // ... and threads and chunk of its group with the most windows
    std::vector<hipEvent_t> pev[2];     // [0] extension, [1] reweight: start/stop pairs of the last spin (group 0's stream)
    size_t pused[2];
    int prof_windows;
    double prof_bytes[2];
    // d_wd holds 2n descriptors: every window's, and the lists the pipeline's launches take
    // panels (gh_panel_*): windows that differ in N, W and L.  N, W above are then the largest window's
    bool panel;
    // gh_panel_viterbi_spin (viterbi_panel.hpp): descriptors, gathered vit_outs and path rows; an event per window that orders
    // its handle's stream before the batch's; what gh_panel_viterbi_info reports
    dev_scratch vit;
    std::vector<hipEvent_t> vit_ev;
    int64_t vit_info[4];
    int64_t vitm_info[4];       // gh_panel_viterbi_marginals_info (viterbi_marg_panel.hpp: the same block and events)
    int64_t vitk_info[4];       // gh_panel_viterbi_kbest_info (viterbi_kbest_panel.hpp: likewise)
};

extern "C" int gh_batch_destroy(gh_batch_t *b)
{
    if (!b) return GH_OK;
    hipSetDevice(b->dev);
    if (b->stream) hipStreamSynchronize(b->stream);
    hipFree(b->d_wd); hipFree(b->d_states); hipFree(b->d_paths); hipFree(b->d_recs); hipFree(b->d_partial); hipFree(b->vit.buf);
    for (hipEvent_t e : b->vit_ev) hipEventDestroy(e);
    for (int g = 0; g < 3; g++) {
        if (b->gstream[g]) { hipStreamSynchronize(b->gstream[g]); hipStreamDestroy(b->gstream[g]); }
        if (b->gevent[g]) hipEventDestroy(b->gevent[g]);
    }
    for (int k = 0; k < 2; k++)
        for (hipEvent_t e : b->pev[k]) hipEventDestroy(e);
    if (b->stream) hipStreamDestroy(b->stream);
    delete b;
    return GH_OK;
}

// gh_batch_create / gh_panel_create: a panel's windows may differ in N and W (and in L, gh_panel_spin)
static int batch_create(gh_t **handles, int n, gh_batch_t **out, bool panel)
{
    if (!handles || n < 1 || !out) return fail(GH_ERR_ARG, "bad argument");
    gh_handle *h0 = handles[0];
    int maxN = 0, maxW = 0;
    for (int w = 0; w < n; w++) {
        gh_handle *h = handles[w];
        if (!h) return fail(GH_ERR_ARG, "null handle at %d", w);
        if ((!panel && (h->N != h0->N || h->W != h0->W)) || h->dev != h0->dev || h->cfg.storage != h0->cfg.storage ||
            h->cfg.cond_mode != h0->cfg.cond_mode || h->cfg.marginal_term != h0->cfg.marginal_term ||
            h->cfg.offer_zero != h0->cfg.offer_zero || memcmp(h->cfg.cand_order, h0->cfg.cand_order, 5) != 0)
            return fail(GH_ERR_ARG, panel ? "window %d differs from window 0 in storage, mode or device"
                                          : "window %d differs from window 0 in shape, storage, mode or device", w);
        for (int v = 0; v < w; v++)
            if (handles[v] == h) return fail(GH_ERR_ARG, "window %d is the same handle as window %d", w, v);
        if (h->N > maxN) maxN = h->N;
        if (h->W > maxW) maxW = h->W;
    }
    HIPCHK(hipSetDevice(h0->dev));
    gh_batch *b = new (std::nothrow) gh_batch();
    if (!b) return fail(GH_ERR_NOMEM, "host allocation failed");
    b->n = n; b->dev = h0->dev; b->N = maxN; b->W = maxW; b->L = 0;
    b->hs.assign(handles, handles + n);
    b->stream = nullptr; b->d_wd = nullptr; b->d_states = nullptr; b->d_paths = nullptr; b->d_recs = nullptr; b->d_partial = nullptr;
    for (int g = 0; g < 3; g++) { b->gstream[g] = nullptr; b->gevent[g] = nullptr; }
    b->cap_paths = 0;
    b->pipe_windows = b->pipe_aborted = 0;
    b->prof_every = 0; b->pused[0] = b->pused[1] = 0; b->prof_windows = 0; b->prof_bytes[0] = b->prof_bytes[1] = 0.0;
    b->panel = panel; b->pinfo_nt = b->pinfo_c = 0;
    b->nb = (int)(((size_t)(b->N + 1) * (b->W > 8 ? b->W : 8) + 255) / 256);   // >= blocks of k_marg<.., true>
    hipError_t e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_wd, sizeof(win_desc) * n * 2);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_states, sizeof(dev_state) * n);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_partial, sizeof(double) * (size_t)b->nb * n);
    if (e != hipSuccess) { gh_batch_destroy(b); return fail(GH_ERR_NOMEM, "batch allocation failed: %s", hipGetErrorString(e)); }
    *out = b;
    return GH_OK;
}
extern "C" int gh_batch_create(gh_t **handles, int n, gh_batch_t **out) { return batch_create(handles, n, out, false); }
extern "C" int gh_panel_create(gh_t **handles, int n, gh_batch_t **out) { return batch_create(handles, n, out, true); }

// gh_batch_spin's bookkeeping over all windows in one launch each: the control words a spin starts from (k_spin_reset's), and
// every window's state into one array the host fetches with one copy (256 small copies cost 4 ms)
__global__ void k_batch_reset(const win_desc *wd)
{
    dev_state *st = wd[blockIdx.x].st;
    if (threadIdx.x == 0) { st->stop = 0; st->hole_at = 0; st->n_done = 0; st->lt_stale = 0; st->cw_unres = 0; st->pipe_status = 0; }
}
__global__ void k_batch_states(const win_desc *wd, dev_state *out)
{
    const unsigned *src = reinterpret_cast<const unsigned *>(wd[blockIdx.x].st);
    unsigned *dst = reinterpret_cast<unsigned *>(out + blockIdx.x);
    for (unsigned q = threadIdx.x; q < sizeof(dev_state) / 4; q += blockDim.x) dst[q] = src[q];
}

// ---- the window pipeline (wpipe.hpp): one persistent workgroup per window -------------------------------------------------
// threads per workgroup for lag count L (what the walker's register rotation leaves of 512 registers per SIMD lane); 0 = none
static int pipe_threads(int L)
{
    const int env = env_int("GH_PIPE_NT", 0);      // (read on every call: the tests switch)
    // (beyond ten lags the 512-thread form walks chunks of 11..14 positions and loses to the candidate pools on their own streams:
    // 20-25k against 31k haplotypes/s at 128 windows, scratch/pipe_lsweep.py; GH_PIPE_MAX_L=14 takes it all the same -- the tests)
    const int max_l = env_int("GH_PIPE_MAX_L", 10);
    if (L < 2 || L > 14 || L > max_l) return 0;
    if (env == 512 || env == 768 || env == 1024) return env;
    return L <= 6 ? 1024 : (L <= 10 ? 768 : 512);
}
// which specs the pipeline carries: every conditional -- the row conditionals A, B, D and, on the to-major copy of the band, the
// column conditionals C, E --, with or without the marginal term (the walker adds it in front of the lag-1 term from the
// log-marginals the sweep keeps by rank).  GH_PIPE_COL=0 / GH_PIPE_MT=0 leave those to the batched launches (A/B measurements).
static bool pipe_spec_ok(const gh_handle *h)
{
    const bool col = h->cfg.cond_mode == GH_COND_C || h->cfg.cond_mode == GH_COND_E;
    const bool no_mt = env_off("GH_PIPE_MT");
    const bool no_col = env_off("GH_PIPE_COL");
    return !h->lt_full && !(col && no_col) && !(h->cfg.marginal_term && no_mt);
}
static int pipe_sweep_threads(int nt) { return nt == 1024 ? pipe_roles<1024>::NRW * 64 : (nt == 768 ? pipe_roles<768>::NRW * 64 : pipe_roles<512>::NRW * 64); }

// the narrow launch, and for windows with a few five-candidate positions the WIDE one (k_wpipe<.., WIDE = true>, wpipe.hpp): the
// default thread counts only
template <typename T, bool WIDE, int LC, int NT>
static hipError_t launch_wpipe_t(const pipe_params &P, const win_desc *d_wd, int n, size_t lds, hipStream_t st)
{
    hipError_t e = hipFuncSetAttribute((const void *)k_wpipe<T, LC, NT, WIDE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_wpipe<T, LC, NT, WIDE>), dim3(n), dim3(NT), lds, st, P, d_wd);
    return hipGetLastError();
}
template <typename T, bool WIDE>
static hipError_t launch_wpipe(int L, int nt, const pipe_params &P, const win_desc *d_wd, int n, size_t lds, hipStream_t st)
{
#define GH_PIPE_CASE(l, t) case l: return launch_wpipe_t<T, WIDE, l, t>(P, d_wd, n, lds, st);
    if (nt == 1024) {
        switch (L) { GH_PIPE_CASE(2, 1024) GH_PIPE_CASE(3, 1024) GH_PIPE_CASE(4, 1024) GH_PIPE_CASE(5, 1024) GH_PIPE_CASE(6, 1024) }
    } else if (nt == 768) {
        if constexpr (!WIDE) { if (L == 5) return launch_wpipe_t<T, false, 5, 768>(P, d_wd, n, lds, st); }
        switch (L) { GH_PIPE_CASE(7, 768) GH_PIPE_CASE(8, 768) GH_PIPE_CASE(9, 768) GH_PIPE_CASE(10, 768) }
    } else if constexpr (!WIDE) {
        if (nt == 512)
            switch (L) { GH_PIPE_CASE(3, 512) GH_PIPE_CASE(5, 512) GH_PIPE_CASE(11, 512) GH_PIPE_CASE(12, 512) GH_PIPE_CASE(13, 512) GH_PIPE_CASE(14, 512) }
    }
#undef GH_PIPE_CASE
    return hipErrorInvalidValue;
}
static bool pipe_wide_instantiated(int L, int nt) { return (nt == 1024 && L >= 2 && L <= 6) || (nt == 768 && L >= 7 && L <= 10); }

static bool pipe_instantiated(int L, int nt)
{
    if (nt == 1024) return L >= 2 && L <= 6;
    if (nt == 768) return L == 5 || (L >= 7 && L <= 10);
    if (nt == 512) return L == 3 || L == 5 || (L >= 11 && L <= 14);
    return false;
}

// what a spin over the n windows whose descriptors stand at gwd starts with, on `st`: the control words re-armed, marginals, snapshot.
// N, W: the largest window's -- they size the grids; every kernel takes its window's own shape from the descriptor
static void launch_preamble(const gh_handle *h0, hipStream_t st, const win_desc *gwd, int n, int N, int W)
{
    const unsigned marg_gx = (unsigned)(((N + 1) * 8 + 255) / 256);
    marg_args m;
    m.N = N; m.W = W; m.wd = gwd; m.sm = h0->sm; m.offer_zero = h0->cfg.offer_zero;
    hipLaunchKernelGGL(k_rearm, dim3(n), dim3(64), 0, st, (dev_state *)nullptr, gwd, 0);
    launch_marg<false>(h0, dim3(marg_gx, n), st, m);
    hipLaunchKernelGGL(k_snapshot, dim3(marg_gx, n), dim3(256), 0, st, (double *)nullptr, (const double *)nullptr, N, gwd);
}
// the arguments of a batched k_lt over windows of up to N SNPs (every pointer from the descriptors)
static lt_args batch_lt_args(const gh_handle *h0, const win_desc *gwd, int N, int W, int L)
{
    lt_args a;
    a.N = N; a.W = W; a.L = L; a.cond_mode = h0->cfg.cond_mode; a.wd = gwd;
    a.allow_ranked = walk_depth2_ok(h0->wmode == WM_SEG ? WM_SPEC : h0->wmode, L); a.sm = h0->sm;
    return a;
}
// the pipeline's preamble: the above and the full table of every window
static void pipe_preamble(const gh_handle *h0, hipStream_t st, const win_desc *gwd, int n, int N, int W, int L)
{
    size_t lt_nb = ((size_t)(N + LT_PAD) * L * LT_BLK + 255) / 256;
    if (lt_nb > 4096) lt_nb = 4096;
    launch_preamble(h0, st, gwd, n, N, W);
    // (the table WITHOUT the marginal term baked into its lag-1 entries: the pipeline's walker adds it itself)
    launch_lt(h0, dim3((unsigned)lt_nb, n), st, batch_lt_args(h0, gwd, N, W, L));
}
// the pipeline's launch parameters for windows of up to N SNPs (C and the LDS: sized by the largest window) and their LDS bytes
static pipe_params pipe_make_params(const gh_handle *h0, int N, int W, int L, int nt, bool wide, int max_paths, double min_remove, size_t *lds)
{
    const int es = (int)esize(h0);
    const int nr = pipe_sweep_threads(nt);
    pipe_params P;
    P.N = N; P.W = W; P.L = L; P.mt = h0->cfg.marginal_term ? 1 : 0; P.col = (h0->cfg.cond_mode == GH_COND_C || h0->cfg.cond_mode == GH_COND_E) ? 1 : 0;
    P.C = wide ? pipe_chunk_w(N, L, nr, es, P.mt) : pipe_chunk(N, L, nr, es, P.mt);
    P.max_paths = max_paths; P.cond_mode = h0->cfg.cond_mode;
    P.synth = env_int("GH_PIPE_SYNTH", 1) != 0;          // (wpipe.hpp, the loaders: what it gains and costs)
    P.offer_zero = h0->cfg.offer_zero; P.prof = 0; P.min_remove = min_remove; P.sm = h0->sm;
    *lds = wide ? pipe_lds_bytes_w(N, L, P.C, nr, es, P.mt) : pipe_lds_bytes(N, L, P.C, nr, es, P.mt);
    return P;
}

// the batched launches of rounds 1-4 over the windows `wd` describes (a path = k_lt's flag check, one serial walker per window, the
// fused reweight k_marg<T,true>, the removed mass); returns with every stream drained
static int batch_run_launches(gh_batch *b, const std::vector<win_desc> &wd, int max_paths, double min_remove, bool reset = true)
{
    const int n = (int)wd.size();
    if (n == 0) return GH_OK;
    HIPCHK(hipMemcpyAsync(b->d_wd, wd.data(), sizeof(win_desc) * n, hipMemcpyHostToDevice, b->stream));
    if (reset) hipLaunchKernelGGL(k_batch_reset, dim3(n), dim3(64), 0, b->stream, (const win_desc *)b->d_wd);
    HIPCHK(hipStreamSynchronize(b->stream));        // wd is a host temporary

    gh_handle *h0 = b->hs[0];
    const int N = b->N, W = b->W, L = b->L;
    const int bwm = h0->wmode == WM_SEG ? WM_SPEC : h0->wmode;     // batched launches: one serial walker per window
    const unsigned marg_gx = (unsigned)(((N + 1) * 8 + 255) / 256);
    size_t lt_nb = ((size_t)(N + LT_PAD) * L * LT_BLK + 255) / 256;
    if (lt_nb > 4096) lt_nb = 4096;
    walk_params P;
    P.N = N; P.L = L; P.chunk = 0; P.rearm = 1; P.G = nullptr; P.Ht = nullptr; P.Yt = nullptr; P.minfo = nullptr; P.path_out = nullptr; P.rec = nullptr; P.st = nullptr;
    P.min_remove = min_remove; P.sm = h0->sm;
    size_t lt_nb_inc = 64;                  // batched launches keep no walker tables: the steady-state k_lt only checks flags
    if (lt_nb_inc > 4096) lt_nb_inc = 4096;
    const bool inc_mode = lt_incremental_ok(h0);
    // the fused reweight over the windows: path, partial sums and records from the descriptors
    marg_args rw;
    rw.N = N; rw.W = W; rw.use_state_ratio = 1; rw.G = inc_mode ? (double *)b->d_paths : nullptr;   // (non-null: take G from wd)
    rw.L = L; rw.cond_mode = h0->cfg.cond_mode; rw.sm = h0->sm; rw.offer_zero = h0->cfg.offer_zero;
    // The windows go in up to three GROUPS, each on its own stream and one phase behind the group in front: a path is a
    // serial extension (one workgroup per window, 0.6 ms for 10k SNPs whatever the number of windows: latency) followed by
    // a reweight (HBM-bound, ~4 us per window).  In step, every group would wait out the extension with an idle memory
    // system and then share it; staggered, one group reweights while the others extend.
    static const int groups_env = env_int("GH_BATCH_GROUPS", 0);
    int NG = groups_env > 0 ? groups_env : (n >= 96 ? 3 : (n >= 32 ? 2 : 1));
    if (NG > 3) NG = 3;
    if (NG > n) NG = n;
    for (int g = 0; g < NG; g++) {
        if (!b->gstream[g]) HIPCHK(hipStreamCreateWithFlags(&b->gstream[g], hipStreamNonBlocking));
        if (!b->gevent[g]) HIPCHK(hipEventCreateWithFlags(&b->gevent[g], hipEventDisableTiming));
    }
    b->pused[0] = b->pused[1] = 0;
    auto pmark = [&](int k, hipStream_t st) {            // one event of a start/stop pair of kernel k
        if (b->pused[k] >= b->pev[k].size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            b->pev[k].push_back(e);
        }
        hipEventRecord(b->pev[k][b->pused[k]++], st);
    };
    for (int s = 0; s < max_paths; s++) {
        // any non-null pointer tells k_lt that the fused reweight of spin s-1 has already rewritten the rows it changed
        const uint8_t *inc = (s > 0 && inc_mode) ? b->d_paths : nullptr;
        for (int g = 0; g < NG; g++) {
            const int w0 = (int)((long long)n * g / NG), ng = (int)((long long)n * (g + 1) / NG) - w0;
            const win_desc *gwd = b->d_wd + w0;
            hipStream_t st = b->gstream[g];
            if (s == 0) {
                // (group g starts when group g-1 has finished its first extension)
                if (g > 0) hipStreamWaitEvent(st, b->gevent[g - 1], 0);
                launch_preamble(h0, st, gwd, ng, N, W);
            }
            lt_args la = batch_lt_args(h0, gwd, N, W, L);
            la.bake_lm = h0->cfg.marginal_term; la.inc_path = inc; la.spin = s;
            launch_lt(h0, dim3((unsigned)(inc ? lt_nb_inc : lt_nb), ng), st, la);
            const bool sample = g == 0 && b->prof_every > 0 && s > 0 && (s % b->prof_every) == 0;
            if (sample) { b->prof_windows = ng; pmark(0, st); }
            launch_walk_any(bwm, N, L, P, st, ng, gwd, s);
            if (sample) pmark(0, st);
            if (s == 0 && g + 1 < NG) hipEventRecord(b->gevent[g], st);
            if (sample) pmark(1, st);
            rw.wd = gwd; rw.spin = s;
            launch_marg<true>(h0, dim3(marg_gx, ng), st, rw);
            if (sample) pmark(1, st);
            hipLaunchKernelGGL(k_reweight_finish, dim3(ng), dim3(256), 0, st, (const double *)nullptr, (int)marg_gx,
                               (dev_state *)nullptr, 1, (gh_path_rec *)nullptr, gwd, s);
        }
        {
            const hipError_t le = hipGetLastError();            // (a launch that failed is named with its path, not found at the end)
            if (le != hipSuccess) return fail(GH_ERR_HIP, "gh_batch_spin: a launch of path %d failed: %s", s, hipGetErrorString(le));
        }
    }
    for (int g = 0; g < NG; g++) HIPCHK(hipStreamSynchronize(b->gstream[g]));
    HIPCHK(hipGetLastError());
    {
        // algorithmic bytes per window and launch (launch_walk / launch_reweight_marg use the same definitions)
        b->prof_bytes[0] = walk_bytes(N, L, esize(h0));
        b->prof_bytes[1] = reweight_bytes(N, W, L, esize(h0), inc_mode);
    }
    return GH_OK;
}

// gh_spin over some windows of a batch from a few host threads, every window on its own stream (the windows' kernel chains
// interleave on the GPU).  A job is (window, paths it already has): the spin writes the window's remaining paths behind them.
// Window w's paths stand at paths_out + paths_off[w], [max_paths][N_w + 1].
static int batch_spin_on_streams(gh_batch *b, const std::vector<std::pair<int, int>> &jobs, int max_paths, double min_remove,
                                 uint8_t *paths_out, const int64_t *paths_off, gh_path_rec *recs, int *n_out, int *hole_at)
{
    const int nj = (int)jobs.size();
    if (nj == 0) return GH_OK;
    static const int nthr_env = env_int("GH_BATCH_THREADS", 8);
    const int nthr = nthr_env < 1 ? 1 : (nthr_env > nj ? nj : nthr_env);
    std::vector<int> rcs(nj, GH_OK);
    std::vector<std::string> errs(nj);
    std::atomic<int> next(0);
    auto work = [&]() {
        hipSetDevice(b->dev);
        for (;;) {
            const int q = next.fetch_add(1);
            if (q >= nj) break;
            const int w = jobs[q].first, nd = jobs[q].second;
            int n2 = 0, hole2 = 0;
            if (nd < max_paths) {
                const size_t n1 = (size_t)b->hs[w]->N + 1;
                uint8_t *pw = paths_out + paths_off[w] + n1 * nd;
                rcs[q] = gh_spin(b->hs[w], max_paths - nd, min_remove, pw, recs + (size_t)max_paths * w + nd, &n2, &hole2);
                if (rcs[q]) errs[q] = gh_last_error();
            }
            n_out[w] = nd + n2;
            hole_at[w] = hole2;
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthr; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    for (int q = 0; q < nj; q++)
        if (rcs[q]) return fail(rcs[q], "window %d: %s", jobs[q].first, errs[q].c_str());
    return GH_OK;
}

// ---- the window pipeline's host driver: gh_batch_spin and gh_panel_spin both run it --------------------------------------------
// GH_PIPE_STAMPS: the host phases of a spin on stderr
struct spin_phases {
    const char *who;
    bool on;
    double t;
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    explicit spin_phases(const char *w) : who(w), on(getenv("GH_PIPE_STAMPS") != nullptr), t(now()) {}
    void operator()(const char *what)
    {
        if (!on) return;
        const double t1 = now();
        fprintf(stderr, "%s: %-28s %8.3f ms\n", who, what, t1 - t);
        t = t1;
    }
};

// both spins start here: every window's table allocated, and whatever the handles' own streams still carry (fills) done before the
// batch's streams touch the tensors -- those streams, not the device: a device-wide wait also waits for whatever else the process
// runs (ResultExchange's gather on its side stream in a multi-rank run)
static int batch_spin_begin(gh_batch *b)
{
    int rc;
    for (int w = 0; w < b->n; w++)
        if ((rc = alloc_lt(b->hs[w]))) return rc;
    for (int w = 0; w < b->n; w++) HIPCHK(hipStreamSynchronize(b->hs[w]->stream));
    return GH_OK;
}

// where window w's paths stand in the batch's device buffer: [max_paths][N_w + 1] per window, back to back in window order (for a
// batch [n][max_paths][N + 1], the caller's layout too); off[n] = the whole buffer
static std::vector<int64_t> batch_path_offsets(const gh_batch *b, int max_paths)
{
    std::vector<int64_t> off((size_t)b->n + 1, 0);
    for (int w = 0; w < b->n; w++) off[w + 1] = off[w] + ((int64_t)b->hs[w]->N + 1) * max_paths;
    return off;
}
// the device homes of the results: paths at those offsets, records [n][max_paths]
static int batch_buffers(gh_batch *b, int max_paths, const std::vector<int64_t> &off)
{
    if (max_paths <= b->cap_paths) return GH_OK;
    HIPCHK(hipStreamSynchronize(b->stream));
    hipFree(b->d_paths); hipFree(b->d_recs);
    b->d_paths = nullptr; b->d_recs = nullptr; b->cap_paths = 0;
    HIPCHK(hipMalloc((void **)&b->d_paths, (size_t)off[b->n]));
    HIPCHK(hipMalloc((void **)&b->d_recs, sizeof(gh_path_rec) * (size_t)max_paths * b->n));
    b->cap_paths = max_paths;
    return GH_OK;
}

// window w's descriptor (kernels.hpp): its tensors and state, its share of the batch's buffers, the pipeline buffers it has
static win_desc batch_desc(gh_batch *b, int w, int max_paths, const std::vector<int64_t> &off)
{
    gh_handle *h = b->hs[w];
    win_desc d;
    memset(&d, 0, sizeof(d));
    d.band = h->band; d.cnt = h->cnt; d.marg = h->marg; d.minfo = h->minfo; d.nvalid = h->nvalid; d.cmask = h->cmask;
    d.rinfo = h->need_rinfo ? h->rinfo : nullptr; d.G = h->lt; d.Ht = nullptr; d.Yt = nullptr; d.st = h->dstate;   // no walker tables in batches (kernels.hpp)
    d.partial = b->d_partial + (size_t)w * b->nb;
    d.paths = b->d_paths + off[w];
    d.recs = b->d_recs + (size_t)max_paths * w;
    d.snap = h->have_orig ? 0 : 1;       // the first batched k_marg is followed by a batched snapshot
    d.pk = h->pipe_pk; d.gp = h->pipe_gp; d.lmr = h->pipe_lm; d.tband = h->tband; d.gw = h->pipe_gw;
    d.wdir = h->pipe_gw ? reinterpret_cast<int *>(h->pipe_gw + (size_t)PIPE_WMAX * pipe_wrec_doubles(h->L)) : nullptr;
    d.N = h->N; d.W = h->W;
    h->have_orig = true;
    return d;
}

// the states of the windows ws, whose descriptors stand at b->d_wd[0 ..) in that order, into hs[ws[i]]: one launch, one copy
static int batch_gather_states(gh_batch *b, const std::vector<int> &ws, std::vector<dev_state> &hs)
{
    const int m = (int)ws.size();
    if (m == 0) return GH_OK;
    std::vector<dev_state> tmp(m);
    hipLaunchKernelGGL(k_batch_states, dim3(m), dim3(64), 0, b->stream, (const win_desc *)b->d_wd, b->d_states);
    HIPCHK(hipMemcpyAsync(tmp.data(), b->d_states, sizeof(dev_state) * m, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (int i = 0; i < m; i++) hs[ws[i]] = tmp[i];
    return GH_OK;
}

// the pipeline's buffers of one window, at its own N and L; under the column conditionals also the to-major copy of the band,
// brought in step with it on b->stream (the pipeline's sweep then keeps both, element by element)
static int pipe_buffers(gh_batch *b, gh_handle *h)
{
    if (!h->pipe_pk) HIPCHK(hipMalloc((void **)&h->pipe_pk, sizeof(unsigned long long) * ((size_t)h->N + 2)));
    const size_t need = sizeof(double) * ((size_t)h->N + LT_PAD) * 16 * (size_t)h->L;
    if (h->pipe_gp_bytes < need) {
        hipFree(h->pipe_gp); h->pipe_gp = nullptr; h->pipe_gp_bytes = 0;
        HIPCHK(hipMalloc((void **)&h->pipe_gp, need));
        h->pipe_gp_bytes = need;
    }
    if (h->cfg.marginal_term && !h->pipe_lm) HIPCHK(hipMalloc((void **)&h->pipe_lm, sizeof(double) * 4 * ((size_t)h->N + 2)));
    if (h->cfg.cond_mode == GH_COND_C || h->cfg.cond_mode == GH_COND_E) {
        int rc = ensure_tband(h, b->stream);
        if (rc) return rc;
        h->tband_epoch = h->band_epoch;
    }
    return GH_OK;
}

// windows the pipeline carries together: one lag count (it is instantiated per lag count), sized by the largest window
struct pipe_group { int L, nt, N, W; std::vector<int> ws; };

// The window pipeline (wpipe.hpp) takes row and column conditionals with or without the marginal term, 2..14 lags, a path that fits
// the LDS beside the walker's tables; from GH_PIPE_MIN windows on (a window alone runs at one walker's pace, ~2 000 paths/s: below two
// dozen windows the segment-parallel spins on their own streams are faster).  GH_PIPE=0: none.  The windows go in one group per L;
// a window joins its group if its spec and the sweep's 32-bit element offsets allow, a group runs if it has enough windows and a chunk
// at its largest N.  `left` gets the windows no group takes.  A batch (one L) makes at most one group.  Also clears what
// gh_batch_pipe_info reports: the spin that follows sets it.
static std::vector<pipe_group> pipe_groups(gh_batch *b, std::vector<int> &left)
{
    const gh_handle *h0 = b->hs[0];
    const int pipe_env = env_int("GH_PIPE", 1);
    const int pipe_min = env_int("GH_PIPE_MIN", 24);
    const int bwm0 = h0->wmode == WM_SEG ? WM_SPEC : h0->wmode;
    const int es = (int)esize(h0), mt = h0->cfg.marginal_term ? 1 : 0;
    b->pipe_windows = b->pipe_aborted = b->pinfo_nt = b->pinfo_c = 0;
    std::map<int, std::vector<int>> byL;
    for (int w = 0; w < b->n; w++) byL[b->hs[w]->L].push_back(w);
    std::vector<pipe_group> groups;
    for (auto &kv : byL) {
        pipe_group g{kv.first, pipe_threads(kv.first), 0, 0, {}};
        const bool ok = pipe_env && g.nt && pipe_instantiated(g.L, g.nt) && walk_depth2_ok(bwm0, g.L);
        for (int w : kv.second) {
            const gh_handle *h = b->hs[w];
            if (ok && pipe_spec_ok(h) && (unsigned long long)(h->N + 2) * 49ull * (unsigned long long)h->W < (1ull << 31)) {
                g.ws.push_back(w);
                if (h->N > g.N) g.N = h->N;
                if (h->W > g.W) g.W = h->W;
            } else left.push_back(w);
        }
        if (!g.ws.empty() && (int)g.ws.size() >= pipe_min && pipe_chunk(g.N, g.L, pipe_sweep_threads(g.nt), es, mt) > 0) groups.push_back(std::move(g));
        else left.insert(left.end(), g.ws.begin(), g.ws.end());
    }
    return groups;
}

// The window pipeline over the groups' windows: their buffers and descriptors (into wd), one reset, each group's preamble (marginals,
// snapshot, full table) on one of the batch's four streams, one gather of the control words; then per group the narrow launch over
// its ranked windows and the WIDE one over those in which a position offers five candidates (deletion columns), round robin over the
// same streams, and a second gather (into hs).  Which launch takes a window is only known once its marginals stand: hence the one
// host round trip between the two phases (~30 us).  GH_PIPE_WIDE=0: the narrow launches alone.  not_started: the windows no launch
// took (a hole; too many five-candidate positions for the WIDE launch's records; any five-candidate window without the WIDE launch);
// later gets (window, paths done) of those the pipeline stopped at a moved candidate mask: paths 0 .. n_done-1 are complete and
// reweighted, gh_spin takes the rest.  Records the windows carried and handed back, and the threads and chunk of the group with the
// most windows, whose narrow launch gh_batch_profile_* brackets.
static int pipe_spin_groups(gh_batch *b, const std::vector<pipe_group> &groups, int max_paths, double min_remove,
                            const std::vector<int64_t> &off, std::vector<win_desc> &wd, std::vector<dev_state> &hs,
                            std::vector<int> &not_started, std::vector<std::pair<int, int>> &later, spin_phases &phase)
{
    const int n = b->n;
    gh_handle *h0 = b->hs[0];
    const int es = (int)esize(h0), mt = h0->cfg.marginal_term ? 1 : 0;
    const bool wide_env = !env_off("GH_PIPE_WIDE");
    int rc;
    for (int g = 0; g < 3; g++)
        if (!b->gstream[g]) HIPCHK(hipStreamCreateWithFlags(&b->gstream[g], hipStreamNonBlocking));
    const hipStream_t streams[4] = {b->stream, b->gstream[0], b->gstream[1], b->gstream[2]};
    // every pipeline window's descriptor, group by group at d_wd[0 .. np); ord[i] = the window of descriptor i
    std::vector<win_desc> all;
    std::vector<int> ord, gfirst;
    size_t big = 0;
    for (size_t gi = 0; gi < groups.size(); gi++) {
        gfirst.push_back((int)ord.size());
        for (int w : groups[gi].ws) {
            if ((rc = pipe_buffers(b, b->hs[w]))) return rc;
            wd[w] = batch_desc(b, w, max_paths, off);
            all.push_back(wd[w]);
            ord.push_back(w);
        }
        if (groups[gi].ws.size() > groups[big].ws.size()) big = gi;
    }
    const int np = (int)ord.size();
    phase("descriptors");
    HIPCHK(hipMemcpyAsync(b->d_wd, all.data(), sizeof(win_desc) * np, hipMemcpyHostToDevice, b->stream));
    hipLaunchKernelGGL(k_batch_reset, dim3(np), dim3(64), 0, b->stream, (const win_desc *)b->d_wd);
    HIPCHK(hipStreamSynchronize(b->stream));
    for (size_t gi = 0; gi < groups.size(); gi++) {
        const pipe_group &g = groups[gi];
        pipe_preamble(h0, streams[gi % 4], b->d_wd + gfirst[gi], (int)g.ws.size(), g.N, g.W, g.L);
    }
    HIPCHK(hipGetLastError());
    for (int s = 0; s < 4; s++) HIPCHK(hipStreamSynchronize(streams[s]));
    if ((rc = batch_gather_states(b, ord, hs))) return rc;
    // the launches: per group the narrow one and the WIDE one, their descriptor lists at d_wd[n ..], launch k on stream k % 4
    struct plaunch { int gi; bool wide; int off, cnt; };
    std::vector<plaunch> launches;
    std::vector<win_desc> lists;
    std::vector<char> listed(n, 0);
    for (size_t gi = 0; gi < groups.size(); gi++) {
        const pipe_group &g = groups[gi];
        const bool wide_on = wide_env && pipe_wide_instantiated(g.L, g.nt) && !h0->cfg.offer_zero &&
                             pipe_chunk_w(g.N, g.L, pipe_sweep_threads(g.nt), es, mt) > 0;
        std::vector<win_desc> nar, wid;
        for (int w : g.ws) {
            gh_handle *h = b->hs[w];
            const bool live = !hs[w].stop && hs[w].first_hole > h->N;
            if (live && hs[w].ranked != 0 && hs[w].narrow != 0) { nar.push_back(wd[w]); listed[w] = 1; }
            else if (live && hs[w].ranked == 0 && wide_on && h->N < 65536) {
                const size_t need = pipe_gw_bytes(h->N, h->L);
                if (h->pipe_gw_bytes < need) {
                    hipFree(h->pipe_gw); h->pipe_gw = nullptr; h->pipe_gw_bytes = 0;
                    HIPCHK(hipMalloc((void **)&h->pipe_gw, need));
                    h->pipe_gw_bytes = need;
                }
                wd[w].gw = h->pipe_gw;
                wd[w].wdir = reinterpret_cast<int *>(h->pipe_gw + (size_t)PIPE_WMAX * pipe_wrec_doubles(h->L));
                wid.push_back(wd[w]);
                listed[w] = 1;
            }
        }
        if (!nar.empty()) { launches.push_back({(int)gi, false, n + (int)lists.size(), (int)nar.size()}); lists.insert(lists.end(), nar.begin(), nar.end()); }
        if (!wid.empty()) { launches.push_back({(int)gi, true, n + (int)lists.size(), (int)wid.size()}); lists.insert(lists.end(), wid.begin(), wid.end()); }
    }
    if (!lists.empty()) HIPCHK(hipMemcpyAsync(b->d_wd + n, lists.data(), sizeof(win_desc) * lists.size(), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->pused[0] = b->pused[1] = 0;
    auto pmark = [&](hipStream_t st) {            // one event of the start/stop pair around the largest group's narrow launch
        if (b->pused[0] >= b->pev[0].size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            b->pev[0].push_back(e);
        }
        hipEventRecord(b->pev[0][b->pused[0]++], st);
    };
    for (size_t k = 0; k < launches.size(); k++) {
        const plaunch &q = launches[k];
        const pipe_group &g = groups[q.gi];
        const hipStream_t st = streams[k % 4];
        const bool mark = !q.wide && q.gi == (int)big;
        size_t lds = 0;
        pipe_params P = pipe_make_params(h0, g.N, g.W, g.L, g.nt, q.wide, max_paths, min_remove, &lds);
        if (mark) P.prof = (b->prof_every > 0 || getenv("GH_PIPE_STAMPS")) ? 1 : 0;
        if (mark && b->prof_every > 0) { b->prof_windows = q.cnt; pmark(st); }
        const win_desc *gwd = b->d_wd + q.off;
        const hipError_t le = with_storage(h0, [&](auto z) {
            using T = decltype(z);
            return q.wide ? launch_wpipe<T, true>(g.L, g.nt, P, gwd, q.cnt, lds, st) : launch_wpipe<T, false>(g.L, g.nt, P, gwd, q.cnt, lds, st);
        });
        if (le != hipSuccess)
            return fail(GH_ERR_HIP, "%s: the %s pipeline launch failed (L=%d, %d threads, %zu bytes of LDS): %s", phase.who, q.wide ? "wide" : "narrow",
                        g.L, g.nt, lds, hipGetErrorString(le));
        if (mark && b->prof_every > 0) pmark(st);
        if (mark) {
            // algorithmic bytes per window over the whole launch, the pipeline's own accounting: per position
            // and path the walk reads its compact table (4 rows x L lags x 32 bytes) and the bookkeeper the counts, the original
            // log-marginals and the packed word (64 + 48 + 8) and writes a path byte; the sweep reads the W rows of the path's symbol
            // (7 elements each), the counts and two packed words, writes W cells, two counts and min(L, W) x 32 bytes of table
            const int Lw = (h0->cfg.cond_mode == GH_COND_B || g.W >= g.L) ? g.L : g.W;
            const double ext = (double)g.N * (128.0 * g.L + 64 + 48 + 8 + 1);
            const double rw = (double)(g.N + 1) * (7.0 * es * g.W + es * g.W + 64 + 16 + 16 + 32.0 * Lw + 1);
            b->prof_bytes[0] = (ext + rw) * max_paths;
            b->prof_bytes[1] = 0.0;
        }
    }
    for (int s = 0; s < 4; s++) HIPCHK(hipStreamSynchronize(streams[s]));
    phase("preamble + pipeline kernel");
    if ((rc = batch_gather_states(b, ord, hs))) return rc;
    phase("states to host");
    for (int w : ord) {
        if (!listed[w]) hs[w].pipe_status = PIPE_NOT_STARTED;
        if (hs[w].pipe_status == PIPE_NOT_STARTED) not_started.push_back(w);
        else if (hs[w].pipe_status == PIPE_ABORTED) { later.emplace_back(w, hs[w].n_done); b->pipe_aborted++; }
        else if (hs[w].pipe_status != PIPE_DONE) return fail(GH_ERR_STATE, "%s: window %d left the pipeline in state %d", phase.who, w, hs[w].pipe_status);
    }
    b->pipe_windows = np - (int)not_started.size();
    b->pinfo_nt = groups[big].nt;
    b->pinfo_c = pipe_chunk(groups[big].N, groups[big].L, pipe_sweep_threads(groups[big].nt), es, mt);
    if (getenv("GH_PIPE_STAMPS")) {         // 100 MHz ticks per path as the bookkeepers of a few windows saw them
        for (int i = 0; i < np; i += (np > 4 ? np / 4 : 1)) {
            const int w = ord[i];
#ifdef PIPE_PROF
            fprintf(stderr, "pipe window %d, Mcycles (work, own memory, barrier): sweeper %.2f %.2f %.2f  loader %.2f %.2f %.2f  bookkeeper %.2f %.2f %.2f\n", w,
                    hs[w].dbg8[0] / 1e6, hs[w].dbg8[1] / 1e6, hs[w].dbg8[2] / 1e6, hs[w].dbg8[3] / 1e6, hs[w].dbg8[4] / 1e6, hs[w].dbg8[5] / 1e6,
                    hs[w].dbg8[6] / 1e6, hs[w].dbg8[7] / 1e6, hs[w].dbg8[8] / 1e6);
            fprintf(stderr, "walker: %.2f Mcycles walking, %.2f at its barriers; bookkeeper: %.2f per-position part, %.2f sequential sums\n", hs[w].dbg8[10] / 1e6, hs[w].dbg8[11] / 1e6, hs[w].dbg[0] / 1e6, hs[w].dbg[1] / 1e6);
            fprintf(stderr, "wide walker: %.2f Mcycles in %llu groups by the exact stepper, %.2f Mcycles inside the speculative blocks, %llu primes\n", (double)(hs[w].dbg[2] & ((1ull << 40) - 1)) / 1e6,
                    (unsigned long long)(hs[w].dbg[2] >> 40), (double)(hs[w].dbg[3] & ((1ull << 40) - 1)) / 1e6, (unsigned long long)(hs[w].dbg[3] >> 40));
            fprintf(stderr, "SIMD of waves 0..15:");
            for (int q = 0; q < 16; q++) fprintf(stderr, " %d", (int)((hs[w].dbg8[9] >> (2 * q)) & 3));
            fprintf(stderr, "\n");
            break;
#else
            fprintf(stderr, "pipe window %d, us per path:", w);
            for (int q = 0; q < 12 && q < max_paths; q++) fprintf(stderr, " %.1f", (double)hs[w].dbg8[q] / 100.0);
            fprintf(stderr, "\n");
#endif
        }
    }
    return GH_OK;
}

// what the device computed for the windows ws (ascending) to the caller: paths in runs of windows that lie back to back on both sides,
// records [n][max_paths]; then each window's outcome and flags -- its tensor has changed, marginals and table are rebuilt from it on
// next use, the to-major band stays in step where the pipeline's sweep wrote both
static int batch_finish(gh_batch *b, const std::vector<int> &ws, const std::vector<dev_state> &hs, int max_paths, const std::vector<int64_t> &off,
                        uint8_t *paths_out, const int64_t *paths_off, gh_path_rec *recs, int *n_out, int *hole_at)
{
    for (size_t i = 0; i < ws.size();) {
        const int w = ws[i];
        size_t j = i + 1;
        while (j < ws.size() && ws[j] == ws[j - 1] + 1 && paths_off[ws[j]] - paths_off[w] == off[ws[j]] - off[w]) j++;
        const int e = ws[j - 1] + 1;
        HIPCHK(hipMemcpyAsync(paths_out + paths_off[w], b->d_paths + off[w], (size_t)(off[e] - off[w]), hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipMemcpyAsync(recs + (size_t)max_paths * w, b->d_recs + (size_t)max_paths * w, sizeof(gh_path_rec) * (size_t)max_paths * (e - w),
                              hipMemcpyDeviceToHost, b->stream));
        i = j;
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    for (int w : ws) {
        gh_handle *h = b->hs[w];
        n_out[w] = hs[w].n_done;
        hole_at[w] = hs[w].stop ? hs[w].hole_at : 0;
        const bool kept = tband_current(h) &&
                          (hs[w].pipe_status == PIPE_DONE || hs[w].pipe_status == PIPE_ABORTED) &&
                          (h->cfg.cond_mode == GH_COND_C || h->cfg.cond_mode == GH_COND_E);
        h->dirty_marg = h->dirty_lt = true; h->band_epoch++;
        if (kept) h->tband_epoch = h->band_epoch;       // (the pipeline's sweep wrote both)
        h->lt_inc_path = nullptr;       // the batch reweighted many paths and maintains no walker tables: rebuild in full
    }
    return GH_OK;
}

extern "C" int gh_batch_spin(gh_batch_t *b, int max_paths, double min_remove, uint8_t *paths_out,
                             gh_path_rec *recs, int *n_out, int *hole_at)
{
    if (!b || !paths_out || !recs || !n_out || !hole_at || max_paths < 1) return fail(GH_ERR_ARG, "bad argument");
    if (b->panel) return fail(GH_ERR_ARG, "gh_batch_spin: this is a panel (gh_panel_create): spin it with gh_panel_spin");
    HIPCHK(hipSetDevice(b->dev));
    spin_phases phase("gh_batch_spin");
    const int n = b->n;
    int rc;
    for (int w = 0; w < n; w++)
        if (b->hs[w]->L != b->hs[0]->L)
            return fail(GH_ERR_STATE, "window %d has L=%d but window 0 has L=%d: set one L (gh_set_L) for the batch", w, b->hs[w]->L, b->hs[0]->L);
    if ((rc = batch_spin_begin(b))) return rc;
    b->L = b->hs[0]->L;
    phase("tables allocated, device idle");
    // (measured on C3, MI355X: 8 windows 37k haplotypes/s this way against ~16k batched; 32 windows 45k either way -- the
    // chip is then busy with k_seg; from 48 windows on the batched serial walkers, one workgroup per window, win: 114k at 256)
    // (read on every call: the tests switch between the two ways; -1 = always the batched kernels)
    const int batch_cut = env_int("GH_BATCH_STREAMS_MAX", 47);
    const bool seg = seg_ok(b->hs[0]->wmode, b->L), cw = cw_ok(b->hs[0]->wmode, b->L);
    std::vector<int> rest;                      // windows no pipeline group takes, then those it leaves PIPE_NOT_STARTED
    const std::vector<pipe_group> groups = pipe_groups(b, rest);
    const std::vector<int64_t> off = batch_path_offsets(b, max_paths);
    std::vector<std::pair<int, int>> later;     // (window, paths done): windows gh_spin finishes on their own streams behind the batch's copy
    if (groups.empty() && batch_cut >= 0 && ((seg && n <= batch_cut) || cw)) {
        // The segment-parallel extensions fill the chip poorly with ONE window (four small dependent kernels per path, most
        // of their time launch and first-touch latency) but every window has its own stream: a few host threads each
        // run gh_spin over their share of the windows, and the windows' kernel chains interleave on the GPU.
        for (int w = 0; w < n; w++) later.emplace_back(w, 0);
        return batch_spin_on_streams(b, later, max_paths, min_remove, paths_out, off.data(), recs, n_out, hole_at);
    }
    if ((rc = batch_buffers(b, max_paths, off))) return rc;
    std::vector<win_desc> wd(n);
    std::vector<dev_state> hs(n);
    if (!groups.empty()) {
        std::vector<int> not_started;
        if ((rc = pipe_spin_groups(b, groups, max_paths, min_remove, off, wd, hs, not_started, later, phase))) return rc;
        rest.insert(rest.end(), not_started.begin(), not_started.end());
        // What the pipeline left (a hole; too many five-candidate positions for the WIDE launch's records; every five-candidate
        // window under GH_PIPE_WIDE=0).  A FEW such windows go the single window's way, each on its own stream from a few host
        // threads -- the segment-parallel / candidate-pool spins (mixed radix at five lags): 25-37k haplotypes/s where the batched
        // serial walkers, one wavefront per window, give 16k for eight windows; from four dozen on the batched launches over all of them.
        if (!rest.empty() && batch_cut >= 0 && (int)rest.size() <= batch_cut && (seg || cw)) {
            for (int w : rest) later.emplace_back(w, 0);
            rest.clear();
        }
    }
    if (!rest.empty()) {
        std::sort(rest.begin(), rest.end());
        std::vector<win_desc> rd;
        for (int w : rest) {
            if (!wd[w].st) wd[w] = batch_desc(b, w, max_paths, off);       // (not one of the pipeline's windows)
            rd.push_back(wd[w]);
        }
        if ((rc = batch_run_launches(b, rd, max_paths, min_remove))) return rc;
        if ((rc = batch_gather_states(b, rest, hs))) return rc;
    }
    std::vector<int> every(n);
    for (int w = 0; w < n; w++) every[w] = w;
    if ((rc = batch_finish(b, every, hs, max_paths, off, paths_out, off.data(), recs, n_out, hole_at))) return rc;
    phase("paths and records to host");
    // In a deep spin many windows stop once counts reach zero: they, and the few the pipeline did not take, are finished side by
    // side (one after the other on the calling thread they were the tail of the batch)
    return batch_spin_on_streams(b, later, max_paths, min_remove, paths_out, off.data(), recs, n_out, hole_at);
}

// ---- panels: windows of differing N, W and L (gh_panel_*) ----------------------------------------------------------------------
// The window pipeline carries every group it can (pipe_groups, pipe_spin_groups); every kernel takes its window's own N and W from
// the descriptor.  What no group carries (a group too small, a lag count beyond the pipeline, a hole, too many five-candidate
// positions, the remaining paths of an aborted window) is finished by gh_spin window by window on its own stream.
extern "C" int gh_panel_spin(gh_batch_t *b, int max_paths, double min_remove, uint8_t *paths_out, const int64_t *paths_off,
                             gh_path_rec *recs, int *n_out, int *hole_at)
{
    if (!b || !paths_out || !paths_off || !recs || !n_out || !hole_at || max_paths < 1) return fail(GH_ERR_ARG, "bad argument");
    if (!b->panel) return fail(GH_ERR_ARG, "gh_panel_spin: not a panel (gh_panel_create)");
    HIPCHK(hipSetDevice(b->dev));
    spin_phases phase("gh_panel_spin");
    const int n = b->n;
    int rc;
    for (int w = 0; w < n; w++)
        if (paths_off[w] < 0) return fail(GH_ERR_ARG, "gh_panel_spin: window %d has a negative path offset", w);
    if ((rc = batch_spin_begin(b))) return rc;
    std::vector<int> left;
    const std::vector<pipe_group> groups = pipe_groups(b, left);
    std::vector<std::pair<int, int>> later;     // (window, paths done): gh_spin finishes them
    for (int w : left) later.emplace_back(w, 0);
    if (!groups.empty()) {
        const std::vector<int64_t> off = batch_path_offsets(b, max_paths);
        if ((rc = batch_buffers(b, max_paths, off))) return rc;
        std::vector<win_desc> wd(n);
        std::vector<dev_state> hs(n);
        std::vector<int> not_started, ws;
        if ((rc = pipe_spin_groups(b, groups, max_paths, min_remove, off, wd, hs, not_started, later, phase))) return rc;
        for (int w : not_started) later.emplace_back(w, 0);
        for (const pipe_group &g : groups) ws.insert(ws.end(), g.ws.begin(), g.ws.end());
        std::sort(ws.begin(), ws.end());
        if ((rc = batch_finish(b, ws, hs, max_paths, off, paths_out, paths_off, recs, n_out, hole_at))) return rc;
        phase("paths and records to host");
    }
    return batch_spin_on_streams(b, later, max_paths, min_remove, paths_out, paths_off, recs, n_out, hole_at);
}

extern "C" int gh_host_alloc(size_t bytes, void **out)
{
    if (!out || bytes == 0) return fail(GH_ERR_ARG, "bad argument");
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return fail(GH_ERR_NOMEM, "hipHostMalloc of %zu bytes failed", bytes); }
    *out = p;
    return GH_OK;
}
extern "C" int gh_host_free(void *p)
{
    if (p && hipHostFree(p) != hipSuccess) return fail(GH_ERR_HIP, "hipHostFree failed");
    return GH_OK;
}

extern "C" int gh_batch_pipe_info(gh_batch_t *b, int32_t out[4])
{
    if (!b || !out) return fail(GH_ERR_ARG, "bad argument");
    out[0] = b->pipe_windows; out[1] = b->pipe_aborted;
    out[2] = b->pipe_windows ? b->pinfo_nt : 0;
    out[3] = b->pipe_windows ? b->pinfo_c : 0;
    return GH_OK;
}

extern "C" int gh_batch_profile_enable(gh_batch_t *b, int every)
{
    if (!b) return fail(GH_ERR_ARG, "null batch");
    b->prof_every = every > 0 ? every : 0;
    return GH_OK;
}

extern "C" int gh_batch_profile_get(gh_batch_t *b, int kernel, double *total_ms, int64_t *launches, int32_t *windows, double *bytes_per_launch)
{
    if (!b || (kernel != GH_K_WALK && kernel != GH_K_REWEIGHT)) return fail(GH_ERR_ARG, "bad argument");
    const int k = kernel == GH_K_WALK ? 0 : 1;
    double ms = 0.0;
    int64_t n = 0;
    for (size_t q = 0; q + 1 < b->pused[k]; q += 2) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, b->pev[k][q], b->pev[k][q + 1]) == hipSuccess) { ms += t; n++; }
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = n;
    if (windows) *windows = b->prof_windows;
    if (bytes_per_launch) *bytes_per_launch = b->prof_bytes[k] * b->prof_windows;
    return GH_OK;
}

// export / import -----------------------------------------------------------------------------
extern "C" int gh_export_band(gh_t *h, double *out)
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    if (set_dev(h)) return GH_ERR_HIP;
    const size_t n = h->n_cells * CELL;
    double *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, n * sizeof(double)));
    const unsigned nb = (unsigned)((n + 255) / 256);
    with_storage(h, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(k_export<T>, dim3(nb), dim3(256), 0, h->stream, (const T *)h->band, d, n, h->W);
    });
    hipError_t e = hipMemcpyAsync(out, d, n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    hipFree(d);
    if (e != hipSuccess) return fail(GH_ERR_HIP, "export failed: %s", hipGetErrorString(e));
    return GH_OK;
}

extern "C" int gh_import_band(gh_t *h, const double *in)
{
    if (!h || !in) return fail(GH_ERR_ARG, "null argument");
    if (set_dev(h)) return GH_ERR_HIP;
    const size_t n = h->n_cells * CELL;
    double *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, n * sizeof(double)));
    hipError_t e = hipMemcpyAsync(d, in, n * sizeof(double), hipMemcpyHostToDevice, h->stream);
    const unsigned nb = (unsigned)((n + 255) / 256);
    with_storage(h, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(k_import<T>, dim3(nb), dim3(256), 0, h->stream, (T *)h->band, d, n, h->W);
    });
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    hipFree(d);
    h->dirty_marg = h->dirty_lt = true; h->lt_inc_path = nullptr; h->band_zero = false; h->band_epoch++;
    if (e != hipSuccess) return fail(GH_ERR_HIP, "import failed: %s", hipGetErrorString(e));
    return GH_OK;
}

extern "C" int gh_export_dense(gh_t *h, double *out)
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    const size_t np = (size_t)h->N + 2;
    std::vector<double> band(h->n_cells * CELL);
    int rc = gh_export_band(h, band.data());
    if (rc) return rc;
    memset(out, 0, sizeof(double) * NSYM * NSYM * np * np);
    for (size_t i = 0; i < np; i++)
        for (int d = 1; d <= h->W; d++) {
            size_t j = i + d;
            if (j >= np) break;
            const double *cell = band.data() + (i * h->W + (d - 1)) * CELL;
            for (int a = 0; a < NSYM; a++)
                for (int b = 0; b < NSYM; b++)
                    out[(((size_t)a * NSYM + b) * np + i) * np + j] = cell[a * NSYM + b];
        }
    return GH_OK;
}

// gretel-snpper -------------------------------------------------------------------------------
extern "C" int gh_coverage_sites(int device, const int32_t *ref_start, const int64_t *off, const uint8_t *codes, int64_t n_runs,
                                 int32_t start0, int32_t len, int32_t depth, int32_t *counts_out, uint8_t *site_out)
{
    if (n_runs < 0 || len < 0 || !site_out || (n_runs > 0 && (!ref_start || !off || !codes))) return fail(GH_ERR_ARG, "bad argument");
    if (len == 0) return GH_OK;
    if (device >= 0) HIPCHK(hipSetDevice(device));
    const int64_t n_bases = n_runs ? off[n_runs] : 0;
    int32_t *d_ref = nullptr;
    int64_t *d_off = nullptr;
    uint8_t *d_codes = nullptr, *d_site = nullptr;
    unsigned *d_counts = nullptr;
    hipError_t e = hipMalloc((void **)&d_counts, sizeof(unsigned) * 4 * (size_t)len);
    if (e == hipSuccess) e = hipMalloc((void **)&d_site, (size_t)len);
    if (e == hipSuccess) e = hipMalloc((void **)&d_ref, sizeof(int32_t) * (size_t)(n_runs ? n_runs : 1));
    if (e == hipSuccess) e = hipMalloc((void **)&d_off, sizeof(int64_t) * (size_t)(n_runs + 1));
    if (e == hipSuccess) e = hipMalloc((void **)&d_codes, (size_t)(n_bases ? n_bases : 1));
    if (e == hipSuccess) e = hipMemset(d_counts, 0, sizeof(unsigned) * 4 * (size_t)len);
    if (e == hipSuccess && n_runs) {
        e = hipMemcpy(d_ref, ref_start, sizeof(int32_t) * (size_t)n_runs, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_off, off, sizeof(int64_t) * (size_t)(n_runs + 1), hipMemcpyHostToDevice);
        if (e == hipSuccess && n_bases) e = hipMemcpy(d_codes, codes, (size_t)n_bases, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        if (n_runs) {
            int64_t nb = (n_runs + 3) / 4;                  // one wavefront per run, four per workgroup
            if (nb > 256 * 16) nb = 256 * 16;
            hipLaunchKernelGGL(k_cov, dim3((unsigned)nb), dim3(256), 0, 0, d_ref, d_off, d_codes, n_runs, start0, len, d_counts);
        }
        hipLaunchKernelGGL(k_sites, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, 0, d_counts, len, depth, d_site);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(site_out, d_site, (size_t)len, hipMemcpyDeviceToHost);
    if (e == hipSuccess && counts_out) e = hipMemcpy(counts_out, d_counts, sizeof(unsigned) * 4 * (size_t)len, hipMemcpyDeviceToHost);
    hipFree(d_counts); hipFree(d_site); hipFree(d_ref); hipFree(d_off); hipFree(d_codes);
    if (e != hipSuccess) return fail(GH_ERR_HIP, "gh_coverage_sites failed: %s", hipGetErrorString(e));
    return GH_OK;
}

// profiling -----------------------------------------------------------------------------------
extern "C" int gh_profile_enable(gh_t *h, int on)
{
    if (!h) return fail(GH_ERR_ARG, "null handle");
    h->prof = on > 0 ? on : 0;
    for (int k = 0; k < GH_K_COUNT; k++) { h->ps[k].seq = 0; h->ps[k].open = false; }
    return GH_OK;
}

extern "C" int gh_profile_reset(gh_t *h)
{
    if (!h) return fail(GH_ERR_ARG, "null handle");
    if (set_dev(h)) return GH_ERR_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int k = 0; k < GH_K_COUNT; k++) {
        h->ps[k].used = 0; h->ps[k].ms = 0.0; h->ps[k].launches = 0;
    }
    return GH_OK;
}

extern "C" int gh_profile_get(gh_t *h, int kernel, double *total_ms, int64_t *launches)
{
    if (!h || kernel < 0 || kernel >= GH_K_COUNT) return fail(GH_ERR_ARG, "bad argument");
    if (set_dev(h)) return GH_ERR_HIP;
    HIPCHK(hipStreamSynchronize(h->stream));
    prof_collect(h);
    if (total_ms) *total_ms = h->ps[kernel].ms;
    if (launches) *launches = h->ps[kernel].launches;
    return GH_OK;
}

__global__ void k_nop() {}

// What a HIP-event bracket reads beyond the kernel inside it, on this handle's stream: out[0] = two events with nothing
// between them, out[1] = the same around an empty one-workgroup kernel (ms, medians of `reps`).  bench.py reports them
// next to the bracketed kernel times: for kernels of 5-15 us the bracket itself is a fifth of the reading.
extern "C" int gh_profile_overhead(gh_t *h, int reps, double out[2])
{
    if (!h || !out || reps < 1) return fail(GH_ERR_ARG, "bad argument");
    if (set_dev(h)) return GH_ERR_HIP;
    std::vector<float> a, b;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); return fail(GH_ERR_HIP, "hipEventCreate failed"); }
    for (int pass = 0; pass < 2; pass++)
        for (int r = 0; r < reps; r++) {
            // a kernel in front, as in the timed region (the stream is never idle there)
            hipLaunchKernelGGL(k_nop, dim3(256), dim3(256), 0, h->stream);
            hipEventRecord(e0, h->stream);
            if (pass == 1) hipLaunchKernelGGL(k_nop, dim3(1), dim3(64), 0, h->stream);
            hipEventRecord(e1, h->stream);
            hipLaunchKernelGGL(k_nop, dim3(256), dim3(256), 0, h->stream);
            if (hipStreamSynchronize(h->stream) != hipSuccess) {
                hipEventDestroy(e0); hipEventDestroy(e1);
                return fail(GH_ERR_HIP, "gh_profile_overhead: hipStreamSynchronize failed");
            }
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) (pass ? b : a).push_back(ms);
        }
    hipEventDestroy(e0); hipEventDestroy(e1);
    auto med = [](std::vector<float> &v) { if (v.empty()) return 0.0; std::sort(v.begin(), v.end()); return (double)v[v.size() / 2]; };
    out[0] = med(a);
    out[1] = med(b);
    return GH_OK;
}

extern "C" int gh_debug_pool_geometry(int32_t n_snps, int32_t L, int32_t five, int64_t out[6])
{
    if (!out || n_snps < 1 || L < CW_MIN_L || L > CW_MAX_LG) return fail(GH_ERR_ARG, "pool geometry: n_snps >= 1, %d <= L <= %d", CW_MIN_L, CW_MAX_LG);
    const int R = five ? 5 : 4;
    const cw_geom g = cw_geometry(n_snps, L);
    const bool packed = five ? L <= CW_MAX_L5 : L <= CW_MAX_L;
    out[0] = g.S; out[1] = g.seglen;
    out[2] = packed ? cw_chunk(L, R) : cwg_chunk(L, R);
    out[3] = (int64_t)(packed ? cw_lds_bytes(L, R) : cwg_lds_bytes(L, R));
    out[4] = packed ? 1 : 0;
    out[5] = CW_K * cw_lanes(R);
    return GH_OK;
}

extern "C" int gh_debug_walk_clock(gh_t *h, uint64_t out[4])
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    if (set_dev(h)) return GH_ERR_HIP;
    dev_state hs;
    int rc = read_state(h, &hs);
    if (rc) return rc;
    out[0] = hs.dbg[0]; out[1] = hs.dbg[1]; out[2] = hs.dbg[2]; out[3] = hs.dbg[3];
    if (out[3] == 3) {
        // out[1]: the state space the extension walked -- 4 ranks, 5 symbols, 6 mixed radix (seg_class, from the same control words);
        // out[2]: the most states entering a target as k_classify found them (0: not taken)
        out[0] = (uint64_t)h->spin_requeues;
        out[1] = hs.ranked ? 4u : ((h->L == SEGM_L && hs.maxstates > 0 && hs.maxstates <= SEGM_NS) ? (uint64_t)SEG_CLS_MIXED : 5u);
        out[2] = (uint64_t)hs.maxstates;
    }
    if (out[3] == 4) { out[0] = (uint64_t)h->spin_requeues; out[1] = (uint64_t)h->cw_stat[1]; out[2] = (uint64_t)h->cw_stat[2]; }
    if (getenv("GH_PRINT_STAMPS"))      // diagnostic builds (-DSEG_STAMPS / -DGH_STAMPS)
    {
        fprintf(stderr, "stamps:");
        for (int q = 1; q < 12 && hs.dbg8[q] >= hs.dbg8[q - 1] && hs.dbg8[q - 1]; q++) fprintf(stderr, " %llu", hs.dbg8[q] - hs.dbg8[q - 1]);
        fprintf(stderr, "\n");
    }
    return GH_OK;
}

// diagnostic builds (-DRWS_STAMPS_ALL): the stamps every k_rwseg workgroup of the last launch left, 16 doubles per workgroup
extern "C" int gh_debug_segment_stamps(gh_t *h, double *out, int n_workgroups)
{
    if (!h || !out || n_workgroups < 1) return fail(GH_ERR_ARG, "bad argument");
    if (set_dev(h)) return GH_ERR_HIP;
#if !defined(RWS_STAMPS_ALL)
    return fail(GH_ERR_STATE, "gh_debug_segment_stamps: this library was not built with -DRWS_STAMPS_ALL (there are no stamps to read)");
#else
    if (!h->seg_smin) return fail(GH_ERR_STATE, "no segment-parallel walk has run on this handle");
    if ((size_t)n_workgroups * 16 * sizeof(double) > h->seg_smin_bytes)
        return fail(GH_ERR_ARG, "gh_debug_segment_stamps: %d workgroups asked for, the buffer holds %zu", n_workgroups, h->seg_smin_bytes / (16 * sizeof(double)));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->seg_smin, (size_t)n_workgroups * 16 * sizeof(double), hipMemcpyDeviceToHost));
    return GH_OK;
#endif
}

extern "C" int gh_profile_bytes(gh_t *h, int kernel, double *bytes_per_launch)
{
    if (!h || !bytes_per_launch || kernel < 0 || kernel >= GH_K_COUNT) return fail(GH_ERR_ARG, "bad argument");
    *bytes_per_launch = h->ps[kernel].bytes;
    return GH_OK;
}

// path rows a caller hands in ([n_paths][n1] symbol indices): the first cell that is none, reported under `code`
static int check_symbol_rows(const uint8_t *paths, int n_paths, size_t n1, int code)
{
    const size_t path_bytes = (size_t)n_paths * n1;
    uint8_t top = 0;
    for (size_t q = 0; q < path_bytes; q++) top = std::max(top, paths[q]);
    if (top > 6)
        for (size_t q = 0; q < path_bytes; q++)
            if (paths[q] > 6) return fail(code, "path %d holds %d at SNP %d: not a symbol index", (int)(q / n1), paths[q], (int)(q % n1));
    return GH_OK;
}

// read assignment (gh_assign_reads) -----------------------------------------------------------
#include "assign.hpp"
// scoring given haplotypes (gh_score_paths) ---------------------------------------------------
#include "score.hpp"
// the chain table and the recovery loop the two decoders below share -----------------------------------
#include "chain_table.hpp"
// beam search over the chain likelihood (gh_beam_paths, gh_beam_spin, gh_beam_info) ------------------
#include "beam.hpp"
// exact decoding of the chain likelihood (gh_viterbi_path, gh_viterbi_spin, gh_viterbi_info) -----------
#include "viterbi.hpp"
// max-marginals of the chain likelihood: the decoder's forward walk with its scores kept, a backward walk, a parallel reduction
#include "viterbi_marg.hpp"
// k-best exact decoding: a ranked list of prefixes per state, merged by counting (gh_viterbi_kbest)
#include "viterbi_kbest.hpp"
// ... over every window of a batch or panel, the decoders of a round side by side: gh_panel_viterbi_spin, gh_viterbi_states
#include "viterbi_panel.hpp"
// ... and the max-marginals over every window: gh_panel_viterbi_marginals
#include "viterbi_marg_panel.hpp"
// ... and the k best haplotypes of every window: gh_panel_viterbi_kbest
#include "viterbi_kbest_panel.hpp"
// exact decoding under per-position allele masks, many constraint sets over one table: gh_viterbi_path_masked (the walk's body is
// viterbi_panel.hpp's, hence behind it)
#include "viterbi_masked.hpp"
// exact decoding beyond the states two LDS rows hold: the score rows in global memory, one launch per position (gh_viterbi_path_grid,
// gh_viterbi_spin_grid, gh_viterbi_grid_info)
#include "viterbi_grid.hpp"
// ... and the max-marginals there: the step with every row kept, a backward step per position, the maxima per workgroup as it goes
// (gh_viterbi_marginals_grid)
#include "viterbi_grid_marg.hpp"
