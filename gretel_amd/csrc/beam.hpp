// beam.hpp -- beam search over the chain likelihood (gh_beam_paths, gh_beam_spin, gh_beam_info: include/gretel_hip.h, where the
// definition stands; INTEGRATION.md "Beam search").  Width B hypotheses walk the window together; every score is a sequential
// binary64 sum in ascending p and every weight k_score_pos' additions in k_score_pos' order, so what comes out is what
// gh_score_paths says of the same paths bit for bit, and B = 1 is gh_generate_path.  The tensor is only read.
//
//   k_beam_table  (parallel) the beam's own plain table in its own scratch block, never the handle's G (which may be ranked, may
//                 carry the marginal term, may be mid-way through an incremental refresh):  per source position i one block of
//                 30 L + 6 doubles,  Gb[i][a6][l-1][b5] = lt_entry(bake_lm = 0)  and behind them what target i + 1 needs besides:
//                 its five log10 marginals (minfo[i+1][0..4]) and its candidate bits (minfo[i+1][10]).  With that header the
//                 walk's whole input is ONE contiguous stream in source order.  (The issue's sketch had the bare 30 L doubles
//                 and LT_PAD zero blocks behind N: the header saves the walk a second stream, and no reader overruns N sources.)
//   k_beam_walk   one workgroup, N dependent steps.  Eight lanes per hypothesis, lane s < 5 = candidate b5 = s (k_score_pos'
//                 grouping): a child lane sums its weight, adds it to its parent's score, puts the key (score, w) into LDS;
//                 behind a barrier it counts the children that precede it in the total order (score desc, parent rank asc, w
//                 desc, candidate index asc: plain > and ==), and where that rank is below B it IS the new hypothesis of that
//                 rank: it writes the score, the back-pointer byte (parent | b5 << 5, a plain byte store) and copies its
//                 parent's ring of the last L symbols into the other ring buffer with its own symbol added.  Two barriers a
//                 step, over LDS only (beam_barrier).  Histories never leave LDS; nothing is chased through back-pointers during the walk.
//                 STAGED: the stream goes through a ring of R source blocks in LDS, one block per step, A = R - L - 1 steps
//                 ahead of its first reader -- every thread loads its 16-byte pieces of block p + A - 1 into registers in step
//                 p and stores them to LDS in step p + 1, so the load has a whole step to land and a step reads LDS only.
//                 (The sketch had two buffers of chunk + L sources; a ring needs L + 1 blocks beside the run-ahead instead
//                 of 2 L and loads every block once, not 1 + L / chunk times: at L = 16 that is 23 steps ahead in place of 4.)
//                 Otherwise the same body reads the blocks from global memory: same additions, same order.
//   k_beam_trace  one lane per surviving hypothesis follows the back-pointers from the end down to 1 (they pass through LDS 1024
//                 positions at a time, so the chain is LDS reads) and writes the path rows.
// ---------------------------------------------------------------------------------------------

#define BEAM_KEYS (GH_BEAM_MAX * 5)
#define BEAM_LDS_MAX (160 * 1024)  /* LDS one workgroup can have on gfx950 */
#define BEAM_AHEAD_MIN 16          /* staged only where the loader can run this many steps ahead: a step is a few LDS round trips and
                                      two barriers, a block from HBM a few of those -- 16 leaves it room under load */
#define BEAM_AHEAD_MAX 64          /* ... and never more: nothing is gained, and a short window would be preloaded whole */
#define BEAM_LOAD_UNITS 5          /* 16-byte pieces of a block one thread of the smallest workgroup (64) carries from step to step */
#define BEAM_MAX_L 2048            /* the two ring buffers of 32 hypotheses stay within the LDS */
#define BEAM_TRACE_POS 1024

__host__ __device__ constexpr int beam_src_doubles(int L) { return 30 * L + 6; }
__host__ __device__ constexpr int beam_ring_bytes(int L) { return (L + 3) & ~3; }             // one hypothesis' ring, whole words
// keys, two score rows, two ring buffers
__host__ __device__ constexpr size_t beam_fixed_lds(int L) { return (size_t)BEAM_KEYS * 16 + 2 * GH_BEAM_MAX * 8 + 2 * (size_t)GH_BEAM_MAX * beam_ring_bytes(L); }
// source blocks of the LDS ring for lag count L; 0 = the slice does not fit with BEAM_AHEAD_MIN steps of run-ahead (L >= 19)
__host__ __device__ constexpr int beam_ring_sources(int L)
{
    if (beam_fixed_lds(L) >= BEAM_LDS_MAX || beam_src_doubles(L) / 2 > BEAM_LOAD_UNITS * 64) return 0;
    int r = (int)((BEAM_LDS_MAX - beam_fixed_lds(L)) / ((size_t)beam_src_doubles(L) * 8));
    if (r > BEAM_AHEAD_MAX + L + 1) r = BEAM_AHEAD_MAX + L + 1;
    return r - L - 1 >= BEAM_AHEAD_MIN ? r : 0;
}
static_assert(beam_ring_sources(3) == 68 && beam_ring_sources(16) >= 16 + 17 && beam_ring_sources(20) == 0, "the staged path covers L <= 16");
static_assert(beam_fixed_lds(BEAM_MAX_L) < BEAM_LDS_MAX, "the rings of the longest history fit");

struct beam_out {
    int n_out, hole_at;
    int end, rows;     // what k_beam_trace follows: `rows` hypotheses from position `end` down
};

template <typename T>
__global__ void __launch_bounds__(256)
k_beam_table(const T *__restrict__ band, const T *__restrict__ tband, int N, int W, int L, int cond_mode,
             const double *__restrict__ cnt, const int32_t *__restrict__ nvalid, const uint32_t *__restrict__ cmask,
             const double *__restrict__ minfo, symmap sm, double *__restrict__ Gb)
{
    const int sd = beam_src_doubles(L);
    const size_t total = (size_t)N * sd, gsize = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gsize) {
        const int i = (int)(t / sd), q = (int)(t % sd);
        double v;
        if (q < 30 * L) {
            const int b5 = q % LT_ROW, r = q / LT_ROW;
            v = lt_entry(band, N, W, cond_mode, 0, cnt, nvalid, cmask, minfo, i, r / L, r % L + 1, b5, sm, tband);
        } else {
            const int hq = q - 30 * L;                       // target i + 1 <= N: its log10 marginals, then its candidate bits
            v = minfo[(size_t)(i + 1) * MINFO + (hq < 5 ? hq : 10)];
        }
        Gb[t] = v;
    }
}

// The walk's barrier orders LDS only: __syncthreads() also waits for every global access in flight (vmcnt(0)), which would drain
// the loader's block and the step's back-pointer store twice a step.  Nothing k_beam_walk writes to global memory is read inside
// it, and what it reads there nobody writes, so the workgroup needs no order on global memory.  (Measured, DESIGN.md 4.9: by
// itself this did not move the time of a step -- the loader's own wait for its block still stands behind the back-pointer store.)
__device__ __forceinline__ void beam_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// B hypotheses, 8 lanes each (at least one wavefront); dynamic LDS: [R blocks (STAGED)] [keys] [scores 2 x 32] [rings 2 x 32 x Lr]
template <bool STAGED>
__global__ void __launch_bounds__(256)
k_beam_walk(const double *__restrict__ Gb, int N, int L, int B, int marginal_term, int R,
            uint8_t *__restrict__ bp, int bps, double *__restrict__ ll, beam_out *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char beam_smem[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int sd = beam_src_doubles(L), su = sd / 2, Lr = beam_ring_bytes(L);
    const size_t tab_bytes = STAGED ? (size_t)R * sd * 8 : 0;
    double *tab = reinterpret_cast<double *>(beam_smem);
    double2 *tab2 = reinterpret_cast<double2 *>(beam_smem);
    double2 *keys = reinterpret_cast<double2 *>(beam_smem + tab_bytes);
    double *score = reinterpret_cast<double *>(beam_smem + tab_bytes + (size_t)BEAM_KEYS * 16);
    uint8_t *ring = reinterpret_cast<uint8_t *>(score + 2 * GH_BEAM_MAX);
    const double2 *Gb2 = reinterpret_cast<const double2 *>(Gb);
    const int k = tid >> 3, s = tid & 7;
    const int A = R - L - 1;

    if (tid == 0) { score[0] = 0.0; ring[0] = 5; }            // one hypothesis: '_' at position 0, score +0.0
    if (STAGED) {
        // sources 0 .. A-1 straight in (source i lies in slot i % R)
        const int pre = A < N ? A : N;
        for (int u = tid; u < pre * su; u += nt) tab2[u] = Gb2[u];
    }
    __syncthreads();

    double2 reg[BEAM_LOAD_UNITS];
    bool have_reg = false;
    int wslot = 0, ldslot = STAGED ? A % R : 0;               // slot of the block in `reg`; slot of source p + A - 1
    int n = 1, cur = 0, hole = 0;
    int ps = 0;                                               // ring slot of position p - 1
    int ts = 0;                                               // LDS slot of source p - 1
    for (int p = 1; p <= N; p++) {
        if (STAGED) {
            // the block loaded in the last step replaces source p - L - 3, which nobody reads any more; the next one sets out
            if (have_reg) {
#pragma unroll
                for (int j = 0; j < BEAM_LOAD_UNITS; j++) {
                    const int u = tid + j * nt;
                    if (u < su) tab2[(size_t)wslot * su + u] = reg[j];
                }
            }
            const int src = p + A - 1;
            have_reg = src < N;
            if (have_reg) {
#pragma unroll
                for (int j = 0; j < BEAM_LOAD_UNITS; j++) {
                    const int u = tid + j * nt;
                    if (u < su) reg[j] = Gb2[(size_t)src * su + u];
                }
                wslot = ldslot;
            }
            ldslot = ldslot + 1 == R ? 0 : ldslot + 1;
        }
        const double *blk = STAGED ? tab + (size_t)ts * sd : Gb + (size_t)(p - 1) * sd;
        const uint32_t cm5 = (uint32_t)__double_as_longlong(blk[30 * L + 5]);
        if (cm5 == 0) { hole = p; break; }                    // (the same word in every thread: all leave together)
        const bool child = k < n && s < 5 && ((cm5 >> s) & 1u);
        double w = 0.0, sc = 0.0;
        if (child) {
            // k_score_pos' additions in k_score_pos' order: the marginal term first, then lags 1, 2, ...
            if (marginal_term) w += blk[30 * L + s];
            const uint8_t *rg = ring + (size_t)(cur * GH_BEAM_MAX + k) * Lr;
            const int lmax = L < p ? L : p;
            int rs = ps, tl = ts;
            // (four lags at a time: their symbols, then their entries, are independent reads in flight together; the additions
            // stay in lag order)
            for (int l0 = 1; l0 <= lmax; l0 += 4) {
                int a6[4];
                double v[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    a6[j] = l0 + j <= lmax ? rg[rs] : 0;                      // (a lag beyond lmax: row 0 of a valid block, dropped below)
                    rs = rs == 0 ? Lr - 1 : rs - 1;
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int l = l0 + j, i = p - l > 0 ? p - l : 0;
                    const double *src = STAGED ? tab + (size_t)tl * sd : Gb + (size_t)i * sd;
                    v[j] = src[(a6[j] * L + (l <= L ? l - 1 : 0)) * LT_ROW + s];
                    tl = tl == 0 ? R - 1 : tl - 1;
                }
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (l0 + j <= lmax) w += v[j];
            }
            sc = score[cur * GH_BEAM_MAX + k] + w;
            keys[k * 5 + s] = make_double2(sc, w);
        }
        beam_barrier();
        const int psn = ps + 1 == Lr ? 0 : ps + 1;
        if (child) {
            int rank = 0;
            // (cm(p) is the same for every parent: slot s2 of every live parent holds a key exactly where cm5 has bit s2)
            for (int k2 = 0; k2 < n; k2++) {
#pragma unroll
                for (int s2 = 0; s2 < 5; s2++) {
                    const double2 o = keys[k2 * 5 + s2];
                    const bool before = o.x > sc || (o.x == sc && (k2 < k || (k2 == k && (o.y > w || (o.y == w && s2 < s)))));
                    rank += (before && ((cm5 >> s2) & 1u)) ? 1 : 0;
                }
            }
            if (rank < B) {
                score[(cur ^ 1) * GH_BEAM_MAX + rank] = sc;
                bp[(size_t)p * bps + rank] = (uint8_t)(k | (s << 5));
                const uint32_t *from = reinterpret_cast<const uint32_t *>(ring + (size_t)(cur * GH_BEAM_MAX + k) * Lr);
                uint32_t *to = reinterpret_cast<uint32_t *>(ring + (size_t)((cur ^ 1) * GH_BEAM_MAX + rank) * Lr);
                for (int q = 0; q < Lr / 4; q++) to[q] = from[q];
                reinterpret_cast<uint8_t *>(to)[psn] = (uint8_t)s;
            }
        }
        const int born = n * __popc(cm5);
        n = born < B ? born : B;
        cur ^= 1;
        ps = psn;
        ts = ts + 1 == R ? 0 : ts + 1;
        beam_barrier();
    }
    if (tid == 0) {
        out->n_out = hole ? 0 : n;
        out->hole_at = hole;
        out->end = hole ? hole - 1 : N;                       // at a hole: the prefix of the rank-0 hypothesis
        out->rows = hole ? 1 : n;
    }
    if (!hole && tid < n) ll[tid] = score[cur * GH_BEAM_MAX + tid];
}

__global__ void __launch_bounds__(256)
k_beam_trace(const uint8_t *__restrict__ bp, int bps, int N, const beam_out *__restrict__ out, symmap sm, uint8_t *__restrict__ paths)
{
    __shared__ __attribute__((aligned(16))) uint32_t blk[BEAM_TRACE_POS * GH_BEAM_MAX / 4];
    const int tid = threadIdx.x;
    const int end = out->end, rows = out->rows;
    const size_t row = (size_t)tid * ((size_t)N + 1);
    const int wps = bps / 4;                                  // (bps is a multiple of 4: whole words per position)
    int r = tid;
    if (tid < rows) paths[row] = SYM_US;
    for (int hi = end; hi >= 1; hi -= BEAM_TRACE_POS) {
        const int lo = hi - BEAM_TRACE_POS + 1 > 1 ? hi - BEAM_TRACE_POS + 1 : 1;
        const uint32_t *from = reinterpret_cast<const uint32_t *>(bp + (size_t)lo * bps);
        for (int q = tid; q < (hi - lo + 1) * wps; q += blockDim.x) blk[q] = from[q];
        __syncthreads();
        if (tid < rows) {
            const uint8_t *b8 = reinterpret_cast<const uint8_t *>(blk);
            for (int q = hi; q >= lo; q--) {
                const int v = b8[(q - lo) * bps + r];
                paths[row + q] = (uint8_t)vsym(sm, v >> 5);
                r = v & 31;
            }
        }
        __syncthreads();
    }
}

// host ----------------------------------------------------------------------------------------
struct beam_bufs {
    double *Gb;
    uint8_t *bp, *paths;
    double *ll;
    beam_out *out;
    int bps;
};

static int beam_check(const gh_handle *h, int width, const char *who)
{
    if (width < 1 || width > GH_BEAM_MAX) return fail(GH_ERR_ARG, "%s: width must be 1..%d (got %d)", who, GH_BEAM_MAX, width);
    if (h->cfg.offer_zero)
        return fail(GH_ERR_ARG, "%s: the handle offers zero-count candidates (offer_zero), whose weights can be NaN (-inf + +inf): no order ranks them", who);
    if (h->band_zero) return fail(GH_ERR_STATE, "%s before any fill or import: the tensor holds no evidence", who);
    const int Le = h->L < h->N ? h->L : h->N;
    if (Le > BEAM_MAX_L) return fail(GH_ERR_ARG, "%s: the beam keeps %d-symbol histories in LDS: L up to %d", who, Le, BEAM_MAX_L);
    return GH_OK;
}

// one beam over the tensor as it stands: the results stay in the handle's beam scratch (`b`), *ho = counts and hole
static int beam_run(gh_handle *h, int width, beam_bufs *b, beam_out *ho)
{
    const int N = h->N;
    // (lags beyond the window's first position are never summed: a table of min(L, N) lags gives the same weights)
    const int L = h->L < N ? h->L : N;
    int rc = ensure_marg(h);
    if (rc) return rc;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const int bps = (width + 3) & ~3;
    const size_t n1 = (size_t)N + 1;
    const size_t gb_b = up((size_t)N * beam_src_doubles(L) * 8), bp_b = up(n1 * bps), path_b = up(n1 * GH_BEAM_MAX);
    const size_t need = gb_b + bp_b + path_b + up(GH_BEAM_MAX * 8) + up(sizeof(beam_out));
    if (need > h->beam_cap) {
        HIPCHK(hipStreamSynchronize(h->stream));
        hipFree(h->beam_buf);
        h->beam_buf = nullptr;
        h->beam_cap = 0;
        if (hipMalloc(&h->beam_buf, need) != hipSuccess) {
            (void)hipGetLastError();
            return fail(GH_ERR_NOMEM, "the beam's scratch (%zu bytes: it grows with N * L) cannot be had", need);
        }
        h->beam_cap = need;
    }
    char *base = (char *)h->beam_buf;
    b->Gb = (double *)base;
    b->bp = (uint8_t *)(base + gb_b);
    b->paths = b->bp + bp_b;
    b->ll = (double *)(b->paths + path_b);
    b->out = (beam_out *)((char *)b->ll + up(GH_BEAM_MAX * 8));
    b->bps = bps;

    const void *tb = (h->tband && h->tband_epoch == h->band_epoch) ? h->tband : nullptr;
    const size_t total = (size_t)N * beam_src_doubles(L);
    const unsigned nb = (unsigned)std::min<size_t>((total + 255) / 256, 256 * 16);
    with_storage(h, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(k_beam_table<T>, dim3(nb), dim3(256), 0, h->stream, (const T *)h->band, (const T *)tb, N, h->W, L, h->cfg.cond_mode,
                           h->cnt, h->nvalid, h->cmask, h->minfo, h->sm, b->Gb);
    });
    if ((rc = post_launch(h, "k_beam_table"))) return rc;

    static const bool no_stage = env_off("GH_BEAM_STAGE");      // (A/B: every L through the global loader)
    const int R = no_stage ? 0 : beam_ring_sources(L);
    const int threads = std::max(64, 8 * width);
    const size_t lds = (R ? (size_t)R * beam_src_doubles(L) * 8 : 0) + beam_fixed_lds(L);
    // (without staging R only has to be a ring size the slot arithmetic can wrap on)
    if (R) {
        lds_limit<k_beam_walk<true>>(lds, h->dev);
        hipLaunchKernelGGL(k_beam_walk<true>, dim3(1), dim3(threads), lds, h->stream, (const double *)b->Gb, N, L, width, h->cfg.marginal_term, R,
                           b->bp, bps, b->ll, b->out);
    } else {
        lds_limit<k_beam_walk<false>>(lds, h->dev);
        hipLaunchKernelGGL(k_beam_walk<false>, dim3(1), dim3(threads), lds, h->stream, (const double *)b->Gb, N, L, width, h->cfg.marginal_term, L + 2,
                           b->bp, bps, b->ll, b->out);
    }
    if ((rc = post_launch(h, "k_beam_walk"))) return rc;
    hipLaunchKernelGGL(k_beam_trace, dim3(1), dim3(256), 0, h->stream, (const uint8_t *)b->bp, bps, N, (const beam_out *)b->out, h->sm, b->paths);
    if ((rc = post_launch(h, "k_beam_trace"))) return rc;
    HIPCHK(hipMemcpyAsync(ho, b->out, sizeof *ho, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->beam_last[0] = R ? 1 : 0;
    h->beam_last[1] = R;
    h->beam_last[2] = threads;
    h->beam_last[3] = (int64_t)need;
    return GH_OK;
}

extern "C" int gh_beam_paths(gh_t *h, int width, uint8_t *paths_out, double *ll_chain, int *n_out, int *hole_at)
{
    if (!h || !paths_out || !n_out || !hole_at) return fail(GH_ERR_ARG, "null argument");
    int rc = beam_check(h, width, "gh_beam_paths");
    if (rc) return rc;
    if (set_dev(h)) return GH_ERR_HIP;
    beam_bufs b;
    beam_out ho;
    if ((rc = beam_run(h, width, &b, &ho))) return rc;
    const size_t n1 = (size_t)h->N + 1;
    if (ho.hole_at) {
        if (ho.end + 1 > 0) HIPCHK(hipMemcpyAsync(paths_out, b.paths, (size_t)ho.end + 1, hipMemcpyDeviceToHost, h->stream));
    } else {
        HIPCHK(hipMemcpyAsync(paths_out, b.paths, n1 * ho.n_out, hipMemcpyDeviceToHost, h->stream));
        if (ll_chain) HIPCHK(hipMemcpyAsync(ll_chain, b.ll, (size_t)ho.n_out * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    *n_out = ho.n_out;
    *hole_at = ho.hole_at;
    return GH_OK;
}

extern "C" int gh_beam_spin(gh_t *h, int width, int max_paths, double min_remove, uint8_t *paths_out, gh_path_rec *recs, double *ll_chain,
                            int *n_out, int *hole_at)
{
    if (!h || !paths_out || !recs || !n_out || !hole_at) return fail(GH_ERR_ARG, "null argument");
    if (max_paths < 0) return fail(GH_ERR_ARG, "max_paths < 0");
    int rc = beam_check(h, width, "gh_beam_spin");
    if (rc) return rc;
    if (set_dev(h)) return GH_ERR_HIP;
    *n_out = 0; *hole_at = 0;
    if (max_paths == 0) return GH_OK;
    if (!h->have_orig && (rc = gh_snapshot_original(h))) return rc;
    const size_t n1 = (size_t)h->N + 1;
    for (int s = 0; s < max_paths; s++) {
        beam_bufs b;
        beam_out ho;
        if ((rc = beam_run(h, width, &b, &ho))) return rc;
        if (ho.hole_at) { *hole_at = ho.hole_at; break; }
        uint8_t *path = paths_out + n1 * s;
        double ll = 0.0;
        HIPCHK(hipMemcpyAsync(path, b.paths, n1, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(&ll, b.ll, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        // the record of that path on the tensor as it stands (hp_original under the snapshot), then the reweight
        gh_score_rec sr;
        if ((rc = gh_score_paths(h, path, 1, &sr, nullptr, nullptr, nullptr))) return rc;
        gh_path_rec &r = recs[s];
        r.hp_current = sr.hp_current;
        r.hp_original = sr.hp_original;
        r.min_marginal = sr.min_marginal;
        r.ratio = sr.min_marginal < min_remove ? min_remove : sr.min_marginal;
        if ((rc = gh_reweight_path(h, path, r.ratio, &r.magnitude))) return rc;
        if (ll_chain) ll_chain[s] = ll;
        *n_out = s + 1;
    }
    return GH_OK;
}

extern "C" int gh_beam_info(const gh_t *h, int64_t out[4])
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    for (int q = 0; q < 4; q++) out[q] = h->beam_last[q];
    return GH_OK;
}
