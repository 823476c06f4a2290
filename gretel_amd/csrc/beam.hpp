// beam.hpp -- beam search over the chain likelihood (gh_beam_paths, gh_beam_spin, gh_beam_info: include/gretel_hip.h, where the
// definition stands; INTEGRATION.md "Beam search").  Width B hypotheses walk the window together; every score is a sequential
// binary64 sum in ascending p and every weight k_score_pos' additions in k_score_pos' order, so what comes out is what
// gh_score_paths says of the same paths bit for bit, and B = 1 is gh_generate_path.  The tensor is only read.
//
//   k_beam_table  chain_table.hpp: the plain table, one block of 30 L + 6 doubles per source position, in the beam's own scratch block
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
#define BEAM_AHEAD_MIN 16          /* staged only where the loader can run this many steps ahead: a step is a few LDS round trips and
                                      two barriers, a block from HBM a few of those -- 16 leaves it room under load */
#define BEAM_AHEAD_MAX 64          /* ... and never more: nothing is gained, and a short window would be preloaded whole */
#define BEAM_LOAD_UNITS 5          /* 16-byte pieces of a block one thread of the smallest workgroup (64) carries from step to step */
#define BEAM_MAX_L 2048            /* the two ring buffers of 32 hypotheses stay within the LDS */
#define BEAM_TRACE_POS 1024

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

// host ---------------------------------------------------------------------------------------- (beam_out, beam_bufs: scratch_layout.hpp)
static int beam_check(const gh_handle *h, int width, const char *who)
{
    if (width < 1 || width > GH_BEAM_MAX) return fail(GH_ERR_ARG, "%s: width must be 1..%d (got %d)", who, GH_BEAM_MAX, width);
    int rc = decode_check(h, who);
    if (rc) return rc;
    const int Le = chain_lags(h);
    if (Le > BEAM_MAX_L) return fail(GH_ERR_ARG, "%s: the beam keeps %d-symbol histories in LDS: L up to %d", who, Le, BEAM_MAX_L);
    return GH_OK;
}

// one beam over the tensor as it stands: the results stay in the handle's beam scratch (`b`), *ho = counts and hole
static int beam_run(gh_handle *h, int width, beam_bufs *b, beam_out *ho)
{
    const int N = h->N, L = chain_lags(h);
    const size_t table_doubles = (size_t)N * beam_src_doubles(L);
    const size_t need = beam_layout(nullptr, N, table_doubles, width).total;
    int rc = scratch_reserve(h, &h->beam, need, "the beam's scratch, which grows with N * L,");
    if (rc) return rc;
    *b = beam_layout(h->beam.buf, N, table_doubles, width);
    if ((rc = chain_table_build(h, L, b->Gb))) return rc;

    static const bool no_stage = env_off("GH_BEAM_STAGE");      // (A/B: every L through the global loader)
    const int R = no_stage ? 0 : beam_ring_sources(L);
    const int threads = std::max(64, 8 * width);
    const size_t lds = (R ? (size_t)R * beam_src_doubles(L) * 8 : 0) + beam_fixed_lds(L);
    // (without staging R only has to be a ring size the slot arithmetic can wrap on)
    if (R) {
        lds_limit<k_beam_walk<true>>(lds, h->dev);
        hipLaunchKernelGGL(k_beam_walk<true>, dim3(1), dim3(threads), lds, h->stream, (const double *)b->Gb, N, L, width, h->cfg.marginal_term, R,
                           b->bp, b->bps, b->ll, b->out);
    } else {
        lds_limit<k_beam_walk<false>>(lds, h->dev);
        hipLaunchKernelGGL(k_beam_walk<false>, dim3(1), dim3(threads), lds, h->stream, (const double *)b->Gb, N, L, width, h->cfg.marginal_term, L + 2,
                           b->bp, b->bps, b->ll, b->out);
    }
    if ((rc = post_launch(h, "k_beam_walk"))) return rc;
    hipLaunchKernelGGL(k_beam_trace, dim3(1), dim3(256), 0, h->stream, (const uint8_t *)b->bp, b->bps, N, (const beam_out *)b->out, h->sm, b->paths);
    if ((rc = post_launch(h, "k_beam_trace"))) return rc;
    HIPCHK(hipMemcpyAsync(ho, b->out, sizeof *ho, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->beam_last[0] = R ? 1 : 0; h->beam_last[1] = R; h->beam_last[2] = threads; h->beam_last[3] = (int64_t)need;
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
    return decode_spin(h, max_paths, min_remove, paths_out, recs, ll_chain, n_out, hole_at, [&](decoded *d) -> int {
        beam_bufs b;
        beam_out ho;
        if ((rc = beam_run(h, width, &b, &ho))) return rc;
        d->hole = ho.hole_at;
        d->d_path = b.paths;                                   // (rank 0: the best hypothesis and its score)
        d->d_ll = b.ll;
        return GH_OK;
    });
}

extern "C" int gh_beam_info(const gh_t *h, int64_t out[4])
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    for (int q = 0; q < 4; q++) out[q] = h->beam_last[q];
    return GH_OK;
}
