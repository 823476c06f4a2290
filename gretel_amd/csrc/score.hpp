// score.hpp -- scoring given haplotypes against the tensor (gh_score_paths, include/gretel_hip.h; the definition: INTEGRATION.md
// "Scoring haplotypes").  A given path fixes every history, so all positions of all paths are independent: nothing of the spin
// loop's machinery is needed, the tensor is only read.  Every output is an integer or a binary64 value whose additions run in a
// fixed order, so the results are those of gh_edge_weights_at and gh_generate_path bit for bit.
//
//   k_score_pos   eight lanes per (path, position): lane s < 7 takes the weight of symbol s where it is a candidate -- the marginal
//                 term first, then lags 1, 2, ... in that order through log_conditional (kernels.hpp: any history symbol, all five
//                 conditionals, both storage types; under C / E the to-major copy where the handle has a current one) -- the group
//                 exchanges the seven weights (__shfl over 8 lanes) and lane 0 writes the position's weight, margin and pick.
//                 32 positions of one path per workgroup, grid (positions / 32, paths of the slab).
//   k_score_sum   the ordered pass, per path three wavefronts (blockIdx.y): the chain weight, hp_current and hp_original, each
//                 a strictly sequential binary64 sum over the on positions in ascending p (the addends go through LDS 512 at a time
//                 and are read back by broadcast, as k_hp takes its sums: segwalk.hpp); the first of them also takes the counts
//                 and the minima, which no order can change.
//
// The per-position values lie in one scratch block of the handle, SCORE_SLAB_BYTES at most whatever n_paths is: the paths are
// processed in slabs of as many as fit, each slab's results copied out before the next one overwrites them.
// ---------------------------------------------------------------------------------------------

#define SCORE_BLOCK 256
#define SCORE_POS_PER_BLOCK (SCORE_BLOCK / 8)
#define SCORE_SLAB_BYTES ((size_t)16 << 20)   /* per-position scratch of one slab: weight + margin (f64), pick + path (u8) per (path, position) */
#define SCORE_CHUNK 512

// is position p of a path that carries symbol xs there ON: xs among the candidates of p (N and '_' never are)
__device__ __forceinline__ bool score_on(uint32_t cmask_word, int xs) { return (CM_CAND(cmask_word) >> xs) & 1u; }

template <typename T>
__global__ void __launch_bounds__(SCORE_BLOCK)
k_score_pos(const T *__restrict__ band, const T *__restrict__ tband, int N, int W, int cond_mode, int L, int marginal_term,
            const double *__restrict__ cnt, const double *__restrict__ marg, const int32_t *__restrict__ nvalid,
            const uint32_t *__restrict__ cmask, symmap sm, const uint8_t *__restrict__ paths,
            double *__restrict__ weight, double *__restrict__ margin, uint8_t *__restrict__ pick)
{
    const int p = blockIdx.x * SCORE_POS_PER_BLOCK + (threadIdx.x >> 3);
    const int s = threadIdx.x & 7;
    const size_t row = (size_t)blockIdx.y * (size_t)(N + 1);
    const uint8_t *x = paths + row;
    const bool act = p >= 1 && p <= N;
    const uint32_t cm = act ? CM_CAND(cmask[p]) : 0u;
    // the weight of candidate s given the path's own history: k_edge_weights' additions in k_edge_weights' order
    double w = 0.0;
    if (s < NSYM && ((cm >> s) & 1u)) {
        if (marginal_term) w += gh_log10(marg[(size_t)p * 8 + s]);
        const int lmax = L < p ? L : p;
        for (int l = 1; l <= lmax; l++)      // (index 0 of a row is the '_' sentinel whatever the caller left there)
            w += log_conditional(band, W, cond_mode, cnt, nvalid, l < p ? (int)x[p - l] : SYM_US, s, p - l, p, tband);
    }
    double ws[NSYM];
#pragma unroll
    for (int c = 0; c < NSYM; c++) ws[c] = __shfl(w, c, 8);
    if (s != 0 || p > N) return;
    if (p == 0) { weight[row] = 0.0; margin[row] = 0.0; pick[row] = SYM_US; return; }
    // pick: the first candidate in the order they are offered in, replaced only by a strictly larger weight (gretel.py:166-174)
    int pk = 255;
    double best = 0.0;
#pragma unroll
    for (int b5 = 0; b5 < 5; b5++) {
        const int c = vsym(sm, b5);
        double wc = ws[0];
#pragma unroll
        for (int q = 1; q < NSYM; q++) wc = (c == q) ? ws[q] : wc;
        if (((cm >> c) & 1u) && (pk == 255 || wc > best)) { pk = c; best = wc; }
    }
    // the path's own symbol against the best of the others
    const int xs = x[p];
    const bool on = (cm >> xs) & 1u;
    double mine = 0.0, other = 0.0;
    bool have_other = false;
#pragma unroll
    for (int c = 0; c < NSYM; c++) {
        if (!((cm >> c) & 1u)) continue;
        if (c == xs) mine = ws[c];
        else if (!have_other || ws[c] > other) { other = ws[c]; have_other = true; }
    }
    weight[row + p] = on ? mine : -INFINITY;
    margin[row + p] = on ? (have_other ? mine - other : INFINITY) : -INFINITY;
    pick[row + p] = (uint8_t)pk;
}

// a strictly sequential binary64 sum of value(1) .. value(N), from 0.0 (one wavefront; an unused slot adds +0.0)
template <typename F>
__device__ __forceinline__ double score_ordered_sum(int N, double (*buf)[SCORE_CHUNK], F value)
{
    const int lane = threadIdx.x;
    constexpr int PER = SCORE_CHUNK / 64;
    double r[PER];
#pragma unroll
    for (int k = 0; k < PER; k++) r[k] = value(1 + lane + 64 * k);
    const int nchunks = (N + SCORE_CHUNK - 1) / SCORE_CHUNK;
    double acc = 0.0;
    for (int c = 0; c < nchunks; c++) {
        double *b = buf[c & 1];
#pragma unroll
        for (int k = 0; k < PER; k++) b[lane + 64 * k] = r[k];
        __syncthreads();
        if (c + 1 < nchunks) {
#pragma unroll
            for (int k = 0; k < PER; k++) r[k] = value(1 + (c + 1) * SCORE_CHUNK + lane + 64 * k);
        }
#pragma unroll 32
        for (int j = 0; j < SCORE_CHUNK; j++) acc += b[j];
    }
    return acc;
}

// blockIdx.x = path of the slab, blockIdx.y = 0: chain weight + counts + minima, 1: hp_current, 2: hp_original
__global__ void __launch_bounds__(64)
k_score_sum(const double *__restrict__ weight, const double *__restrict__ margin, const uint8_t *__restrict__ pick,
            const uint8_t *__restrict__ paths, const uint32_t *__restrict__ cmask, const double *__restrict__ marg,
            const double *__restrict__ minfo, int orig_slot, int N, symmap sm, gh_score_rec *__restrict__ recs)
{
    __shared__ double buf[2][SCORE_CHUNK];
    const int which = blockIdx.y, lane = threadIdx.x;
    const size_t row = (size_t)blockIdx.x * (size_t)(N + 1);
    const uint8_t *x = paths + row;
    gh_score_rec *rec = recs + blockIdx.x;
    if (which != 0) {
        // log10 marginal of the path's symbol, current (minfo[0..4]) or as the snapshot froze it (minfo[11..15]): k_marg's values
        const int slot = which == 1 ? 0 : orig_slot;
        const double acc = score_ordered_sum(N, buf, [&](int t) -> double {
            const int tt = t <= N ? t : N;
            const int xs = x[tt];
            const bool on = t <= N && score_on(cmask[tt], xs);
            const double v = minfo[(size_t)tt * MINFO + slot + (on ? a6_of_sym(sm, xs) : 0)];
            return on ? v : 0.0;
        });
        if (lane == 0) { if (which == 1) rec->hp_current = acc; else rec->hp_original = acc; }
        return;
    }
    const double acc = score_ordered_sum(N, buf, [&](int t) -> double {
        const int tt = t <= N ? t : N;
        const double v = weight[row + tt];
        return (t <= N && score_on(cmask[tt], x[tt])) ? v : 0.0;
    });
    // counts and minima: every lane over its positions in ascending order, then across the lanes; a minimum is taken by
    // strict <, the earlier position winning among equals -- what one pass in ascending p leaves
    int n_on = 0, n_greedy = 0, first_off = 0x7fffffff, first_on = 0x7fffffff, arg = 0x7fffffff;
    double min_marginal = INFINITY, min_margin = INFINITY;
    for (int p = 1 + lane; p <= N; p += 64) {
        const int xs = x[p];
        if (!score_on(cmask[p], xs)) { first_off = first_off < p ? first_off : p; continue; }
        n_on++;
        first_on = first_on < p ? first_on : p;
        if (pick[row + p] == xs) n_greedy++;
        const double m = marg[(size_t)p * 8 + xs], g = margin[row + p];
        if (m < min_marginal) min_marginal = m;
        if (g < min_margin) { min_margin = g; arg = p; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_on += __shfl_xor(n_on, o);
        n_greedy += __shfl_xor(n_greedy, o);
        const int fo = __shfl_xor(first_off, o);
        first_off = fo < first_off ? fo : first_off;
        const int fn = __shfl_xor(first_on, o);
        first_on = fn < first_on ? fn : first_on;
        const double mm = __shfl_xor(min_marginal, o);
        if (mm < min_marginal) min_marginal = mm;
        const double og = __shfl_xor(min_margin, o);
        const int oa = __shfl_xor(arg, o);
        if (og < min_margin || (og == min_margin && oa < arg)) { min_margin = og; arg = oa; }
    }
    if (lane == 0) {
        rec->ll_chain = acc;
        rec->min_marginal = min_marginal;
        rec->min_margin = min_margin;
        rec->n_on = n_on;
        rec->n_greedy = n_greedy;
        rec->first_off = first_off == 0x7fffffff ? 0 : first_off;
        // (a minimum of +inf: every on position has it, the first of them is its position; nothing on: 0)
        if (arg == 0x7fffffff) arg = first_on;
        rec->argmin_margin = arg == 0x7fffffff ? 0 : arg;
    }
}

// host ----------------------------------------------------------------------------------------
extern "C" int gh_score_paths(gh_t *h, const uint8_t *paths, int n_paths, gh_score_rec *recs,
                              double *weight, double *margin, uint8_t *pick)
{
    if (!h || !paths || !recs) return fail(GH_ERR_ARG, "null argument");
    if (n_paths < 0) return fail(GH_ERR_ARG, "n_paths must be >= 0 (got %d)", n_paths);
    if (n_paths == 0) return GH_OK;
    const int N = h->N;
    const size_t n1 = (size_t)N + 1;
    int rc = check_symbol_rows(paths, n_paths, n1, GH_ERR_SYMBOL);
    if (rc) return rc;
    if (h->band_zero) return fail(GH_ERR_STATE, "gh_score_paths before any fill or import: the tensor holds no evidence");
    if (set_dev(h)) return GH_ERR_HIP;
    if ((rc = ensure_marg(h))) return rc;

    // one device block, kept on the handle: per slab its paths, records, weights, margins and picks (score_layout)
    const size_t per_path = n1 * (8 + 8 + 1 + 1);
    const int slab = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)n_paths, 65535), SCORE_SLAB_BYTES / per_path));
    if ((rc = scratch_reserve(h, &h->score, score_layout(nullptr, slab, n1).total, "gh_score_paths: the scratch of one slab of paths"))) return rc;
    const score_bufs d = score_layout(h->score.buf, slab, n1);

    const void *tb = tband_current(h);
    const int orig_slot = h->have_orig ? 11 : 0;
    for (int q0 = 0; q0 < n_paths; q0 += slab) {
        const int k = std::min(slab, n_paths - q0);
        const size_t o = (size_t)q0 * n1, cells = (size_t)k * n1;
        HIPCHK(hipMemcpyAsync(d.paths, paths + o, cells, hipMemcpyHostToDevice, h->stream));
        with_storage(h, [&](auto z) {
            using T = decltype(z);
            hipLaunchKernelGGL(k_score_pos<T>, dim3((unsigned)((n1 + SCORE_POS_PER_BLOCK - 1) / SCORE_POS_PER_BLOCK), (unsigned)k),
                               dim3(SCORE_BLOCK), 0, h->stream, (const T *)h->band, (const T *)tb, N, h->W, h->cfg.cond_mode, h->L,
                               h->cfg.marginal_term, h->cnt, h->marg, h->nvalid, h->cmask, h->sm, d.paths, d.weight, d.margin, d.pick);
        });
        if ((rc = post_launch(h, "k_score_pos"))) return rc;
        hipLaunchKernelGGL(k_score_sum, dim3((unsigned)k, 3), dim3(64), 0, h->stream, d.weight, d.margin, d.pick, d.paths, h->cmask,
                           h->marg, h->minfo, orig_slot, N, h->sm, d.recs);
        if ((rc = post_launch(h, "k_score_sum"))) return rc;
        HIPCHK(hipMemcpyAsync(recs + q0, d.recs, (size_t)k * sizeof(gh_score_rec), hipMemcpyDeviceToHost, h->stream));
        if (weight) HIPCHK(hipMemcpyAsync(weight + o, d.weight, cells * 8, hipMemcpyDeviceToHost, h->stream));
        if (margin) HIPCHK(hipMemcpyAsync(margin + o, d.margin, cells * 8, hipMemcpyDeviceToHost, h->stream));
        if (pick) HIPCHK(hipMemcpyAsync(pick + o, d.pick, cells, hipMemcpyDeviceToHost, h->stream));
        // (the next slab overwrites the block: its results have left, and the caller's path rows have been read, behind this)
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return GH_OK;
}
