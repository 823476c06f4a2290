// viterbi_grid.hpp -- the grid decoder: exact decoding of the chain likelihood beyond the 4096 states k_vit_walk's two LDS rows
// hold (gh_viterbi_path_grid, gh_viterbi_spin_grid, gh_viterbi_grid_info: include/gretel_hip.h; INTEGRATION.md "Exact decoding on
// the grid").  The definition, the state index, the table and every addition are viterbi.hpp's: where both decoders serve a window
// their results agree bit for bit.  What differs is where the dynamic programme lives: two score rows of `states` doubles in
// GLOBAL memory, ONE LAUNCH PER POSITION on the handle's stream.  The launch boundary is the only synchronisation: no workgroup
// waits for another, no grid barrier, no counter, nothing that could hang; the host does not wait between the steps.
//
//   k_vit_cands   (viterbi_marg.hpp, as it stands) the candidate bits of every position.  The host takes the N + 1 bytes home ONCE
//                 and forms from them U, S, the state count (checked against the cap in 64 bits), the first hole -- a hole ends
//                 the call before any step is launched -- and per step the mask words below.
//   k_vitg_step<S>  step p.  A thread owns r = j mod S^(Le-1): the Le - 1 picks at positions p-1 .. p-Le+1 that a group of S new
//                 states b S^(Le-1) + r shares with its S predecessors r S + x.  It decodes r's digits once (S is a template
//                 parameter: the divisions are by constants, and at S = 2, 4 the digits are r's bits), tests each against its
//                 position's mask (positions <= 0 offer digit 0 alone: the host says so in the mask words), reads Vc[r S + x] for
//                 the x that position p - Le offers, and per candidate b of position p forms the prefix in the definition's order
//                 (+0.0, the marginal term if the spec has it, lags 1 .. min(Le - 1, p)), then per x ascending
//                 cand = Vc[pred] + (prefix + T_Le[x][b]), kept by strict >; for p < Le the one predecessor, cand = Vc[pred] +
//                 prefix.  The lag that reaches position 0 reads the '_' row.  Adjacent threads read adjacent runs of S doubles
//                 and write adjacent doubles (and back-pointer bytes) per b.  Unreachable entries are never written and never read.
//                 The step's numbers are kernel arguments: p, the masks of positions p .. p-Le+1 (5 bits each, twelve a word: two
//                 words hold the 24 positions the cap allows a window of two symbols) and the mask of position p - Le.
//                 A workgroup first stages what the step reads of the table -- of source p - l only lag l: 30 doubles a lag, and
//                 target p's five marginals -- into LDS.  S = 1 is one state whatever L is (no digits, no masks, L may exceed
//                 24): its one thread reads the table from global memory.
//   k_vitg_end<S>   the end rule, first level: a workgroup per GH_VITG_END_CHUNK states in ascending j, a thread's own states
//                 ascending (the first stays unless strictly beaten), then pairwise, where of two equal scores the smaller j stays.
//   k_vitg_end2   second level: one workgroup over the partials, the same two rules.
//   k_vitg_trace  one lane follows the back-pointers from N down and writes the path row: a dependent global read per position
//                 (rows of up to 16 MB do not go through LDS).
// ---------------------------------------------------------------------------------------------

#define VITG_THREADS 256
#define VITG_MAX_LE 24                                   /* 2^24 = the cap: no window with two slots or more has a longer state */
#define VITG_END_THREADS 1024

static_assert(GH_VITERBI_GRID_MAX_STATES == 1 << VITG_MAX_LE && 5 * 12 <= 64, "two symbols, 24 lags; twelve masks a word");
static_assert(GH_VITG_END_CHUNK % VITG_THREADS == 0 && GH_VITERBI_GRID_MAX_STATES / GH_VITG_END_CHUNK <= 4 * VITG_END_THREADS,
              "whole strides a chunk; the second level is one workgroup");

// the n digits of v, most significant first (k = 1 .. n).  S = 2, 4: v's own bits.  S = 3, 5: three bits a digit at bit 3k
// (n <= 15: 3^15 and 5^10 are the longest states below the cap)
template <int S> __device__ __forceinline__ unsigned long long vitg_pack(int v, int n)
{
    if constexpr (S == 3 || S == 5) {
        unsigned long long pk = 0;
        int rest = v;
        for (int k = n; k >= 1; k--) {
            pk |= (unsigned long long)(rest % S) << (3 * k);
            rest /= S;
        }
        return pk;
    } else {
        return (unsigned long long)v;
    }
}

template <int S> __device__ __forceinline__ int vitg_digit(unsigned long long pk, int k, int n)
{
    if constexpr (S == 1) return 0;
    else if constexpr (S == 2) return (int)(pk >> (n - k)) & 1;
    else if constexpr (S == 4) return (int)(pk >> (2 * (n - k))) & 3;
    else return (int)(pk >> (3 * k)) & 7;
}

// digit -> compact index b5: three bits a digit (the host packs them, ascending: the candidate order)
__device__ __forceinline__ int vitg_slot(uint32_t sp, int d) { return (int)(sp >> (3 * d)) & 7; }
// the candidate mask of position p - k
__device__ __forceinline__ uint32_t vitg_mask(unsigned long long m0, unsigned long long m1, int k)
{
    return (uint32_t)(k < 12 ? m0 >> (5 * k) : m1 >> (5 * (k - 12))) & 31u;
}

// KEEP (viterbi_grid_marg.hpp): the forward pass of the max-marginals on the grid -- the same step, the caller hands it rows of
// its kept block; no back-pointers (bp is not touched)
template <int S, bool KEEP = false>
__global__ void __launch_bounds__(VITG_THREADS)
k_vitg_step(const double *__restrict__ Gb, int p, int L, int pw, int marginal_term, uint32_t sp, unsigned long long m0, unsigned long long m1,
            uint32_t cm_old, const double *__restrict__ Vc, double *__restrict__ Vn, uint8_t *__restrict__ bp)
{
    __shared__ double tab[S > 1 ? 30 * VITG_MAX_LE + 5 : 1];  // [lag l - 1][a6][b5] of source p - l, then target p's marginals
    const int sd = beam_src_doubles(L);
    const int nl = L < p ? L : p;                             // the lags that reach a position >= 0
    if constexpr (S > 1) {
        for (int t = threadIdx.x; t < 30 * nl + 5; t += VITG_THREADS) {
            const int l = t / 30 + 1, q = t % 30;
            tab[t] = t < 30 * nl ? Gb[(size_t)(p - l) * sd + ((q / LT_ROW) * L + (l - 1)) * LT_ROW + q % LT_ROW]
                                 : Gb[(size_t)(p - 1) * sd + 30 * L + (t - 30 * nl)];
        }
        __syncthreads();
    }
    auto lag = [&](int l, int a6, int b) -> double {
        if constexpr (S > 1) return tab[(l - 1) * 30 + a6 * LT_ROW + b];
        else return Gb[(size_t)(p - l) * sd + (a6 * L + (l - 1)) * LT_ROW + b];
    };
    auto marg = [&](int b) -> double {
        if constexpr (S > 1) return tab[30 * nl + b];
        else return Gb[(size_t)(p - 1) * sd + 30 * L + b];
    };
    const int r = blockIdx.x * VITG_THREADS + threadIdx.x;
    if (r >= pw) return;
    const int n = L - 1;
    const unsigned long long pk = S > 1 ? vitg_pack<S>(r, n) : 0;
    if constexpr (S > 1) {
        for (int k = 1; k <= n; k++)                          // the picks at p - 1 .. p - Le + 1: offered there, or nothing to do
            if (!((vitg_mask(m0, m1, k) >> vitg_slot(sp, vitg_digit<S>(pk, k, n))) & 1u)) return;
    }
    const uint32_t cm_p = vitg_mask(m0, m1, 0);
    double v[S];
#pragma unroll
    for (int x = 0; x < S; x++) {
        v[x] = 0.0;
        if (p < L ? x == 0 : (cm_old >> vitg_slot(sp, x)) & 1u) v[x] = Vc[r * S + x];
    }
    const int npre = L - 1 < p ? L - 1 : p;                   // lags of the prefix
#pragma unroll
    for (int d = 0; d < S; d++) {
        const int b = vitg_slot(sp, d);
        if (!((cm_p >> b) & 1u)) continue;
        double w = 0.0;
        if (marginal_term) w += marg(b);
        for (int l = 1; l <= npre; l++) {
            const int a6 = p - l == 0 ? 5 : vitg_slot(sp, vitg_digit<S>(pk, l, n));
            w += lag(l, a6, b);
        }
        double best = 0.0;
        int arg = -1;
        if (p < L) {
            best = v[0] + w;                                  // warm-up: the one predecessor, no lag Le
            arg = 0;
        } else {
#pragma unroll
            for (int x = 0; x < S; x++) {
                const int sx = vitg_slot(sp, x);
                if (!((cm_old >> sx) & 1u)) continue;
                const double cand = v[x] + (w + lag(L, p == L ? 5 : sx, b));
                if (arg < 0 || cand > best) { best = cand; arg = x; }
            }
        }
        Vn[d * pw + r] = best;
        if constexpr (!KEEP) bp[d * pw + r] = (uint8_t)arg;
    }
}

// block-wide: of the threads' (score, state) the largest score, of two equal scores the smaller state; bi < 0 = none
template <int T> __device__ __forceinline__ void vitg_best(double &bv, int &bi, double *rv, int *ri)
{
    const int tid = threadIdx.x;
    rv[tid] = bv;
    ri[tid] = bi;
    __syncthreads();
    for (int h = T / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            const double ov = rv[tid + h];
            const int oi = ri[tid + h], mi = ri[tid];
            if (oi >= 0 && (mi < 0 || ov > rv[tid] || (ov == rv[tid] && oi < mi))) { rv[tid] = ov; ri[tid] = oi; }
        }
        __syncthreads();
    }
    bv = rv[0];
    bi = ri[0];
}

// V: the score row of position N; m0, m1: the masks of positions N .. N - Le + 1
template <int S>
__global__ void __launch_bounds__(VITG_THREADS)
k_vitg_end(const double *__restrict__ V, int states, int L, uint32_t sp, unsigned long long m0, unsigned long long m1,
           double *__restrict__ pv, int32_t *__restrict__ pj)
{
    __shared__ double rv[VITG_THREADS];
    __shared__ int ri[VITG_THREADS];
    double bv = 0.0;
    int bi = -1;
    for (int i = 0; i < GH_VITG_END_CHUNK / VITG_THREADS; i++) {
        const int j = (int)blockIdx.x * GH_VITG_END_CHUNK + i * VITG_THREADS + (int)threadIdx.x;
        if (j >= states) break;
        bool ok = true;
        if constexpr (S > 1) {
            const unsigned long long pk = vitg_pack<S>(j, L);
            for (int k = 0; k < L; k++) ok = ok && ((vitg_mask(m0, m1, k) >> vitg_slot(sp, vitg_digit<S>(pk, k + 1, L))) & 1u);
        }
        if (ok) {
            const double v = V[j];
            if (bi < 0 || v > bv) { bv = v; bi = j; }
        }
    }
    vitg_best<VITG_THREADS>(bv, bi, rv, ri);
    if (threadIdx.x == 0) {
        pv[blockIdx.x] = bv;
        pj[blockIdx.x] = bi;
    }
}

__global__ void __launch_bounds__(VITG_END_THREADS)
k_vitg_end2(const double *__restrict__ pv, const int32_t *__restrict__ pj, int parts, uint32_t U, vit_out *__restrict__ out)
{
    __shared__ double rv[VITG_END_THREADS];
    __shared__ int ri[VITG_END_THREADS];
    double bv = 0.0;
    int bi = -1;
    for (int q = threadIdx.x; q < parts; q += VITG_END_THREADS) {     // (a chunk's states lie below the next chunk's: ascending j)
        const int j = pj[q];
        if (j >= 0) {
            const double v = pv[q];
            if (bi < 0 || v > bv) { bv = v; bi = j; }
        }
    }
    vitg_best<VITG_END_THREADS>(bv, bi, rv, ri);
    if (threadIdx.x == 0) {
        out->U = U;
        out->hole_at = 0;
        out->end_state = bi;
        out->ll = bv;
    }
}

__global__ void __launch_bounds__(64)
k_vitg_trace(const uint8_t *__restrict__ bp, size_t states, int N, int S, int pw, uint32_t sp, symmap sm, const vit_out *__restrict__ out,
             uint8_t *__restrict__ path)
{
    if (threadIdx.x) return;
    int j = out->end_state;
    if (j < 0) return;                                        // (no reachable state: the host has met the hole before any launch)
    path[0] = SYM_US;
    for (int q = N; q >= 1; q--) {
        path[q] = (uint8_t)vsym(sm, vitg_slot(sp, j / pw));
        const int x = bp[(size_t)q * states + j];
        if (x >= S) return;                                   // (a reachable state's byte is a digit: never leave the rows)
        j = (j % pw) * S + x;
    }
}

// host ----------------------------------------------------------------------------------------
static const char VITG_SCRATCH[] = "the grid decoder's scratch, whose back-pointers grow with N * states and whose score rows with states,";

// f(std::integral_constant<int, S>): one launch site per kernel, instantiated for the five S
template <typename F> static void vitg_with_S(int S, F &&f)
{
    switch (S) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    default: f(std::integral_constant<int, 5>()); break;
    }
}

// what a grid call opens with (the decoder here, the max-marginals of viterbi_grid_marg.hpp): the candidate bytes at home, and what
// the host forms from them
struct vitg_win {
    std::vector<uint8_t> cm5;  // [N + 1] candidate bits over the compact indices
    uint32_t U = 0;
    uint32_t sp = 0;           // digit -> compact index b5, ascending: the candidate order
    uint32_t d0 = 0;           // positions <= 0 offer digit 0 alone
    int S = 0, L = 0;
    int pw = 0;                // S^(Le-1)
    int hole = 0;              // the first position that offers nothing: the call ends there
    int64_t states = 0;
    uint32_t at(int p) const { return p >= 1 ? (uint32_t)cm5[p] : d0; }
    // the masks of positions p, p-1, ... p-Le+1 at bits 0, 5, ... of m[0], from the thirteenth on of m[1]; S = 1 has no digits
    void masks(int p, unsigned long long m[2]) const
    {
        m[0] = m[1] = 0;
        for (int k = 0; k < (S > 1 ? L : 1); k++) m[k / 12] |= (unsigned long long)at(p - k) << (5 * (k % 12));
    }
};

// the candidate bytes first: they decide whether the grid serves this window at all.  A hole (w->hole) ends the call before any
// step is launched and before anything large is reserved; gh_viterbi_grid_info then names the small reservation.
static int vitg_open(gh_handle *h, vitg_win *w, const char *who)
{
    const int N = h->N, L = chain_lags(h);
    int rc = ensure_marg(h);                                    // (k_vit_cands reads minfo)
    if (rc) return rc;
    const size_t small = vitg_layout(nullptr, N, 0, 0).total;
    if ((rc = scratch_reserve(h, &h->vit, small, VITG_SCRATCH))) return rc;
    const vitg_bufs s = vitg_layout(h->vit.buf, N, 0, 0);
    hipLaunchKernelGGL(k_vit_cands, dim3((unsigned)std::min<size_t>(((size_t)N + 256) / 256, 1024)), dim3(256), 0, h->stream,
                       (const double *)h->minfo, N, h->sm, s.cm5, s.cm);
    if ((rc = post_launch(h, "k_vit_cands"))) return rc;
    std::vector<uint8_t> &cm5 = w->cm5;
    cm5.assign((size_t)N + 1, 0);
    HIPCHK(hipMemcpyAsync(cm5.data(), s.cm5, (size_t)N + 1, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    uint32_t U = 0;
    int hole = 0;
    for (int p = N; p >= 1; p--) {
        U |= cm5[p];
        if (!cm5[p]) hole = p;
    }
    const int S = __builtin_popcount(U);
    w->U = U; w->S = S; w->L = L;
    if (S == 0) {                                             // nothing offered anywhere: the hole is the first position
        w->hole = 1;
        h->vitg_last[0] = 0; h->vitg_last[1] = L; h->vitg_last[2] = 0; h->vitg_last[3] = (int64_t)h->vit.cap;
        return GH_OK;
    }
    int64_t states = 1;
    for (int k = 0; k < L && S > 1 && states <= GH_VITERBI_GRID_MAX_STATES; k++) states *= S;
    if (states > GH_VITERBI_GRID_MAX_STATES) {
        char cnt[32];
        const double full = pow((double)S, (double)L);
        snprintf(cnt, sizeof cnt, full < 1e15 ? "%.0f" : "%.3g", full);
        return fail(GH_ERR_ARG, "%s: S = %d candidate symbols and Le = min(L, N) = %d make %s states, more than the %d the grid decoder "
                    "serves: lower L, or use the beam (--beam, gh_beam_paths)", who, S, L, cnt, GH_VITERBI_GRID_MAX_STATES);
    }
    w->states = states;
    if (hole) {                                               // the call ends here: no step is launched, nothing else is written
        w->hole = hole;
        h->vitg_last[0] = S; h->vitg_last[1] = L; h->vitg_last[2] = states; h->vitg_last[3] = (int64_t)small;
        return GH_OK;
    }
    for (int b5 = 0, d = 0; b5 < 5; b5++)
        if ((U >> b5) & 1u) w->sp |= (uint32_t)b5 << (3 * d++);
    w->d0 = 1u << (w->sp & 7);
    w->pw = (int)(states / S);
    return GH_OK;
}

// one exact decoding of the tensor as it stands on the grid: the path row stays in the handle's scratch (`b`), *ho = hole, score, U
static int vitg_run(gh_handle *h, vitg_bufs *b, vit_out *ho, const char *who)
{
    const int N = h->N;
    vitg_win w;
    int rc = vitg_open(h, &w, who);
    if (rc) return rc;
    *ho = vit_out{};
    ho->U = w.U;
    ho->hole_at = w.hole;
    if (w.hole) return GH_OK;
    const int S = w.S, L = w.L, pw = w.pw;
    const uint32_t U = w.U, sp = w.sp;
    const int64_t states = w.states;
    const size_t ns = (size_t)states, table_doubles = (size_t)N * beam_src_doubles(L);
    const size_t need = vitg_layout(nullptr, N, table_doubles, ns).total;
    if ((rc = scratch_reserve(h, &h->vit, need, VITG_SCRATCH))) return rc;
    *b = vitg_layout(h->vit.buf, N, table_doubles, ns);
    if ((rc = chain_table_build(h, L, b->Gb))) return rc;
    HIPCHK(hipMemsetAsync(b->rows, 0, sizeof(double), h->stream));      // the one prefix at p = 0: every digit 0, score +0.0

    const unsigned nb = (unsigned)((pw + VITG_THREADS - 1) / VITG_THREADS);
    unsigned long long m[2];
    for (int p = 1; p <= N; p++) {
        w.masks(p, m);
        const uint32_t cm_old = w.at(p - L);
        const double *Vc = b->rows + (size_t)((p - 1) & 1) * ns;
        double *Vn = b->rows + (size_t)(p & 1) * ns;
        uint8_t *bp = b->bp + (size_t)p * ns;
        vitg_with_S(S, [&](auto sc) {
            hipLaunchKernelGGL(k_vitg_step<decltype(sc)::value>, dim3(nb), dim3(VITG_THREADS), 0, h->stream, (const double *)b->Gb, p, L, pw,
                               h->cfg.marginal_term, sp, m[0], m[1], cm_old, Vc, Vn, bp);
        });
        if ((rc = post_launch(h, "k_vitg_step"))) return rc;
    }
    w.masks(N, m);
    vitg_with_S(S, [&](auto sc) {
        hipLaunchKernelGGL(k_vitg_end<decltype(sc)::value>, dim3((unsigned)b->parts), dim3(VITG_THREADS), 0, h->stream,
                           (const double *)(b->rows + (size_t)(N & 1) * ns), (int)states, L, sp, m[0], m[1], b->pv, b->pj);
    });
    if ((rc = post_launch(h, "k_vitg_end"))) return rc;
    hipLaunchKernelGGL(k_vitg_end2, dim3(1), dim3(VITG_END_THREADS), 0, h->stream, (const double *)b->pv, (const int32_t *)b->pj, (int)b->parts,
                       U, b->out);
    if ((rc = post_launch(h, "k_vitg_end2"))) return rc;
    hipLaunchKernelGGL(k_vitg_trace, dim3(1), dim3(64), 0, h->stream, (const uint8_t *)b->bp, ns, N, S, pw, sp, h->sm, (const vit_out *)b->out,
                       b->path);
    if ((rc = post_launch(h, "k_vitg_trace"))) return rc;
    HIPCHK(hipMemcpyAsync(ho, b->out, sizeof *ho, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->vitg_last[0] = S; h->vitg_last[1] = L; h->vitg_last[2] = states; h->vitg_last[3] = (int64_t)need;
    return GH_OK;
}

extern "C" int gh_viterbi_path_grid(gh_t *h, uint8_t *path_out, double *ll_chain, int *hole_at)
{
    if (!h || !path_out || !ll_chain || !hole_at) return fail(GH_ERR_ARG, "null argument");
    int rc = decode_check(h, "gh_viterbi_path_grid");
    if (rc) return rc;
    if (set_dev(h)) return GH_ERR_HIP;
    vitg_bufs b;
    vit_out ho;
    if ((rc = vitg_run(h, &b, &ho, "gh_viterbi_path_grid"))) return rc;
    *hole_at = ho.hole_at;
    if (ho.hole_at) return GH_OK;
    HIPCHK(hipMemcpyAsync(path_out, b.path, (size_t)h->N + 1, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *ll_chain = ho.ll;
    return GH_OK;
}

extern "C" int gh_viterbi_spin_grid(gh_t *h, int max_paths, double min_remove, uint8_t *paths_out, gh_path_rec *recs, double *ll_chain,
                                    int *n_out, int *hole_at)
{
    if (!h || !paths_out || !recs || !n_out || !hole_at) return fail(GH_ERR_ARG, "null argument");
    if (max_paths < 0) return fail(GH_ERR_ARG, "max_paths < 0");
    int rc = decode_check(h, "gh_viterbi_spin_grid");
    if (rc) return rc;
    if (set_dev(h)) return GH_ERR_HIP;
    return decode_spin(h, max_paths, min_remove, paths_out, recs, ll_chain, n_out, hole_at, [&](decoded *d) -> int {
        vitg_bufs b;
        vit_out ho;
        if ((rc = vitg_run(h, &b, &ho, "gh_viterbi_spin_grid"))) return rc;
        d->hole = ho.hole_at;
        d->d_path = b.path;
        d->ll = ho.ll;                                          // (it came home with vit_out)
        return GH_OK;
    });
}

extern "C" int gh_viterbi_grid_info(const gh_t *h, int64_t out[4])
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    for (int q = 0; q < 4; q++) out[q] = h->vitg_last[q];
    return GH_OK;
}
