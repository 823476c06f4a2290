// viterbi_grid_marg.hpp -- max-marginals on the grid (gh_viterbi_marginals_grid: include/gretel_hip.h; INTEGRATION.md "Max-marginals
// on the grid").  The definition -- F, B, M, the association of every addition, the output, the hole rule -- is
// gh_viterbi_marginals'; state index, digits, masks, table and the opening of a call are viterbi_grid.hpp's.  The discipline is
// the grid decoder's: ONE LAUNCH PER POSITION on the handle's stream, the launch boundary the only synchronisation, no workgroup
// waiting for another, no counter, nothing that could hang; the host does not wait between the steps.
//
//   k_vitg_step<S, KEEP = true> (viterbi_grid.hpp)  F_p, every row kept: step p reads row p - 1 and writes row p of the F block,
//                 nothing ping-pongs; no back-pointers, no end rule, no trace.
//   k_vitgm_back<S>  step p = N .. 1, the step's mirror image.  A thread owns q = j div S: the Le - 1 newest picks (positions
//                 p .. p-Le+2) that the S states q S + x at p share with their S successors c S^(Le-1) + q at p + 1.  It decodes
//                 q's digits once and tests each against its position's mask.  Per c in cm(p+1) it forms the successor's prefix
//                 P_c once (+0.0, the marginal term if the spec has it, lags 1 .. min(Le - 1, p + 1) of target p + 1 in that
//                 order) and reads Bn[c S^(Le-1) + q] -- adjacent threads read adjacent doubles; then per x offered at p - Le + 1
//                   B_p(q S + x) = max over c of  (P_c + T_Le[x][c]) + Bn[succ]     (the weight on the left, plain >, c ascending)
//                 without the lag-Le term while p + 1 < Le, with the '_' row where a lag reaches position 0, +0.0 at p = N:
//                 k_vit_back's arithmetic (viterbi_marg.hpp).  It writes S adjacent doubles of Bc; the two rows of B ping-pong in
//                 global memory.  The slice of the table the step reads -- of source p + 1 - l only lag l, and target p + 1's
//                 five marginals -- is staged into LDS per workgroup, as k_vitg_step does it.
//                 In the same kernel F_p(j) + B_p(j), ONE addition, and its maximum per newest pick over the workgroup's states:
//                 within a wavefront by exchange, across the four through LDS, NaN = nothing seen yet; five doubles go to the
//                 partials block [p][workgroup][5].  No pass over the N * states block follows.
//   k_vitgm_mm    one launch at the end: a workgroup per position at a time reduces the position's partials and writes mm and cm
//                 as k_vit_mm does.  A maximum does not depend on the order: the bits are the definition's.
// REACHABILITY COMES FROM THE MASKS ALONE.  The grid step never writes an unreachable entry and the handle's block is shared by
// every decoder and never cleared: unreachable entries of F and B hold bytes of earlier calls.  The backward step reads F[j] and
// Bn[succ] only behind the mask tests that make j and succ reachable, and a thread that fails them contributes NaN.
// S = 1 is one state whatever L is (no digits, no masks, L may exceed 24): its one thread reads the table from global memory.
// ---------------------------------------------------------------------------------------------

#define VITGM_THREADS GH_VITGM_THREADS
#define VITGM_WAVE 64

static_assert(VITGM_THREADS == VITG_THREADS && VITGM_THREADS % VITGM_WAVE == 0, "the step's workgroup; whole wavefronts");

// m <- max(m, v), NaN = none (k_vit_mm's rule)
__device__ __forceinline__ void vitgm_take(double &m, double v)
{
    if (v == v && !(m >= v)) m = v;
}

template <int S>
__global__ void __launch_bounds__(VITGM_THREADS)
k_vitgm_back(const double *__restrict__ Gb, int p, int N, int L, int pw, int marginal_term, uint32_t sp, unsigned long long m0,
             unsigned long long m1, uint32_t cm_up, const double *__restrict__ F, const double *__restrict__ Bn, double *__restrict__ Bc,
             double *__restrict__ part)
{
    __shared__ double tab[S > 1 ? 30 * VITG_MAX_LE + 5 : 1];  // [lag l - 1][a6][b5] of source p + 1 - l, then target p + 1's marginals
    __shared__ double red[VITGM_THREADS / VITGM_WAVE][5];
    const int sd = beam_src_doubles(L);
    const int tp = p + 1;                                     // the target whose weights this step adds (none at p = N)
    const int nl = p < N ? (L < tp ? L : tp) : 0;             // its lags that reach a position >= 0
    if constexpr (S > 1) {
        if (p < N) {
            for (int t = threadIdx.x; t < 30 * nl + 5; t += VITGM_THREADS) {
                const int l = t / 30 + 1, q = t % 30;
                tab[t] = t < 30 * nl ? Gb[(size_t)(tp - l) * sd + ((q / LT_ROW) * L + (l - 1)) * LT_ROW + q % LT_ROW]
                                     : Gb[(size_t)(tp - 1) * sd + 30 * L + (t - 30 * nl)];
            }
        }
        __syncthreads();
    }
    auto lag = [&](int l, int a6, int b) -> double {
        if constexpr (S > 1) return tab[(l - 1) * 30 + a6 * LT_ROW + b];
        else return Gb[(size_t)(tp - l) * sd + (a6 * L + (l - 1)) * LT_ROW + b];
    };
    auto marg = [&](int b) -> double {
        if constexpr (S > 1) return tab[30 * nl + b];
        else return Gb[(size_t)(tp - 1) * sd + 30 * L + b];
    };
    const double none = __longlong_as_double(0x7ff8000000000000ll);
    const int q = blockIdx.x * VITGM_THREADS + threadIdx.x;
    const int n = L - 1;
    bool live = q < pw;
    unsigned long long pk = 0;
    if constexpr (S > 1) {
        if (live) {
            pk = vitg_pack<S>(q, n);
            for (int k = 1; k <= n; k++)                      // the picks at p .. p - Le + 2: offered there, or nothing to do
                live = live && ((vitg_mask(m0, m1, k - 1) >> vitg_slot(sp, vitg_digit<S>(pk, k, n))) & 1u);
        }
    }
    double top[S];                                            // the largest F + B per newest pick among this thread's states
#pragma unroll
    for (int d = 0; d < S; d++) top[d] = none;
    if (live) {
        const uint32_t cm_x = S > 1 ? vitg_mask(m0, m1, n) : 1u << (sp & 7);      // what position p - Le + 1 offers
        double b[S];
        bool have[S];
#pragma unroll
        for (int x = 0; x < S; x++) {
            b[x] = 0.0;                                       // B_N = +0.0
            have[x] = false;
        }
        if (p < N) {
            const int npre = L - 1 < tp ? L - 1 : tp;         // lags of the successor's prefix
            const bool lagL = tp >= L;                        // target p + 1 has a lag Le
#pragma unroll
            for (int c = 0; c < S; c++) {
                const int sc = vitg_slot(sp, c);
                if (!((cm_up >> sc) & 1u)) continue;
                double w = 0.0;
                if (marginal_term) w += marg(sc);
                for (int l = 1; l <= npre; l++) {
                    const int a6 = tp - l == 0 ? 5 : vitg_slot(sp, vitg_digit<S>(pk, l, n));
                    w += lag(l, a6, sc);
                }
                const double bn = Bn[(size_t)c * pw + q];
#pragma unroll
                for (int x = 0; x < S; x++) {
                    const int sx = vitg_slot(sp, x);
                    if (!((cm_x >> sx) & 1u)) continue;
                    double wx = w;
                    if (lagL) wx += lag(L, tp == L ? 5 : sx, sc);
                    const double cand = wx + bn;
                    if (!have[x] || cand > b[x]) { b[x] = cand; have[x] = true; }
                }
            }
        }
        const int d1 = n >= 1 ? vitg_digit<S>(pk, 1, n) : 0;  // the newest pick where q has one; at Le = 1 it is x itself
#pragma unroll
        for (int x = 0; x < S; x++) {
            if (!((cm_x >> vitg_slot(sp, x)) & 1u)) continue;
            const size_t j = (size_t)q * S + x;
            Bc[j] = b[x];
            const double sum = F[j] + b[x];
            const int d = n >= 1 ? d1 : x;
#pragma unroll
            for (int e = 0; e < S; e++)
                if (e == d) vitgm_take(top[e], sum);
        }
    }
    // the workgroup's maxima: by exchange within a wavefront, through LDS across them
#pragma unroll
    for (int d = 0; d < S; d++)
        for (int off = VITGM_WAVE / 2; off > 0; off >>= 1) vitgm_take(top[d], __shfl_xor(top[d], off));
    if (threadIdx.x % VITGM_WAVE == 0) {
#pragma unroll
        for (int d = 0; d < 5; d++) red[threadIdx.x / VITGM_WAVE][d] = none;
#pragma unroll
        for (int d = 0; d < S; d++) red[threadIdx.x / VITGM_WAVE][d] = top[d];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        double m = none;
        for (int w = 0; w < VITGM_THREADS / VITGM_WAVE; w++) vitgm_take(m, red[w][threadIdx.x]);
        part[(size_t)blockIdx.x * 5 + threadIdx.x] = m;
    }
}

// part: [N][wgs][5], of which a position's first nb entries are filled; one position a workgroup at a time
__global__ void __launch_bounds__(256)
k_vitgm_mm(const double *__restrict__ part, const uint8_t *__restrict__ cm5, int N, int S, size_t wgs, int nb, uint32_t sp, symmap sm,
           double *__restrict__ mm, uint8_t *__restrict__ cm)
{
    __shared__ double red[5][256];
    const int tid = threadIdx.x;
    const double none = __longlong_as_double(0x7ff8000000000000ll);
    for (int p = blockIdx.x; p <= N; p += gridDim.x) {
#pragma unroll
        for (int d = 0; d < 5; d++) {
            double m = none;
            if (d < S && p >= 1) {
                const double *blk = part + (size_t)(p - 1) * wgs * 5;
                for (int w = tid; w < nb; w += 256) vitgm_take(m, blk[(size_t)w * 5 + d]);
            }
            red[d][tid] = m;
        }
        __syncthreads();
        for (int h = 128; h >= 1; h >>= 1) {
            if (tid < h) {
#pragma unroll
                for (int d = 0; d < 5; d++) vitgm_take(red[d][tid], red[d][tid + h]);
            }
            __syncthreads();
        }
        if (tid < GH_NSYM) mm[(size_t)p * GH_NSYM + tid] = -INFINITY;
        __syncthreads();
        const uint32_t c5 = p >= 1 ? (uint32_t)cm5[p] : 0u;
        if (tid < S && p >= 1) {
            const int sc = vitg_slot(sp, tid);
            const double v = red[tid][0];
            if ((c5 >> sc) & 1u) mm[(size_t)p * GH_NSYM + vsym(sm, sc)] = v == v ? v : -INFINITY;
        }
        if (tid == 0) {
            uint32_t c7 = 0;
#pragma unroll
            for (int b = 0; b < 5; b++)
                if ((c5 >> b) & 1u) c7 |= 1u << vsym(sm, b);
            cm[p] = (uint8_t)c7;
        }
        __syncthreads();
    }
}

// host ----------------------------------------------------------------------------------------
static const char VITGM_SCRATCH[] = "the grid max-marginals' scratch, whose kept rows of F grow with N * states,";

extern "C" int gh_viterbi_marginals_grid(gh_t *h, double *mm, uint8_t *cm, int *hole_at)
{
    if (!h || !mm || !cm || !hole_at) return fail(GH_ERR_ARG, "null argument");
    int rc = decode_check(h, "gh_viterbi_marginals_grid");
    if (rc) return rc;
    if (set_dev(h)) return GH_ERR_HIP;
    const int N = h->N;
    vitg_win w;
    if ((rc = vitg_open(h, &w, "gh_viterbi_marginals_grid"))) return rc;
    *hole_at = w.hole;
    if (w.hole) return GH_OK;                                 // (no step is launched, nothing else is reserved)
    const int S = w.S, L = w.L, pw = w.pw;
    const size_t ns = (size_t)w.states, table_doubles = (size_t)N * beam_src_doubles(L);
    const size_t need = vitgm_layout(nullptr, N, table_doubles, ns).total;
    if ((rc = scratch_reserve(h, &h->vit, need, VITGM_SCRATCH))) return rc;
    const vitgm_bufs b = vitgm_layout(h->vit.buf, N, table_doubles, ns);
    if ((rc = chain_table_build(h, L, b.Gb))) return rc;
    // (a block that had to grow is a new one: the candidate bytes k_vitgm_mm reads go back from the host's copy)
    HIPCHK(hipMemcpyAsync(b.cm5, w.cm5.data(), (size_t)N + 1, hipMemcpyHostToDevice, h->stream));
    double *F0 = b.F + (size_t)N * ns;                        // the one prefix at p = 0: every digit 0, score +0.0
    HIPCHK(hipMemsetAsync(F0, 0, sizeof(double), h->stream));

    const unsigned nb = (unsigned)((pw + VITGM_THREADS - 1) / VITGM_THREADS);
    unsigned long long m[2];
    for (int p = 1; p <= N; p++) {                            // F_p, every row kept
        w.masks(p, m);
        const double *Vc = p >= 2 ? b.F + (size_t)(p - 2) * ns : F0;
        double *Vn = b.F + (size_t)(p - 1) * ns;
        vitg_with_S(S, [&](auto sc) {
            hipLaunchKernelGGL((k_vitg_step<decltype(sc)::value, true>), dim3(nb), dim3(VITG_THREADS), 0, h->stream, (const double *)b.Gb, p, L,
                               pw, h->cfg.marginal_term, w.sp, m[0], m[1], w.at(p - L), Vc, Vn, (uint8_t *)nullptr);
        });
        if ((rc = post_launch(h, "k_vitg_step"))) return rc;
    }
    for (int p = N; p >= 1; p--) {                            // B_p, and the partial maxima of F_p + B_p
        w.masks(p, m);
        const uint32_t cm_up = p < N ? (uint32_t)w.cm5[p + 1] : 0u;
        const double *Bn = b.B + (size_t)((p + 1) & 1) * ns;
        double *Bc = b.B + (size_t)(p & 1) * ns;
        vitg_with_S(S, [&](auto sc) {
            hipLaunchKernelGGL(k_vitgm_back<decltype(sc)::value>, dim3(nb), dim3(VITGM_THREADS), 0, h->stream, (const double *)b.Gb, p, N, L, pw,
                               h->cfg.marginal_term, w.sp, m[0], m[1], cm_up, (const double *)(b.F + (size_t)(p - 1) * ns), Bn, Bc,
                               b.part + (size_t)(p - 1) * b.wgs * 5);
        });
        if ((rc = post_launch(h, "k_vitgm_back"))) return rc;
    }
    hipLaunchKernelGGL(k_vitgm_mm, dim3((unsigned)std::min(N + 1, 4096)), dim3(256), 0, h->stream, (const double *)b.part, (const uint8_t *)b.cm5,
                       N, S, b.wgs, (int)nb, w.sp, h->sm, b.mm, b.cm);
    if ((rc = post_launch(h, "k_vitgm_mm"))) return rc;
    HIPCHK(hipMemcpyAsync(mm, b.mm, ((size_t)N + 1) * GH_NSYM * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cm, b.cm, (size_t)N + 1, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->vitg_last[0] = S; h->vitg_last[1] = L; h->vitg_last[2] = w.states; h->vitg_last[3] = (int64_t)need;
    return GH_OK;
}
