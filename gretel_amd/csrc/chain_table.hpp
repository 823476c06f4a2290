// chain_table.hpp -- what the beam (beam.hpp) and the exact decoder (viterbi.hpp) share: the plain table of the chain likelihood
// both walk, and the host side both put around their walk (the refusals, the recovery loop).
//
//   k_beam_table  (parallel) a decoder's own plain table in its own scratch block, never the handle's G (which may be ranked, may
//                 carry the marginal term, may be mid-way through an incremental refresh):  per source position i one block of
//                 30 L + 6 doubles,  Gb[i][a6][l-1][b5] = lt_entry(bake_lm = 0)  and behind them what target i + 1 needs besides:
//                 its five log10 marginals (minfo[i+1][0..4]) and its candidate bits (minfo[i+1][10]).  With that header a
//                 walk's whole input is ONE contiguous stream in source order.  (The issue's sketch had the bare 30 L doubles
//                 and LT_PAD zero blocks behind N: the header saves the walk a second stream, and no reader overruns N sources.)
// ---------------------------------------------------------------------------------------------

#define BEAM_LDS_MAX (160 * 1024)  /* LDS one workgroup can have on gfx950 */

__host__ __device__ constexpr int beam_src_doubles(int L) { return 30 * L + 6; }

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

// A walk's barrier orders LDS only: __syncthreads() also waits for every global access in flight (vmcnt(0)), which would drain
// the loader's block and the step's back-pointer store twice a step.  Nothing k_beam_walk writes to global memory is read inside
// it, and what it reads there nobody writes, so the workgroup needs no order on global memory.  (Measured, DESIGN.md 4.9: by
// itself this did not move the time of a step -- the loader's own wait for its block still stands behind the back-pointer store.)
__device__ __forceinline__ void beam_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// host ----------------------------------------------------------------------------------------
// (lags beyond the window's first position are never summed: a table of min(L, N) lags gives the same weights)
static int chain_lags(const gh_handle *h) { return h->L < h->N ? h->L : h->N; }

// the table of the tensor as it stands for L lags: N * beam_src_doubles(L) doubles into Gb
static int chain_table_build(gh_handle *h, int L, double *Gb)
{
    int rc = ensure_marg(h);
    if (rc) return rc;
    const void *tb = tband_current(h);
    const size_t total = (size_t)h->N * beam_src_doubles(L);
    const unsigned nb = (unsigned)std::min<size_t>((total + 255) / 256, 256 * 16);
    with_storage(h, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(k_beam_table<T>, dim3(nb), dim3(256), 0, h->stream, (const T *)h->band, (const T *)tb, h->N, h->W, L, h->cfg.cond_mode,
                           h->cnt, h->nvalid, h->cmask, h->minfo, h->sm, Gb);
    });
    return post_launch(h, "k_beam_table");
}

// what neither decoder serves
static int decode_check(const gh_handle *h, const char *who)
{
    if (h->cfg.offer_zero)
        return fail(GH_ERR_ARG, "%s: the handle offers zero-count candidates (offer_zero), whose weights can be NaN (-inf + +inf): no order ranks them", who);
    if (h->band_zero) return fail(GH_ERR_STATE, "%s before any fill or import: the tensor holds no evidence", who);
    return GH_OK;
}

// The recovery loop around a decoder (the caller has checked its arguments and set the device): up to max_paths times decode the
// tensor as it stands, take the best path home, record it (gh_score_paths: hp_original under the snapshot) and reweight it.
// decode_one(&d) runs one decoding and says what came of it.
struct decoded {
    int hole;                  // the first position without a candidate, 0 = none; then:
    const uint8_t *d_path;     // the best path's row, on the device
    const double *d_ll;        // its ll_chain on the device (it comes home beside the path), or nullptr where the decoder
    double ll;                 // ... has brought it home already
};

// One recovered path's record and reweight, the same for every decoder and for gh_panel_viterbi_spin's windows: the record of
// `path` on the tensor as it stands (gh_score_paths: hp_original under the snapshot), the ratio, then the reweight.
static int decode_record(gh_handle *h, const uint8_t *path, double min_remove, gh_path_rec *r)
{
    int rc;
    gh_score_rec sr;
    if ((rc = gh_score_paths(h, path, 1, &sr, nullptr, nullptr, nullptr))) return rc;
    r->hp_current = sr.hp_current;
    r->hp_original = sr.hp_original;
    r->min_marginal = sr.min_marginal;
    r->ratio = sr.min_marginal < min_remove ? min_remove : sr.min_marginal;
    return gh_reweight_path(h, path, r->ratio, &r->magnitude);
}

template <typename F>
static int decode_spin(gh_handle *h, int max_paths, double min_remove, uint8_t *paths_out, gh_path_rec *recs, double *ll_chain,
                       int *n_out, int *hole_at, F &&decode_one)
{
    int rc;
    *n_out = 0; *hole_at = 0;
    if (max_paths == 0) return GH_OK;
    if (!h->have_orig && (rc = gh_snapshot_original(h))) return rc;
    const size_t n1 = (size_t)h->N + 1;
    for (int s = 0; s < max_paths; s++) {
        decoded d = {};
        if ((rc = decode_one(&d))) return rc;
        if (d.hole) { *hole_at = d.hole; break; }
        uint8_t *path = paths_out + n1 * s;
        HIPCHK(hipMemcpyAsync(path, d.d_path, n1, hipMemcpyDeviceToHost, h->stream));
        if (d.d_ll) HIPCHK(hipMemcpyAsync(&d.ll, d.d_ll, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if ((rc = decode_record(h, path, min_remove, &recs[s]))) return rc;
        if (ll_chain) ll_chain[s] = d.ll;
        *n_out = s + 1;
    }
    return GH_OK;
}
