// viterbi_masked.hpp -- exact decoding under per-position allele masks (gh_viterbi_path_masked, gh_viterbi_masked_info:
// include/gretel_hip.h, where the definition stands; INTEGRATION.md "Constrained decoding").  The candidate set of a position does
// not depend on the history, so a mask acts on reachability alone: cm'(p) = cm(p) & allow[p], and the scores, the state space
// (that of the UNMASKED window), the tie rules and the cap are gh_viterbi_path's.  Many constraint sets over one window are
// independent workgroups over ONE chain table, built once a call: the shape of the panel decoders (viterbi_panel.hpp) with one
// table instead of one per window.  Nothing depends on another workgroup: a grid larger than the card drains in any order.
//
//   k_vit_walk_masked   grid = n_sets, one workgroup of VIT_THREADS per set, the dynamic LDS of k_vit_walk.  The step is
//                       vit_walk_body's (viterbi_panel.hpp) with MASKED = true: the table's candidate bits meet the set's allowed
//                       bits before the hole test and before `hist` is shifted.  The masks arrive compacted to the five candidate
//                       slots (the b5 indices the table uses), one byte per set and position, made on the host; they reach the
//                       step through a window of two chunks in LDS that is refilled a chunk ahead (vit_walk_body), so the N
//                       dependent steps do not each wait for a global load of their own.  A workgroup that meets its hole writes
//                       its own hole_at and leaves.
//   k_vit_trace_masked  grid = n_sets: vit_trace_body over that set's blocks, into the set's row of a contiguous path block and
//                       its vit_out.  Sets with a hole return at once.
//
// Home: the vit_outs in one copy; the host then knows the holes; the path rows in one copy where no set met one, one copy per run
// of hole-free neighbours otherwise.  A set's scratch is laid out by vitx_layout (scratch_layout.hpp).
// ---------------------------------------------------------------------------------------------

template <bool STAGED>
__global__ void __launch_bounds__(VIT_THREADS)
k_vit_walk_masked(const double *__restrict__ Gb, int N, int L, int S, int states, int marginal_term, uint32_t U,
                  uint8_t *__restrict__ bp, size_t bps, double *__restrict__ vend, uint8_t *__restrict__ okend, vit_out *__restrict__ outs,
                  const uint8_t *__restrict__ a5)
{
    const size_t set = blockIdx.x;
    vit_walk_body<STAGED, false, true>(Gb, N, L, S, states, marginal_term, U, bp + set * bps, vend + set * (size_t)states,
                                       okend + set * (size_t)states, outs + set, a5 + set * ((size_t)N + 1));
}

__global__ void __launch_bounds__(VIT_THREADS)
k_vit_trace_masked(const uint8_t *__restrict__ bp, size_t bps, const double *__restrict__ vend, const uint8_t *__restrict__ okend, int N,
                   int L, int S, int states, int chunk, uint32_t U, symmap sm, vit_out *__restrict__ outs, uint8_t *__restrict__ paths)
{
    const size_t set = blockIdx.x;
    vit_trace_body(bp + set * bps, vend + set * (size_t)states, okend + set * (size_t)states, N, L, S, states, chunk, U, sm, outs + set,
                   paths + set * ((size_t)N + 1));
}

// host ---------------------------------------------------------------------------------------- (vitx_bufs: scratch_layout.hpp)
// allow bytes over the seven symbols -> bits over the compact indices, as the table's candidate word has them (position 0: ignored)
static void vitx_compact(const gh_handle *h, const uint8_t *allow, size_t cells, size_t n1, uint8_t *a5)
{
    for (size_t q = 0; q < cells; q++) {
        uint32_t r = 0;
        for (int b5 = 0; b5 < 5; b5++) r |= (((uint32_t)allow[q] >> h->cfg.cand_order[b5]) & 1u) << b5;
        a5[q] = q % n1 == 0 ? 31 : (uint8_t)r;
    }
}

extern "C" int gh_viterbi_path_masked(gh_t *h, const uint8_t *allow, int n_sets, uint8_t *paths_out, double *ll_chain, int *hole_at)
{
    static const char who[] = "gh_viterbi_path_masked";
    if (!h || !allow || !paths_out || !ll_chain || !hole_at) return fail(GH_ERR_ARG, "null argument");
    if (n_sets < 0 || n_sets > GH_MASKED_MAX_SETS) return fail(GH_ERR_ARG, "%s: n_sets = %d is outside 0..%d", who, n_sets, GH_MASKED_MAX_SETS);
    const int N = h->N, L = chain_lags(h);
    const size_t n1 = (size_t)N + 1, cells = (size_t)n_sets * n1;
    for (size_t q = 0; q < cells; q++)
        if (allow[q] & 0x80)
            return fail(GH_ERR_ARG, "%s: allow[%zu][%zu] = 0x%02x has bit 7 set (bits 0..6 are the symbols ACGTN-_)", who, q / n1, q % n1, allow[q]);
    int rc = decode_check(h, who);
    if (rc) return rc;
    if (set_dev(h)) return GH_ERR_HIP;
    int ns;
    vit_out ho;
    if ((rc = vit_open(h, &ho, who, &ns))) return rc;           // (a window beyond the cap is refused whatever n_sets is)
    if (!n_sets) {                                              // nothing asked: nothing written
        h->vitx_last[0] = 0; h->vitx_last[1] = 0; h->vitx_last[2] = 0; h->vitx_last[3] = (int64_t)h->vit.cap;
        return GH_OK;
    }
    if (!ns) {                                                  // nothing offered anywhere: the hole is position 1, for every set
        for (int s = 0; s < n_sets; s++) hole_at[s] = 1;
        h->vitx_last[0] = n_sets; h->vitx_last[1] = n_sets; h->vitx_last[2] = 0; h->vitx_last[3] = (int64_t)h->vit.cap;
        return GH_OK;
    }
    const uint32_t U = ho.U;
    const int S = __builtin_popcount(U);
    const size_t table_doubles = (size_t)N * beam_src_doubles(L);
    const size_t need = vitx_layout(nullptr, N, table_doubles, ns, n_sets).total;
    if ((rc = scratch_reserve(h, &h->vit, need, VIT_SCRATCH))) return rc;
    const vitx_bufs b = vitx_layout(h->vit.buf, N, table_doubles, ns, n_sets);
    if ((rc = chain_table_build(h, L, b.Gb))) return rc;
    std::vector<uint8_t> a5(cells);                             // (lives until the last synchronisation below)
    vitx_compact(h, allow, cells, n1, a5.data());
    HIPCHK(hipMemcpyAsync(b.a5, a5.data(), cells, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(b.outs, 0, (size_t)n_sets * sizeof(vit_out), h->stream));

    const size_t rows = 2 * (size_t)ns * 8;
    if (!vit_no_stage() && L <= VIT_MAX_LE) {                   // (a longer state has S = 1: its ring need not fit)
        const size_t lds = rows + (size_t)(L + 1) * beam_src_doubles(L) * 8;
        lds_limit<k_vit_walk_masked<true>>(lds, h->dev);
        hipLaunchKernelGGL(k_vit_walk_masked<true>, dim3(n_sets), dim3(VIT_THREADS), lds, h->stream, (const double *)b.Gb, N, L, S, ns,
                           h->cfg.marginal_term, U, b.bp, b.bps, b.vend, b.okend, b.outs, (const uint8_t *)b.a5);
    } else {
        lds_limit<k_vit_walk_masked<false>>(rows, h->dev);
        hipLaunchKernelGGL(k_vit_walk_masked<false>, dim3(n_sets), dim3(VIT_THREADS), rows, h->stream, (const double *)b.Gb, N, L, S, ns,
                           h->cfg.marginal_term, U, b.bp, b.bps, b.vend, b.okend, b.outs, (const uint8_t *)b.a5);
    }
    if ((rc = post_launch(h, "k_vit_walk_masked"))) return rc;
    int chunk = VIT_TRACE_BYTES / ns;
    if (chunk > VIT_TRACE_POS) chunk = VIT_TRACE_POS;
    const size_t tlds = (size_t)chunk * ns + 8;
    lds_limit<k_vit_trace_masked>(tlds, h->dev);
    hipLaunchKernelGGL(k_vit_trace_masked, dim3(n_sets), dim3(VIT_THREADS), tlds, h->stream, (const uint8_t *)b.bp, b.bps,
                       (const double *)b.vend, (const uint8_t *)b.okend, N, L, S, ns, chunk, U, h->sm, b.outs, b.paths);
    if ((rc = post_launch(h, "k_vit_trace_masked"))) return rc;
    std::vector<vit_out> outs((size_t)n_sets);
    HIPCHK(hipMemcpyAsync(outs.data(), b.outs, (size_t)n_sets * sizeof(vit_out), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    int holes = 0;
    for (int s = 0; s < n_sets; s++) {
        hole_at[s] = outs[s].hole_at;
        if (outs[s].hole_at) holes++;
        else ll_chain[s] = outs[s].ll;
    }
    // the path rows: one copy per run of hole-free neighbours (one copy in all where no set met a hole)
    for (int s = 0; s < n_sets;) {
        if (outs[s].hole_at) { s++; continue; }
        int e = s;
        while (e < n_sets && !outs[e].hole_at) e++;
        HIPCHK(hipMemcpyAsync(paths_out + (size_t)s * n1, b.paths + (size_t)s * n1, (size_t)(e - s) * n1, hipMemcpyDeviceToHost, h->stream));
        s = e;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->vit_last[0] = S; h->vit_last[1] = L; h->vit_last[2] = ns; h->vit_last[3] = (int64_t)need;
    h->vitx_last[0] = n_sets; h->vitx_last[1] = holes; h->vitx_last[2] = 1; h->vitx_last[3] = (int64_t)need;
    return GH_OK;
}

extern "C" int gh_viterbi_masked_info(const gh_t *h, int64_t out[4])
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    for (int q = 0; q < 4; q++) out[q] = h->vitx_last[q];
    return GH_OK;
}
