// viterbi.hpp -- exact decoding of the chain likelihood (gh_viterbi_path, gh_viterbi_spin, gh_viterbi_info: include/gretel_hip.h,
// where the definition stands; INTEGRATION.md "Exact decoding").  An edge weight depends on the last Le = min(L, N) picks only, so
// the maximum of gh_score_paths' ll_chain over ALL full paths is a dynamic programme over S^Le states, S = the candidate slots
// the window offers anywhere.  fl(a + w) is monotone in a: keeping the best prefix per state loses nothing, the result is the
// maximum bit for bit.  The tensor is only read; the table is chain_table.hpp's (k_beam_table, beam_src_doubles), in a scratch
// block of the handle of its own.
//
//   k_vit_union  U = the union of the candidate bits (compact indices b5) over p = 1..N.  A digit is a slot's rank within U; the
//                compact order is the candidate order, so ascending digits are ascending q.
//   k_vit_walk   one workgroup of 1024 threads, N dependent steps, two rows of `states` binary64 scores in LDS.  State index
//                j = sum_k digit(x[p-k]) S^(Le-1-k), newest pick most significant: the S predecessors of j are the contiguous
//                doubles (j mod S^(Le-1)) S + x, and ascending j at p = N is the end rule's lexicographic order.  A thread owns
//                j = tid, tid + 1024, ... (at most four): their digits never change, so slots, the predecessor base and the bits
//                that make the state reachable are formed once, before the loop.
//                REACHABILITY is not in the score (a reachable prefix may score -inf and competes as such) and needs no flag
//                either: a state is reachable at p exactly where each of its digits is offered at its position (positions <= 0:
//                digit 0), because the candidate set of a position does not depend on the history.  The last Le candidate masks
//                ride in one 64-bit word (5 bits a position), a state's requirement is one AND against it; a predecessor x is
//                reachable where x is offered at p - Le.  Scores of unreachable states are never written and never read.
//                Per reachable state: the weight prefix in the definition's order (the marginal term if the spec has it, lags
//                1 .. min(Le - 1, p)), then per predecessor digit x ascending  cand = V[pred] + (prefix + T_Le[x][b])  -- two
//                additions, that association -- kept by strict >.  For p < Le there is no lag Le: cand = V[pred] + prefix.  The
//                back-pointer, the winning digit, is one plain byte store per (p, state).  One barrier a step, over LDS only.
//                STAGED: the Le + 1 source blocks a step can touch lie in an LDS ring; the block of source p sets out from global
//                memory in step p - 1 (one 16-byte piece in a register of each of the first threads) and is stored in step p,
//                which reads sources p - 1 .. p - Le.  Otherwise (GH_VIT_STAGE=0, or Le > 12 where S = 1) the same body reads the
//                blocks from global memory: the same bits, measured 1.3-1.5x the time of a step (profiles/r12_viterbi.txt).
//   k_vit_trace  picks the end state (ascending j, first stays unless strictly beaten), then follows the back-pointers from N
//                down, VIT_TRACE_BYTES of them at a time through LDS, and writes the path row.
// ---------------------------------------------------------------------------------------------

#define VIT_THREADS 1024
#define VIT_OWN (GH_VITERBI_MAX_STATES / VIT_THREADS)   /* states a thread owns at most */
#define VIT_MAX_LE 12                                    /* 2^12 = the cap: no window with two slots or more has a longer state */
#define VIT_TRACE_BYTES (64 * 1024)                      /* back-pointers the trace holds in LDS at a time */
#define VIT_TRACE_POS 512                                /* ... and never more positions than this */

static_assert(VIT_OWN * VIT_THREADS == GH_VITERBI_MAX_STATES && 5 * VIT_MAX_LE <= 64, "four states a thread; twelve masks a word");
static_assert(2 * (size_t)GH_VITERBI_MAX_STATES * 8 + (VIT_MAX_LE + 1) * (size_t)beam_src_doubles(VIT_MAX_LE) * 8 <= BEAM_LDS_MAX,
              "two score rows and the ring of the longest state fit");

__global__ void __launch_bounds__(256)
k_vit_union(const double *__restrict__ minfo, int N, vit_out *__restrict__ out)
{
    __shared__ uint32_t u;
    if (threadIdx.x == 0) u = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (int p = 1 + (int)threadIdx.x; p <= N; p += blockDim.x) mine |= (uint32_t)__double_as_longlong(minfo[(size_t)p * MINFO + 10]);
    if (mine) atomicOr(&u, mine);
    __syncthreads();
    if (threadIdx.x == 0) out->U = u & 31u;
}

// dynamic LDS: [two score rows of `states` doubles] [STAGED: Le + 1 source blocks]
// KEEP (viterbi_marg.hpp): the forward pass of the max-marginals -- the same step, but every score a step writes also goes to
// global memory by a plain store behind the LDS-only barrier, and no back-pointer, end row or trace is wanted: `vend` is then
// F[N][states], row p - 1 for position p, and bp and okend are not touched.  The arguments are the same under both, so that the
// KEEP = false instantiations are the kernels they were.
template <bool STAGED, bool KEEP = false>
__global__ void __launch_bounds__(VIT_THREADS)
k_vit_walk(const double *__restrict__ Gb, int N, int L, int S, int states, int marginal_term, uint32_t U,
           uint8_t *__restrict__ bp, double *__restrict__ vend, uint8_t *__restrict__ okend, vit_out *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char vit_smem[];
    const int tid = threadIdx.x;
    const int sd = beam_src_doubles(L), su = sd / 2, R = L + 1;
    double *V = reinterpret_cast<double *>(vit_smem);
    double *tab = V + 2 * (size_t)states;
    double2 *tab2 = reinterpret_cast<double2 *>(tab);
    const double2 *Gb2 = reinterpret_cast<const double2 *>(Gb);

    int slot_of[5] = {0, 0, 0, 0, 0};                         // digit -> compact index b5 (ascending: the candidate order)
    {
        int d = 0;
#pragma unroll
        for (int b = 0; b < 5; b++)
            if ((U >> b) & 1u) {
#pragma unroll
                for (int q = 0; q < 5; q++)
                    if (q == d) slot_of[q] = b;
                d++;
            }
    }
    // S = 1: one state whatever L is, reachable wherever there is no hole -- no digits, no masks (L may exceed VIT_MAX_LE)
    const bool one = S == 1;
    int pw = 1;                                               // S^(Le-1)
    for (int k = 1; k < L; k++) pw *= S;

    // what never changes of the states this thread owns
    unsigned long long need[VIT_OWN], slots[VIT_OWN];         // bit 5k + slot_k per digit k; slot_k at bits 3k..3k+2 (k = 0: newest)
    int base[VIT_OWN];                                        // index of predecessor digit 0
#pragma unroll
    for (int o = 0; o < VIT_OWN; o++) {
        const int j = tid + o * VIT_THREADS;
        need[o] = 0; slots[o] = 0; base[o] = 0;
        if (j < states && !one) {
            base[o] = (j % pw) * S;
            int rest = j;
            for (int k = L - 1; k >= 0; k--) {                // least significant digit = oldest pick
                const int d = rest % S;
                rest /= S;
                int sl = 0;
#pragma unroll
                for (int q = 0; q < 5; q++)
                    if (q == d) sl = slot_of[q];
                need[o] |= 1ull << (5 * k + sl);
                slots[o] |= (unsigned long long)sl << (3 * k);
            }
        }
    }
    // the candidate masks of positions p, p-1, ... at bits 0, 5, ...; positions <= 0 offer digit 0 alone
    unsigned long long hist = 0;
    for (int k = 0; k < L && !one; k++) hist |= 1ull << (5 * k + slot_of[0]);
    const unsigned long long hmask = one ? 0 : (1ull << (5 * L)) - 1;

    if (tid == 0) V[0] = 0.0;                                 // the one prefix at p = 0: every digit 0, score +0.0
    double2 reg = make_double2(0.0, 0.0);
    if (STAGED) {
        if (tid < su) tab2[tid] = Gb2[tid];                   // source 0 straight in; source 1 sets out
        if (1 < N && tid < su) reg = Gb2[(size_t)su + tid];
    }
    __syncthreads();

    int cur = 0, hole = 0;
    int ts = 0;                                               // LDS slot of source p - 1
    for (int p = 1; p <= N; p++) {
        if (STAGED) {
            // source p (first read in step p + 1) replaces source p - Le - 1, last read in step p - 1; source p + 1 sets out
            const int ws = ts + 1 == R ? 0 : ts + 1;
            if (p < N && tid < su) tab2[(size_t)ws * su + tid] = reg;
            if (p + 1 < N && tid < su) reg = Gb2[(size_t)(p + 1) * su + tid];
        }
        const double *blk = STAGED ? tab + (size_t)ts * sd : Gb + (size_t)(p - 1) * sd;
        const uint32_t cm5 = (uint32_t)__double_as_longlong(blk[30 * L + 5]) & 31u;
        if (cm5 == 0) { hole = p; break; }                    // (the same word in every thread: all leave together)
        const uint32_t cm_old = one ? 1u << slot_of[0] : (uint32_t)(hist >> (5 * (L - 1))) & 31u;      // what position p - Le offers
        hist = ((hist << 5) | cm5) & hmask;
        const double *Vc = V + (size_t)cur * states;
        double *Vn = V + (size_t)(cur ^ 1) * states;
        const int npre = L - 1 < p ? L - 1 : p;               // lags of the prefix
#pragma unroll
        for (int o = 0; o < VIT_OWN; o++) {
            const int j = tid + o * VIT_THREADS;
            if (j < states && (hist & need[o]) == need[o]) {
                const unsigned long long sl = slots[o];
                const int b = one ? slot_of[0] : (int)(sl & 7);
                double w = 0.0;
                if (marginal_term) w += blk[30 * L + b];
                int tl = ts;
                for (int l = 1; l <= npre; l++) {
                    const int a6 = p - l == 0 ? 5 : one ? slot_of[0] : (int)((sl >> (3 * l)) & 7);
                    const double *src = STAGED ? tab + (size_t)tl * sd : Gb + (size_t)(p - l) * sd;
                    w += src[(a6 * L + (l - 1)) * LT_ROW + b];
                    tl = tl == 0 ? R - 1 : tl - 1;
                }
                double best = 0.0;
                int arg = -1;
                if (p < L) {
                    best = Vc[base[o]] + w;                   // warm-up: the one predecessor, no lag Le
                    arg = 0;
                } else {
                    const double *src = STAGED ? tab + (size_t)tl * sd : Gb + (size_t)(p - L) * sd;
                    for (int x = 0; x < S; x++) {
                        int sx = 0;
#pragma unroll
                        for (int q = 0; q < 5; q++)
                            if (q == x) sx = slot_of[q];
                        if (!((cm_old >> sx) & 1u)) continue;
                        const int a6 = p == L ? 5 : sx;
                        const double cand = Vc[base[o] + x] + (w + src[(a6 * L + (L - 1)) * LT_ROW + b]);
                        if (arg < 0 || cand > best) { best = cand; arg = x; }
                    }
                }
                Vn[j] = best;
                if (KEEP) vend[(size_t)(p - 1) * states + j] = best;
                else bp[(size_t)p * states + j] = (uint8_t)arg;
            }
        }
        cur ^= 1;
        ts = ts + 1 == R ? 0 : ts + 1;
        beam_barrier();
    }
    if (tid == 0) out->hole_at = hole;
    if (!hole && !KEEP) {
        const double *Vc = V + (size_t)cur * states;
#pragma unroll
        for (int o = 0; o < VIT_OWN; o++) {
            const int j = tid + o * VIT_THREADS;
            if (j < states) {
                const bool ok = (hist & need[o]) == need[o];
                okend[j] = ok ? 1 : 0;
                vend[j] = ok ? Vc[j] : 0.0;
            }
        }
    }
}

// dynamic LDS: the back-pointers of `chunk` positions
__global__ void __launch_bounds__(VIT_THREADS)
k_vit_trace(const uint8_t *__restrict__ bp, const double *__restrict__ vend, const uint8_t *__restrict__ okend, int N, int L, int S,
            int states, int chunk, uint32_t U, symmap sm, vit_out *__restrict__ out, uint8_t *__restrict__ path)
{
    extern __shared__ __attribute__((aligned(16))) char vit_tsmem[];
    __shared__ double rv[VIT_THREADS];
    __shared__ int ri[VIT_THREADS];
    const int tid = threadIdx.x;
    if (out->hole_at) return;                                 // (the same word in every thread)
    // the end rule: ascending j, the first stays unless strictly beaten -- per thread over its own states, then pairwise, where
    // of two equal scores the smaller j stays
    double bv = 0.0;
    int bi = -1;
    for (int j = tid; j < states; j += VIT_THREADS)
        if (okend[j]) {
            const double v = vend[j];
            if (bi < 0 || v > bv) { bv = v; bi = j; }
        }
    rv[tid] = bv;
    ri[tid] = bi;
    __syncthreads();
    for (int h = VIT_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            const double ov = rv[tid + h];
            const int oi = ri[tid + h], mi = ri[tid];
            if (oi >= 0 && (mi < 0 || ov > rv[tid] || (ov == rv[tid] && oi < mi))) { rv[tid] = ov; ri[tid] = oi; }
        }
        __syncthreads();
    }
    int j = ri[0];
    if (tid == 0) {
        out->end_state = j;
        out->ll = rv[0];
        path[0] = SYM_US;
    }
    int slot_of[5] = {0, 0, 0, 0, 0};
    {
        int d = 0;
        for (int b = 0; b < 5; b++)
            if ((U >> b) & 1u) slot_of[d++] = b;
    }
    int pw = 1;
    for (int k = 1; k < L; k++) pw *= S;
    uint32_t *blk = reinterpret_cast<uint32_t *>(vit_tsmem);
    const uint8_t *b8 = reinterpret_cast<const uint8_t *>(vit_tsmem);
    for (int hi = N; hi >= 1; hi -= chunk) {
        const int lo = hi - chunk + 1 > 1 ? hi - chunk + 1 : 1;
        // (states is a multiple of 4 or the whole scratch row is padded to one: whole words per chunk, see vit_run)
        const size_t first = (size_t)lo * states, bytes = (size_t)(hi - lo + 1) * states;
        const size_t w0 = first / 4, w1 = (first + bytes + 3) / 4;
        const uint32_t *from = reinterpret_cast<const uint32_t *>(bp) + w0;
        for (size_t q = tid; q < w1 - w0; q += VIT_THREADS) blk[q] = from[q];
        __syncthreads();
        if (tid == 0) {
            const size_t skew = first - w0 * 4;
            for (int q = hi; q >= lo; q--) {
                path[q] = (uint8_t)vsym(sm, slot_of[j / pw]);
                j = (j % pw) * S + b8[skew + (size_t)(q - lo) * states + j];
            }
        }
        __syncthreads();
    }
}

// host ---------------------------------------------------------------------------------------- (vit_out, vit_bufs: scratch_layout.hpp)
static const char VIT_SCRATCH[] = "the exact decoder's scratch, whose table grows with N * L and whose back-pointers with N * states,";

// S^L, or one more than the cap where it is beyond it
static long long vit_states(int S, int L)
{
    long long states = 1;
    for (int k = 0; k < L && states <= GH_VITERBI_MAX_STATES; k++) states *= S;
    return states;
}

// the refusal of a window beyond the cap
static int vit_too_many(const char *who, int S, int L)
{
    char cnt[32];
    const double full = pow((double)S, (double)L);
    snprintf(cnt, sizeof cnt, full < 1e15 ? "%.0f" : "%.3g", full);
    return fail(GH_ERR_ARG, "%s: S = %d candidate symbols and Le = min(L, N) = %d make %s states, more than the %d the exact decoder "
                "holds on chip: lower L, or use the beam (--beam, gh_beam_paths)", who, S, L, cnt, GH_VITERBI_MAX_STATES);
}

// GH_VIT_STAGE=0, read once (A/B: the table blocks from global memory)
static bool vit_no_stage()
{
    static const bool off = env_off("GH_VIT_STAGE");
    return off;
}

// What the decoder and the max-marginals (viterbi_marg.hpp) open a call with: U of the tensor as it stands (ho->U, S its bits)
// and *ns = S^Le, refused beyond the cap.  *ns = 0 where nothing is offered anywhere: ho->hole_at = 1 and the call is over.  The
// vit_out is the first part of the handle's block under either layout (scratch_layout.hpp).
static int vit_open(gh_handle *h, vit_out *ho, const char *who, int *ns)
{
    const int N = h->N, L = chain_lags(h);
    int rc = ensure_marg(h);                                    // (k_vit_union reads minfo)
    if (rc) return rc;
    // U first: it decides whether the decoder serves this window at all
    if ((rc = scratch_reserve(h, &h->vit, vit_layout(nullptr, N, 0, 0).total, VIT_SCRATCH))) return rc;
    vit_out *d_out = vit_layout(h->vit.buf, N, 0, 0).out;
    hipLaunchKernelGGL(k_vit_union, dim3(1), dim3(256), 0, h->stream, (const double *)h->minfo, N, d_out);
    if ((rc = post_launch(h, "k_vit_union"))) return rc;
    HIPCHK(hipMemcpyAsync(ho, d_out, sizeof *ho, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int S = __builtin_popcount(ho->U);
    *ns = 0;
    if (S == 0) {                                             // nothing offered anywhere: the hole is the first position
        ho->hole_at = 1;
        h->vit_last[0] = 0; h->vit_last[1] = L; h->vit_last[2] = 0; h->vit_last[3] = (int64_t)h->vit.cap;
        return GH_OK;
    }
    const long long states = vit_states(S, L);
    if (states > GH_VITERBI_MAX_STATES) return vit_too_many(who, S, L);
    *ns = (int)states;
    return GH_OK;
}

// one exact decoding of the tensor as it stands: the results stay in the handle's scratch (`b`), *ho = hole, score and U
static int vit_run(gh_handle *h, vit_bufs *b, vit_out *ho, const char *who)
{
    const int N = h->N, L = chain_lags(h);
    int rc, ns;
    if ((rc = vit_open(h, ho, who, &ns)) || !ns) return rc;
    const uint32_t U = ho->U;
    const int S = __builtin_popcount(U);
    const size_t table_doubles = (size_t)N * beam_src_doubles(L);
    const size_t need = vit_layout(nullptr, N, table_doubles, ns).total;
    if ((rc = scratch_reserve(h, &h->vit, need, VIT_SCRATCH))) return rc;
    *b = vit_layout(h->vit.buf, N, table_doubles, ns);
    if ((rc = chain_table_build(h, L, b->Gb))) return rc;

    const bool no_stage = vit_no_stage();
    const size_t rows = 2 * (size_t)ns * 8;
    if (!no_stage && L <= VIT_MAX_LE) {                         // (a longer state has S = 1: its ring need not fit)
        const size_t lds = rows + (size_t)(L + 1) * beam_src_doubles(L) * 8;
        lds_limit<k_vit_walk<true>>(lds, h->dev);
        hipLaunchKernelGGL(k_vit_walk<true>, dim3(1), dim3(VIT_THREADS), lds, h->stream, (const double *)b->Gb, N, L, S, ns, h->cfg.marginal_term, U,
                           b->bp, b->vend, b->okend, b->out);
    } else {
        lds_limit<k_vit_walk<false>>(rows, h->dev);
        hipLaunchKernelGGL(k_vit_walk<false>, dim3(1), dim3(VIT_THREADS), rows, h->stream, (const double *)b->Gb, N, L, S, ns, h->cfg.marginal_term, U,
                           b->bp, b->vend, b->okend, b->out);
    }
    if ((rc = post_launch(h, "k_vit_walk"))) return rc;
    int chunk = VIT_TRACE_BYTES / ns;
    if (chunk > VIT_TRACE_POS) chunk = VIT_TRACE_POS;
    const size_t tlds = (size_t)chunk * ns + 8;
    lds_limit<k_vit_trace>(tlds, h->dev);
    hipLaunchKernelGGL(k_vit_trace, dim3(1), dim3(VIT_THREADS), tlds, h->stream, (const uint8_t *)b->bp, (const double *)b->vend,
                       (const uint8_t *)b->okend, N, L, S, ns, chunk, U, h->sm, b->out, b->path);
    if ((rc = post_launch(h, "k_vit_trace"))) return rc;
    HIPCHK(hipMemcpyAsync(ho, b->out, sizeof *ho, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->vit_last[0] = S; h->vit_last[1] = L; h->vit_last[2] = ns; h->vit_last[3] = (int64_t)need;
    return GH_OK;
}

extern "C" int gh_viterbi_path(gh_t *h, uint8_t *path_out, double *ll_chain, int *hole_at)
{
    if (!h || !path_out || !ll_chain || !hole_at) return fail(GH_ERR_ARG, "null argument");
    int rc = decode_check(h, "gh_viterbi_path");
    if (rc) return rc;
    if (set_dev(h)) return GH_ERR_HIP;
    vit_bufs b;
    vit_out ho;
    if ((rc = vit_run(h, &b, &ho, "gh_viterbi_path"))) return rc;
    *hole_at = ho.hole_at;
    if (ho.hole_at) return GH_OK;
    HIPCHK(hipMemcpyAsync(path_out, b.path, (size_t)h->N + 1, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *ll_chain = ho.ll;
    return GH_OK;
}

extern "C" int gh_viterbi_spin(gh_t *h, int max_paths, double min_remove, uint8_t *paths_out, gh_path_rec *recs, double *ll_chain,
                               int *n_out, int *hole_at)
{
    if (!h || !paths_out || !recs || !n_out || !hole_at) return fail(GH_ERR_ARG, "null argument");
    if (max_paths < 0) return fail(GH_ERR_ARG, "max_paths < 0");
    int rc = decode_check(h, "gh_viterbi_spin");
    if (rc) return rc;
    if (set_dev(h)) return GH_ERR_HIP;
    return decode_spin(h, max_paths, min_remove, paths_out, recs, ll_chain, n_out, hole_at, [&](decoded *d) -> int {
        vit_bufs b;
        vit_out ho;
        if ((rc = vit_run(h, &b, &ho, "gh_viterbi_spin"))) return rc;
        d->hole = ho.hole_at;
        d->d_path = b.path;
        d->ll = ho.ll;                                          // (it came home with vit_out)
        return GH_OK;
    });
}

extern "C" int gh_viterbi_info(const gh_t *h, int64_t out[4])
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    for (int q = 0; q < 4; q++) out[q] = h->vit_last[q];
    return GH_OK;
}
