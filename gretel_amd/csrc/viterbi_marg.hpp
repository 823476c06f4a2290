// viterbi_marg.hpp -- max-marginals of the chain likelihood (gh_viterbi_marginals: include/gretel_hip.h, where the definition
// stands; INTEGRATION.md "Max-marginals").  For every SNP p and candidate c the best chain likelihood of any full path that takes
// c at p:  M[p][c] = max over the reachable states s at p whose newest pick is c of  F_p(s) + B_p(s).  F is what k_vit_walk keeps
// in its score rows; B is the same dynamic programme run from N down.  State space, state index (newest pick most significant),
// reachability masks, table, ring and barrier are viterbi.hpp's and chain_table.hpp's.
//
//   k_vit_cands  (parallel) the candidate bits of every position twice: over the compact indices (what the backward walk shifts
//                into its mask word) and over the seven symbols (the `cm` the caller gets).
//   k_vit_walk<STAGED, KEEP = true> (viterbi.hpp)  the decoder's step with the score of every reachable (p, state) also stored to
//                fb[p - 1][state] (handed over as the kernel's `vend`): a plain store, never read again inside the kernel.  No
//                back-pointers, no end row.
//   k_vit_back   one workgroup of 1024 threads, N dependent steps p = N .. 1, a thread owns the states the forward walk gives it.
//                LDS: two rows of B, two rows of weight prefixes, the ring.  Step p, per reachable state j at p:
//                  B_p(j) = max over c in cm(p+1) of  (P_{p+1}[succ] + T_Le[oldest(j)][c]) + B_{p+1}[succ],  succ = c S^(Le-1) + j div S
//                (+0.0 at p = N; without the lag-Le term while p + 1 < Le).  S consecutive lanes read one successor -- an LDS
//                broadcast -- and consecutive groups of S read consecutive doubles: a lane group of 32 (a 64-bit LDS read is served
//                in two) touches 32 / S doubles in a row, 64 / S <= 64 banks, no conflict.
//                P_{p+1}[succ] is the part of w_{p+1}(c | .) that the successor alone decides: the marginal term and lags
//                1 .. Le - 1 in the definition's order.  It is shared by the successor's S predecessors, so the owner of state j computes P_p[j] in step p, beside B_p(j), for step p - 1 to read: one barrier a step,
//                Le - 1 table reads per state a step where recomputing it per successor would take S (Le - 1).  P is read and
//                written in the same step, hence its two rows.
//                Then F_p(j) -- set out from global memory a step ahead, as the ring's block is -- takes B_p(j) in ONE addition and
//                the sum goes back over it; a state that is not reachable at p gets a NaN there (no sum is one: offer_zero is
//                refused).  Reachability is the forward walk's AND against the mask word, which here shifts the other way: the
//                mask of position p - Le comes in at the top, loaded from cm5 a step ahead.
//                The ring has Le + 2 slots: step p reads sources p .. p - Le (lag Le of target p + 1 in source p + 1 - Le, the
//                prefix of target p in sources p - 1 .. p - Le + 1 and the header of p - 1); source p - Le - 1 is stored in step p
//                for step p - 1, source p - Le - 2 sets out.  Four rows of 4096 states are 128 KB: where the ring does not fit
//                beside them (S = 2 with Le >= 11) the blocks are read from global memory, as under GH_VIT_STAGE=0: the same bits.
//   k_vit_mm     (parallel, a workgroup per position at a time) the maximum of row p over each block of S^(Le-1) states that share
//                their newest pick, NaNs left out; entries of symbols not offered at p are -inf.  The reduction is on neither
//                walk's serial chain and runs at memory speed.
// k_vit_walk keeps its own statement of the digit scheme for the reason viterbi_panel.hpp gives (moved into functions it compiles
// to other instructions); k_vit_back and k_vit_mm state theirs once, in vit_slots and vit_own_digits below.
// ---------------------------------------------------------------------------------------------

static_assert(4 * (size_t)GH_VITERBI_MAX_STATES * 8 <= BEAM_LDS_MAX, "two rows of B and two of prefixes fit without the ring");

// digit -> compact index b5 (ascending: the candidate order)
__device__ __forceinline__ void vit_slots(uint32_t U, int slot_of[5])
{
    int d = 0;
#pragma unroll
    for (int q = 0; q < 5; q++) slot_of[q] = 0;
#pragma unroll
    for (int b = 0; b < 5; b++)
        if ((U >> b) & 1u) {
#pragma unroll
            for (int q = 0; q < 5; q++)
                if (q == d) slot_of[q] = b;
            d++;
        }
}

// state j's digits as k_vit_walk keeps them: bit 5k + slot_k per digit k in `need`, slot_k at bits 3k..3k+2 of `slots` (k = 0: newest)
__device__ __forceinline__ void vit_own_digits(int j, int S, int L, const int slot_of[5], unsigned long long *need, unsigned long long *slots)
{
    unsigned long long nd = 0, sl8 = 0;
    int rest = j;
    for (int k = L - 1; k >= 0; k--) {                        // least significant digit = oldest pick
        const int d = rest % S;
        rest /= S;
        int sl = 0;
#pragma unroll
        for (int q = 0; q < 5; q++)
            if (q == d) sl = slot_of[q];
        nd |= 1ull << (5 * k + sl);
        sl8 |= (unsigned long long)sl << (3 * k);
    }
    *need = nd;
    *slots = sl8;
}

__global__ void __launch_bounds__(256)
k_vit_cands(const double *__restrict__ minfo, int N, symmap sm, uint8_t *__restrict__ cm5, uint8_t *__restrict__ cm)
{
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p <= N; p += gridDim.x * blockDim.x) {
        const uint32_t c5 = p ? (uint32_t)__double_as_longlong(minfo[(size_t)p * MINFO + 10]) & 31u : 0u;
        uint32_t c7 = 0;
#pragma unroll
        for (int b = 0; b < 5; b++)
            if ((c5 >> b) & 1u) c7 |= 1u << vsym(sm, b);
        cm5[p] = (uint8_t)c5;
        cm[p] = (uint8_t)c7;
    }
}

// dynamic LDS: [two rows of B] [two rows of prefixes] [STAGED: Le + 2 source blocks]
template <bool STAGED>
__global__ void __launch_bounds__(VIT_THREADS)
k_vit_back(const double *__restrict__ Gb, const uint8_t *__restrict__ cm5, int N, int L, int S, int states, int marginal_term, uint32_t U,
           double *__restrict__ fb, const vit_out *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char vitb_smem[];
    if (out->hole_at) return;                                 // (the same word in every thread)
    const int tid = threadIdx.x;
    const int sd = beam_src_doubles(L), su = sd / 2, R = L + 2;
    double *Bv = reinterpret_cast<double *>(vitb_smem);
    double *Pv = Bv + 2 * (size_t)states;
    double *tab = Pv + 2 * (size_t)states;
    double2 *tab2 = reinterpret_cast<double2 *>(tab);
    const double2 *Gb2 = reinterpret_cast<const double2 *>(Gb);

    int slot_of[5];
    vit_slots(U, slot_of);
    const bool one = S == 1;                                  // one state whatever L is: no digits, no masks
    int pw = 1;                                               // S^(Le-1)
    for (int k = 1; k < L; k++) pw *= S;
    unsigned long long need[VIT_OWN], slots[VIT_OWN];
#pragma unroll
    for (int o = 0; o < VIT_OWN; o++) {
        const int j = tid + o * VIT_THREADS;
        need[o] = 0; slots[o] = 0;
        if (j < states && !one) vit_own_digits(j, S, L, slot_of, &need[o], &slots[o]);
    }
    // the candidate masks of positions p, p-1, ... at bits 0, 5, ...; positions <= 0 offer digit 0 alone
    const uint32_t d0 = 1u << slot_of[0];
    unsigned long long hist = 0;
    for (int k = 0; k < L && !one; k++) hist |= (unsigned long long)(N - k >= 1 ? (uint32_t)cm5[N - k] : d0) << (5 * k);
    uint32_t enter = one ? 0u : N - L >= 1 ? (uint32_t)cm5[N - L] : d0;     // the mask of position p - Le, for the end of step p
    uint32_t cm_up = 0;                                       // what position p + 1 offers

    double2 reg = make_double2(0.0, 0.0);
    if (STAGED) {
        // sources N - 1 .. N - Le straight in (source i lies in slot i mod R); source N - Le - 1 sets out
        for (int i = N - 1; i >= 0 && i >= N - L; i--)
            if (tid < su) tab2[(size_t)(i % R) * su + tid] = Gb2[(size_t)i * su + tid];
        if (N - L - 1 >= 0 && tid < su) reg = Gb2[(size_t)(N - L - 1) * su + tid];
    }
    double fv[VIT_OWN];                                       // F_p of the owned states: row p - 1 sets out in step p + 1
#pragma unroll
    for (int o = 0; o < VIT_OWN; o++) {
        const int j = tid + o * VIT_THREADS;
        fv[o] = j < states ? fb[(size_t)(N - 1) * states + j] : 0.0;
    }
    __syncthreads();

    int cur = 0;
    int ts = (N - 1) % R;                                     // LDS slot of source p - 1
    for (int p = N; p >= 1; p--) {
        if (STAGED) {
            // source p - Le - 1 (first read in step p - 1) replaces source p + 1, last read in step p + 1; source p - Le - 2 sets out
            const int ws = ts + 2 >= R ? ts + 2 - R : ts + 2;
            if (p - L - 1 >= 0 && tid < su) tab2[(size_t)ws * su + tid] = reg;
            if (p - L - 2 >= 0 && tid < su) reg = Gb2[(size_t)(p - L - 2) * su + tid];
        }
        const uint32_t enter_next = one ? 0u : p - 1 - L >= 1 ? (uint32_t)cm5[p - 1 - L] : d0;
        double fnext[VIT_OWN];
#pragma unroll
        for (int o = 0; o < VIT_OWN; o++) {
            const int j = tid + o * VIT_THREADS;
            fnext[o] = p >= 2 && j < states ? fb[(size_t)(p - 2) * states + j] : 0.0;
        }
        const double *Bn = Bv + (size_t)(cur ^ 1) * states, *Pn = Pv + (size_t)(cur ^ 1) * states;
        double *Bc = Bv + (size_t)cur * states, *Pc = Pv + (size_t)cur * states;
        const double *blk = STAGED ? tab + (size_t)ts * sd : Gb + (size_t)(p - 1) * sd;       // source p - 1: the header of target p
        int tsl = ts + 2 - L;                                 // the slot of source p + 1 - Le: lag Le of target p + 1
        if (tsl < 0) tsl += R;
        if (tsl >= R) tsl -= R;
        const double *last = STAGED ? tab + (size_t)tsl * sd : Gb + (size_t)(p + 1 - L >= 0 ? p + 1 - L : 0) * sd;
        const bool lagL = p + 1 >= L;                         // target p + 1 has a lag Le
        const int npre = L - 1 < p ? L - 1 : p;               // lags of target p's prefix
#pragma unroll
        for (int o = 0; o < VIT_OWN; o++) {
            const int j = tid + o * VIT_THREADS;
            if (j < states) {
                double sum = __longlong_as_double(0x7ff8000000000000ll);
                if ((hist & need[o]) == need[o]) {
                    const unsigned long long sl = slots[o];
                    double b = 0.0;
                    if (p < N) {
                        const int a6 = p + 1 == L ? 5 : one ? slot_of[0] : (int)((sl >> (3 * (L - 1))) & 7);
                        const int rest = j / S;
                        bool have = false;
                        for (int c = 0; c < S; c++) {
                            int sc = 0;
#pragma unroll
                            for (int q = 0; q < 5; q++)
                                if (q == c) sc = slot_of[q];
                            if (!((cm_up >> sc) & 1u)) continue;
                            const int succ = c * pw + rest;
                            double w = Pn[succ];
                            if (lagL) w += last[(a6 * L + (L - 1)) * LT_ROW + sc];
                            const double cand = w + Bn[succ];
                            if (!have || cand > b) { b = cand; have = true; }
                        }
                    }
                    Bc[j] = b;
                    sum = fv[o] + b;
                    if (p >= 2) {                             // the prefix of target p, for the S predecessors of j in step p - 1
                        const int bq = one ? slot_of[0] : (int)(sl & 7);
                        double w = 0.0;
                        if (marginal_term) w += blk[30 * L + bq];
                        int tl = ts;
                        for (int l = 1; l <= npre; l++) {
                            const int a6 = p - l == 0 ? 5 : one ? slot_of[0] : (int)((sl >> (3 * l)) & 7);
                            const double *src = STAGED ? tab + (size_t)tl * sd : Gb + (size_t)(p - l) * sd;
                            w += src[(a6 * L + (l - 1)) * LT_ROW + bq];
                            tl = tl == 0 ? R - 1 : tl - 1;
                        }
                        Pc[j] = w;
                    }
                }
                fb[(size_t)(p - 1) * states + j] = sum;
            }
        }
#pragma unroll
        for (int o = 0; o < VIT_OWN; o++) fv[o] = fnext[o];
        cm_up = one ? d0 : (uint32_t)hist & 31u;
        if (!one) hist = (hist >> 5) | ((unsigned long long)enter << (5 * (L - 1)));
        enter = enter_next;
        cur ^= 1;
        ts = ts == 0 ? R - 1 : ts - 1;
        beam_barrier();
    }
}

// one position a workgroup at a time; pw = S^(Le-1), the states that share their newest pick
__global__ void __launch_bounds__(256)
k_vit_mm(const double *__restrict__ fb, const uint8_t *__restrict__ cm5, int N, int S, int states, int pw, uint32_t U, symmap sm,
         const vit_out *__restrict__ out, double *__restrict__ mm)
{
    __shared__ double red[5][256];
    if (out->hole_at) return;                                 // (the same word in every thread)
    const int tid = threadIdx.x;
    int slot_of[5];
    vit_slots(U, slot_of);
    const double none = __longlong_as_double(0x7ff8000000000000ll);
    for (int p = blockIdx.x; p <= N; p += gridDim.x) {
        // (a maximum does not depend on the order; NaN = no reachable state seen yet)
#pragma unroll
        for (int c = 0; c < 5; c++) {
            double m = none;
            if (c < S && p >= 1) {
                const double *row = fb + (size_t)(p - 1) * states + (size_t)c * pw;
                for (int j = tid; j < pw; j += 256) {
                    const double v = row[j];
                    if (v == v && !(m >= v)) m = v;
                }
            }
            red[c][tid] = m;
        }
        __syncthreads();
        for (int h = 128; h >= 1; h >>= 1) {
            if (tid < h) {
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    const double v = red[c][tid + h];
                    if (v == v && !(red[c][tid] >= v)) red[c][tid] = v;
                }
            }
            __syncthreads();
        }
        if (tid < GH_NSYM) mm[(size_t)p * GH_NSYM + tid] = -INFINITY;
        __syncthreads();
        if (tid < S && p >= 1) {
            int sc = 0;
#pragma unroll
            for (int q = 0; q < 5; q++)
                if (q == tid) sc = slot_of[q];
            const double v = red[tid][0];
            if (((uint32_t)cm5[p] >> sc) & 1u) mm[(size_t)p * GH_NSYM + vsym(sm, sc)] = v == v ? v : -INFINITY;
        }
        __syncthreads();
    }
}

// host ----------------------------------------------------------------------------------------
extern "C" int gh_viterbi_marginals(gh_t *h, double *mm, uint8_t *cm, int *hole_at)
{
    if (!h || !mm || !cm || !hole_at) return fail(GH_ERR_ARG, "null argument");
    int rc = decode_check(h, "gh_viterbi_marginals");
    if (rc) return rc;
    if (set_dev(h)) return GH_ERR_HIP;
    const int N = h->N, L = chain_lags(h);
    vit_out ho;
    int ns;
    if ((rc = vit_open(h, &ho, "gh_viterbi_marginals", &ns))) return rc;
    if (!ns) { *hole_at = ho.hole_at; return GH_OK; }
    const uint32_t U = ho.U;
    const int S = __builtin_popcount(U);
    const size_t table_doubles = (size_t)N * beam_src_doubles(L);
    const size_t need = vitm_layout(nullptr, N, table_doubles, ns).total;
    if ((rc = scratch_reserve(h, &h->vit, need, VIT_SCRATCH))) return rc;
    const vitm_bufs b = vitm_layout(h->vit.buf, N, table_doubles, ns);
    if ((rc = chain_table_build(h, L, b.Gb))) return rc;
    hipLaunchKernelGGL(k_vit_cands, dim3((unsigned)std::min<size_t>(((size_t)N + 256) / 256, 1024)), dim3(256), 0, h->stream,
                       (const double *)h->minfo, N, h->sm, b.cm5, b.cm);
    if ((rc = post_launch(h, "k_vit_cands"))) return rc;

    const bool stage = !vit_no_stage() && L <= VIT_MAX_LE;      // (a longer state has S = 1: its ring need not fit)
    const size_t ring = (size_t)(L + 1) * beam_src_doubles(L) * 8, bring = (size_t)(L + 2) * beam_src_doubles(L) * 8;
    const size_t rows = 2 * (size_t)ns * 8;
    if (stage) {
        lds_limit<k_vit_walk<true, true>>(rows + ring, h->dev);
        hipLaunchKernelGGL((k_vit_walk<true, true>), dim3(1), dim3(VIT_THREADS), rows + ring, h->stream, (const double *)b.Gb, N, L, S, ns,
                           h->cfg.marginal_term, U, (uint8_t *)nullptr, b.fb, (uint8_t *)nullptr, b.out);
    } else {
        lds_limit<k_vit_walk<false, true>>(rows, h->dev);
        hipLaunchKernelGGL((k_vit_walk<false, true>), dim3(1), dim3(VIT_THREADS), rows, h->stream, (const double *)b.Gb, N, L, S, ns,
                           h->cfg.marginal_term, U, (uint8_t *)nullptr, b.fb, (uint8_t *)nullptr, b.out);
    }
    if ((rc = post_launch(h, "k_vit_walk"))) return rc;
    if (stage && 2 * rows + bring <= BEAM_LDS_MAX) {
        lds_limit<k_vit_back<true>>(2 * rows + bring, h->dev);
        hipLaunchKernelGGL(k_vit_back<true>, dim3(1), dim3(VIT_THREADS), 2 * rows + bring, h->stream, (const double *)b.Gb, (const uint8_t *)b.cm5,
                           N, L, S, ns, h->cfg.marginal_term, U, b.fb, (const vit_out *)b.out);
    } else {
        lds_limit<k_vit_back<false>>(2 * rows, h->dev);
        hipLaunchKernelGGL(k_vit_back<false>, dim3(1), dim3(VIT_THREADS), 2 * rows, h->stream, (const double *)b.Gb, (const uint8_t *)b.cm5,
                           N, L, S, ns, h->cfg.marginal_term, U, b.fb, (const vit_out *)b.out);
    }
    if ((rc = post_launch(h, "k_vit_back"))) return rc;
    int pw = 1;
    for (int k = 1; k < L; k++) pw *= S;
    hipLaunchKernelGGL(k_vit_mm, dim3((unsigned)std::min(N + 1, 4096)), dim3(256), 0, h->stream, (const double *)b.fb, (const uint8_t *)b.cm5,
                       N, S, ns, pw, U, h->sm, (const vit_out *)b.out, b.mm);
    if ((rc = post_launch(h, "k_vit_mm"))) return rc;
    HIPCHK(hipMemcpyAsync(&ho, b.out, sizeof ho, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->vit_last[0] = S; h->vit_last[1] = L; h->vit_last[2] = ns; h->vit_last[3] = (int64_t)need;
    *hole_at = ho.hole_at;
    if (ho.hole_at) return GH_OK;
    HIPCHK(hipMemcpyAsync(mm, b.mm, ((size_t)N + 1) * GH_NSYM * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cm, b.cm, (size_t)N + 1, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GH_OK;
}
