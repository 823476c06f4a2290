// viterbi_kbest.hpp -- k-best (list) exact decoding of the chain likelihood (gh_viterbi_kbest: include/gretel_hip.h, where the
// definition stands; INTEGRATION.md "K-best decoding").  The exact decoder's state space, table, tie discipline and scratch block
// (viterbi.hpp), with a ranked list of at most K prefixes per state in place of one: fl(a + w) is monotone in a, so the K best
// prefixes into a state lie among the K best of each predecessor.  A SLOT is (state j, rank r), index j K + r; the window is served
// where states * K <= GH_VITERBI_MAX_STATES, so the two score rows are the decoder's 64 KB and a thread owns at most four slots.
//
//   k_vitk_walk   one workgroup of 1024 threads, N dependent steps, one LDS-only barrier a step; the state index, the need / hist
//                 reachability words and the table ring are k_vit_walk's.  LDS: two rows of states * K scores, two rows of
//                 `states` count bytes (how many entries a state holds; 0 = not reachable -- never a score, -inf is a score), the
//                 ring.  THE MERGE is rank by counting over the OUTPUT-SIDE slots, no serial loop per state: the thread of slot
//                 (j, r') forms, for every offered predecessor digit x, the child of rank r' of predecessor (j mod S^(Le-1)) S + x,
//                 and finds its place in the merged order of state j: r' (the children of one list keep their order: the list is
//                 non-increasing and fl(+) monotone) plus, for every other offered digit x', the number of that list's children
//                 that precede it -- those of score >= its own where x' < x, of score > its own where x' > x (digits ascend with
//                 q).  A list is non-increasing, so each number is one binary search of at most 5 probes; a probe recomputes the
//                 child's score  V + (prefix + T_Le[x'])  by the very expression its own thread stores, so equal is equal.  The
//                 order is strict: every place below K is written exactly once, score and back-pointer, by plain stores.  The step
//                 reads the old row and writes the new one.  For p < Le (and at p = Le, where only digit 0 is offered at position
//                 0) there is one predecessor and the list carries over in order.
//                 Back-pointer: one byte per (p, j, r), (digit << 5) | predecessor's rank, at bp[(p states + j) K + r].
//   k_vitk_trace  ranks the end entries by counting (score descending, then ascending slot index = ascending state, then rank: the
//                 end rule), writes n_out and the scores of the first K, then follows those K chains at once, one lane a path,
//                 through back-pointer chunks staged in LDS as k_vit_trace stages them (a row is states * K <= 4096 bytes).
// ---------------------------------------------------------------------------------------------

static_assert(GH_KBEST_MAX == 32 && GH_KBEST_MAX <= VIT_THREADS, "a back-pointer holds the rank in 5 bits, the digit in 3; a lane a path");
static_assert(2 * (size_t)GH_VITERBI_MAX_STATES * 8 + 2 * (size_t)GH_VITERBI_MAX_STATES +
                      (VIT_MAX_LE + 1) * (size_t)beam_src_doubles(VIT_MAX_LE) * 8 <= BEAM_LDS_MAX,
              "two score rows, two count rows and the ring of the longest state fit");

// bytes of the two count rows, kept a multiple of 16 so that the ring behind them stays aligned
__host__ __device__ constexpr size_t vitk_count_bytes(int states) { return (2 * (size_t)states + 15) & ~(size_t)15; }

// dynamic LDS: [two score rows of states * K doubles] [two count rows of `states` bytes] [STAGED: Le + 1 source blocks]
template <bool STAGED>
__global__ void __launch_bounds__(VIT_THREADS)
k_vitk_walk(const double *__restrict__ Gb, int N, int L, int S, int states, int K, int marginal_term, uint32_t U,
            uint8_t *__restrict__ bp, double *__restrict__ vend, uint8_t *__restrict__ cend, vit_out *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char vitk_smem[];
    const int tid = threadIdx.x;
    const int sd = beam_src_doubles(L), su = sd / 2, R = L + 1;
    const int nslot = states * K;
    double *V = reinterpret_cast<double *>(vitk_smem);
    uint8_t *Cn = reinterpret_cast<uint8_t *>(V + 2 * (size_t)nslot);
    double *tab = reinterpret_cast<double *>(vitk_smem + 2 * (size_t)nslot * 8 + vitk_count_bytes(states));
    double2 *tab2 = reinterpret_cast<double2 *>(tab);
    const double2 *Gb2 = reinterpret_cast<const double2 *>(Gb);

    int slot_of[5];
    vit_slots(U, slot_of);
    // S = 1: one state whatever L is, reachable wherever there is no hole -- no digits, no masks (L may exceed VIT_MAX_LE)
    const bool one = S == 1;
    int pw = 1;                                               // S^(Le-1)
    for (int k = 1; k < L; k++) pw *= S;

    // what never changes of the slots this thread owns
    unsigned long long need[VIT_OWN], slots[VIT_OWN];
    int base[VIT_OWN], sj[VIT_OWN], sr[VIT_OWN];              // index of predecessor digit 0; the slot's state and rank
#pragma unroll
    for (int o = 0; o < VIT_OWN; o++) {
        const int s = tid + o * VIT_THREADS;
        need[o] = 0; slots[o] = 0; base[o] = 0;
        sj[o] = s / K; sr[o] = s - sj[o] * K;
        if (s < nslot && !one) {
            base[o] = (sj[o] % pw) * S;
            vit_own_digits(sj[o], S, L, slot_of, &need[o], &slots[o]);
        }
    }
    // the candidate masks of positions p, p-1, ... at bits 0, 5, ...; positions <= 0 offer digit 0 alone
    unsigned long long hist = 0;
    for (int k = 0; k < L && !one; k++) hist |= 1ull << (5 * k + slot_of[0]);
    const unsigned long long hmask = one ? 0 : (1ull << (5 * L)) - 1;

    for (int j = tid; j < 2 * states; j += VIT_THREADS) Cn[j] = 0;
    __syncthreads();
    if (tid == 0) { V[0] = 0.0; Cn[0] = 1; }                  // the one prefix at p = 0: every digit 0, score +0.0
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
        const double *Vc = V + (size_t)cur * nslot;
        double *Vn = V + (size_t)(cur ^ 1) * nslot;
        const uint8_t *Cc = Cn + (size_t)cur * states;
        uint8_t *Cw = Cn + (size_t)(cur ^ 1) * states;
        const int npre = L - 1 < p ? L - 1 : p;               // lags of the prefix
#pragma unroll
        for (int o = 0; o < VIT_OWN; o++) {
            const int s = tid + o * VIT_THREADS;
            if (s >= nslot) continue;
            const int j = sj[o], r = sr[o];
            if ((hist & need[o]) != need[o]) {
                if (r == 0) Cw[j] = 0;
                continue;
            }
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
            if (p < L) {
                // warm-up: the one predecessor, no lag Le; its list carries over in order
                const int n = Cc[base[o]];
                if (r < n) {
                    Vn[s] = Vc[(size_t)base[o] * K + r] + w;
                    bp[((size_t)p * states + j) * K + r] = (uint8_t)r;
                }
                if (r == 0) Cw[j] = (uint8_t)n;
                continue;
            }
            const double *src = STAGED ? tab + (size_t)tl * sd : Gb + (size_t)(p - L) * sd;
            // per offered predecessor digit: what every child of that list adds, and how many children the list has
            double wt[5];
            int cnt[5], total = 0;
#pragma unroll
            for (int x = 0; x < 5; x++) {
                wt[x] = 0.0; cnt[x] = 0;
                if (x < S) {
                    int sx = 0;
#pragma unroll
                    for (int q = 0; q < 5; q++)
                        if (q == x) sx = slot_of[q];
                    if ((cm_old >> sx) & 1u) {
                        const int a6 = p == L ? 5 : sx;
                        wt[x] = w + src[(a6 * L + (L - 1)) * LT_ROW + b];
                        cnt[x] = Cc[base[o] + x];
                        total += cnt[x];
                    }
                }
            }
            if (r == 0) Cw[j] = (uint8_t)(total < K ? total : K);
#pragma unroll
            for (int x = 0; x < 5; x++) {
                if (r >= cnt[x]) continue;
                const double mine = Vc[(size_t)(base[o] + x) * K + r] + wt[x];
                int place = r;
#pragma unroll
                for (int y = 0; y < 5; y++) {
                    if (y == x || cnt[y] == 0) continue;
                    // the children of list y that precede: a prefix of the list, since it is non-increasing
                    const double *Vy = Vc + (size_t)(base[o] + y) * K;
                    int lo = 0, hi = cnt[y];
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        const double other = Vy[mid] + wt[y];
                        const bool before = y < x ? other >= mine : other > mine;
                        if (before) lo = mid + 1;
                        else hi = mid;
                    }
                    place += lo;
                }
                if (place < K) {
                    Vn[(size_t)j * K + place] = mine;
                    bp[((size_t)p * states + j) * K + place] = (uint8_t)((x << 5) | r);
                }
            }
        }
        cur ^= 1;
        ts = ts + 1 == R ? 0 : ts + 1;
        beam_barrier();
    }
    if (tid == 0) out->hole_at = hole;
    if (!hole) {
        const double *Vc = V + (size_t)cur * nslot;
        const uint8_t *Cc = Cn + (size_t)cur * states;
#pragma unroll
        for (int o = 0; o < VIT_OWN; o++) {
            const int s = tid + o * VIT_THREADS;
            if (s < nslot) {
                const int n = (hist & need[o]) == need[o] ? Cc[sj[o]] : 0;
                vend[s] = sr[o] < n ? Vc[s] : 0.0;
                if (sr[o] == 0) cend[sj[o]] = (uint8_t)n;
            }
        }
    }
}

// dynamic LDS: the end scores (states * K doubles), then over them the back-pointers of `chunk` positions
__global__ void __launch_bounds__(VIT_THREADS)
k_vitk_trace(const uint8_t *__restrict__ bp, const double *__restrict__ vend, const uint8_t *__restrict__ cend, int N, int L, int S,
             int states, int K, int chunk, uint32_t U, symmap sm, vit_out *__restrict__ out, uint8_t *__restrict__ paths,
             double *__restrict__ ll, int32_t *__restrict__ n_out)
{
    extern __shared__ __attribute__((aligned(16))) char vitk_tsmem[];
    __shared__ int sel[GH_KBEST_MAX];
    __shared__ int n_all;
    const int tid = threadIdx.x;
    if (out->hole_at) return;                                 // (the same word in every thread)
    const int nslot = states * K;
    // the end rule by counting: an entry's place is the number of entries before it -- larger score, or equal score and smaller
    // slot index (ascending state, then rank).  A slot that holds nothing is NaN here: it compares false both ways.
    double *E = reinterpret_cast<double *>(vitk_tsmem);
    if (tid == 0) n_all = 0;
    __syncthreads();
    int mine_n = 0;
    for (int s = tid; s < nslot; s += VIT_THREADS) {
        const int j = s / K, r = s - j * K;
        const bool held = r < (int)cend[j];
        E[s] = held ? vend[s] : __longlong_as_double(0x7ff8000000000000ll);
        mine_n += held ? 1 : 0;
    }
    if (mine_n) atomicAdd(&n_all, mine_n);
    __syncthreads();
    const int n = n_all < K ? n_all : K;
    for (int s = tid; s < nslot; s += VIT_THREADS) {
        const double v = E[s];
        if (v != v) continue;
        int place = 0;
        for (int t = 0; t < nslot && place < K; t++) {
            const double u = E[t];
            place += (u > v || (u == v && t < s)) ? 1 : 0;
        }
        if (place < K) {
            sel[place] = s;
            ll[place] = v;
        }
    }
    __syncthreads();
    if (tid == 0) {
        *n_out = n;
        out->end_state = n;                                   // (it comes home with the vit_out)
        out->ll = E[sel[0]];
    }
    int slot_of[5];
    vit_slots(U, slot_of);
    int pw = 1;
    for (int k = 1; k < L; k++) pw *= S;
    int j = 0, r = 0;
    if (tid < n) {
        j = sel[tid] / K;
        r = sel[tid] - j * K;
        paths[(size_t)tid * (N + 1)] = SYM_US;
    }
    __syncthreads();                                          // (the scores are read: the chunks go over them)
    uint32_t *blk = reinterpret_cast<uint32_t *>(vitk_tsmem);
    const uint8_t *b8 = reinterpret_cast<const uint8_t *>(vitk_tsmem);
    for (int hi = N; hi >= 1; hi -= chunk) {
        const int lo = hi - chunk + 1 > 1 ? hi - chunk + 1 : 1;
        // (whole words per chunk: the scratch row is padded by four bytes, see vitk_layout)
        const size_t first = (size_t)lo * nslot, bytes = (size_t)(hi - lo + 1) * nslot;
        const size_t w0 = first / 4, w1 = (first + bytes + 3) / 4;
        const uint32_t *from = reinterpret_cast<const uint32_t *>(bp) + w0;
        for (size_t q = tid; q < w1 - w0; q += VIT_THREADS) blk[q] = from[q];
        __syncthreads();
        if (tid < n) {
            const size_t skew = first - w0 * 4;
            for (int q = hi; q >= lo; q--) {
                paths[(size_t)tid * (N + 1) + q] = (uint8_t)vsym(sm, slot_of[j / pw]);
                const int back = b8[skew + (size_t)(q - lo) * nslot + (size_t)j * K + r];
                j = (j % pw) * S + (back >> 5);
                r = back & 31;
            }
        }
        __syncthreads();
    }
}

// host ---------------------------------------------------------------------------------------- (vitk_bufs: scratch_layout.hpp)
// the refusal of a k whose lists do not fit
static int vitk_too_many(const char *who, int S, int L, int states, int k)
{
    return fail(GH_ERR_ARG, "%s: S = %d candidate symbols and Le = min(L, N) = %d make %d states, and k = %d prefixes a state make %d "
                "slots, more than the %d the exact decoder holds on chip: the largest k this window takes is %d", who, S, L, states, k,
                states * k, GH_VITERBI_MAX_STATES, GH_VITERBI_MAX_STATES / states);
}

// one k-best decoding of the tensor as it stands: the results stay in the handle's scratch (`b`), *ho = hole, n_out (in
// end_state), the best score and U
static int vitk_run(gh_handle *h, int k, vitk_bufs *b, vit_out *ho, const char *who)
{
    const int N = h->N, L = chain_lags(h);
    int rc, ns;
    if ((rc = vit_open(h, ho, who, &ns)) || !ns) return rc;
    const uint32_t U = ho->U;
    const int S = __builtin_popcount(U);
    if ((long long)ns * k > GH_VITERBI_MAX_STATES) return vitk_too_many(who, S, L, ns, k);
    const size_t table_doubles = (size_t)N * beam_src_doubles(L);
    const size_t need = vitk_layout(nullptr, N, table_doubles, ns, k).total;
    if ((rc = scratch_reserve(h, &h->vit, need, VIT_SCRATCH))) return rc;
    *b = vitk_layout(h->vit.buf, N, table_doubles, ns, k);
    if ((rc = chain_table_build(h, L, b->Gb))) return rc;

    const int nslot = ns * k;
    const size_t rows = 2 * (size_t)nslot * 8 + vitk_count_bytes(ns);
    if (!vit_no_stage() && L <= VIT_MAX_LE) {                   // (a longer state has S = 1: its ring need not fit)
        const size_t lds = rows + (size_t)(L + 1) * beam_src_doubles(L) * 8;
        lds_limit<k_vitk_walk<true>>(lds, h->dev);
        hipLaunchKernelGGL(k_vitk_walk<true>, dim3(1), dim3(VIT_THREADS), lds, h->stream, (const double *)b->Gb, N, L, S, ns, k,
                           h->cfg.marginal_term, U, b->bp, b->vend, b->cend, b->out);
    } else {
        lds_limit<k_vitk_walk<false>>(rows, h->dev);
        hipLaunchKernelGGL(k_vitk_walk<false>, dim3(1), dim3(VIT_THREADS), rows, h->stream, (const double *)b->Gb, N, L, S, ns, k,
                           h->cfg.marginal_term, U, b->bp, b->vend, b->cend, b->out);
    }
    if ((rc = post_launch(h, "k_vitk_walk"))) return rc;
    int chunk = VIT_TRACE_BYTES / nslot;
    if (chunk > VIT_TRACE_POS) chunk = VIT_TRACE_POS;
    const size_t tlds = std::max((size_t)chunk * nslot + 8, (size_t)nslot * 8);
    lds_limit<k_vitk_trace>(tlds, h->dev);
    hipLaunchKernelGGL(k_vitk_trace, dim3(1), dim3(VIT_THREADS), tlds, h->stream, (const uint8_t *)b->bp, (const double *)b->vend,
                       (const uint8_t *)b->cend, N, L, S, ns, k, chunk, U, h->sm, b->out, b->paths, b->ll, b->n_out);
    if ((rc = post_launch(h, "k_vitk_trace"))) return rc;
    HIPCHK(hipMemcpyAsync(ho, b->out, sizeof *ho, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->vit_last[0] = S; h->vit_last[1] = L; h->vit_last[2] = ns; h->vit_last[3] = (int64_t)need;
    return GH_OK;
}

extern "C" int gh_viterbi_kbest(gh_t *h, int k, uint8_t *paths_out, double *ll_chain, int *n_out, int *hole_at)
{
    if (!h || !paths_out || !ll_chain || !n_out || !hole_at) return fail(GH_ERR_ARG, "null argument");
    if (k < 1 || k > GH_KBEST_MAX) return fail(GH_ERR_ARG, "gh_viterbi_kbest: k = %d is outside 1..%d", k, GH_KBEST_MAX);
    int rc = decode_check(h, "gh_viterbi_kbest");
    if (rc) return rc;
    if (set_dev(h)) return GH_ERR_HIP;
    vitk_bufs b;
    vit_out ho;
    if ((rc = vitk_run(h, k, &b, &ho, "gh_viterbi_kbest"))) return rc;
    *hole_at = ho.hole_at;
    *n_out = 0;
    if (ho.hole_at) return GH_OK;
    const int n = ho.end_state;
    HIPCHK(hipMemcpyAsync(paths_out, b.paths, (size_t)n * ((size_t)h->N + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ll_chain, b.ll, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *n_out = n;
    return GH_OK;
}
