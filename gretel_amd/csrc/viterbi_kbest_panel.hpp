// viterbi_kbest_panel.hpp -- k-best decoding of the chain likelihood over every window of a batch or panel
// (gh_panel_viterbi_kbest, gh_panel_viterbi_kbest_info: include/gretel_hip.h).  A window's k-best decoder is one
// workgroup of walk and one of trace, the windows are independent: every window's walk runs in ONE launch (two where some windows
// walk without the table ring), every trace in one, block w of a launch taking window list[w] of the launch's list.  The rules are
// viterbi_panel.hpp's: no grid barrier, no shared counter, no assumption that all workgroups are resident -- a grid larger than
// the card drains in any order.  The definition, the arithmetic, the two tie orders and the layout of a window's scratch
// (vitk_layout, the handle's own block) are viterbi_kbest.hpp's, bit for bit.
//
//   vitk_win               one descriptor per window, in window order: the table, the shape, the state geometry, K_w, the parts of
//                          the window's vitk_layout block, the trace's chunk, the symbol map and where the window's rows and scores
//                          go in the batch's gathered arrays.  The descriptors, the launch list and the gathered results are a
//                          block of the batch (vitk_panel_layout).
//   k_vitk_walk_panel      block w walks window list[w]: vitk_walk_body<STAGED>, the statements of k_vitk_walk<STAGED>.  K is a
//                          run-time value there, so windows of differing K share a launch.  Windows that walk without the ring
//                          (S = 1 with Le > 12, or GH_VIT_STAGE=0) go in a launch of their own; a launch's dynamic LDS is the
//                          largest need among its windows (two score rows, two count rows, the ring: at most 109 KB).
//   k_vitk_trace_panel     block w traces window list[w]: vitk_trace_body, the statements of k_vitk_trace, into the window's own
//                          block (nothing where the walk met a hole).
//   k_vitk_home_panel      y: the window.  Its vit_out, and where there is no hole its n_out path rows and scores, gathered back
//                          to back in window order: three copies home where every window is full and the caller's offsets are
//                          the running sums, not three per window.  The trace does not write there directly: its statements stay
//                          k_vitk_trace's, and each handle's block holds what the single call leaves in it.
//
// THE BODIES.  k_vitk_walk and k_vitk_trace of viterbi_kbest.hpp stay as they are, text and instructions; their statements stand
// here a second time, in __forceinline__ functions behind a prologue that reads the descriptor, for the reason viterbi_panel.hpp
// gives (tried once more here, with the single-window kernels as thin shells over these bodies: docs/HISTORY.md has the figures).
// ---------------------------------------------------------------------------------------------

struct vitk_win {
    const double *Gb;          // the window's chain table (vitk_bufs::Gb)
    const double *minfo;       // the handle's marginal table: the union reads the candidate bits
    vit_out *out;
    uint8_t *bp;
    double *vend;
    uint8_t *cend;
    uint8_t *paths;
    double *ll;
    int32_t *n_out;
    int64_t row_home, ll_home; // where the window's rows (bytes) and scores (doubles) go in the batch's gathered arrays
    int N, Le, S, states, K, marginal_term, chunk;   // chunk: positions the trace holds in LDS at a time
    uint32_t U;
    symmap sm;
};
static_assert(sizeof(vitk_win) == 128, "the size tests/native/vitk_panel_layout.cpp lays the descriptor array out with");
static_assert(sizeof(vit_win) <= sizeof(vitk_win), "the union launch's descriptors stand where these will");

// dynamic LDS: [two score rows of states * K doubles] [two count rows of `states` bytes] [STAGED: Le + 1 source blocks]
template <bool STAGED>
__device__ __forceinline__ void
vitk_walk_body(const double *__restrict__ Gb, int N, int L, int S, int states, int K, int marginal_term, uint32_t U,
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
__device__ __forceinline__ void
vitk_trace_body(const uint8_t *__restrict__ bp, const double *__restrict__ vend, const uint8_t *__restrict__ cend, int N, int L, int S,
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

template <bool STAGED>
__global__ void __launch_bounds__(VIT_THREADS)
k_vitk_walk_panel(const vitk_win *__restrict__ wd, const int32_t *__restrict__ list)
{
    const vitk_win &d = wd[list[blockIdx.x]];
    vitk_walk_body<STAGED>(d.Gb, d.N, d.Le, d.S, d.states, d.K, d.marginal_term, d.U, d.bp, d.vend, d.cend, d.out);
}

__global__ void __launch_bounds__(VIT_THREADS)
k_vitk_trace_panel(const vitk_win *__restrict__ wd, const int32_t *__restrict__ list)
{
    const vitk_win &d = wd[list[blockIdx.x]];
    vitk_trace_body(d.bp, d.vend, d.cend, d.N, d.Le, d.S, d.states, d.K, d.chunk, d.U, d.sm, d.out, d.paths, d.ll, d.n_out);
}

// y: the window; x strides over its bytes.  outs is in window order, as the descriptors are.
__global__ void __launch_bounds__(256)
k_vitk_home_panel(const vitk_win *__restrict__ wd, const int32_t *__restrict__ list, int cnt, vit_out *__restrict__ outs,
                  uint8_t *__restrict__ paths, double *__restrict__ ll)
{
    for (int i = blockIdx.y; i < cnt; i += gridDim.y) {
        const int w = list[i];
        const vitk_win &d = wd[w];
        const vit_out o = *d.out;
        if (blockIdx.x == 0 && threadIdx.x == 0) outs[w] = o;
        if (o.hole_at) continue;
        const int n = o.end_state < d.K ? o.end_state : d.K;    // (k_vitk_trace: how many paths it returned)
        const size_t bytes = (size_t)n * ((size_t)d.N + 1), step = (size_t)gridDim.x * blockDim.x;
        const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        uint8_t *to = paths + (size_t)d.row_home;
        for (size_t q = first; q < bytes; q += step) to[q] = d.paths[q];
        for (size_t q = first; q < (size_t)n; q += step) ll[(size_t)d.ll_home + q] = d.ll[q];
    }
}

// host ----------------------------------------------------------------------------------------
// STREAM ORDER, as viterbi_panel.hpp's: a window's marginal tables and chain table on its handle's stream, an event per window
// before the batch's stream, everything panel-wide on the batch's stream, and the host waits for the batch's stream before it
// touches a handle.  The call returns with the batch's stream idle.
typedef vitk_panel_bufs<vitk_win> vitkp_bufs;

extern "C" int gh_panel_viterbi_kbest(gh_batch_t *b, const int *k, uint8_t *paths_out, const int64_t *paths_off, double *ll_chain,
                                      const int64_t *ll_off, int *n_out, int *hole_at)
{
    static const char WHO[] = "gh_panel_viterbi_kbest";
    if (!b || !k || !paths_out || !paths_off || !ll_chain || !ll_off || !n_out || !hole_at) return fail(GH_ERR_ARG, "null argument");
    const int n = b->n;
    int rc;
    for (int w = 0; w < n; w++) {
        if (paths_off[w] < 0 || ll_off[w] < 0) return fail(GH_ERR_ARG, "%s: window %d has a negative offset", WHO, w);
        if (k[w] < 1 || k[w] > GH_KBEST_MAX) return fail(GH_ERR_ARG, "window %d: %s: k = %d is outside 1..%d", w, WHO, k[w], GH_KBEST_MAX);
        if ((rc = decode_check(b->hs[w], WHO))) return vitp_window_fail(rc, w);
    }
    HIPCHK(hipSetDevice(b->dev));
    while ((int)b->vit_ev.size() < n) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        b->vit_ev.push_back(e);
    }
    // window w's first byte in the gathered rows and its first score: the running sums of k_w (N_w + 1) and of k_w
    std::vector<int64_t> rhome((size_t)n + 1, 0), lhome((size_t)n + 1, 0);
    for (int w = 0; w < n; w++) {
        rhome[w + 1] = rhome[w] + (int64_t)k[w] * (b->hs[w]->N + 1);
        lhome[w + 1] = lhome[w] + k[w];
    }
    if ((rc = vitp_reserve(b, vitk_panel_layout<vitk_win>(nullptr, n, (size_t)rhome[n], (size_t)lhome[n]).total))) return rc;
    const vitkp_bufs pb = vitk_panel_layout<vitk_win>(b->vit.buf, n, (size_t)rhome[n], (size_t)lhome[n]);
    std::vector<vitk_win> wd((size_t)n);
    std::vector<vit_out> outs((size_t)n);
    vitp_clock clock(b);                                        // (gh_debug_panel_viterbi_phases: a measuring pass)

    // The refusals, as a whole, before any window's scratch or viterbi_info is touched: every window's U straight into the batch's
    // own gathered array, by the exact decoder's union launch over its own descriptors, which stand for that launch where the
    // k-best descriptors will (only the marginal tables, a cache of the tensor, are brought up to date on the way)
    {
        std::vector<vit_win> uw((size_t)n);
        for (int w = 0; w < n; w++) {
            gh_handle *h = b->hs[w];
            if ((rc = ensure_marg(h))) return vitp_window_fail(rc, w);
            if ((rc = vitp_after_handle(b, w))) return rc;
            memset(&uw[w], 0, sizeof(vit_win));
            uw[w].minfo = h->minfo; uw[w].N = h->N; uw[w].out = pb.outs + w;
        }
        HIPCHK(hipMemcpyAsync(pb.wd, uw.data(), sizeof(vit_win) * n, hipMemcpyHostToDevice, b->stream));
        hipLaunchKernelGGL(k_vit_union_panel, dim3(n), dim3(256), 0, b->stream, (const vit_win *)(const void *)pb.wd);
        if ((rc = vitp_post(b, "k_vit_union_panel"))) return rc;
        HIPCHK(hipMemcpyAsync(outs.data(), pb.outs, sizeof(vit_out) * n, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));                // (uw is read by then)
    }
    std::vector<int> ns((size_t)n);
    std::vector<size_t> need((size_t)n);
    size_t asked = 0;                                           // what the whole panel asks of the handles' blocks
    for (int w = 0; w < n; w++) {
        const gh_handle *h = b->hs[w];
        const int S = __builtin_popcount(outs[w].U), Le = chain_lags(h);
        const long long st = S ? vit_states(S, Le) : 0;
        if (st > GH_VITERBI_MAX_STATES) return vitp_window_fail(vit_too_many(WHO, S, Le), w);
        if (st * k[w] > GH_VITERBI_MAX_STATES) return vitp_window_fail(vitk_too_many(WHO, S, Le, (int)st, k[w]), w);
        ns[w] = (int)st;
        // (nothing offered anywhere: the vit_out alone, as vit_open leaves the block)
        need[w] = st ? vitk_layout(nullptr, h->N, (size_t)h->N * beam_src_doubles(Le), ns[w], k[w]).total : vit_layout(nullptr, h->N, 0, 0).total;
        asked += need[w];
    }

    // every window's block, its handle's own under vitk_layout, before the first walk is launched
    for (int w = 0; w < n; w++) {
        gh_handle *h = b->hs[w];
        if ((rc = scratch_reserve(h, &h->vit, need[w], VIT_SCRATCH))) {
            if (rc != GH_ERR_NOMEM) return vitp_window_fail(rc, w);
            const std::string msg = g_err;
            return fail(rc, "window %d: %s; the panel's %d windows ask for %zu bytes in all ((N + 1) * states * k a window, the tables and "
                        "the small parts)", w, msg.c_str(), n, asked);
        }
    }

    // per window: the table on its own stream, the descriptor, the list (walks with the ring first)
    const bool no_stage = vit_no_stage();
    std::vector<int32_t> list((size_t)n);
    std::vector<int> plain;
    int n_staged = 0, max_n = 0;
    size_t lds_walk[2] = {0, 0}, lds_trace = 0;
    int64_t holes = 0, bytes = 0;
    for (int w = 0; w < n; w++) {
        gh_handle *h = b->hs[w];
        const int Le = chain_lags(h), S = __builtin_popcount(outs[w].U);
        n_out[w] = 0;
        hole_at[w] = 0;
        if (!ns[w]) {                                           // nothing offered anywhere: the hole is the first position
            hole_at[w] = 1;
            holes++;
            h->vit_last[0] = 0; h->vit_last[1] = Le; h->vit_last[2] = 0; h->vit_last[3] = (int64_t)h->vit.cap;
            bytes += h->vit_last[3];
            continue;
        }
        const vitk_bufs vb = vitk_layout(h->vit.buf, h->N, (size_t)h->N * beam_src_doubles(Le), ns[w], k[w]);
        if ((rc = chain_table_build(h, Le, vb.Gb))) return vitp_window_fail(rc, w);
        if ((rc = vitp_after_handle(b, w))) return rc;
        const int nslot = ns[w] * k[w];
        vitk_win &d = wd[w];
        memset(&d, 0, sizeof d);
        d.Gb = vb.Gb; d.minfo = h->minfo; d.out = vb.out; d.bp = vb.bp; d.vend = vb.vend; d.cend = vb.cend; d.paths = vb.paths; d.ll = vb.ll;
        d.n_out = vb.n_out; d.row_home = rhome[w]; d.ll_home = lhome[w];
        d.N = h->N; d.Le = Le; d.S = S; d.states = ns[w]; d.K = k[w]; d.marginal_term = h->cfg.marginal_term;
        d.chunk = VIT_TRACE_BYTES / nslot > VIT_TRACE_POS ? VIT_TRACE_POS : VIT_TRACE_BYTES / nslot;
        d.U = outs[w].U;
        d.sm = h->sm;
        max_n = std::max(max_n, h->N);
        // (gh_viterbi_kbest's decisions, window by window)
        const size_t rows = 2 * (size_t)nslot * 8 + vitk_count_bytes(ns[w]);
        if (!no_stage && Le <= VIT_MAX_LE) {                    // (a longer state has S = 1: its ring need not fit)
            list[n_staged++] = w;
            lds_walk[0] = std::max(lds_walk[0], rows + (size_t)(Le + 1) * beam_src_doubles(Le) * 8);
        } else {
            plain.push_back(w);
            lds_walk[1] = std::max(lds_walk[1], rows);
        }
        lds_trace = std::max(lds_trace, std::max((size_t)d.chunk * nslot + 8, (size_t)nslot * 8));
    }
    int cnt = n_staged;                                         // the windows that walk at all
    for (int w : plain) list[cnt++] = w;
    int64_t launches = 0;
    if (cnt) {
        const unsigned gy = (unsigned)std::min(cnt, 65535);
        HIPCHK(hipMemcpyAsync(pb.wd, wd.data(), sizeof(vitk_win) * n, hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(pb.list, list.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, b->stream));
        clock(0);
        if (n_staged) {
            lds_limit<k_vitk_walk_panel<true>>(lds_walk[0], b->dev);
            hipLaunchKernelGGL(k_vitk_walk_panel<true>, dim3(n_staged), dim3(VIT_THREADS), lds_walk[0], b->stream, (const vitk_win *)pb.wd,
                               (const int32_t *)pb.list);
            if ((rc = vitp_post(b, "k_vitk_walk_panel"))) return rc;
            launches++;
        }
        if (cnt > n_staged) {
            lds_limit<k_vitk_walk_panel<false>>(lds_walk[1], b->dev);
            hipLaunchKernelGGL(k_vitk_walk_panel<false>, dim3(cnt - n_staged), dim3(VIT_THREADS), lds_walk[1], b->stream,
                               (const vitk_win *)pb.wd, (const int32_t *)pb.list + n_staged);
            if ((rc = vitp_post(b, "k_vitk_walk_panel"))) return rc;
            launches++;
        }
        clock(1);
        lds_limit<k_vitk_trace_panel>(lds_trace, b->dev);
        hipLaunchKernelGGL(k_vitk_trace_panel, dim3(cnt), dim3(VIT_THREADS), lds_trace, b->stream, (const vitk_win *)pb.wd,
                           (const int32_t *)pb.list);
        if ((rc = vitp_post(b, "k_vitk_trace_panel"))) return rc;
        clock(2);
        // the gather, then the vit_outs home: they say how many rows a window has and where the holes are
        hipLaunchKernelGGL(k_vitk_home_panel, dim3((unsigned)std::min<size_t>(((size_t)max_n + 256) / 256 * 4, 64), gy), dim3(256), 0, b->stream,
                           (const vitk_win *)pb.wd, (const int32_t *)pb.list, cnt, pb.outs, pb.paths, pb.ll);
        if ((rc = vitp_post(b, "k_vitk_home_panel"))) return rc;
        HIPCHK(hipMemcpyAsync(outs.data(), pb.outs, sizeof(vit_out) * n, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        std::vector<int> got((size_t)n, 0);
        for (int w = 0; w < n; w++) {
            gh_handle *h = b->hs[w];
            if (!ns[w]) continue;
            h->vit_last[0] = wd[w].S; h->vit_last[1] = wd[w].Le; h->vit_last[2] = ns[w]; h->vit_last[3] = (int64_t)need[w];
            bytes += h->vit_last[3];
            hole_at[w] = outs[w].hole_at;
            if (outs[w].hole_at) { holes++; continue; }
            got[w] = std::min(outs[w].end_state, k[w]);
        }
        // rows and scores home: one copy each per run of neighbouring FULL windows (n_out = k, no hole) whose destinations lie as
        // the gathered ranges do -- one run where the caller's offsets are the running sums and every window is full; a window
        // with fewer rows than it asked for is a run of its own, of the rows it has
        for (int w = 0; w < n;) {
            if (!got[w]) { w++; continue; }
            int e = w + 1;
            size_t row_bytes = (size_t)got[w] * ((size_t)b->hs[w]->N + 1), scores = (size_t)got[w];
            if (got[w] == k[w]) {
                while (e < n && got[e] == k[e] && paths_off[e] - rhome[e] == paths_off[w] - rhome[w] && ll_off[e] - lhome[e] == ll_off[w] - lhome[w])
                    e++;
                row_bytes = (size_t)(rhome[e] - rhome[w]);
                scores = (size_t)(lhome[e] - lhome[w]);
            }
            HIPCHK(hipMemcpyAsync(paths_out + paths_off[w], pb.paths + rhome[w], row_bytes, hipMemcpyDeviceToHost, b->stream));
            HIPCHK(hipMemcpyAsync(ll_chain + ll_off[w], pb.ll + lhome[w], scores * sizeof(double), hipMemcpyDeviceToHost, b->stream));
            w = e;
        }
        HIPCHK(hipStreamSynchronize(b->stream));
        for (int w = 0; w < n; w++) n_out[w] = got[w];
        clock(3);
    }
    b->vitk_info[0] = n; b->vitk_info[1] = holes; b->vitk_info[2] = launches; b->vitk_info[3] = bytes;
    return GH_OK;
}

extern "C" int gh_panel_viterbi_kbest_info(gh_batch_t *b, int64_t out[4])
{
    if (!b || !out) return fail(GH_ERR_ARG, "null argument");
    for (int q = 0; q < 4; q++) out[q] = b->vitk_info[q];
    return GH_OK;
}
