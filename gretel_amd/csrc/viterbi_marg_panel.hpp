// viterbi_marg_panel.hpp -- the max-marginals of the chain likelihood over every window of a batch or panel
// (gh_panel_viterbi_marginals, gh_panel_viterbi_marginals_info: include/gretel_hip.h).  A window's forward walk
// and its backward walk are one workgroup each, the windows are independent: every window's forward walk runs in ONE launch
// (two where some windows walk without the table ring), every backward walk likewise, block w of a launch taking window w of the
// launch's list.  The rules are viterbi_panel.hpp's: no grid barrier, no shared counter, no assumption that all workgroups are
// resident -- a grid larger than the card drains in any order.  The definition, the arithmetic and the layout of a window's
// scratch (vitm_layout, the handle's own block) are viterbi_marg.hpp's, bit for bit.
//
//   vitm_win               one descriptor per window, in window order: the table, the shape, the state geometry, the parts of the
//                          window's vitm_layout block, the marginal table and the symbol map.  A launch takes a list of window
//                          indices beside the descriptors (the forward and the backward walk split the windows differently); the
//                          descriptors, the lists and the gathered results are a block of the batch (vitm_panel_layout).
//   k_vitm_union_panel     block w: U of window w (vit_union_body, viterbi_panel.hpp).
//   k_vit_cands_panel      k_vit_cands over a 2-D grid: y the window, x strides over positions.
//   k_vit_keep_panel       block w walks window w forward and keeps F: vit_walk_body<STAGED, KEEP = true> (viterbi_panel.hpp), the
//                          statements of k_vit_walk<STAGED, true>.  Windows that walk without the ring (S = 1 with Le > 12, or
//                          GH_VIT_STAGE=0) go in a launch of their own; a launch's dynamic LDS is the largest need among its windows.
//   k_vit_back_panel       block w walks window w backward.  Staged where two rows of B, two of prefixes and the ring of Le + 2
//                          blocks fit BEAM_LDS_MAX, the decision of gh_viterbi_marginals per window; the others in a launch of
//                          the global-memory loader.  At the cap a workgroup takes a CU's whole LDS: one workgroup a CU, the rest
//                          of the grid waits its turn.
//   k_vit_mm_panel         k_vit_mm over a 2-D grid (y the window), the same NaN-skipping maximum, into the window's own mm.
//   k_vit_mhome_panel      the vit_outs, and for windows without a hole their mm and cm, gathered back to back in window order:
//                          three copies home where the windows' destinations lie as the gathered ranges do, not two per window.
//
// THE BODIES.  k_vit_cands, k_vit_back and k_vit_mm of viterbi_marg.hpp stay as they are, text and instructions; their statements
// stand here a second time behind a prologue that reads the descriptor, for the reason viterbi_panel.hpp gives (moved into
// shared __device__ functions the single-window kernels came out with other instructions: docs/HISTORY.md).  vit_walk_body took
// a KEEP switch instead: both k_vit_walk_panel instantiations compile to the instructions they had (scratch/device_isa_cmp.py).
// ---------------------------------------------------------------------------------------------

struct vitm_win {
    const double *Gb;          // the window's chain table (vitm_bufs::Gb)
    const double *minfo;       // the handle's marginal table: the union and the candidate bits
    vit_out *out;
    double *fb;
    uint8_t *cm5;
    double *mm;
    uint8_t *cm;
    int64_t home;              // where mm and cm go in the batch's gathered arrays, in positions
    int N, Le, S, states, pw, marginal_term;         // pw = S^(Le-1)
    uint32_t U;
    symmap sm;
};
static_assert(sizeof(vitm_win) == 104, "the size tests/native/vitm_panel_layout.cpp lays the descriptor array out with");

__global__ void __launch_bounds__(256)
k_vitm_union_panel(const vitm_win *__restrict__ wd)
{
    const vitm_win &d = wd[blockIdx.x];
    vit_union_body(d.minfo, d.N, d.out);
}

__global__ void __launch_bounds__(256)
k_vit_cands_panel(const vitm_win *__restrict__ wd, const int32_t *__restrict__ list, int cnt)
{
    for (int i = blockIdx.y; i < cnt; i += gridDim.y) {
        const vitm_win &d = wd[list[i]];
        const double *__restrict__ minfo = d.minfo;
        const int N = d.N;
        const symmap sm = d.sm;
        uint8_t *__restrict__ cm5 = d.cm5, *__restrict__ cm = d.cm;
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
}

template <bool STAGED>
__global__ void __launch_bounds__(VIT_THREADS)
k_vit_keep_panel(const vitm_win *__restrict__ wd, const int32_t *__restrict__ list)
{
    const vitm_win &d = wd[list[blockIdx.x]];
    vit_walk_body<STAGED, true>(d.Gb, d.N, d.Le, d.S, d.states, d.marginal_term, d.U, nullptr, d.fb, nullptr, d.out);
}

// dynamic LDS: [two rows of B] [two rows of prefixes] [STAGED: Le + 2 source blocks] -- k_vit_back's statements
template <bool STAGED>
__global__ void __launch_bounds__(VIT_THREADS)
k_vit_back_panel(const vitm_win *__restrict__ wd, const int32_t *__restrict__ list)
{
    extern __shared__ __attribute__((aligned(16))) char vitb_smem[];
    const vitm_win &d = wd[list[blockIdx.x]];
    const double *__restrict__ Gb = d.Gb;
    const uint8_t *__restrict__ cm5 = d.cm5;
    const int N = d.N, L = d.Le, S = d.S, states = d.states, marginal_term = d.marginal_term, pw = d.pw;
    const uint32_t U = d.U;
    double *__restrict__ fb = d.fb;
    const vit_out *__restrict__ out = d.out;

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

// one position a workgroup at a time -- k_vit_mm's statements
__global__ void __launch_bounds__(256)
k_vit_mm_panel(const vitm_win *__restrict__ wd, const int32_t *__restrict__ list, int cnt)
{
    __shared__ double red[5][256];
    const int tid = threadIdx.x;
    const double none = __longlong_as_double(0x7ff8000000000000ll);
    for (int i = blockIdx.y; i < cnt; i += gridDim.y) {
        const vitm_win &d = wd[list[i]];
        if (d.out->hole_at) continue;                         // (the same word in every thread)
        const double *__restrict__ fb = d.fb;
        const uint8_t *__restrict__ cm5 = d.cm5;
        const int N = d.N, S = d.S, states = d.states, pw = d.pw;
        const symmap sm = d.sm;
        double *__restrict__ mm = d.mm;
        int slot_of[5];
        vit_slots(d.U, slot_of);
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
}

// y: the window; x strides over its positions.  outs is in window order, as the descriptors are.
__global__ void __launch_bounds__(256)
k_vit_mhome_panel(const vitm_win *__restrict__ wd, const int32_t *__restrict__ list, int cnt, vit_out *__restrict__ outs,
                  double *__restrict__ mm, uint8_t *__restrict__ cm)
{
    for (int i = blockIdx.y; i < cnt; i += gridDim.y) {
        const int w = list[i];
        const vitm_win &d = wd[w];
        const vit_out o = *d.out;
        if (blockIdx.x == 0 && threadIdx.x == 0) outs[w] = o;
        if (o.hole_at) continue;
        const size_t n1 = (size_t)d.N + 1, step = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        double *to = mm + (size_t)d.home * GH_NSYM;
        for (size_t q = first; q < n1 * GH_NSYM; q += step) to[q] = d.mm[q];
        for (size_t q = first; q < n1; q += step) cm[(size_t)d.home + q] = d.cm[q];
    }
}

// host ----------------------------------------------------------------------------------------
// STREAM ORDER, as viterbi_panel.hpp's: a window's marginal tables and chain table on its handle's stream, an event per window
// before the batch's stream, everything panel-wide on the batch's stream, and the host waits for the batch's stream before it
// touches a handle.  The call returns with the batch's stream idle.
typedef vitm_panel_bufs<vitm_win> vitmp_bufs;

extern "C" int gh_panel_viterbi_marginals(gh_batch_t *b, double *mm, uint8_t *cm, const int64_t *pos_off, int *hole_at)
{
    static const char WHO[] = "gh_panel_viterbi_marginals";
    if (!b || !mm || !cm || !pos_off || !hole_at) return fail(GH_ERR_ARG, "null argument");
    const int n = b->n;
    int rc;
    for (int w = 0; w < n; w++) {
        if (pos_off[w] < 0) return fail(GH_ERR_ARG, "%s: window %d has a negative offset", WHO, w);
        if ((rc = decode_check(b->hs[w], WHO))) return vitp_window_fail(rc, w);
    }
    HIPCHK(hipSetDevice(b->dev));
    while ((int)b->vit_ev.size() < n) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        b->vit_ev.push_back(e);
    }
    std::vector<int64_t> home((size_t)n + 1, 0);                // window w's first position in the gathered mm and cm
    for (int w = 0; w < n; w++) home[w + 1] = home[w] + b->hs[w]->N + 1;
    if ((rc = vitp_reserve(b, vitm_panel_layout<vitm_win>(nullptr, n, (size_t)home[n]).total))) return rc;
    const vitmp_bufs pb = vitm_panel_layout<vitm_win>(b->vit.buf, n, (size_t)home[n]);
    std::vector<vitm_win> wd((size_t)n);
    std::vector<vit_out> outs((size_t)n);
    vitp_clock clock(b);                                        // (gh_debug_panel_viterbi_phases: a measuring pass)

    // The refusals, as a whole, before any window's scratch or viterbi_info is touched: every window's U straight into the batch's
    // own gathered array (only the marginal tables, a cache of the tensor, are brought up to date on the way)
    for (int w = 0; w < n; w++) {
        gh_handle *h = b->hs[w];
        if ((rc = ensure_marg(h))) return vitp_window_fail(rc, w);
        if ((rc = vitp_after_handle(b, w))) return rc;
        memset(&wd[w], 0, sizeof(vitm_win));
        wd[w].minfo = h->minfo; wd[w].N = h->N; wd[w].out = pb.outs + w;
    }
    HIPCHK(hipMemcpyAsync(pb.wd, wd.data(), sizeof(vitm_win) * n, hipMemcpyHostToDevice, b->stream));
    hipLaunchKernelGGL(k_vitm_union_panel, dim3(n), dim3(256), 0, b->stream, (const vitm_win *)pb.wd);
    if ((rc = vitp_post(b, "k_vitm_union_panel"))) return rc;
    HIPCHK(hipMemcpyAsync(outs.data(), pb.outs, sizeof(vit_out) * n, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    std::vector<int> ns((size_t)n);
    size_t asked = 0;                                           // what the whole panel asks of the handles' blocks
    for (int w = 0; w < n; w++) {
        const gh_handle *h = b->hs[w];
        const int S = __builtin_popcount(outs[w].U), Le = chain_lags(h);
        const long long st = S ? vit_states(S, Le) : 0;
        if (st > GH_VITERBI_MAX_STATES) return vitp_window_fail(vit_too_many(WHO, S, Le), w);
        ns[w] = (int)st;
        asked += vitm_layout(nullptr, h->N, (size_t)h->N * beam_src_doubles(Le), ns[w]).total;
    }

    // every window's block, its handle's own under vitm_layout, before the first walk is launched
    for (int w = 0; w < n; w++) {
        gh_handle *h = b->hs[w];
        const int Le = chain_lags(h);
        const size_t need = vitm_layout(nullptr, h->N, (size_t)h->N * beam_src_doubles(Le), ns[w]).total;
        if ((rc = scratch_reserve(h, &h->vit, need, VIT_SCRATCH))) {
            if (rc != GH_ERR_NOMEM) return vitp_window_fail(rc, w);
            const std::string msg = g_err;
            return fail(rc, "window %d: %s; the panel's %d windows ask for %zu bytes in all (N * states * 8 a window and the small parts)",
                        w, msg.c_str(), n, asked);
        }
    }

    // per window: the table on its own stream, the descriptor, the lists (walks with the ring first)
    const bool no_stage = vit_no_stage();
    std::vector<int32_t> list(2 * (size_t)n);
    std::vector<int> fwd_plain, back_plain;
    int n_fwd = 0, n_back = 0, max_n = 0;
    size_t lds_fwd[2] = {0, 0}, lds_back[2] = {0, 0};
    int64_t holes = 0, bytes = 0;
    for (int w = 0; w < n; w++) {
        gh_handle *h = b->hs[w];
        const int Le = chain_lags(h), S = __builtin_popcount(outs[w].U);
        if (!ns[w]) {                                           // nothing offered anywhere: the hole is the first position
            hole_at[w] = 1;
            holes++;
            h->vit_last[0] = 0; h->vit_last[1] = Le; h->vit_last[2] = 0; h->vit_last[3] = (int64_t)h->vit.cap;
            bytes += h->vit_last[3];
            continue;
        }
        const size_t td = (size_t)h->N * beam_src_doubles(Le);
        const vitm_bufs vb = vitm_layout(h->vit.buf, h->N, td, ns[w]);
        if ((rc = chain_table_build(h, Le, vb.Gb))) return vitp_window_fail(rc, w);
        if ((rc = vitp_after_handle(b, w))) return rc;
        vitm_win &d = wd[w];
        d.Gb = vb.Gb; d.minfo = h->minfo; d.out = vb.out; d.fb = vb.fb; d.cm5 = vb.cm5; d.mm = vb.mm; d.cm = vb.cm;
        d.home = home[w]; d.N = h->N; d.Le = Le; d.S = S; d.states = ns[w]; d.marginal_term = h->cfg.marginal_term;
        d.pw = 1;
        for (int k = 1; k < Le; k++) d.pw *= S;
        d.U = outs[w].U;
        d.sm = h->sm;
        max_n = std::max(max_n, h->N);
        // (gh_viterbi_marginals' decisions, window by window)
        const bool stage = !no_stage && Le <= VIT_MAX_LE;       // (a longer state has S = 1: its ring need not fit)
        const size_t ring = (size_t)(Le + 1) * beam_src_doubles(Le) * 8, bring = (size_t)(Le + 2) * beam_src_doubles(Le) * 8;
        const size_t rows = 2 * (size_t)ns[w] * 8;
        if (stage) { list[n_fwd++] = w; lds_fwd[0] = std::max(lds_fwd[0], rows + ring); }
        else { fwd_plain.push_back(w); lds_fwd[1] = std::max(lds_fwd[1], rows); }
        if (stage && 2 * rows + bring <= BEAM_LDS_MAX) { list[n + n_back++] = w; lds_back[0] = std::max(lds_back[0], 2 * rows + bring); }
        else { back_plain.push_back(w); lds_back[1] = std::max(lds_back[1], 2 * rows); }
    }
    const int n_fwd_staged = n_fwd, n_back_staged = n_back;
    for (int w : fwd_plain) list[n_fwd++] = w;
    for (int w : back_plain) list[n + n_back++] = w;
    const int cnt = n_fwd;                                      // the windows that walk at all
    int64_t launches = 0;
    if (cnt) {
        const int32_t *fl = pb.list, *bl = pb.list + n;
        const unsigned gy = (unsigned)std::min(cnt, 65535);
        HIPCHK(hipMemcpyAsync(pb.wd, wd.data(), sizeof(vitm_win) * n, hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(pb.list, list.data(), sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, b->stream));
        hipLaunchKernelGGL(k_vit_cands_panel, dim3((unsigned)std::min<size_t>(((size_t)max_n + 256) / 256, 1024), gy), dim3(256), 0, b->stream,
                           (const vitm_win *)pb.wd, fl, cnt);
        if ((rc = vitp_post(b, "k_vit_cands_panel"))) return rc;
        clock(0);
        if (n_fwd_staged) {
            lds_limit<k_vit_keep_panel<true>>(lds_fwd[0], b->dev);
            hipLaunchKernelGGL(k_vit_keep_panel<true>, dim3(n_fwd_staged), dim3(VIT_THREADS), lds_fwd[0], b->stream, (const vitm_win *)pb.wd, fl);
            if ((rc = vitp_post(b, "k_vit_keep_panel"))) return rc;
            launches++;
        }
        if (cnt > n_fwd_staged) {
            lds_limit<k_vit_keep_panel<false>>(lds_fwd[1], b->dev);
            hipLaunchKernelGGL(k_vit_keep_panel<false>, dim3(cnt - n_fwd_staged), dim3(VIT_THREADS), lds_fwd[1], b->stream,
                               (const vitm_win *)pb.wd, fl + n_fwd_staged);
            if ((rc = vitp_post(b, "k_vit_keep_panel"))) return rc;
            launches++;
        }
        clock(1);
        if (n_back_staged) {
            lds_limit<k_vit_back_panel<true>>(lds_back[0], b->dev);
            hipLaunchKernelGGL(k_vit_back_panel<true>, dim3(n_back_staged), dim3(VIT_THREADS), lds_back[0], b->stream, (const vitm_win *)pb.wd, bl);
            if ((rc = vitp_post(b, "k_vit_back_panel"))) return rc;
            launches++;
        }
        if (cnt > n_back_staged) {
            lds_limit<k_vit_back_panel<false>>(lds_back[1], b->dev);
            hipLaunchKernelGGL(k_vit_back_panel<false>, dim3(cnt - n_back_staged), dim3(VIT_THREADS), lds_back[1], b->stream,
                               (const vitm_win *)pb.wd, bl + n_back_staged);
            if ((rc = vitp_post(b, "k_vit_back_panel"))) return rc;
            launches++;
        }
        clock(2);
        hipLaunchKernelGGL(k_vit_mm_panel, dim3((unsigned)std::min(max_n + 1, 4096), gy), dim3(256), 0, b->stream, (const vitm_win *)pb.wd, fl, cnt);
        if ((rc = vitp_post(b, "k_vit_mm_panel"))) return rc;
        hipLaunchKernelGGL(k_vit_mhome_panel, dim3((unsigned)std::min<size_t>(((size_t)max_n + 256) / 256, 64), gy), dim3(256), 0, b->stream,
                           (const vitm_win *)pb.wd, fl, cnt, pb.outs, pb.mm, pb.cm);
        if ((rc = vitp_post(b, "k_vit_mhome_panel"))) return rc;
        HIPCHK(hipMemcpyAsync(outs.data(), pb.outs, sizeof(vit_out) * n, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        for (int w = 0; w < n; w++) {
            gh_handle *h = b->hs[w];
            if (!ns[w]) continue;
            h->vit_last[0] = wd[w].S; h->vit_last[1] = wd[w].Le; h->vit_last[2] = ns[w];
            h->vit_last[3] = (int64_t)vitm_layout(nullptr, h->N, (size_t)h->N * beam_src_doubles(wd[w].Le), ns[w]).total;
            bytes += h->vit_last[3];
            hole_at[w] = outs[w].hole_at;
            if (outs[w].hole_at) holes++;
        }
        // mm and cm home: one copy each per run of neighbouring windows without a hole whose destinations lie as the gathered
        // ranges do -- one run where the caller's offsets are the running sum of N_w + 1 and no window met a hole
        for (int w = 0; w < n;) {
            if (hole_at[w]) { w++; continue; }
            int e = w + 1;
            while (e < n && !hole_at[e] && pos_off[e] - home[e] == pos_off[w] - home[w]) e++;
            const size_t span = (size_t)(home[e] - home[w]);
            HIPCHK(hipMemcpyAsync(mm + (size_t)pos_off[w] * GH_NSYM, pb.mm + (size_t)home[w] * GH_NSYM, span * GH_NSYM * sizeof(double),
                                  hipMemcpyDeviceToHost, b->stream));
            HIPCHK(hipMemcpyAsync(cm + pos_off[w], pb.cm + home[w], span, hipMemcpyDeviceToHost, b->stream));
            w = e;
        }
        HIPCHK(hipStreamSynchronize(b->stream));
        clock(3);
    }
    b->vitm_info[0] = n; b->vitm_info[1] = holes; b->vitm_info[2] = launches; b->vitm_info[3] = bytes;
    return GH_OK;
}

extern "C" int gh_panel_viterbi_marginals_info(gh_batch_t *b, int64_t out[4])
{
    if (!b || !out) return fail(GH_ERR_ARG, "null argument");
    for (int q = 0; q < 4; q++) out[q] = b->vitm_info[q];
    return GH_OK;
}
