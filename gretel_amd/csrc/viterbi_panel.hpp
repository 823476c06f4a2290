// viterbi_panel.hpp -- exact decoding over every window of a batch or panel (gh_panel_viterbi_spin, gh_panel_viterbi_info,
// gh_viterbi_states: include/gretel_hip.h).  The windows are independent, a decoder is one workgroup: a round of the recovery loop
// decodes every live window in ONE launch each of the union, the walk and the trace, block w taking window w of the launch's
// descriptor list.  Nothing depends on another workgroup -- no grid barrier, no shared counter, no assumption that all workgroups
// are resident: a grid larger than the card drains in any order.  The definition, the arithmetic and the layout of a window's
// scratch are viterbi.hpp's, bit for bit.
//
//   vit_win              one descriptor per window of a launch: the window's table, shape, state geometry and the parts of its own
//                        h->vit scratch block (vit_layout).  The descriptor array, the gathered vit_outs and the gathered path
//                        rows are a block of the batch (vit_panel_layout, scratch_layout.hpp).
//   k_vit_union_panel    block w: U of window w.
//   k_vit_walk_panel     block w walks window w.  The dynamic LDS of a launch is the largest need among its windows; windows that
//                        take the non-staged body (S = 1 with Le > VIT_MAX_LE, or GH_VIT_STAGE=0) go in a launch of their own.
//                        A window with a hole or a short N leaves early: its workgroup ends, the others run on.
//   k_vit_trace_panel    block w traces window w (nothing where the walk met a hole).
//   k_vit_home_panel     block w copies window w's vit_out, and its path row where there is one, into the batch's gathered arrays:
//                        two copies to the host a round, not two per window (256 small copies cost 4 ms).
//
// THE BODIES.  k_vit_union, k_vit_walk and k_vit_trace of viterbi.hpp stay as they are: moved into __device__ functions and called
// from thin shells, k_vit_walk<true>, k_vit_walk<false> and k_vit_trace came out with other instructions (13-16 more in the
// walks, one to three more spilled scalar registers; with or without __restrict__ on the functions' parameters:
// scratch/device_isa_cmp.py, docs/HISTORY.md).  So the single-window kernels are the old ones, and the panel's shells stand over
// the __forceinline__ bodies below, which are those kernels' statements line for line.
// ---------------------------------------------------------------------------------------------

struct vit_win {
    const double *Gb;          // the window's chain table (vit_bufs::Gb)
    const double *minfo;       // the handle's marginal table: k_vit_union_panel reads the candidate bits
    uint8_t *bp;
    double *vend;
    uint8_t *okend;
    vit_out *out;
    uint8_t *path;
    int64_t home;              // where the path row goes in the batch's gathered rows
    int N, Le, S, states, marginal_term, chunk;      // chunk: positions the trace holds in LDS at a time
    uint32_t U;
    symmap sm;
};
static_assert(sizeof(vit_win) == 104, "the size tests/native/vit_panel_layout.cpp lays the descriptor array out with");

__device__ __forceinline__ void vit_union_body(const double *__restrict__ minfo, int N, vit_out *__restrict__ out)
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
// KEEP (viterbi_marg_panel.hpp): as k_vit_walk's -- `vend` is F[N][states], no back-pointers, no end row
// MASKED (viterbi_masked.hpp): a5[0..N] holds the allowed bits of a constraint set over the compact indices; the candidate bits of
// step p are ANDed with a5[p] before the hole test and before `hist` is shifted, so a predecessor's reachability (cm_old) is the
// masked one without further code.  The bytes reach the step through a window of two chunks of VIT_MCH positions in LDS (512
// static bytes, in the MASKED instantiations only): chunk c + 1 is stored in the middle of chunk c from a register of the first
// VIT_MCH threads, into which it set out from global memory a whole chunk earlier, and the byte of step p + 1 is read from the
// window in step p.  So no step waits for a global load of its own: the one wait for global memory the masks cost falls once in
// VIT_MCH steps, on a load that has had VIT_MCH steps to arrive.  (A plain a5[p + 1] in step p does NOT do that: the byte is the
// same in every thread, the compiler moves it into a scalar register right behind the load and drains vmcnt there -- the table
// block's piece and the back-pointer stores with it, 0.2-0.3 us in every step; profiles/r19_masked.txt.)  MASKED = false (every
// other shell) never touches a5 or the window, and those instantiations are the kernels they were.
#define VIT_MCH 256
template <bool STAGED, bool KEEP = false, bool MASKED = false>
__device__ __forceinline__ void
vit_walk_body(const double *__restrict__ Gb, int N, int L, int S, int states, int marginal_term, uint32_t U,
              uint8_t *__restrict__ bp, double *__restrict__ vend, uint8_t *__restrict__ okend, vit_out *__restrict__ out,
              const uint8_t *__restrict__ a5 = nullptr)
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
    __shared__ uint8_t vit_mk[MASKED ? 2 * VIT_MCH : 4];       // MASKED: the window; position q lies at q mod 2 VIT_MCH
    uint32_t allow = 31u, allow_next = 31u;                   // ... the allowed bits of step p, those of step p + 1
    uint8_t mreg = 31;                                        // ... and a byte of the chunk that is on its way
    if (MASKED) {
        if (tid < VIT_MCH && tid <= N) vit_mk[tid] = a5[tid];                   // chunk 0 straight in; chunk 1 sets out
        if (tid < VIT_MCH && VIT_MCH + tid <= N) mreg = a5[VIT_MCH + tid];
    }
    __syncthreads();
    if (MASKED) allow = vit_mk[1];

    int cur = 0, hole = 0;
    int ts = 0;                                               // LDS slot of source p - 1
    for (int p = 1; p <= N; p++) {
        if (STAGED) {
            // source p (first read in step p + 1) replaces source p - Le - 1, last read in step p - 1; source p + 1 sets out
            const int ws = ts + 1 == R ? 0 : ts + 1;
            if (p < N && tid < su) tab2[(size_t)ws * su + tid] = reg;
            if (p + 1 < N && tid < su) reg = Gb2[(size_t)(p + 1) * su + tid];
        }
        if (MASKED) {
            if ((p & (VIT_MCH - 1)) == VIT_MCH / 2) {
                // chunk c + 1 (first read in step nx - 1) replaces chunk c - 1, last read in step nx - VIT_MCH - 2; chunk c + 2 sets out
                const int nx = (p / VIT_MCH + 1) * VIT_MCH;
                if (tid < VIT_MCH) vit_mk[(nx + tid) & (2 * VIT_MCH - 1)] = mreg;
                if (tid < VIT_MCH && nx + VIT_MCH + tid <= N) mreg = a5[nx + VIT_MCH + tid];
            }
            if (p < N) allow_next = vit_mk[(p + 1) & (2 * VIT_MCH - 1)];
        }
        const double *blk = STAGED ? tab + (size_t)ts * sd : Gb + (size_t)(p - 1) * sd;
        uint32_t cm5 = (uint32_t)__double_as_longlong(blk[30 * L + 5]) & 31u;
        if (MASKED) cm5 &= allow;
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
        if (MASKED) allow = allow_next;
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
__device__ __forceinline__ void
vit_trace_body(const uint8_t *__restrict__ bp, const double *__restrict__ vend, const uint8_t *__restrict__ okend, int N, int L, int S,
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

__global__ void __launch_bounds__(256)
k_vit_union_panel(const vit_win *__restrict__ wd)
{
    const vit_win &d = wd[blockIdx.x];
    vit_union_body(d.minfo, d.N, d.out);
}

template <bool STAGED>
__global__ void __launch_bounds__(VIT_THREADS)
k_vit_walk_panel(const vit_win *__restrict__ wd)
{
    const vit_win &d = wd[blockIdx.x];
    vit_walk_body<STAGED>(d.Gb, d.N, d.Le, d.S, d.states, d.marginal_term, d.U, d.bp, d.vend, d.okend, d.out);
}

__global__ void __launch_bounds__(VIT_THREADS)
k_vit_trace_panel(const vit_win *__restrict__ wd)
{
    const vit_win &d = wd[blockIdx.x];
    vit_trace_body(d.bp, d.vend, d.okend, d.N, d.Le, d.S, d.states, d.chunk, d.U, d.sm, d.out, d.path);
}

__global__ void __launch_bounds__(256)
k_vit_home_panel(const vit_win *__restrict__ wd, vit_out *__restrict__ outs, uint8_t *__restrict__ paths, int with_paths)
{
    const vit_win &d = wd[blockIdx.x];
    const vit_out o = *d.out;
    if (threadIdx.x == 0) outs[blockIdx.x] = o;
    if (!with_paths || o.hole_at) return;
    for (int q = threadIdx.x; q <= d.N; q += blockDim.x) paths[d.home + q] = d.path[q];
}

// host ----------------------------------------------------------------------------------------
// STREAM ORDER.  Every panel launch and every copy home runs on the batch's stream; what belongs to one window (its marginal
// tables, its chain table, the record and the reweight of its path) runs on its handle's stream, as in the single decoder.
// Handle -> batch: after a window's table build an event recorded on the handle's stream is waited for on the batch's, so the
// union and the walk read finished tables (and whatever the handle's stream still carried, a fill for one).  Batch -> handle: the
// host waits for the batch's stream before it touches a handle again (it needs the results anyway), twice a round.  The call
// returns with the batch's stream idle and every handle's stream as gh_reweight_path leaves it.
typedef vit_panel_bufs<vit_win> vitp_bufs;

static int vitp_window_fail(int rc, int w)
{
    const std::string msg = g_err;
    return fail(rc, "window %d: %s", w, msg.c_str());
}

static int vitp_reserve(gh_batch *b, size_t need)
{
    if (need <= b->vit.cap) return GH_OK;
    HIPCHK(hipStreamSynchronize(b->stream));
    hipFree(b->vit.buf);
    b->vit.buf = nullptr;
    b->vit.cap = 0;
    if (hipMalloc(&b->vit.buf, need) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GH_ERR_NOMEM, "the panel decoder's descriptors and gathered results cannot be had (%zu bytes)", need);
    }
    b->vit.cap = need;
    return GH_OK;
}

static int vitp_post(gh_batch *b, const char *what)
{
    static const bool dbg = env_int("GH_DEBUG_SYNC", 0) != 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && dbg) e = hipStreamSynchronize(b->stream);
    if (e != hipSuccess) return fail(GH_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return GH_OK;
}

// the batch's stream waits for what window w's handle has queued so far
static int vitp_after_handle(gh_batch *b, int w)
{
    HIPCHK(hipEventRecord(b->vit_ev[w], b->hs[w]->stream));
    HIPCHK(hipStreamWaitEvent(b->stream, b->vit_ev[w], 0));
    return GH_OK;
}

// gh_debug_panel_viterbi_phases: host clocks around synchronised phases (a measuring pass, never the timed one)
static bool g_vitp_phases = false;
static double g_vitp_ms[4];
struct vitp_clock {
    gh_batch *b;
    double t;
    explicit vitp_clock(gh_batch *bb) : b(bb), t(spin_phases::now()) {}
    void operator()(int k)
    {
        if (!g_vitp_phases) return;
        for (gh_handle *h : b->hs) hipStreamSynchronize(h->stream);
        hipStreamSynchronize(b->stream);
        const double t1 = spin_phases::now();
        g_vitp_ms[k] += t1 - t;
        t = t1;
    }
};

extern "C" int gh_debug_panel_viterbi_phases(int on, double out[4])
{
    if (out) for (int k = 0; k < 4; k++) out[k] = g_vitp_ms[k];
    for (int k = 0; k < 4; k++) g_vitp_ms[k] = 0.0;
    g_vitp_phases = on != 0;
    return GH_OK;
}

extern "C" int gh_viterbi_states(gh_t *h, int64_t out[3])
{
    if (!h || !out) return fail(GH_ERR_ARG, "null argument");
    int rc = decode_check(h, "gh_viterbi_states");
    if (rc) return rc;
    if (set_dev(h)) return GH_ERR_HIP;
    if ((rc = ensure_marg(h))) return rc;
    if ((rc = scratch_reserve(h, &h->vit, vit_layout(nullptr, h->N, 0, 0).total, VIT_SCRATCH))) return rc;
    vit_out *d_out = vit_layout(h->vit.buf, h->N, 0, 0).out;
    vit_out ho;
    hipLaunchKernelGGL(k_vit_union, dim3(1), dim3(256), 0, h->stream, (const double *)h->minfo, h->N, d_out);
    if ((rc = post_launch(h, "k_vit_union"))) return rc;
    HIPCHK(hipMemcpyAsync(&ho, d_out, sizeof ho, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int S = __builtin_popcount(ho.U), Le = chain_lags(h);
    int64_t states = S ? 1 : 0;
    for (int k = 0; k < Le && S > 1; k++) states = states > INT64_MAX / S ? INT64_MAX : states * S;
    out[0] = S; out[1] = Le; out[2] = states;
    return GH_OK;
}

extern "C" int gh_panel_viterbi_spin(gh_batch_t *b, int max_paths, double min_remove, uint8_t *paths_out, const int64_t *paths_off,
                                     gh_path_rec *recs, double *ll_chain, int *n_out, int *hole_at)
{
    if (!b || !paths_out || !paths_off || !recs || !n_out || !hole_at) return fail(GH_ERR_ARG, "null argument");
    if (max_paths < 0) return fail(GH_ERR_ARG, "max_paths < 0");
    const int n = b->n;
    int rc;
    for (int w = 0; w < n; w++) {
        if (paths_off[w] < 0) return fail(GH_ERR_ARG, "gh_panel_viterbi_spin: window %d has a negative path offset", w);
        if ((rc = decode_check(b->hs[w], "gh_panel_viterbi_spin"))) return vitp_window_fail(rc, w);
    }
    if (max_paths == 0) {
        for (int w = 0; w < n; w++) n_out[w] = hole_at[w] = 0;
        b->vit_info[0] = n; b->vit_info[1] = b->vit_info[2] = b->vit_info[3] = 0;
        return GH_OK;
    }
    HIPCHK(hipSetDevice(b->dev));
    while ((int)b->vit_ev.size() < n) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        b->vit_ev.push_back(e);
    }
    std::vector<int64_t> home((size_t)n + 1, 0);                // window w's row in the gathered path rows
    for (int w = 0; w < n; w++) home[w + 1] = home[w] + b->hs[w]->N + 1;
    if ((rc = vitp_reserve(b, vit_panel_layout<vit_win>(nullptr, n, (size_t)home[n]).total))) return rc;
    const vitp_bufs pb = vit_panel_layout<vit_win>(b->vit.buf, n, (size_t)home[n]);
    std::vector<vit_win> wd((size_t)n);
    std::vector<vit_out> outs((size_t)n);
    std::vector<uint8_t> rows((size_t)home[n]);
    vitp_clock clock(b);

    // U of `cnt` described windows to outs[0 .. cnt): the union launch, the gather where the outs stand in the windows' blocks
    auto unions_home = [&](int cnt, bool gather) -> int {
        HIPCHK(hipMemcpyAsync(pb.wd, wd.data(), sizeof(vit_win) * cnt, hipMemcpyHostToDevice, b->stream));
        hipLaunchKernelGGL(k_vit_union_panel, dim3(cnt), dim3(256), 0, b->stream, (const vit_win *)pb.wd);
        int r = vitp_post(b, "k_vit_union_panel");
        if (r) return r;
        if (gather) {
            hipLaunchKernelGGL(k_vit_home_panel, dim3(cnt), dim3(256), 0, b->stream, (const vit_win *)pb.wd, pb.outs, pb.paths, 0);
            if ((r = vitp_post(b, "k_vit_home_panel"))) return r;
        }
        HIPCHK(hipMemcpyAsync(outs.data(), pb.outs, sizeof(vit_out) * cnt, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        return GH_OK;
    };

    // The refusals, as a whole, before any window's tensor, snapshot or scratch is touched: every window's U straight into the
    // batch's own gathered array (only the marginal tables, a cache of the tensor, are brought up to date on the way)
    for (int w = 0; w < n; w++) {
        gh_handle *h = b->hs[w];
        if ((rc = ensure_marg(h))) return vitp_window_fail(rc, w);
        if ((rc = vitp_after_handle(b, w))) return rc;
        memset(&wd[w], 0, sizeof(vit_win));
        wd[w].minfo = h->minfo; wd[w].N = h->N; wd[w].out = pb.outs + w;
    }
    if ((rc = unions_home(n, false))) return rc;
    std::vector<int> ns0((size_t)n);
    std::vector<uint32_t> Uw((size_t)n);                        // this round's U by window
    for (int w = 0; w < n; w++) {
        const int S = __builtin_popcount(outs[w].U), Le = chain_lags(b->hs[w]);
        const long long st = S ? vit_states(S, Le) : 1;
        if (st > GH_VITERBI_MAX_STATES) return vitp_window_fail(vit_too_many("gh_panel_viterbi_spin", S, Le), w);
        ns0[w] = (int)st;
    }
    // Candidate masks only lose bits under a reweight: round 0's state count bounds every later round's, so each window's
    // scratch is had once, for round 0, and its parts stay where they are (the table stands at the same offset whatever the count)
    for (int w = 0; w < n; w++) {
        gh_handle *h = b->hs[w];
        n_out[w] = hole_at[w] = 0;
        if (!h->have_orig && (rc = gh_snapshot_original(h))) return vitp_window_fail(rc, w);
        const size_t td = (size_t)h->N * beam_src_doubles(chain_lags(h));
        if ((rc = scratch_reserve(h, &h->vit, vit_layout(nullptr, h->N, td, ns0[w]).total, VIT_SCRATCH))) return vitp_window_fail(rc, w);
    }
    clock(0);

    static const bool no_stage = env_off("GH_VIT_STAGE");
    std::vector<int> live((size_t)n), run, plain;
    for (int w = 0; w < n; w++) live[w] = w;
    int64_t rounds = 0, most = 0, launches = 0;
    while (!live.empty()) {
        const int nl = (int)live.size();
        // the tables of the tensors as they stand, each on its window's stream; then every U
        for (int i = 0; i < nl; i++) {
            const int w = live[i];
            gh_handle *h = b->hs[w];
            const int Le = chain_lags(h);
            const size_t td = (size_t)h->N * beam_src_doubles(Le);
            if ((rc = ensure_marg(h))) return vitp_window_fail(rc, w);
            if ((rc = chain_table_build(h, Le, vit_layout(h->vit.buf, h->N, td, 1).Gb))) return vitp_window_fail(rc, w);
            if ((rc = vitp_after_handle(b, w))) return rc;
            memset(&wd[i], 0, sizeof(vit_win));
            wd[i].minfo = h->minfo; wd[i].N = h->N; wd[i].out = vit_layout(h->vit.buf, h->N, 0, 0).out;
        }
        clock(0);
        if ((rc = unions_home(nl, true))) return rc;
        // per window: the states of this round (the per-round check all the same), its descriptor; staged walks first
        run.clear(); plain.clear();
        size_t lds_staged = 0, lds_plain = 0, lds_trace = 0;
        for (int i = 0; i < nl; i++) {
            const int w = live[i];
            gh_handle *h = b->hs[w];
            const uint32_t U = outs[i].U;
            const int S = __builtin_popcount(U), Le = chain_lags(h);
            if (S == 0) {                                       // nothing offered anywhere: the hole is the first position
                hole_at[w] = 1;
                h->vit_last[0] = 0; h->vit_last[1] = Le; h->vit_last[2] = 0; h->vit_last[3] = (int64_t)h->vit.cap;
                continue;
            }
            const long long st = vit_states(S, Le);
            if (st > GH_VITERBI_MAX_STATES) return vitp_window_fail(vit_too_many("gh_panel_viterbi_spin", S, Le), w);
            const size_t td = (size_t)h->N * beam_src_doubles(Le);
            const size_t need = vit_layout(nullptr, h->N, td, (int)st).total;
            if (need > h->vit.cap)
                return fail(GH_ERR_STATE, "window %d: the states of a round grew beyond round 0's (%lld, %d)", w, st, ns0[w]);
            h->vit_last[0] = S; h->vit_last[1] = Le; h->vit_last[2] = st; h->vit_last[3] = (int64_t)need;
            Uw[w] = U;
            ((S == 1 && Le > VIT_MAX_LE) || no_stage ? plain : run).push_back(w);
        }
        const int n_staged = (int)run.size();
        run.insert(run.end(), plain.begin(), plain.end());
        const int nr = (int)run.size();
        int64_t used = 0;
        for (int i = 0; i < nr; i++) {
            gh_handle *h = b->hs[run[i]];
            const int ns = (int)h->vit_last[2], Le = (int)h->vit_last[1];
            const vit_bufs vb = vit_layout(h->vit.buf, h->N, (size_t)h->N * beam_src_doubles(Le), ns);
            vit_win &d = wd[i];
            d.Gb = vb.Gb; d.minfo = h->minfo; d.bp = vb.bp; d.vend = vb.vend; d.okend = vb.okend; d.out = vb.out; d.path = vb.path;
            d.home = used; d.N = h->N; d.Le = Le; d.S = (int)h->vit_last[0]; d.states = ns; d.marginal_term = h->cfg.marginal_term;
            d.chunk = VIT_TRACE_BYTES / ns > VIT_TRACE_POS ? VIT_TRACE_POS : VIT_TRACE_BYTES / ns;
            d.U = Uw[run[i]];
            d.sm = h->sm;
            used += h->N + 1;
            const size_t rws = 2 * (size_t)ns * 8;
            if (i < n_staged) lds_staged = std::max(lds_staged, rws + (size_t)(Le + 1) * beam_src_doubles(Le) * 8);
            else lds_plain = std::max(lds_plain, rws);
            lds_trace = std::max(lds_trace, (size_t)d.chunk * ns + 8);
        }
        if (nr) {
            HIPCHK(hipMemcpyAsync(pb.wd, wd.data(), sizeof(vit_win) * nr, hipMemcpyHostToDevice, b->stream));
            if (n_staged) {
                lds_limit<k_vit_walk_panel<true>>(lds_staged, b->dev);
                hipLaunchKernelGGL(k_vit_walk_panel<true>, dim3(n_staged), dim3(VIT_THREADS), lds_staged, b->stream, (const vit_win *)pb.wd);
                if ((rc = vitp_post(b, "k_vit_walk_panel"))) return rc;
                launches++;
                most = std::max<int64_t>(most, n_staged);
            }
            if (nr > n_staged) {
                lds_limit<k_vit_walk_panel<false>>(lds_plain, b->dev);
                hipLaunchKernelGGL(k_vit_walk_panel<false>, dim3(nr - n_staged), dim3(VIT_THREADS), lds_plain, b->stream,
                                   (const vit_win *)(pb.wd + n_staged));
                if ((rc = vitp_post(b, "k_vit_walk_panel"))) return rc;
                launches++;
                most = std::max<int64_t>(most, nr - n_staged);
            }
            lds_limit<k_vit_trace_panel>(lds_trace, b->dev);
            hipLaunchKernelGGL(k_vit_trace_panel, dim3(nr), dim3(VIT_THREADS), lds_trace, b->stream, (const vit_win *)pb.wd);
            if ((rc = vitp_post(b, "k_vit_trace_panel"))) return rc;
            clock(1);
            // the vit_outs and the path rows home: one gather, two copies
            hipLaunchKernelGGL(k_vit_home_panel, dim3(nr), dim3(256), 0, b->stream, (const vit_win *)pb.wd, pb.outs, pb.paths, 1);
            if ((rc = vitp_post(b, "k_vit_home_panel"))) return rc;
            HIPCHK(hipMemcpyAsync(outs.data(), pb.outs, sizeof(vit_out) * nr, hipMemcpyDeviceToHost, b->stream));
            HIPCHK(hipMemcpyAsync(rows.data(), pb.paths, (size_t)used, hipMemcpyDeviceToHost, b->stream));
            HIPCHK(hipStreamSynchronize(b->stream));
            clock(2);
        }
        // per window: a hole ends it; otherwise the path's record and reweight, decode_spin's own piece, on the window's stream
        live.clear();
        for (int i = 0; i < nr; i++) {
            const int w = run[i], s = n_out[w];
            gh_handle *h = b->hs[w];
            if (outs[i].hole_at) { hole_at[w] = outs[i].hole_at; continue; }
            const size_t n1 = (size_t)h->N + 1;
            uint8_t *path = paths_out + paths_off[w] + n1 * s;
            memcpy(path, rows.data() + wd[i].home, n1);
            if ((rc = decode_record(h, path, min_remove, &recs[(size_t)max_paths * w + s]))) return vitp_window_fail(rc, w);
            if (ll_chain) ll_chain[(size_t)max_paths * w + s] = outs[i].ll;
            n_out[w] = s + 1;
            if (s + 1 < max_paths) live.push_back(w);
        }
        std::sort(live.begin(), live.end());
        clock(3);
        rounds++;
    }
    b->vit_info[0] = n; b->vit_info[1] = rounds; b->vit_info[2] = most; b->vit_info[3] = launches;
    return GH_OK;
}

extern "C" int gh_panel_viterbi_info(gh_batch_t *b, int64_t out[4])
{
    if (!b || !out) return fail(GH_ERR_ARG, "null argument");
    for (int q = 0; q < 4; q++) out[q] = b->vit_info[q];
    return GH_OK;
}
