// scratch_layout.hpp -- how gh_assign_reads, gh_score_paths, the beam and the exact decoder lay out their device scratch blocks
// (dev_scratch, gretel_hip.hip).  Host only, plain C++17, no HIP: tests/native/scratch_layout.cpp compiles it alone and checks
// every layout below against its sizes written out by hand.  Each user lists its parts ONCE, in a *_layout function: called with
// base = nullptr it sizes the block (`total`, every part null), called with the block it hands out the typed parts.  A struct's
// members stand in the order of the block, and a braced list is evaluated left to right: the list IS the layout.
// ---------------------------------------------------------------------------------------------
#pragma once
#include <cstddef>
#include <cstdint>

#include "gretel_hip.h"

constexpr size_t scratch_up(size_t x) { return (x + 255) & ~(size_t)255; }      // every part starts on a 256-byte boundary

struct scratch_carver {
    char *base;            // nullptr: the sizing pass
    size_t used = 0;
    template <typename T> T *take(size_t count)
    {
        T *p = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += scratch_up(count * sizeof(T));
        return p;
    }
};

// gh_assign_reads: counters [3][n_paths] with the totals [8] right behind them, the paths, the match masks [nw][N+1][5],
// and where the caller wants them the per-read results [3][n_reads]
struct assign_bufs {
    unsigned long long *cnt;
    uint8_t *paths;
    unsigned long long *mask;
    int32_t *read;
    size_t total;
};

inline assign_bufs assign_layout(void *base, int n_paths, int N, int64_t n_reads, bool per_read)
{
    scratch_carver c{(char *)base};
    const size_t n1 = (size_t)N + 1, nw = ((size_t)n_paths + 63) / 64;
    return {c.take<unsigned long long>(3 * (size_t)n_paths + 8), c.take<uint8_t>((size_t)n_paths * n1), c.take<unsigned long long>(nw * n1 * 5),
            per_read ? c.take<int32_t>((size_t)n_reads * 3) : nullptr, c.used};
}

// gh_score_paths: one slab's weights, margins, records, paths and picks
struct score_bufs {
    double *weight, *margin;
    gh_score_rec *recs;
    uint8_t *paths, *pick;
    size_t total;
};

inline score_bufs score_layout(void *base, int slab, size_t n1)
{
    scratch_carver c{(char *)base};
    const size_t cells = (size_t)slab * n1;
    return {c.take<double>(cells), c.take<double>(cells), c.take<gh_score_rec>((size_t)slab), c.take<uint8_t>(cells), c.take<uint8_t>(cells), c.used};
}

// the beam: its chain table (`table_doubles` = N * beam_src_doubles(L)), a row of back-pointer bytes per position (whole words:
// `bps` bytes), GH_BEAM_MAX path rows and scores, and what the walk leaves for the trace and the host
struct beam_out {
    int n_out, hole_at;
    int end, rows;     // what k_beam_trace follows: `rows` hypotheses from position `end` down
};

struct beam_bufs {
    double *Gb;
    uint8_t *bp, *paths;
    double *ll;
    beam_out *out;
    int bps;
    size_t total;
};

inline beam_bufs beam_layout(void *base, int N, size_t table_doubles, int width)
{
    scratch_carver c{(char *)base};
    const size_t n1 = (size_t)N + 1;
    const int bps = (width + 3) & ~3;
    return {c.take<double>(table_doubles), c.take<uint8_t>(n1 * bps), c.take<uint8_t>(n1 * GH_BEAM_MAX), c.take<double>(GH_BEAM_MAX),
            c.take<beam_out>(1), bps, c.used};
}

// the exact decoder.  `out` is the FIRST part: vit_run reserves the block twice in one call -- `states` = 0 while only k_vit_union's
// word is wanted, then in full once U has said how many states there are -- and finds `out` at offset 0 under both.
struct vit_out {
    uint32_t U;        // k_vit_union
    int hole_at;       // k_vit_walk
    int end_state;     // k_vit_trace; k_vitk_trace: how many paths it returned
    int pad;
    double ll;         // k_vit_trace
};

struct vit_bufs {
    vit_out *out;
    double *Gb;
    uint8_t *bp;           // [N + 1][states] and four bytes more: k_vit_trace copies whole words
    double *vend;
    uint8_t *okend, *path;
    size_t total;
};

inline vit_bufs vit_layout(void *base, int N, size_t table_doubles, int states)
{
    scratch_carver c{(char *)base};
    const size_t n1 = (size_t)N + 1, ns = (size_t)states;
    vit_out *out = c.take<vit_out>(1);
    if (!states) return {out, nullptr, nullptr, nullptr, nullptr, nullptr, c.used};
    return {out, c.take<double>(table_doubles), c.take<uint8_t>(n1 * ns + 4), c.take<double>(ns), c.take<uint8_t>(ns), c.take<uint8_t>(n1), c.used};
}

// the max-marginals (viterbi_marg.hpp), in the exact decoder's block of the handle.  `out` is the first part for the same reason as
// above.  `fb` is the one stored row per position: the forward walk leaves F there, the backward walk puts F + B over it (NaN where
// a state is not reachable), k_vit_mm reduces it -- N * states doubles, the part that grows (328 MB at 10k SNPs and 4096 states).
struct vitm_bufs {
    vit_out *out;
    double *Gb;
    double *fb;            // [N][states]: row p - 1 belongs to position p
    uint8_t *cm5;          // [N + 1] candidate bits over the compact indices, 0 at position 0
    double *mm;            // [N + 1][7]
    uint8_t *cm;           // [N + 1] candidate bits over the seven symbols
    size_t total;
};

inline vitm_bufs vitm_layout(void *base, int N, size_t table_doubles, int states)
{
    scratch_carver c{(char *)base};
    const size_t n1 = (size_t)N + 1, ns = (size_t)states;
    vit_out *out = c.take<vit_out>(1);
    if (!states) return {out, nullptr, nullptr, nullptr, nullptr, nullptr, c.used};
    return {out, c.take<double>(table_doubles), c.take<double>((size_t)N * ns), c.take<uint8_t>(n1), c.take<double>(n1 * GH_NSYM), c.take<uint8_t>(n1),
            c.used};
}

// k-best decoding (viterbi_kbest.hpp), in the exact decoder's block of the handle, `out` first for the same reason.  A slot is
// (state, rank), `states * k` of them (at most GH_VITERBI_MAX_STATES): one back-pointer byte per position and slot, the end lists
// (scores per slot, a count per state), and what goes home: k path rows, k scores and how many of them are filled.
struct vitk_bufs {
    vit_out *out;
    double *Gb;
    uint8_t *bp;           // [N + 1][states][k] and four bytes more: k_vitk_trace copies whole words
    double *vend;          // [states][k]
    uint8_t *cend;         // [states] entries a state holds at p = N, 0 = not reachable
    uint8_t *paths;        // [k][N + 1]
    double *ll;            // [k]
    int32_t *n_out;
    size_t total;
};

inline vitk_bufs vitk_layout(void *base, int N, size_t table_doubles, int states, int k)
{
    scratch_carver c{(char *)base};
    const size_t n1 = (size_t)N + 1, ns = (size_t)states, nk = (size_t)k;
    return {c.take<vit_out>(1), c.take<double>(table_doubles), c.take<uint8_t>(n1 * ns * nk + 4), c.take<double>(ns * nk), c.take<uint8_t>(ns),
            c.take<uint8_t>(nk * n1), c.take<double>(nk), c.take<int32_t>(1), c.used};
}

// constrained decoding (viterbi_masked.hpp), in the exact decoder's block of the handle, `out` first for the same reason: the table
// ONCE, and per constraint set a block of back-pointer bytes, the end row with its flags, a vit_out, a path row and the masks over
// the five compact candidate indices.  A set's back-pointers are [N + 1][states] as the decoder's; `bps` = that rounded up to whole
// words is the stride from set to set, so that every set's block starts on a four-byte boundary (k_vit_trace copies whole words,
// and with an odd state count such as 3 or 9 a block would otherwise begin mid-word).  No slab scheme: the block grows with n_sets.
struct vitx_bufs {
    vit_out *out;
    double *Gb;
    uint8_t *bp;           // [n_sets] blocks of bps bytes
    double *vend;          // [n_sets][states]
    uint8_t *okend;        // [n_sets][states]
    vit_out *outs;         // [n_sets]
    uint8_t *paths;        // [n_sets][N + 1]
    uint8_t *a5;           // [n_sets][N + 1] allowed bits over the compact indices
    size_t bps;
    size_t total;
};

inline vitx_bufs vitx_layout(void *base, int N, size_t table_doubles, int states, int n_sets)
{
    scratch_carver c{(char *)base};
    const size_t n1 = (size_t)N + 1, ns = (size_t)states, m = (size_t)n_sets;
    const size_t bps = (n1 * ns + 3) & ~(size_t)3;
    return {c.take<vit_out>(1), c.take<double>(table_doubles), c.take<uint8_t>(m * bps), c.take<double>(m * ns), c.take<uint8_t>(m * ns),
            c.take<vit_out>(m), c.take<uint8_t>(m * n1), c.take<uint8_t>(m * n1), bps, c.used};
}

// the grid decoder (viterbi_grid.hpp), in the exact decoder's block of the handle.  `out` is the first part as above, and the
// candidate bytes stand right behind it under both sizings: the call reserves the block with `states` = 0 while only k_vit_cands'
// bytes are wanted (they say how many states there are), then in full.  What grows: a back-pointer byte per position and state
// (at 2^24 states and 128 SNPs they alone pass 2^31 bytes, so every product with `states` or N is formed in size_t) and the two
// score rows.  The end rule's first level leaves one (score, state) per GH_VITG_END_CHUNK states.
#define GH_VITG_END_CHUNK 4096

struct vitg_bufs {
    vit_out *out;
    uint8_t *cm5, *cm;     // [N + 1] each: candidate bits over the compact indices (what the host reads) and over the seven symbols
    double *Gb;
    uint8_t *bp;           // [N + 1][states]
    double *rows;          // [2][states]
    double *pv;            // [parts] the end rule's partial maxima ...
    int32_t *pj;           // [parts] ... and their states, -1 = no reachable state in the chunk
    uint8_t *path;         // [N + 1]
    size_t parts;
    size_t total;
};

inline vitg_bufs vitg_layout(void *base, int N, size_t table_doubles, size_t states)
{
    scratch_carver c{(char *)base};
    const size_t n1 = (size_t)N + 1, parts = (states + GH_VITG_END_CHUNK - 1) / GH_VITG_END_CHUNK;
    vit_out *out = c.take<vit_out>(1);
    uint8_t *cm5 = c.take<uint8_t>(n1), *cm = c.take<uint8_t>(n1);
    if (!states) return {out, cm5, cm, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, c.used};
    return {out, cm5, cm, c.take<double>(table_doubles), c.take<uint8_t>(n1 * states), c.take<double>(2 * states), c.take<double>(parts),
            c.take<int32_t>(parts), c.take<uint8_t>(n1), parts, c.used};
}

// the max-marginals on the grid (viterbi_grid_marg.hpp), in the exact decoder's block of the handle: `out` and the candidate bytes
// first under both sizings, exactly as in vitg_layout (the call opens as the grid decoder does).  What grows: ONE KEPT ROW of F
// per position, N * states doubles (0.5 GB at 60 SNPs and 4^10 states, 4.7 GB at 5^10; it is not bounded by checkpointing), with
// the one +0.0 of position 0 behind the last row so that every row starts as the part does.  Then the two rows of B, the
// partial maxima -- five doubles per position and workgroup of GH_VITGM_THREADS threads; a thread owns S consecutive states, and
// the part is sized for S = 2, the most workgroups a state count can make, so that the layout is a function of N, Le and the
// state count alone (at S = 5 two fifths of it are used; it is a hundredth of F either way) -- and what goes home.  Every
// product with `states` or N is formed in size_t.
#define GH_VITGM_THREADS 256

struct vitgm_bufs {
    vit_out *out;
    uint8_t *cm5, *cm0;    // [N + 1] each, k_vit_cands' bytes: what the host reads, and the symbol bits of the opening (not read)
    double *Gb;
    double *F;             // [N][states]: row p - 1 belongs to position p; F[N * states] = +0.0, the empty prefix of position 0
    double *B;             // [2][states]: position p in row p & 1
    double *part;          // [N][wgs][5]: block p - 1 belongs to position p (a launch fills its first ceil(states / S / 256) entries)
    double *mm;            // [N + 1][7]
    uint8_t *cm;           // [N + 1] candidate bits over the seven symbols
    size_t wgs;
    size_t total;
};

inline vitgm_bufs vitgm_layout(void *base, int N, size_t table_doubles, size_t states)
{
    scratch_carver c{(char *)base};
    const size_t n1 = (size_t)N + 1, wgs = (states + 2 * GH_VITGM_THREADS - 1) / (2 * GH_VITGM_THREADS);
    vit_out *out = c.take<vit_out>(1);
    uint8_t *cm5 = c.take<uint8_t>(n1), *cm0 = c.take<uint8_t>(n1);
    if (!states) return {out, cm5, cm0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, c.used};
    return {out, cm5, cm0, c.take<double>(table_doubles), c.take<double>((size_t)N * states + 1), c.take<double>(2 * states),
            c.take<double>((size_t)N * wgs * 5), c.take<double>(n1 * GH_NSYM), c.take<uint8_t>(n1), wgs, c.used};
}

// the exact decoder over a panel (viterbi_panel.hpp), a block of the batch: one descriptor per window (WD = vit_win, which holds
// device types and so stands in viterbi_panel.hpp), the windows' vit_outs gathered for one copy to the host, and their path rows
// gathered back to back (`path_bytes` = the sum of N_w + 1)
template <typename WD> struct vit_panel_bufs {
    WD *wd;
    vit_out *outs;
    uint8_t *paths;
    size_t total;
};

template <typename WD> inline vit_panel_bufs<WD> vit_panel_layout(void *base, int n, size_t path_bytes)
{
    scratch_carver c{(char *)base};
    return {c.take<WD>((size_t)n), c.take<vit_out>((size_t)n), c.take<uint8_t>(path_bytes), c.used};
}

// the max-marginals over a panel (viterbi_marg_panel.hpp), in the same block of the batch: one descriptor per window in window
// order (WD = vitm_win), the launch lists (window indices: the forward walk's launches in the first n ints, the backward walk's
// in the second n), the windows' vit_outs gathered for one copy to the host, and their mm and cm gathered back to back in window
// order (`positions` = the sum of N_w + 1: window w's mm at 7 * home_w doubles, its cm at home_w bytes, home_w the sum before it)
template <typename WD> struct vitm_panel_bufs {
    WD *wd;
    int32_t *list;         // [2 n]
    vit_out *outs;         // [n]
    double *mm;            // [positions][7]
    uint8_t *cm;           // [positions]
    size_t total;
};

template <typename WD> inline vitm_panel_bufs<WD> vitm_panel_layout(void *base, int n, size_t positions)
{
    scratch_carver c{(char *)base};
    return {c.take<WD>((size_t)n), c.take<int32_t>(2 * (size_t)n), c.take<vit_out>((size_t)n), c.take<double>(positions * GH_NSYM),
            c.take<uint8_t>(positions), c.used};
}

// k-best decoding over a panel (viterbi_kbest_panel.hpp), in the same block of the batch: one descriptor per window in window
// order (WD = vitk_win), the two walk launches' lists (window indices: the walks with the table ring from the front of the n ints,
// those without behind them), the windows' vit_outs gathered for one copy to the host, and their path rows and scores gathered
// back to back in window order (`path_bytes` = the sum of k_w * (N_w + 1), `scores` = the sum of k_w: window w's rows at the
// sum of k_v * (N_v + 1) before it, its scores at the sum of k_v before it)
template <typename WD> struct vitk_panel_bufs {
    WD *wd;
    int32_t *list;         // [n]
    vit_out *outs;         // [n]
    uint8_t *paths;        // [path_bytes]
    double *ll;            // [scores]
    size_t total;
};

template <typename WD> inline vitk_panel_bufs<WD> vitk_panel_layout(void *base, int n, size_t path_bytes, size_t scores)
{
    scratch_carver c{(char *)base};
    return {c.take<WD>((size_t)n), c.take<int32_t>((size_t)n), c.take<vit_out>((size_t)n), c.take<uint8_t>(path_bytes), c.take<double>(scores),
            c.used};
}
