"""
Device-backed `Hansel`: the drop-in for `hansel.Hansel` (hanselx==0.0.92, reference
setup.py:8) as Gretel consumes it.  The tensor lives in HBM behind libgretel_hip.so;
this class only marshals arguments (ctypes) and re-exposes the reference's names:

    Hansel.init_matrix(symbols, unsymbols, n)      gretel/util.py:83
    add_observation / get_observation              gretel/util.py:266-286, tests/test_test.py:41-52
    reweight_observation                           gretel/gretel.py:84,96
    get_counts_at / get_marginal_of_at             gretel/cmd.py:86,127, gretel/gretel.py:182,186
    get_edge_weights_at                            gretel/gretel.py:155
    copy / save_hansel_dump                        gretel/cmd.py:79,82
    symbols_d, L, n_slices, n_crumbs               gretel/gretel.py:138, gretel/util.py:329-333

plus the fused fast paths used by gretel_amd.gretel / gretel_amd.util
(`fill_from_support`, `generate_path`, `reweight_from_path`, `spin`).

There is no CPU implementation here: without libgretel_hip.so or without a GPU
every operation raises (gretel_amd._lib).
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import check

SYMBOLS = ['A', 'C', 'G', 'T', 'N', '-', '_']
UNSYMBOLS = ['N', '_']
_SYM_LUT = np.frombuffer("".join(SYMBOLS).encode(), dtype=np.uint8)
SCORE_REC = np.dtype(_lib.gh_score_rec)       # gh_score_rec as a numpy record: five float64, four int32


class HanselSymbol:
    """A symbol object: str() gives its character (gretel/cmd.py:128,164,211), it equals the same symbol object
    (gretel/cmd.py:201) and is hashable (a key of get_counts_at / get_edge_weights_at).  It is NOT a str and does not
    compare or hash equal to one: the reference has to coerce the keys of get_counts_at with str() before it can look
    "A" up (gretel/cmd.py:128; SURVEY.md App. A-3 [R]), so hanselx's symbols are not strings either."""
    __slots__ = ("c", "i")

    def __init__(self, char, i):
        self.c = char
        self.i = i

    def __str__(self):
        return self.c

    def __repr__(self):
        return self.c

    def __eq__(self, other):
        return isinstance(other, HanselSymbol) and other.i == self.i

    def __ne__(self, other):
        return not self.__eq__(other)

    def __hash__(self):
        return hash(("HanselSymbol", self.i))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def margins_of(mm, cm, paths, cand_order="ACGT-"):
    """What Hansel.viterbi_marginals()' table says per SNP and about the haplotypes `paths` (uint8[H][N+1], or one uint8[N+1]).
    Host only, no handle.  mm float64[N+1][7], cm uint8[N+1].  Returns a dict:
      best uint8[N+1]      the candidate of largest max-marginal, the first of cand_order among the maximisers (6, '_', at 0);
      gap float64[N+1]     mm[p][best] minus the largest OTHER offered entry: the exact phasing confidence of the call at p.  +inf
                           where nothing else is offered or the largest other is -inf; 0.0 where every entry is -inf (and at 0);
      regret float64[H][N+1]  mm[p][best[p]] - mm[p][x[p]]: what the best full path through x[p] lacks to the best of all.  +inf
                           where x[p] is not offered, or its entry is -inf while the best is finite; 0.0 where both are -inf;
      max_regret float64[H], argmax_regret int32[H] (the first position that has it), n_best int32[H] (positions where
      x[p] == best[p])."""
    mm = np.asarray(mm, dtype=np.float64)
    cm = np.asarray(cm, dtype=np.uint8)
    n = len(cm) - 1
    x = np.asarray(paths, dtype=np.uint8)
    if x.ndim == 1:
        x = x.reshape(1, -1) if x.size else x.reshape(0, n + 1)
    if mm.shape != (n + 1, 7) or x.ndim != 2 or x.shape[1] != n + 1:
        raise ValueError("margins_of: mm must be [N+1][7], cm [N+1] and paths [H][N+1] (got %s, %s, %s)" % (mm.shape, cm.shape, x.shape))
    order = [SYMBOLS.index(c) for c in cand_order]
    best = np.full(n + 1, 6, dtype=np.uint8)
    gap = np.zeros(n + 1)
    ninf = float("-inf")
    for p in range(1, n + 1):
        offered = [s for s in order if (int(cm[p]) >> s) & 1]
        if not offered:
            continue
        b = offered[0]
        for s in offered[1:]:
            if mm[p, s] > mm[p, b]:
                b = s
        best[p] = b
        other = max((float(mm[p, s]) for s in offered if s != b), default=ninf)
        if mm[p, b] == ninf:
            gap[p] = 0.0
        elif other == ninf:
            gap[p] = np.inf
        else:
            gap[p] = mm[p, b] - other
    regret = np.zeros(x.shape)
    for q, row in enumerate(x):
        for p in range(1, n + 1):
            s, top = int(row[p]), float(mm[p, best[p]])
            if s > 6 or not (int(cm[p]) >> s) & 1:
                regret[q, p] = np.inf
            elif mm[p, s] == ninf:
                regret[q, p] = 0.0 if top == ninf else np.inf
            else:
                regret[q, p] = top - mm[p, s]
    if n:
        arg = (regret[:, 1:].argmax(axis=1) + 1).astype(np.int32)
        mx = regret[np.arange(len(x)), arg]
    else:
        arg, mx = np.zeros(len(x), dtype=np.int32), np.zeros(len(x))
    return dict(best=best, gap=gap, regret=regret, max_regret=mx, argmax_regret=arg,
                n_best=(x[:, 1:] == best[None, 1:]).sum(axis=1).astype(np.int32))


def kbest_of(res, recovered=None):
    """What Hansel.viterbi_kbest()'s dict `res` says per rank.  Host only, no handle.  Returns a dict of arrays with one entry per
    returned path:
      gap float64[n]       ll_chain[0] - ll_chain[i]: what rank i lacks to the best (0.0 where both are -inf);
      hamming0 int32[n]    the SNPs at which it differs from rank 0: a near-tie flipped at one SNP, or another sequence;
    and with `recovered` (uint8[H][N+1], the haplotypes a run recovered):
      nearest int32[n]     the row of `recovered` that differs from it at the fewest SNPs, the first of them at a tie;
      distance int32[n]    at how many SNPs -- 0 means it IS that haplotype.  Both are -1 where H = 0."""
    x = np.asarray(res["paths"], dtype=np.uint8)
    ll = np.asarray(res["ll_chain"], dtype=np.float64)
    n = len(ll)
    if x.ndim != 2 or len(x) != n:
        raise ValueError("kbest_of: paths must be [n][N+1] and ll_chain [n] (got %s, %s)" % (x.shape, ll.shape))
    gap = np.zeros(n)
    for i in range(n):
        gap[i] = 0.0 if ll[i] == ll[0] else ll[0] - ll[i]
    out = dict(gap=gap, hamming0=(x[:, 1:] != x[:1, 1:]).sum(axis=1).astype(np.int32))
    if recovered is not None:
        rec = np.asarray(recovered, dtype=np.uint8)
        if rec.ndim == 1:
            rec = rec.reshape(1, -1) if rec.size else rec.reshape(0, x.shape[1])
        if rec.ndim != 2 or rec.shape[1] != x.shape[1]:
            raise ValueError("kbest_of: recovered must be [H][N+1] with N+1 = %d (got %s)" % (x.shape[1], rec.shape))
        near = np.full(n, -1, dtype=np.int32)
        dist = np.full(n, -1, dtype=np.int32)
        if len(rec) and n:
            d = (x[:, None, 1:] != rec[None, :, 1:]).sum(axis=2)
            near = d.argmin(axis=1).astype(np.int32)                 # (argmin: the first of equals)
            dist = d[np.arange(n), near].astype(np.int32)
        out.update(nearest=near, distance=dist)
    return out


def _allele_bits(who, symbols):
    """The bits over the seven symbols of `symbols`: characters of "ACGT-" or their indices (0, 1, 2, 3, 5), one or several."""
    if isinstance(symbols, (int, np.integer)):
        symbols = [symbols]
    bits = 0
    for s in symbols:
        if isinstance(s, str):
            i = SYMBOLS.index(s) if s in SYMBOLS else -1
        else:
            i = int(s)
        if i not in (0, 1, 2, 3, 5):
            raise ValueError("%s: %r is no allele of ACGT-" % (who, s))
        bits |= 1 << i
    return bits


def grid_scratch_bytes(n, le, states):
    """vitg_layout's total (gretel_amd/csrc/scratch_layout.hpp) for a window of n SNPs, Le lags and `states` states: what a grid
    decoding reserves.  Host only.  Every part starts on a 256-byte boundary: the decoder's result words, two rows of n + 1
    candidate bytes, the table (n sources of 30 Le + 6 doubles), a back-pointer byte per position and state, two score rows, a
    (score, state) per 4096 states for the end rule, the path row.  0 beyond the grid decoder's cap; no states (nothing offered
    anywhere) leaves the first three parts."""
    def up(x):
        return (x + 255) & ~255
    if states > _lib.GH_VITERBI_GRID_MAX_STATES:
        return 0
    n1 = int(n) + 1
    head = up(24) + 2 * up(n1)
    if states < 1:
        return head
    parts = (states + 4095) // 4096
    return head + up(n * (30 * le + 6) * 8) + up(n1 * states) + up(16 * states) + up(8 * parts) + up(4 * parts) + up(n1)


def grid_marginals_scratch_bytes(n, le, states):
    """vitgm_layout's total (gretel_amd/csrc/scratch_layout.hpp) for a window of n SNPs, Le lags and `states` states: what the
    max-marginals on the grid reserve.  Host only.  Every part starts on a 256-byte boundary: grid_scratch_bytes' first three
    parts and the table, then one kept row of F per position (n * states doubles and the one +0.0 of position 0), two rows of B,
    five partial maxima per position and 512 states, mm [n + 1][7] and cm [n + 1].  0 beyond the grid's cap; no states leaves
    the first three parts."""
    def up(x):
        return (x + 255) & ~255
    if states > _lib.GH_VITERBI_GRID_MAX_STATES:
        return 0
    n1 = int(n) + 1
    head = up(24) + 2 * up(n1)
    if states < 1:
        return head
    wgs = (states + 511) // 512
    return (head + up(n * (30 * le + 6) * 8) + up((n * states + 1) * 8) + up(16 * states) + up(n * wgs * 5 * 8) + up(n1 * 7 * 8)
            + up(n1))


def allow_of(n, pins=None, bans=None):
    """One constraint set of Hansel.viterbi_path_masked for a window of n SNPs: uint8[n+1], all 0x7f (everything allowed) except
    where given.  Host only.  pins {p: symbols}: only these are allowed at SNP p; bans {p: symbols}: these are not (a ban on a
    pinned position takes from the pinned ones).  Symbols are characters of "ACGT-" or symbol indices, one or several.
    ValueError for a p outside 1..n or a symbol outside the five."""
    allow = np.full(int(n) + 1, 0x7F, dtype=np.uint8)
    for what, table in (("pins", pins), ("bans", bans)):
        for p, symbols in (table or {}).items():
            if not 1 <= int(p) <= n:
                raise ValueError("allow_of: %s at SNP %r, outside 1..%d" % (what, p, n))
            bits = _allele_bits("allow_of", symbols)
            allow[int(p)] = bits if what == "pins" else int(allow[int(p)]) & ~bits & 0x7F
    return allow


def alternatives_of(mm, cm, m, cand_order="ACGT-"):
    """The constraint sets `--alternatives m` decodes, and what they pin.  Host only.  mm, cm: Hansel.viterbi_marginals' table.
    Of the SNPs that offer at least two candidates the m of smallest margins_of gap (ascending gap, then ascending p); per SNP the
    runner-up is the offered candidate other than best[p] of largest mm[p][.], the first of cand_order among equals, and its set
    is all-allowed with allow[p] = 1 << runner-up: the best haplotype that carries the runner-up there.  Returns dict(p int32[m'],
    best uint8[m'], alt uint8[m'], gap float64[m'], allow uint8[m'][N+1]) with m' <= m."""
    mm = np.asarray(mm, dtype=np.float64)
    cm = np.asarray(cm, dtype=np.uint8)
    n = len(cm) - 1
    marg = margins_of(mm, cm, [], cand_order)
    order = [SYMBOLS.index(c) for c in cand_order]
    offered = {p: [s for s in order if (int(cm[p]) >> s) & 1] for p in range(1, n + 1)}
    ps = sorted((p for p in offered if len(offered[p]) >= 2), key=lambda p: (marg["gap"][p], p))[:max(0, int(m))]
    alt = []
    for p in ps:
        others = [s for s in offered[p] if s != marg["best"][p]]
        r = others[0]
        for s in others[1:]:
            if mm[p, s] > mm[p, r]:
                r = s
        alt.append(r)
    allow = np.full((len(ps), n + 1), 0x7F, dtype=np.uint8)
    for q, (p, r) in enumerate(zip(ps, alt)):
        allow[q, p] = 1 << r
    return dict(p=np.array(ps, dtype=np.int32), best=marg["best"][ps].astype(np.uint8) if ps else np.zeros(0, dtype=np.uint8),
                alt=np.array(alt, dtype=np.uint8), gap=marg["gap"][ps] if ps else np.zeros(0), allow=allow)


class Hansel:
    def __init__(self, n_snps, band=None, storage="f32", cond_mode="A", marginal_term=False, device=-1,
                 cand_order="ACGT-", offer_zero=False):
        """storage / cond_mode / marginal_term / cand_order / offer_zero: the switches of the Hansel arithmetic that the
        reference leaves to hanselx (include/gretel_hip.h: gh_config; same names as oracle.hansel_ref.HanselSpec)."""
        self._lib = _lib.load()
        self.n = int(n_snps)
        if sorted(cand_order) != sorted("ACGT-"):
            raise ValueError("cand_order must be a permutation of 'ACGT-' (got %r)" % (cand_order,))
        self._cfg = dict(storage=storage, cond_mode=cond_mode, marginal_term=bool(marginal_term), device=device,
                         cand_order=str(cand_order), offer_zero=bool(offer_zero))
        self.symbols = [HanselSymbol(c, i) for i, c in enumerate(SYMBOLS)]
        self.unsymbols = list(UNSYMBOLS)
        self.symbols_d = {str(s): s for s in self.symbols}
        self.is_weighted = False
        self._h = None
        self._band = None
        self._L = 1
        # observations staged on the host until the band width is known (init_matrix gives no hint)
        self._staged = []
        self.reads = None           # the device support table, kept by fill_from_support(..., keep_reads=True)
        if band is not None:
            self._create(int(band))

    # -- construction ----------------------------------------------------------------------
    @staticmethod
    def init_matrix(symbols, unsymbols, n_snps, band=None, **kw):
        """gretel/util.py:83.  The reference's fixed alphabet is the only one supported."""
        if list(symbols) != SYMBOLS or list(unsymbols) != UNSYMBOLS:
            raise ValueError("gretel_amd.Hansel supports the alphabet %r / unsymbols %r only" % (SYMBOLS, UNSYMBOLS))
        return Hansel(n_snps, band=band, **kw)

    def _create(self, band):
        order = (C.c_uint8 * 8)(*[SYMBOLS.index(c) for c in self._cfg["cand_order"]], 0, 0, 0)
        cfg = _lib.gh_config(self.n, max(1, band), _lib.GH_STORAGE[self._cfg["storage"]],
                             _lib.GH_COND[self._cfg["cond_mode"]], int(self._cfg["marginal_term"]),
                             self._cfg["device"], int(self._cfg["offer_zero"]), order)
        h = C.c_void_p()
        check(self._lib.gh_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._band = max(1, band)
        check(self._lib.gh_set_L(self._h, self._L))

    def _destroy(self):
        if getattr(self, "_h", None):
            self._lib.gh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _ensure(self, need_band=1):
        """Make the device tensor exist with band >= need_band and no staged observations."""
        st, self._staged = self._staged, []
        if st:
            need_band = max(need_band, max(j - i for (_, _, i, j) in st))
        if self._h is None:
            self._create(need_band)
        elif need_band > self._band:
            self._reband(need_band)
        if st:
            a = np.array([s[0] for s in st], dtype=np.uint8)
            b = np.array([s[1] for s in st], dtype=np.uint8)
            i = np.array([s[2] for s in st], dtype=np.int32)
            j = np.array([s[3] for s in st], dtype=np.int32)
            check(self._lib.gh_add_batch(self._h, _p(a), _p(b), _p(i), _p(j), len(st)))

    def _reband(self, band):
        old = self.export_band()
        stats = self._get_stats()
        self._destroy()
        self._create(band)
        new = np.zeros((self.n + 2, band, 7, 7))
        new[:, :old.shape[1]] = old
        check(self._lib.gh_import_band(self._h, _p(new)))
        check(self._lib.gh_set_fill_stats(self._h, C.byref(stats)))

    def copy(self):
        """gretel/cmd.py:79"""
        self._ensure()
        o = Hansel(self.n, **self._cfg)
        h = C.c_void_p()
        check(self._lib.gh_copy(self._h, C.byref(h)))
        o._h, o._band, o._L = h, self._band, self._L
        o.is_weighted = self.is_weighted
        return o

    # -- attributes ------------------------------------------------------------------------
    def _get_stats(self):
        st = _lib.gh_fill_stats()
        check(self._lib.gh_get_fill_stats(self._h, C.byref(st)))
        return st

    @property
    def L(self):
        return self._L

    @L.setter
    def L(self, v):
        self._L = int(v)
        if self._h is not None:
            check(self._lib.gh_set_L(self._h, self._L))

    @property
    def n_slices(self):
        return int(self._get_stats().n_slices) if self._h is not None else 0

    @n_slices.setter
    def n_slices(self, v):
        self._ensure()
        st = self._get_stats()
        st.n_slices = int(v)
        check(self._lib.gh_set_fill_stats(self._h, C.byref(st)))

    @property
    def n_crumbs(self):
        # (an attribute that only its setter and the fused fill write, like the reference's: staging an observation leaves it)
        return int(self._get_stats().n_crumbs) if self._h is not None else 0

    @n_crumbs.setter
    def n_crumbs(self, v):
        self._ensure()
        st = self._get_stats()
        st.n_crumbs = int(v)
        check(self._lib.gh_set_fill_stats(self._h, C.byref(st)))

    @property
    def band(self):
        return self._band

    # -- symbols ---------------------------------------------------------------------------
    def _num(self, sym):
        if isinstance(sym, HanselSymbol):
            return sym.i
        if isinstance(sym, (int, np.integer)):
            return int(sym)
        return self.symbols_d[sym].i        # KeyError like the reference for an unknown symbol

    def _path_indices(self, path, upto=None):
        n = len(path) if upto is None else upto
        return np.fromiter((self._num(path[q]) for q in range(n)), dtype=np.uint8, count=n)

    # -- one-cell API (compatibility; a host round trip per call) ---------------------------
    def add_observation(self, symbol_from, symbol_to, pos_from, pos_to):
        a, b = self._num(symbol_from), self._num(symbol_to)
        if not (0 <= pos_from < pos_to <= self.n + 1):
            raise IndexError("observation positions (%d,%d) outside 0 <= i < j <= %d" % (pos_from, pos_to, self.n + 1))
        self._staged.append((a, b, int(pos_from), int(pos_to)))
        if len(self._staged) >= (1 << 20):
            self._ensure()

    def get_observation(self, symbol_from, symbol_to, pos_from, pos_to):
        self._ensure()
        out = C.c_double()
        check(self._lib.gh_get(self._h, self._num(symbol_from), self._num(symbol_to), int(pos_from), int(pos_to), C.byref(out)))
        return out.value

    def reweight_observation(self, symbol_from, symbol_to, pos_from, pos_to, ratio):
        self._ensure()
        out = C.c_double()
        check(self._lib.gh_reweight_obs(self._h, self._num(symbol_from), self._num(symbol_to),
                                        int(pos_from), int(pos_to), float(ratio), C.byref(out)))
        return out.value

    # -- lookups ---------------------------------------------------------------------------
    def counts_array(self, at_pos):
        self._ensure()
        out = np.zeros(8)
        check(self._lib.gh_counts_at(self._h, int(at_pos), _p(out)))
        return out

    def get_counts_at(self, at_pos):
        """gretel/cmd.py:86,127 -- keys: symbol objects with a positive count, plus "total"."""
        c = self.counts_array(at_pos)
        marg = {"total": float(c[7])}
        for s in self.symbols:
            if c[s.i] > 0:
                marg[s] = float(c[s.i])
        return marg

    def get_marginal_of_at(self, of_symbol, at_pos):
        """gretel/gretel.py:182,186"""
        self._ensure()
        out = C.c_double()
        check(self._lib.gh_marginal_of_at(self._h, self._num(of_symbol), int(at_pos), C.byref(out)))
        return out.value

    def get_edge_weights_at(self, at_pos, current_path, debug=False):
        """gretel/gretel.py:155"""
        self._ensure()
        path = self._path_indices(current_path, upto=at_pos)
        w = np.zeros(7)
        mask = C.c_int()
        check(self._lib.gh_edge_weights_at(self._h, int(at_pos), _p(path), _p(w), C.byref(mask)))
        # (keys in the order the candidates are offered in: the tie-break of gretel/gretel.py:166-174)
        offered = [self.symbols_d[c] for c in self._cfg["cand_order"]]
        return {s: float(w[s.i]) for s in offered if (mask.value >> s.i) & 1}

    def candidate_masks(self):
        """uint32[N+1]: bit s set <=> valid symbol s is a candidate at that position."""
        self._ensure()
        out = np.zeros(self.n + 1, dtype=np.uint32)
        check(self._lib.gh_export_cmask(self._h, _p(out)))
        return out

    def gap_check(self):
        """gretel/cmd.py:85-118: first position in [0,N] without evidence, or -1."""
        self._ensure()
        g = C.c_int()
        check(self._lib.gh_gap_check(self._h, C.byref(g)))
        return g.value

    # -- fused fast paths --------------------------------------------------------------------
    def fill_from_support(self, rank, off, bases, use_end_sentinels=False, reads_handle=None, max_k=None, keep_reads=False):
        """The pair loop of gretel/util.py:226-286 for a whole support table at once.
        Returns (n_slices, n_crumbs, covered_snps) and sets L like util.py:333.
        max_k: the longest row of the table, where the caller knows it (the native decoder reports it: gio_stats.max_row_len) --
        a pass over off[] less; gh_reads_upload finds it again on the device and the band is checked against that.
        keep_reads: keep the device copy of the table as self.reads (a DeviceReads) for assign_reads; otherwise it is freed."""
        if reads_handle is None:
            reads_handle = DeviceReads(self, rank, off, bases, max_k=max_k)
        else:
            self._ensure(max(1, reads_handle.max_k - 1))
        st = _lib.gh_fill_stats()
        check(self._lib.gh_fill(self._h, reads_handle._r, int(bool(use_end_sentinels)), C.byref(st)))
        self._L = int(st.L)
        if keep_reads:
            self.reads = reads_handle
        return int(st.n_slices), int(st.n_crumbs), int(st.covered_snps)

    def assign_reads(self, paths, reads=None, min_snps=2, max_mismatch=-1, per_read=False):
        """Which of the haplotypes `paths` (uint8[H][N+1] symbol indices: rows of spin()'s paths) every read of a support table
        supports (gh_assign_reads; the definition: INTEGRATION.md "Read assignment").  reads: a DeviceReads of this Hansel's
        window; default self.reads (fill_from_support(..., keep_reads=True)).  Returns a dict: unique, shared, mismatches
        (int64[H]), n_reads, n_informative, n_unique, n_ambiguous, n_unexplained (ints) and, with per_read, hap, best,
        informative (int32[n_reads]; hap: the haplotype, -1 uninformative, -2 ambiguous, -3 unexplained).  The tensor is not
        touched."""
        if reads is None:
            reads = getattr(self, "reads", None)
        if reads is None:
            raise ValueError("assign_reads needs a support table on the device: pass reads=DeviceReads(...), or fill with "
                             "fill_from_support(..., keep_reads=True) / util.load_from_bam(..., keep_reads=True)")
        self._ensure()
        p = np.ascontiguousarray(paths, dtype=np.uint8)
        if p.ndim == 1 and p.size == 0:
            p = p.reshape(0, self.n + 1)
        if p.ndim != 2 or p.shape[1] != self.n + 1:
            raise ValueError("paths must be uint8[H][N+1] with N+1 = %d (got shape %s)" % (self.n + 1, p.shape))
        H = p.shape[0]
        unique = np.zeros(H, dtype=np.int64)
        shared = np.zeros(H, dtype=np.int64)
        mism = np.zeros(H, dtype=np.int64)
        out = {}
        if per_read:
            for k in ("hap", "best", "informative"):
                out[k] = np.zeros(reads.n_reads, dtype=np.int32)
        st = _lib.gh_assign_stats()
        rp = [_p(out[k]) if per_read else None for k in ("hap", "best", "informative")]
        check(self._lib.gh_assign_reads(self._h, reads._r, _p(p), H, int(min_snps), int(max_mismatch), _p(unique), _p(shared),
                                        _p(mism), rp[0], rp[1], rp[2], C.byref(st)))
        out.update(unique=unique, shared=shared, mismatches=mism, n_reads=int(st.n_reads), n_informative=int(st.n_informative),
                   n_unique=int(st.n_unique), n_ambiguous=int(st.n_ambiguous), n_unexplained=int(st.n_unexplained))
        return out

    def score_paths(self, paths, per_position=False):
        """How the haplotypes `paths` (uint8[H][N+1] symbol indices: rows of spin()'s paths; one path may come as uint8[N+1])
        stand against the tensor as it is now (gh_score_paths; the definition: INTEGRATION.md "Scoring haplotypes").  Returns a
        dict of arrays with one entry per haplotype: ll_chain, hp_current, hp_original, min_marginal, min_margin (float64),
        n_on, n_greedy, first_off, argmin_margin (int32); with per_position also weight, margin (float64[H][N+1]) and pick
        (uint8[H][N+1]).  The tensor is not touched."""
        self._ensure()
        p = np.ascontiguousarray(paths, dtype=np.uint8)
        if p.ndim == 1:
            p = p.reshape(1, -1) if p.size else p.reshape(0, self.n + 1)
        if p.ndim != 2 or p.shape[1] != self.n + 1:
            raise ValueError("paths must be uint8[H][N+1] with N+1 = %d (got shape %s)" % (self.n + 1, p.shape))
        H = p.shape[0]
        recs = np.zeros(H, dtype=SCORE_REC)
        out = {}
        if per_position:
            out = dict(weight=np.zeros(p.shape), margin=np.zeros(p.shape), pick=np.zeros(p.shape, dtype=np.uint8))
        pp = [_p(out[k]) if per_position else None for k in ("weight", "margin", "pick")]
        check(self._lib.gh_score_paths(self._h, _p(p), H, _p(recs), pp[0], pp[1], pp[2]))
        out.update((k, recs[k].copy()) for k in SCORE_REC.names)
        return out

    def beam_paths(self, width):
        """Beam search of `width` (1..32) hypotheses over the chain likelihood on the tensor as it is now (gh_beam_paths; the
        definition: INTEGRATION.md "Beam search").  Returns dict(n, hole_at, paths uint8[n][N+1] in rank order, ll_chain
        float64[n]); at a hole n = 0 and `prefix` holds what the rank-0 hypothesis had walked.  The tensor is not touched."""
        self._ensure()
        width = int(width)
        paths = np.zeros((max(1, min(width, _lib.GH_BEAM_MAX)), self.n + 1), dtype=np.uint8)
        ll = np.zeros(len(paths))
        n, hole = C.c_int(), C.c_int()
        check(self._lib.gh_beam_paths(self._h, width, _p(paths), _p(ll), C.byref(n), C.byref(hole)))
        out = dict(n=n.value, hole_at=hole.value, paths=paths[:n.value], ll_chain=ll[:n.value])
        if hole.value:
            out["prefix"] = paths[0, :hole.value].copy()
        return out

    def beam_spin(self, width, max_paths=100, min_remove=0.01):
        """gretel/cmd.py:148-179 with the rank-0 path of a beam of `width` in place of generate_path (gh_beam_spin: a host loop,
        not the throughput path).  Returns spin()'s dict plus ll_chain float64[n], the beam score of every path."""
        return self._decode_spin(self._lib.gh_beam_spin, int(width), max_paths=max_paths, min_remove=min_remove)

    def _decode_spin(self, fn, *lead_args, max_paths, min_remove):
        """A decoder's recovery loop in the library (gh_beam_spin, gh_viterbi_spin: `lead_args` between the handle and max_paths)."""
        self._ensure()
        nrec = C.sizeof(_lib.gh_path_rec) // 8
        paths = np.empty((max(0, max_paths), self.n + 1), dtype=np.uint8)
        recs = np.empty((max(1, max_paths), nrec), dtype=np.float64)
        ll = np.zeros(max(1, max_paths))
        n, hole = C.c_int(), C.c_int()
        check(fn(self._h, *lead_args, int(max_paths), float(min_remove), _p(paths), _p(recs), _p(ll), C.byref(n), C.byref(hole)))
        k = n.value
        if k:
            self.is_weighted = True
        r = recs[:k]
        return dict(n=k, hole_at=hole.value, paths=paths[:k], hp_current=r[:, 0].copy(), hp_original=r[:, 1].copy(),
                    ratio=r[:, 2].copy(), magnitude=r[:, 3].copy(), min_marginal=r[:, 4].copy(), ll_chain=ll[:k].copy())

    def _info4(self, fn):
        self._ensure()
        out = np.zeros(4, dtype=np.int64)
        check(fn(self._h, _p(out)))
        return tuple(int(v) for v in out)

    def beam_info(self):
        """The last beam run on this handle (gh_beam_info): (1 if the table slice was staged through LDS, source positions the
        LDS ring holds, threads of the walk workgroup, bytes of the beam's device scratch)."""
        return self._info4(self._lib.gh_beam_info)

    def viterbi_path(self):
        """The full path of largest chain likelihood on the tensor as it is now, exactly (gh_viterbi_path; the definition and
        the tie rule: INTEGRATION.md "Exact decoding").  Returns dict(path uint8[N+1], ll_chain, hole_at); at a hole path and
        ll_chain are None.  Served where S^min(L, N) <= 4096 states (S = the candidate symbols the window offers); beyond that
        GretelHipError, and viterbi_path_grid() (up to 2^24 states) or the beam is the tool.  The tensor is not touched."""
        self._ensure()
        path = np.zeros(self.n + 1, dtype=np.uint8)
        ll, hole = C.c_double(), C.c_int()
        check(self._lib.gh_viterbi_path(self._h, _p(path), C.byref(ll), C.byref(hole)))
        if hole.value:
            return dict(path=None, ll_chain=None, hole_at=hole.value)
        return dict(path=path, ll_chain=ll.value, hole_at=0)

    def viterbi_spin(self, max_paths=100, min_remove=0.01):
        """gretel/cmd.py:148-179 with the exact path in place of generate_path (gh_viterbi_spin: a host loop, not the
        throughput path).  Returns beam_spin()'s dict: ll_chain float64[n] is the exact maximum when each path was found."""
        return self._decode_spin(self._lib.gh_viterbi_spin, max_paths=max_paths, min_remove=min_remove)

    def viterbi_info(self):
        """The last exact decoding on this handle (gh_viterbi_info): (S candidate symbols, Le = min(L, N), states = S^Le,
        bytes of the decoder's device scratch)."""
        return self._info4(self._lib.gh_viterbi_info)

    def viterbi_marginals(self):
        """The max-marginals of the chain likelihood on the tensor as it is now (gh_viterbi_marginals; the definition:
        INTEGRATION.md "Max-marginals"): per SNP p and symbol s the best chain likelihood of any full path that takes s at p.
        Returns dict(mm float64[N+1][7], cm uint8[N+1] the candidate bits over the seven symbols, hole_at); entries of symbols
        not offered are -inf; at a hole mm and cm are None.  Served where viterbi_path() is; margins_of() reads the table.  The
        tensor is not touched."""
        self._ensure()
        mm = np.full((self.n + 1, 7), -np.inf)
        cm = np.zeros(self.n + 1, dtype=np.uint8)
        hole = C.c_int()
        check(self._lib.gh_viterbi_marginals(self._h, _p(mm), _p(cm), C.byref(hole)))
        if hole.value:
            return dict(mm=None, cm=None, hole_at=hole.value)
        return dict(mm=mm, cm=cm, hole_at=0)

    def viterbi_kbest(self, k):
        """The k full paths of largest chain likelihood on the tensor as it is now, exactly, best first (gh_viterbi_kbest; the
        definition and the two tie orders: INTEGRATION.md "K-best decoding").  Returns dict(n, hole_at, paths uint8[n][N+1],
        ll_chain float64[n]), n = min(k, the number of full paths); at a hole n = 0 and the arrays are empty.  Served for
        1 <= k <= 32 where k * S^min(L, N) <= 4096; beyond that GretelHipError, whose message names the largest k the window
        takes.  kbest_of() reads the result.  The tensor is not touched."""
        self._ensure()
        k = int(k)
        paths = np.zeros((max(1, min(k, _lib.GH_KBEST_MAX)), self.n + 1), dtype=np.uint8)
        ll = np.zeros(len(paths))
        n, hole = C.c_int(), C.c_int()
        check(self._lib.gh_viterbi_kbest(self._h, k, _p(paths), _p(ll), C.byref(n), C.byref(hole)))
        return dict(n=n.value, hole_at=hole.value, paths=paths[:n.value], ll_chain=ll[:n.value])

    def viterbi_path_masked(self, allow):
        """Exact decoding under per-position allele masks, one constraint set per row of `allow` (gh_viterbi_path_masked; the
        definition: INTEGRATION.md "Constrained decoding").  allow: uint8[n_sets][N+1] or one uint8[N+1], bit s of allow[.][p] set =
        symbol s (ACGTN-_) is allowed at SNP p (allow_of() builds a row from pins and bans); at most 256 sets a call, decoded side
        by side over one table.  Returns dict(paths uint8[n_sets][N+1], ll_chain float64[n_sets], hole_at int32[n_sets]): per set
        the best full path that respects it and its chain likelihood, exactly.  Where a set leaves some SNP p without a candidate,
        hole_at is p, ll_chain NaN (-inf is a legitimate score) and the row all 6.  Served where viterbi_path() is.  The tensor is
        not touched."""
        self._ensure()
        allow = np.ascontiguousarray(allow, dtype=np.uint8)
        if allow.ndim == 1:
            allow = allow.reshape(1, -1)
        if allow.ndim != 2 or allow.shape[1] != self.n + 1:
            raise ValueError("viterbi_path_masked: allow must be [n_sets][N+1] with N+1 = %d (got %s)" % (self.n + 1, allow.shape))
        m = len(allow)
        paths = np.full((m, self.n + 1), 6, dtype=np.uint8)
        ll = np.full(m, np.nan)
        hole = np.zeros(m, dtype=np.int32)
        check(self._lib.gh_viterbi_path_masked(self._h, _p(allow), m, _p(paths), _p(ll), _p(hole)))
        return dict(paths=paths, ll_chain=ll, hole_at=hole)

    def viterbi_masked_info(self):
        """The last viterbi_path_masked() on this handle (gh_viterbi_masked_info): (sets, sets that met a hole, walk launches,
        bytes of the decoder's device scratch)."""
        return self._info4(self._lib.gh_viterbi_masked_info)

    def viterbi_kbest_max(self):
        """The largest k viterbi_kbest() takes on the tensor as it stands: min(32, 4096 // states) from viterbi_states(), and 0
        where the window is beyond the exact decoder's cap (or offers nothing anywhere).  Host arithmetic over that call."""
        states = self.viterbi_states()[2]
        if states < 1 or states > _lib.GH_VITERBI_MAX_STATES:
            return 0
        return min(_lib.GH_KBEST_MAX, _lib.GH_VITERBI_MAX_STATES // states)

    def viterbi_states(self):
        """(S, Le, states = S^Le) of the tensor as it stands, without decoding (gh_viterbi_states): what viterbi_path would need.
        The count is given however large it is (it saturates at 2^63 - 1); the decoder serves up to 4096."""
        self._ensure()
        out = np.zeros(3, dtype=np.int64)
        check(self._lib.gh_viterbi_states(self._h, _p(out)))
        return tuple(int(v) for v in out)

    def viterbi_path_grid(self):
        """viterbi_path() through the grid decoder (gh_viterbi_path_grid; INTEGRATION.md "Exact decoding on the grid"): the same
        definition and the same dict, bit for bit where both serve a window, for up to 2^24 states -- the score rows lie in device
        memory and every SNP is a kernel launch.  Always the grid kernels, whatever the state count; viterbi_grid_bytes() says
        beforehand what it reserves.  The tensor is not touched."""
        self._ensure()
        path = np.zeros(self.n + 1, dtype=np.uint8)
        ll, hole = C.c_double(), C.c_int()
        check(self._lib.gh_viterbi_path_grid(self._h, _p(path), C.byref(ll), C.byref(hole)))
        if hole.value:
            return dict(path=None, ll_chain=None, hole_at=hole.value)
        return dict(path=path, ll_chain=ll.value, hole_at=0)

    def viterbi_spin_grid(self, max_paths=100, min_remove=0.01):
        """viterbi_spin() with the grid decoding per path (gh_viterbi_spin_grid): the same dict."""
        return self._decode_spin(self._lib.gh_viterbi_spin_grid, max_paths=max_paths, min_remove=min_remove)

    def viterbi_grid_info(self):
        """The last grid decoding on this handle (gh_viterbi_grid_info): viterbi_info()'s tuple, (S, Le, states, bytes of the
        device scratch it reserved); all 0 before the first."""
        return self._info4(self._lib.gh_viterbi_grid_info)

    def viterbi_grid_bytes(self):
        """The device scratch a grid decoding of the tensor as it stands reserves where it meets no hole, and 0 where the window
        is beyond the grid decoder's cap.  Host arithmetic over viterbi_states(): vitg_layout of gretel_amd/csrc/scratch_layout.hpp."""
        _, le, states = self.viterbi_states()
        return grid_scratch_bytes(self.n, le, states)

    def viterbi_marginals_grid(self):
        """viterbi_marginals() on the grid (gh_viterbi_marginals_grid; INTEGRATION.md "Max-marginals on the grid"): the same
        definition and the same dict, equal as IEEE values where both serve a window, for up to 2^24 states -- one kept row of F
        per SNP in device memory, two launches per SNP.  Always the grid kernels, whatever the state count;
        viterbi_marginals_grid_bytes() says beforehand what it reserves, viterbi_grid_info() afterwards describes the call.  The
        tensor is not touched."""
        self._ensure()
        mm = np.full((self.n + 1, 7), -np.inf)
        cm = np.zeros(self.n + 1, dtype=np.uint8)
        hole = C.c_int()
        check(self._lib.gh_viterbi_marginals_grid(self._h, _p(mm), _p(cm), C.byref(hole)))
        if hole.value:
            return dict(mm=None, cm=None, hole_at=hole.value)
        return dict(mm=mm, cm=cm, hole_at=0)

    def viterbi_marginals_grid_bytes(self):
        """The device scratch viterbi_marginals_grid() reserves on the tensor as it stands where it meets no hole, and 0 where the
        window is beyond the grid's cap.  Host arithmetic over viterbi_states(): vitgm_layout of
        gretel_amd/csrc/scratch_layout.hpp."""
        _, le, states = self.viterbi_states()
        return grid_marginals_scratch_bytes(self.n, le, states)

    def clear(self):
        self._staged = []
        if self._h is not None:
            check(self._lib.gh_clear(self._h))
        self._L = 1

    def snapshot_original(self):
        self._ensure()
        check(self._lib.gh_snapshot_original(self._h))

    def generate_path(self, original=None):
        """gretel/gretel.py:102-189 as one kernel.  Returns (indices uint8[N+1], hp_current,
        hp_original, min_marginal) or (None, hole_at, prefix walked)."""
        self._ensure()
        oh = None
        if original is not None and original is not self:
            original._ensure()
            oh = original._h
        path = np.zeros(self.n + 1, dtype=np.uint8)
        hc, ho, mn, hole = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        check(self._lib.gh_generate_path(self._h, oh, _p(path), C.byref(hc), C.byref(ho), C.byref(mn), C.byref(hole)))
        if hole.value:
            return None, hole.value, path[:hole.value]
        return path, hc.value, ho.value, mn.value

    def reweight_from_path(self, path_indices, ratio):
        """gretel/gretel.py:79-98 as one kernel."""
        self._ensure()
        p = np.ascontiguousarray(path_indices, dtype=np.uint8)
        if p.shape[0] != self.n + 1:
            raise ValueError("path must have N+1 = %d entries" % (self.n + 1))
        out = C.c_double()
        check(self._lib.gh_reweight_path(self._h, _p(p), float(ratio), C.byref(out)))
        self.is_weighted = True
        return out.value

    def spin(self, max_paths=100, min_remove=0.01, out_paths=None, out_recs=None):
        """gretel/cmd.py:148-179 on the device.  Returns dict(n, hole_at, paths uint8[n][N+1],
        hp_current, hp_original, ratio, magnitude).  out_paths uint8[max_paths][N+1] / out_recs float64[max_paths][5]: write the
        results there (C-contiguous; e.g. views of a pinned buffer that a gather sends on, gretel_amd.dist.ResultExchange) --
        `paths` of the returned dict is then a view of out_paths."""
        self._ensure()
        # (gh_spin writes rows 0 .. n-1 of both; gh_path_rec is five doubles -- include/gretel_hip.h)
        nrec = C.sizeof(_lib.gh_path_rec) // 8
        if out_paths is not None:
            if out_paths.dtype != np.uint8 or out_paths.shape != (max_paths, self.n + 1) or not out_paths.flags.c_contiguous:
                raise ValueError("out_paths must be a C-contiguous uint8[%d][%d]" % (max_paths, self.n + 1))
            paths = out_paths
        else:
            paths = np.empty((max_paths, self.n + 1), dtype=np.uint8)
        if out_recs is not None:
            if out_recs.dtype != np.float64 or out_recs.shape != (max(1, max_paths), nrec) or not out_recs.flags.c_contiguous:
                raise ValueError("out_recs must be a C-contiguous float64[%d][%d]" % (max(1, max_paths), nrec))
            recs = out_recs
        else:
            recs = np.empty((max(1, max_paths), nrec), dtype=np.float64)
        n, hole = C.c_int(), C.c_int()
        check(self._lib.gh_spin(self._h, int(max_paths), float(min_remove), _p(paths), _p(recs), C.byref(n), C.byref(hole)))
        k = n.value
        if k:
            self.is_weighted = True
        r = recs[:k]
        return dict(n=k, hole_at=hole.value, paths=paths[:k], hp_current=r[:, 0].copy(), hp_original=r[:, 1].copy(),
                    ratio=r[:, 2].copy(), magnitude=r[:, 3].copy(), min_marginal=r[:, 4].copy())

    def path_symbols(self, indices):
        return [self.symbols[int(q)] for q in indices]

    @staticmethod
    def path_str(indices):
        return _SYM_LUT[np.asarray(indices, dtype=np.uint8)].tobytes().decode()

    # -- export ----------------------------------------------------------------------------
    def export_band(self):
        self._ensure()
        out = np.zeros((self.n + 2, self._band, 7, 7))
        check(self._lib.gh_export_band(self._h, _p(out)))
        return out

    def export_dense(self):
        """[7][7][N+2][N+2] like the reference tensor (gretel/cmd.py:76-77); small N only."""
        self._ensure()
        out = np.zeros((7, 7, self.n + 2, self.n + 2))
        check(self._lib.gh_export_dense(self._h, _p(out)))
        return out

    def save_hansel_dump(self, path):
        """gretel/cmd.py:82 (--dumpmatrix).  hanselx's dump format is not in the reference
        tree; this writes an .npz with the banded tensor and the attributes."""
        np.savez_compressed(path, band=self.export_band(), n_snps=self.n, L=self.L,
                            n_slices=self.n_slices, n_crumbs=self.n_crumbs, symbols=np.array(SYMBOLS))

    # -- profiling (bench.py) ----------------------------------------------------------------
    def profile_enable(self, on=True):
        self._ensure()
        check(self._lib.gh_profile_enable(self._h, int(on)))

    def profile_reset(self):
        check(self._lib.gh_profile_reset(self._h))

    def profile_get(self):
        out = {}
        for name, k in _lib.GH_K.items():
            ms, n, by = C.c_double(), C.c_int64(), C.c_double()
            check(self._lib.gh_profile_get(self._h, k, C.byref(ms), C.byref(n)))
            check(self._lib.gh_profile_bytes(self._h, k, C.byref(by)))
            out[name] = dict(ms=ms.value, launches=n.value, bytes_per_launch=by.value)
        return out

    def profile_overhead(self, reps=20):
        """(ms of an empty HIP-event bracket, ms of a bracket around an empty kernel) on this handle's stream."""
        out = (C.c_double * 2)()
        check(self._lib.gh_profile_overhead(self._h, int(reps), out))
        return float(out[0]), float(out[1])

    def walk_clock(self):
        """(shader cycles, 100 MHz ticks, steps, variant) of the walker wave in the last path-extension launch."""
        out = (C.c_uint64 * 4)()
        check(self._lib.gh_debug_walk_clock(self._h, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def spin_plan(self):
        """Which kernels the last spin() ran for every path (gh_spin_plan of include/gretel_hip.h as a dict: flow, emit_small, seg6,
        stride, rw_lanes, S, mixed, lds); flow "none" before the first spin."""
        self._ensure()
        out = _lib.gh_spin_plan()
        check(self._lib.gh_debug_last_spin_plan(self._h, C.byref(out)))
        return out.as_dict()

    def sync(self):
        if self._h is not None:
            check(self._lib.gh_sync(self._h))


class _PinnedBlock:
    """One gh_host_alloc block; freed (gh_host_free) when the last numpy array made over it has gone."""

    def __init__(self, lib, nbytes):
        self._lib = lib
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(lib.gh_host_alloc(self.nbytes, C.byref(p)))
        self._p = p

    def array(self, dtype, count):
        dtype = np.dtype(dtype)
        assert count * dtype.itemsize <= self.nbytes
        raw = (C.c_uint8 * max(1, count * dtype.itemsize)).from_address(self._p.value)
        raw._gh_owner = self            # numpy keeps `raw` as the array's base, `raw` keeps the block
        return np.frombuffer(raw, dtype=dtype, count=count)

    def __del__(self):
        try:
            if getattr(self, "_p", None):
                self._lib.gh_host_free(self._p)
                self._p = None
        except Exception:
            pass


class PinnedTableArena:
    """Page-locked homes for a support table's three arrays (rank, off, bases), kept and grown from window to window: the native
    decoder writes the table straight into them (gretel_amd.bamio.native_support_table(arena=...), include/gretel_io.h:
    gio_support_table_from_bam_alloc) and gh_reads_upload reads them by DMA -- no 17 MB of fresh pages per million reads for the
    decoder to fault in, no staging copy for the upload.  The arrays handed out are views: their contents stand until the arena
    takes the next table, the memory for as long as a view refers to it (_PinnedBlock)."""

    def __init__(self):
        self._lib = _lib.load()
        self._blocks = [None, None, None]

    def alloc(self, which, nbytes):
        b = self._blocks[which]
        if b is None or b.nbytes < nbytes:
            # (half as much again: the next window of a contig is about as deep, not exactly)
            b = self._blocks[which] = _PinnedBlock(self._lib, max(4096, nbytes + nbytes // 2))
        return b._p.value

    def view(self, which, dtype, count):
        if count == 0:
            return np.zeros(0, dtype=dtype)
        return self._blocks[which].array(dtype, count)


_table_arena = None
# (one table at a time in the process-wide arena: load_from_bam holds this from the decode until the upload has read the table --
# ctypes releases the GIL inside both, and a second thread's decode would write into the blocks the first one is uploading from)
table_arena_lock = threading.RLock()


def table_arena():
    """The process's PinnedTableArena (made at first use; None where page-locked memory cannot be had: no GPU runtime)."""
    global _table_arena
    if _table_arena is None:
        try:
            a = PinnedTableArena()
            a.alloc(2, 4096)
            _table_arena = a
        except Exception:
            _table_arena = False
    return _table_arena or None


class HanselBatch:
    """Many windows of one shape recovered together (gh_batch_*): every kernel of the spin loop
    (gretel/cmd.py:148-179) is launched over all windows at once, one path-extension workgroup per
    window.  The Hansels must already be filled and agree on n_snps, band, storage, modes and L."""

    def __init__(self, hansels):
        self.hansels = list(hansels)
        if not self.hansels:
            raise ValueError("empty batch")
        for h in self.hansels:
            h._ensure()
        self._lib = self.hansels[0]._lib
        arr = (C.c_void_p * len(self.hansels))(*[h._h for h in self.hansels])
        b = C.c_void_p()
        check(self._create(arr, len(self.hansels), C.byref(b)))
        self._b = b

    def _create(self, arr, n, out):
        return self._lib.gh_batch_create(arr, n, out)

    def __del__(self):
        try:
            self._free_host_buffers()
            if getattr(self, "_b", None):
                self._lib.gh_batch_destroy(self._b)
                self._b = None
        except Exception:
            pass

    def pipe_info(self):
        """The last spin(): windows the window pipeline (csrc/wpipe.hpp) carried, windows it handed back to gh_spin, its
        threads per workgroup and positions per chunk."""
        out = (C.c_int32 * 4)()
        check(self._lib.gh_batch_pipe_info(self._b, out))
        return dict(windows=out[0], handed_back=out[1], threads=out[2], chunk=out[3])

    def profile_enable(self, every=10):
        """HIP events around the batched extension and the batched reweight of every `every`-th path (first window group)."""
        check(self._lib.gh_batch_profile_enable(self._b, int(every)))

    def profile_get(self):
        out = {}
        for name in ("walk", "reweight"):
            ms, n, w, by = C.c_double(), C.c_int64(), C.c_int32(), C.c_double()
            check(self._lib.gh_batch_profile_get(self._b, _lib.GH_K[name], C.byref(ms), C.byref(n), C.byref(w), C.byref(by)))
            out[name] = dict(ms=ms.value, launches=n.value, windows=w.value, bytes_per_launch=by.value)
        return out

    def _host_buffers(self, max_paths):
        """Page-locked result buffers, kept from call to call (gh_host_alloc): the copies of 256 windows x 100 paths run at the
        link's rate and no 256 MB array is faulted in per call.  Window w's paths are max_paths rows of n_w + 1 bytes from
        self._hb_off[w], back to back (for a batch: [n][max_paths][n + 1]); self._hb_win[w] is that [max_paths][n_w + 1] view.
        Every block is owned by a _PinnedBlock that the arrays made over it keep alive: a view handed out by spin(copy=False)
        stays valid memory for as long as anything refers to it, also when the batch has moved on to buffers of another shape or
        is gone (they used to point at freed pinned memory)."""
        n1s = tuple(h.n + 1 for h in self.hansels)
        key = (max_paths, n1s)
        if getattr(self, "_hb_key", None) != key:
            self._free_host_buffers()
            n = len(n1s)
            off = np.zeros(n, dtype=np.int64)
            off[1:] = np.cumsum(np.asarray(n1s[:-1], dtype=np.int64) * max_paths)
            sizes = (sum(n1s) * max_paths, n * max_paths * 5 * 8)
            blocks = [_PinnedBlock(self._lib, max(1, sz)) for sz in sizes]
            self._hb_paths = blocks[0].array(np.uint8, sizes[0])
            self._hb_recs = blocks[1].array(np.float64, sizes[1] // 8).reshape(n, max_paths, 5)
            self._hb_off = off
            self._hb_win = [self._hb_paths[o:o + max_paths * k].reshape(max_paths, k) for o, k in zip(off.tolist(), n1s)]
            self._hb_key = key
        return self._hb_paths, self._hb_recs

    def _free_host_buffers(self):
        # (the blocks free themselves when the last array over them is gone)
        self._hb_key, self._hb_paths, self._hb_recs, self._hb_off, self._hb_win = None, None, None, None, None

    def _spin(self, max_paths, min_remove, paths, recs, n_out, hole):
        check(self._lib.gh_batch_spin(self._b, int(max_paths), float(min_remove), _p(paths), _p(recs), _p(n_out), _p(hole)))

    def spin(self, max_paths=100, min_remove=0.01, copy=True):
        """One dict per window, the keys and dtypes of Hansel.spin.  copy=False: the returned arrays are views of the batch's
        page-locked buffers (no 256 MB copy on the host); their CONTENTS stand until the next spin() of this batch overwrites
        them, the memory itself for as long as a view refers to it.  copy=True (default): every window gets its own arrays."""
        n = len(self.hansels)
        paths, recs = self._host_buffers(max_paths)
        n_out = np.zeros(n, dtype=np.int32)
        hole = np.zeros(n, dtype=np.int32)
        self._spin(max_paths, min_remove, paths, recs, n_out, hole)
        out = []
        for w in range(n):
            k = int(n_out[w])
            if k:
                self.hansels[w].is_weighted = True
            pw, rw = self._hb_win[w][:k], recs[w, :k]
            if copy:
                pw, rw = pw.copy(), rw.copy()
            out.append(dict(n=k, hole_at=int(hole[w]), paths=pw, hp_current=rw[:, 0], hp_original=rw[:, 1], ratio=rw[:, 2],
                            magnitude=rw[:, 3], min_marginal=rw[:, 4]))
        return out


    def viterbi_spin(self, max_paths=100, min_remove=0.01):
        """Hansel.viterbi_spin over every window, the exact decoders of a round side by side in one launch each
        (gh_panel_viterbi_spin).  One dict per window, shaped as Hansel.viterbi_spin's (ll_chain included), each the result of
        that call on the window alone.  A window beyond the decoder's cap refuses the whole call before anything is touched
        (GretelHipError names the window): ask Hansel.viterbi_states() first."""
        n = len(self.hansels)
        paths, recs = self._host_buffers(max(1, max_paths))
        ll = np.zeros((n, max(1, max_paths)))
        n_out = np.zeros(n, dtype=np.int32)
        hole = np.zeros(n, dtype=np.int32)
        check(self._lib.gh_panel_viterbi_spin(self._b, int(max_paths), float(min_remove), _p(paths), _p(self._hb_off), _p(recs), _p(ll),
                                              _p(n_out), _p(hole)))
        out = []
        for w in range(n):
            k = int(n_out[w])
            if k:
                self.hansels[w].is_weighted = True
            pw, rw = self._hb_win[w][:k].copy(), recs[w, :k].copy()
            out.append(dict(n=k, hole_at=int(hole[w]), paths=pw, hp_current=rw[:, 0], hp_original=rw[:, 1], ratio=rw[:, 2],
                            magnitude=rw[:, 3], min_marginal=rw[:, 4], ll_chain=ll[w, :k].copy()))
        return out

    def viterbi_info(self):
        """The last viterbi_spin() of this batch (gh_panel_viterbi_info): (windows, rounds run, the most windows one walk launch
        carried, walk launches in all)."""
        out = np.zeros(4, dtype=np.int64)
        check(self._lib.gh_panel_viterbi_info(self._b, _p(out)))
        return tuple(int(v) for v in out)


    def viterbi_marginals(self):
        """Hansel.viterbi_marginals over every window, the forward walks side by side in one launch and the backward walks in
        another (gh_panel_viterbi_marginals).  One dict per window, shaped as Hansel.viterbi_marginals': mm float64[n+1][7], cm
        uint8[n+1], hole_at; mm and cm are None at a hole.  Each window gets its own arrays, each the result of that call on
        the window alone.  The tensors are not touched.  A window beyond the decoder's cap refuses the whole call before
        anything is touched (GretelHipError names the window): ask Hansel.viterbi_states() first.  The scratch is the sum of
        the windows' N * states * 8 bytes."""
        n = len(self.hansels)
        n1s = np.asarray([h.n + 1 for h in self.hansels], dtype=np.int64)
        off = np.zeros(n, dtype=np.int64)
        off[1:] = np.cumsum(n1s[:-1])
        mm = np.full((int(n1s.sum()), 7), -np.inf)
        cm = np.zeros(int(n1s.sum()), dtype=np.uint8)
        hole = np.zeros(n, dtype=np.int32)
        check(self._lib.gh_panel_viterbi_marginals(self._b, _p(mm), _p(cm), _p(off), _p(hole)))
        out = []
        for w in range(n):
            if hole[w]:
                out.append(dict(mm=None, cm=None, hole_at=int(hole[w])))
            else:
                a, e = int(off[w]), int(off[w] + n1s[w])
                out.append(dict(mm=mm[a:e].copy(), cm=cm[a:e].copy(), hole_at=0))
        return out

    def viterbi_marginals_info(self):
        """The last viterbi_marginals() of this batch (gh_panel_viterbi_marginals_info): (windows, windows that met a hole, walk
        launches -- forward and backward together --, scratch bytes summed over the handles' blocks)."""
        out = np.zeros(4, dtype=np.int64)
        check(self._lib.gh_panel_viterbi_marginals_info(self._b, _p(out)))
        return tuple(int(v) for v in out)


    def viterbi_kbest(self, k):
        """Hansel.viterbi_kbest over every window, the walks side by side in one launch and the traces in another
        (gh_panel_viterbi_kbest).  k: an int for all windows, or a sequence with one entry per window (regions differ in their
        states, so the largest k they take differs: Hansel.viterbi_kbest_max()).  One dict per window, shaped as
        Hansel.viterbi_kbest's: n, hole_at, paths uint8[n][n_snps + 1], ll_chain float64[n]; each window gets its own arrays, each
        the result of that call on the window alone.  The tensors are not touched.  A window the single call would refuse (too
        many states, or k lists of them too many slots) refuses the whole call before anything is touched (GretelHipError names
        the window).  The scratch is the sum of the windows' (N + 1) * states * k bytes and their tables."""
        n = len(self.hansels)
        try:
            ks = [int(k)] * n
        except TypeError:
            ks = [int(v) for v in k]
            if len(ks) != n:
                raise ValueError("viterbi_kbest: k has %d entries for %d windows" % (len(ks), n))
        ka = np.asarray(ks, dtype=np.int32)
        # (room for what a refused k would ask is not needed: the call refuses before it writes)
        room = np.clip(ka, 1, _lib.GH_KBEST_MAX).astype(np.int64)
        n1s = np.asarray([h.n + 1 for h in self.hansels], dtype=np.int64)
        poff = np.zeros(n, dtype=np.int64)
        poff[1:] = np.cumsum((room * n1s)[:-1])
        loff = np.zeros(n, dtype=np.int64)
        loff[1:] = np.cumsum(room[:-1])
        paths = np.zeros(int((room * n1s).sum()), dtype=np.uint8)
        ll = np.zeros(int(room.sum()))
        n_out = np.zeros(n, dtype=np.int32)
        hole = np.zeros(n, dtype=np.int32)
        check(self._lib.gh_panel_viterbi_kbest(self._b, _p(ka), _p(paths), _p(poff), _p(ll), _p(loff), _p(n_out), _p(hole)))
        out = []
        for w in range(n):
            m, n1, a, e = int(n_out[w]), int(n1s[w]), int(poff[w]), int(loff[w])
            out.append(dict(n=m, hole_at=int(hole[w]), paths=paths[a:a + m * n1].reshape(m, n1).copy(), ll_chain=ll[e:e + m].copy()))
        return out

    def viterbi_kbest_info(self):
        """The last viterbi_kbest() of this batch (gh_panel_viterbi_kbest_info): (windows, windows that met a hole, walk launches,
        scratch bytes summed over the handles' blocks)."""
        out = np.zeros(4, dtype=np.int64)
        check(self._lib.gh_panel_viterbi_kbest_info(self._b, _p(out)))
        return tuple(int(v) for v in out)


class HanselPanel(HanselBatch):
    """Many windows of DIFFERING shape recovered together (gh_panel_*): one region (gene) per window, each with its own n_snps,
    band and L.  The windows go in one group per L; the window pipeline (csrc/wpipe.hpp) carries every group it can, gh_spin
    the rest.  Every window's results are those of its Hansel.spin alone.  The Hansels must already be filled and agree on
    storage, modes and device."""

    def _create(self, arr, n, out):
        return self._lib.gh_panel_create(arr, n, out)

    def _spin(self, max_paths, min_remove, paths, recs, n_out, hole):
        check(self._lib.gh_panel_spin(self._b, int(max_paths), float(min_remove), _p(paths), _p(self._hb_off), _p(recs), _p(n_out),
                                      _p(hole)))


class DeviceReads:
    """A support table resident in HBM (gh_reads_upload)."""

    def __init__(self, hansel, rank, off, bases, max_k=None):
        rank = np.ascontiguousarray(rank, dtype=np.int32)
        off = np.ascontiguousarray(off, dtype=np.int64)
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        self.n_reads = len(rank)
        if max_k is None:
            max_k = int(np.diff(off).max()) if self.n_reads else 0
        hansel._ensure(max(1, int(max_k) - 1))
        self._lib = hansel._lib
        r = C.c_void_p()
        check(self._lib.gh_reads_upload(hansel._h, _p(rank), _p(off), _p(bases), self.n_reads, C.byref(r)))
        self._r = r
        # (what the device found: a caller's max_k that is too small shows as GH_ERR_BAND in the fill, as any read too long for the band)
        mk = C.c_int()
        check(self._lib.gh_reads_max_k(r, C.byref(mk)))
        self.max_k = int(mk.value)

    def info(self):
        """What the upload found out about the table (gh_reads_info): dict(max_k, sorted, span_pos, dens128, first_at)."""
        inf = np.zeros(5, dtype=np.int64)
        check(self._lib.gh_reads_info(self._r, _p(inf), None))
        fa = np.zeros(int(inf[4]), dtype=np.int64)
        if len(fa):
            check(self._lib.gh_reads_info(self._r, _p(inf), _p(fa)))
        return dict(max_k=int(inf[0]), sorted=bool(inf[1]), span_pos=int(inf[2]), dens128=int(inf[3]), first_at=fa)

    def __del__(self):
        try:
            if getattr(self, "_r", None):
                self._lib.gh_reads_free(self._r)
                self._r = None
        except Exception:
            pass
