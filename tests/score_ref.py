"""The definition of haplotype scoring (include/gretel_hip.h: gh_score_paths; INTEGRATION.md "Scoring haplotypes") in plain
Python, over any object `o` that offers

    o.edge_weights(p, path) -> (candidate mask over the seven symbols, the seven weights)      oracle.c_oracle.COracle has it
    o.marginal(s, p)        -> the current marginal of symbol s at p
    o.L

Not a test file: tests/test_score_host.py pins it against the Python oracle, tests/test_gpu_score.py holds the GPU to it.
Every sum is a Python float loop over the on positions in ascending p, from 0.0 -- the order gh_score_paths keeps."""
import math

import numpy as np

SYMS = "ACGTN-_"
FIELDS = ("ll_chain", "hp_current", "hp_original", "min_marginal", "min_margin", "n_on", "n_greedy", "first_off", "argmin_margin")
INF = math.inf


def log10(x):
    """math.log10 (the running libm's: what COracle(use_libm=True) and oracle.hansel_ref take) with IEEE's answer at 0."""
    return -INF if x == 0.0 else math.log10(x)


def marginals(o, n):
    """The marginals of every symbol at positions 0..n as they stand now: keep them when the handle takes its snapshot and
    hand them to score() as `original`."""
    return [[o.marginal(s, p) for s in range(7)] for p in range(n + 1)]


def score_one(o, path, n, cand_order="ACGT-", original=None):
    """One path (N+1 symbol indices; index 0 is ignored, the history reads '_' there).  Returns (record dict, weight, margin,
    pick) with the three per-position lists N+1 long."""
    order = [SYMS.index(c) for c in cand_order]
    x = np.array([6] + [int(v) for v in path[1:n + 1]], dtype=np.uint8)
    weight, margin, pick = [0.0] * (n + 1), [0.0] * (n + 1), [6] + [255] * n
    ll = hc = ho = 0.0
    min_marginal = min_margin = INF
    n_on = n_greedy = first_off = first_on = argmin = 0
    for p in range(1, n + 1):
        mask, w = o.edge_weights(p, x)
        w = [float(v) for v in w]
        cands = [s for s in order if (mask >> s) & 1]
        pk, best = 255, 0.0
        for s in cands:                                   # gretel/gretel.py:166-174: first key, replaced only on strict >
            if pk == 255 or w[s] > best:
                pk, best = s, w[s]
        pick[p] = pk
        xp = int(x[p])
        if xp not in cands:
            weight[p] = margin[p] = -INF
            if first_off == 0:
                first_off = p
            continue
        other = None
        for s in range(7):
            if s != xp and (mask >> s) & 1 and (other is None or w[s] > other):
                other = w[s]
        weight[p] = w[xp]
        margin[p] = INF if other is None else w[xp] - other
        n_on += 1
        n_greedy += int(pk == xp)
        if first_on == 0:
            first_on = p
        ll += weight[p]
        m = o.marginal(xp, p)
        hc += log10(m)
        ho += log10(m if original is None else original[p][xp])
        if m < min_marginal:
            min_marginal = m
        if margin[p] < min_margin:                         # strict: the first position that has the minimum
            min_margin, argmin = margin[p], p
    if argmin == 0:                                        # a minimum of +inf: every on position has it, the first is its position
        argmin = first_on
    rec = dict(ll_chain=ll, hp_current=hc, hp_original=ho, min_marginal=min_marginal, min_margin=min_margin, n_on=n_on,
               n_greedy=n_greedy, first_off=first_off, argmin_margin=argmin)
    return rec, weight, margin, pick


def score(o, paths, n, cand_order="ACGT-", original=None):
    """Hansel.score_paths(paths, per_position=True) as lists: one entry per record field, plus weight, margin and pick."""
    paths = np.asarray(paths, dtype=np.uint8).reshape(-1, n + 1)
    out = {k: [] for k in FIELDS + ("weight", "margin", "pick")}
    for row in paths:
        rec, w, g, pk = score_one(o, row, n, cand_order, original)
        for k in FIELDS:
            out[k].append(rec[k])
        out["weight"].append(w)
        out["margin"].append(g)
        out["pick"].append(pk)
    return out


def recover_spin(o, n, max_paths, min_remove, original, decode):
    """gretel/cmd.py:148-179 around any decoder: decode() -> (hole_at, path, ll) on `o` as it stands, the path then recorded and
    reweighted.  Hansel.beam_spin's / viterbi_spin's dict as arrays.  original: the marginals the handle's snapshot froze
    (marginals() at that moment); None = no snapshot yet, it is taken here."""
    if original is None:
        original = marginals(o, n)
    out = dict(paths=[], hp_current=[], hp_original=[], ratio=[], magnitude=[], min_marginal=[], ll_chain=[])
    hole_at = 0
    for _ in range(max_paths):
        hole_at, x, ll = decode()
        if hole_at:
            break
        hc = ho = 0.0
        mn = float("inf")
        for p in range(1, n + 1):
            m = o.marginal(int(x[p]), p)
            mn = min(mn, m)
            hc += log10(m)
            ho += log10(original[p][int(x[p])])
        ratio = max(mn, min_remove)
        out["paths"].append(x)
        out["hp_current"].append(hc)
        out["hp_original"].append(ho)
        out["min_marginal"].append(mn)
        out["ratio"].append(ratio)
        out["magnitude"].append(o.reweight_path(x, ratio))
        out["ll_chain"].append(ll)
    k = len(out["paths"])
    res = {key: np.array(v, dtype=np.float64) for key, v in out.items() if key != "paths"}
    res.update(n=k, hole_at=hole_at, paths=np.array(out["paths"], dtype=np.uint8).reshape(k, n + 1))
    return res


def _nan_named(v):
    """== on lists takes an infinity as equal to itself but not a NaN: name the NaNs, so that a NaN must meet a NaN."""
    if isinstance(v, list):
        return [_nan_named(q) for q in v]
    return "nan" if isinstance(v, float) and v != v else v


def assert_same(got, ref, per_position=True):
    """Every field of Hansel.score_paths' dict exactly equal to score()'s (== on lists: an infinity equals itself)."""
    for k in FIELDS + (("weight", "margin", "pick") if per_position else ()):
        g, r = _nan_named(np.asarray(got[k]).tolist()), _nan_named(ref[k])
        assert g == r, (k, next((q, a, b) for q, (a, b) in enumerate(zip(g, r)) if a != b) if len(g) == len(r) else (len(g), len(r)))
