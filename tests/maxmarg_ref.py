"""The definition of the max-marginals of the chain likelihood (include/gretel_hip.h: gh_viterbi_marginals; INTEGRATION.md
"Max-marginals") in plain Python, over any object `o` that offers

    o.edge_weights(p, path) -> (candidate mask over the seven symbols, the seven weights)      oracle.c_oracle.COracle has it
    o.L

Not a test file: tests/test_maxmarg_host.py pins it against an exhaustive enumeration, tests/test_gpu_maxmarg.py holds the GPU to
it.  Dicts of the reachable states (the last min(Le, p) picks, oldest first) forward and backward; every addition is a Python
float addition in the association the definition states: F = F' + w, B = w + B', M = F + B."""
import math

import numpy as np

SYMS = "ACGTN-_"
INF = math.inf


def _weights(o, hist, p, key):
    """(mask, weights) at target p behind the state `key` = the picks at p - len(key) .. p - 1.  (edge_weights reads positions
    p - min(L, p) .. p - 1: the state, and index 0, which stays '_'.)"""
    if key:
        hist[p - len(key):p] = key
    mask, w = o.edge_weights(p, hist)
    return int(mask), [float(v) for v in w]


def marginals(o, n):
    """dict(mm float64[N+1][7] or None, cm uint8[N+1] or None, hole_at)."""
    le = min(o.L, n)
    valid = (0, 1, 2, 3, 5)
    hist = np.full(n + 1, 6, dtype=np.uint8)
    fwd = [{(): 0.0}]                                         # fwd[p]: state -> F_p
    cm = np.zeros(n + 1, dtype=np.uint8)
    for p in range(1, n + 1):
        born = {}
        for key, score in fwd[p - 1].items():
            mask, w = _weights(o, hist, p, key)
            cm[p] = mask & 0x2F
            for c in valid:
                if (mask >> c) & 1:
                    new = (key + (c,))[-le:]
                    cand = score + w[c]
                    if new not in born or cand > born[new]:
                        born[new] = cand
        if not born:
            return dict(mm=None, cm=None, hole_at=p)
        fwd.append(born)
    mm = np.full((n + 1, 7), -INF)
    bwd = {key: 0.0 for key in fwd[n]}                        # B_N
    for p in range(n, 0, -1):
        for key, f in fwd[p].items():
            v = f + bwd[key]
            if v > mm[p, key[-1]]:
                mm[p, key[-1]] = v
        if p == 1:
            break
        prev = {}
        for key in fwd[p - 1]:
            mask, w = _weights(o, hist, p, key)
            best = None
            for c in valid:
                if (mask >> c) & 1:
                    cand = w[c] + bwd[(key + (c,))[-le:]]
                    if best is None or cand > best:
                        best = cand
            prev[key] = best
        bwd = prev
    return dict(mm=mm, cm=cm, hole_at=0)


def margins_of(mm, cm, paths, cand_order="ACGT-"):
    """gretel_amd.hansel.margins_of's rules, as lists."""
    n = len(cm) - 1
    order = [SYMS.index(c) for c in cand_order]
    best, gap = [6] * (n + 1), [0.0] * (n + 1)
    for p in range(1, n + 1):
        offered = [s for s in order if (int(cm[p]) >> s) & 1]
        if not offered:
            continue
        top = max(float(mm[p][s]) for s in offered)
        b = next(s for s in offered if float(mm[p][s]) == top)       # the first of cand_order among the maximisers
        best[p] = b
        others = [float(mm[p][s]) for s in offered if s != b]
        if top == -INF:
            gap[p] = 0.0
        elif not others or max(others) == -INF:
            gap[p] = INF
        else:
            gap[p] = top - max(others)
    paths = np.asarray(paths, dtype=np.uint8).reshape(-1, n + 1)
    out = dict(best=best, gap=gap, regret=[], max_regret=[], argmax_regret=[], n_best=[])
    for x in paths:
        reg = [0.0] * (n + 1)
        for p in range(1, n + 1):
            s, top = int(x[p]), float(mm[p][best[p]])
            if s > 6 or not (int(cm[p]) >> s) & 1:
                reg[p] = INF
            elif float(mm[p][s]) == -INF:
                reg[p] = 0.0 if top == -INF else INF
            else:
                reg[p] = top - float(mm[p][s])
        mx = max(reg[1:]) if n else 0.0
        out["regret"].append(reg)
        out["max_regret"].append(mx)
        out["argmax_regret"].append(1 + reg[1:].index(mx) if n else 0)
        out["n_best"].append(sum(int(x[p]) == best[p] for p in range(1, n + 1)))
    return out
