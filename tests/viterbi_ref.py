"""The definition of the exact decoding of the chain likelihood (include/gretel_hip.h: gh_viterbi_path, gh_viterbi_spin;
INTEGRATION.md "Exact decoding") in plain Python, over any object `o` that offers

    o.edge_weights(p, path) -> (candidate mask over the seven symbols, the seven weights)      oracle.c_oracle.COracle has it
    o.marginal(s, p)        -> the current marginal of symbol s at p
    o.reweight_path(path, ratio) -> the removed mass
    o.L

Not a test file: tests/test_viterbi_host.py pins it against an exhaustive enumeration, tests/test_gpu_viterbi.py holds the GPU to
it.  A dict of the reachable states (the last Le picks) -> (score, prefix); every score is a Python float sum in ascending p from
0.0; the two tie rules are spelled out.  A reachable score of -inf is a score like any other: reachability is the dict's keys."""
import numpy as np

import score_ref

SYMS = "ACGTN-_"


def viterbi(o, n, cand_order="ACGT-"):
    """dict(path uint8[N+1] or None, ll_chain, hole_at); at a hole path and ll_chain are None."""
    order = [SYMS.index(c) for c in cand_order]
    q = {c: k for k, c in enumerate(order)}
    le = min(o.L, n)
    # the last min(Le, p) picks, oldest first -> (score, prefix); a prefix is the chain (shorter prefix, pick), so that states
    # share what they have in common
    states = {(): (0.0, None)}
    hist = np.full(n + 1, 6, dtype=np.uint8)                  # edge_weights reads positions p - min(L, p) .. p - 1: the state
    for p in range(1, n + 1):
        born = {}                                             # new state -> [(q of the pick that falls out of the state, score, prefix)]
        for key, (score, x) in states.items():
            hist[p - len(key):p] = key
            mask, w = o.edge_weights(p, hist)
            for c in order:
                if (mask >> c) & 1:
                    new = key + (c,)
                    # p <= Le: the state is the whole prefix, nothing competes; p > Le: the competitors differ at x[p - Le]
                    drop = q[new[0]] if len(new) > le else 0
                    born.setdefault(new[-le:], []).append((drop, score + float(w[c]), (x, c)))
        if not born:
            return dict(path=None, ll_chain=None, hole_at=p)
        states = {}
        for key, comp in born.items():
            assert p > le or len(comp) == 1
            comp.sort(key=lambda t: t[0])                     # ascending q(x[p - Le]) ...
            best = comp[0]
            for t in comp[1:]:
                if t[1] > best[1]:                            # ... the first stays, replaced only by a strictly larger score
                    best = t
            states[key] = (best[1], best[2])
    # the end: ascending lexicographic order of (q(x[N]), q(x[N-1]), ..., q(x[N-Le+1])), the first stays unless strictly beaten
    best = None
    for key in sorted(states, key=lambda k: [q[c] for c in reversed(k)]):
        if best is None or states[key][0] > best[0]:
            best = states[key]
    path, x = [], best[1]
    while x is not None:
        path.append(x[1])
        x = x[0]
    return dict(path=np.array([6] + path[::-1], dtype=np.uint8), ll_chain=best[0], hole_at=0)


def viterbi_spin(o, n, max_paths, min_remove=0.01, cand_order="ACGT-", original=None):
    """gretel/cmd.py:148-179 with the exact path in place of generate_path: Hansel.viterbi_spin's dict as arrays.
    original: the marginals the handle's snapshot froze (score_ref.marginals at that moment); None = no snapshot yet, it is
    taken here, as gh_viterbi_spin takes it."""
    def decode():
        res = viterbi(o, n, cand_order)
        return res["hole_at"], res["path"], res["ll_chain"]

    return score_ref.recover_spin(o, n, max_paths, min_remove, original, decode)
