"""The definition of k-best exact decoding of the chain likelihood (include/gretel_hip.h: gh_viterbi_kbest; INTEGRATION.md "K-best
decoding") in plain Python, over any object `o` that offers

    o.edge_weights(p, path) -> (candidate mask over the seven symbols, the seven weights)      oracle.c_oracle.COracle has it
    o.L

Not a test file: tests/test_kbest_host.py pins it against an exhaustive enumeration, tests/test_gpu_kbest.py holds the GPU to it.
A dict of the reachable states (the last Le picks) -> the ranked list of (score, prefix), at most K long; every score is a Python
float sum in ascending p from 0.0; the two orders are spelled out.  A reachable score of -inf is a score like any other:
reachability is the dict's keys and the lists' lengths."""
import numpy as np

SYMS = "ACGTN-_"


def kbest(o, n, k, cand_order="ACGT-"):
    """dict(n, hole_at, paths uint8[n][N+1], ll_chain float64[n]); at a hole n = 0 and the arrays are empty."""
    order = [SYMS.index(c) for c in cand_order]
    q = {c: i for i, c in enumerate(order)}
    le = min(o.L, n)
    # the last min(Le, p) picks, oldest first -> [(score, prefix)] in rank order; a prefix is the chain (shorter prefix, pick)
    states = {(): [(0.0, None)]}
    hist = np.full(n + 1, 6, dtype=np.uint8)                  # edge_weights reads positions p - min(L, p) .. p - 1: the state
    for p in range(1, n + 1):
        born = {}                  # new state -> [(score, q of the pick that falls out of the state, the parent's rank, prefix)]
        for key, ranked in states.items():
            hist[p - len(key):p] = key
            mask, w = o.edge_weights(p, hist)
            for c in order:
                if (mask >> c) & 1:
                    new = key + (c,)
                    # p <= Le: the state is the whole prefix, one predecessor; p > Le: the children differ at x[p - Le] or in r
                    drop = q[new[0]] if len(new) > le else 0
                    for r, (score, x) in enumerate(ranked):
                        born.setdefault(new[-le:], []).append((score + float(w[c]), drop, r, (x, c)))
        if not born:
            return dict(n=0, hole_at=p, paths=np.zeros((0, n + 1), dtype=np.uint8), ll_chain=np.zeros(0))
        states = {}
        for key, children in born.items():
            assert p > le or len(children) == 1
            states[key] = [(t[0], t[3]) for t in _ordered(children)[:k]]
    # the end: score descending, then ascending lexicographic (q(x[N]), q(x[N-1]), ..., q(x[N-Le+1])), then the rank
    fin = [(score, [q[c] for c in reversed(key)], r, x) for key, ranked in states.items() for r, (score, x) in enumerate(ranked)]
    paths, ll = [], []
    for score, _, _, x in _ordered(fin)[:k]:
        path = []
        while x is not None:
            path.append(x[1])
            x = x[0]
        paths.append([6] + path[::-1])
        ll.append(score)
    return dict(n=len(ll), hole_at=0, paths=np.array(paths, dtype=np.uint8).reshape(len(ll), n + 1), ll_chain=np.array(ll))


def _ordered(entries):
    """(score, second key, third key, ...) tuples in the definition's total order: score descending by plain > and ==, then the
    second key ascending, then the third.  There is no NaN (offer_zero is refused), -(-inf) = +inf sorts last, and -0.0 == 0.0
    under the key as under ==: the key's order IS the definition's."""
    return sorted(entries, key=lambda t: (-t[0], t[1], t[2]))
