"""The definition of the beam search over the chain likelihood (include/gretel_hip.h: gh_beam_paths, gh_beam_spin;
INTEGRATION.md "Beam search") in plain Python, over any object `o` that offers

    o.edge_weights(p, path) -> (candidate mask over the seven symbols, the seven weights)      oracle.c_oracle.COracle has it
    o.marginal(s, p)        -> the current marginal of symbol s at p
    o.reweight_path(path, ratio) -> the removed mass
    o.L

Not a test file: tests/test_beam_host.py pins it against the C oracle's greedy walk and an exhaustive ranking,
tests/test_gpu_beam.py holds the GPU to it.  Every score is a Python float sum in ascending p from 0.0, the ranking is `sorted`
on the key the definition gives."""
import numpy as np

import score_ref

SYMS = "ACGTN-_"


def beam(o, n, width, cand_order="ACGT-"):
    """dict(n, hole_at, paths uint8[n][N+1] in rank order, ll_chain list[n]); at a hole n = 0 and `prefix` = what the rank-0
    hypothesis had walked (hole_at symbols, '_' first)."""
    order = [SYMS.index(c) for c in cand_order]
    hyps = [(0.0, [6])]                                     # (score, prefix) in rank order
    for p in range(1, n + 1):
        children = []
        for k, (score, x) in enumerate(hyps):
            hist = np.array(x + [6] * (n + 1 - len(x)), dtype=np.uint8)
            mask, w = o.edge_weights(p, hist)
            for q, c in enumerate(order):
                if (mask >> c) & 1:
                    wc = float(w[c])
                    # score descending, parent rank ascending, w descending, index in cand_order ascending
                    children.append(((-(score + wc), k, -wc, q), score + wc, x + [c]))
        if not children:
            return dict(n=0, hole_at=p, paths=np.zeros((0, n + 1), dtype=np.uint8), ll_chain=[],
                        prefix=np.array(hyps[0][1], dtype=np.uint8))
        children.sort(key=lambda ch: ch[0])
        hyps = [(s, x) for _, s, x in children[:width]]
    return dict(n=len(hyps), hole_at=0, paths=np.array([x for _, x in hyps], dtype=np.uint8).reshape(len(hyps), n + 1),
                ll_chain=[s for s, _ in hyps])


def beam_spin(o, n, width, max_paths, min_remove=0.01, cand_order="ACGT-", original=None):
    """gretel/cmd.py:148-179 with the beam's rank-0 path in place of generate_path: Hansel.beam_spin's dict as arrays.
    original: the marginals the handle's snapshot froze (score_ref.marginals at that moment); None = no snapshot yet, it is
    taken here, as gh_beam_spin takes it."""
    def decode():
        res = beam(o, n, width, cand_order)
        return (res["hole_at"], None, None) if res["hole_at"] else (0, res["paths"][0], res["ll_chain"][0])

    return score_ref.recover_spin(o, n, max_paths, min_remove, original, decode)
