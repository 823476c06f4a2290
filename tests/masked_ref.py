"""The definition of constrained exact decoding (include/gretel_hip.h: gh_viterbi_path_masked; INTEGRATION.md "Constrained
decoding") in plain Python: the candidate set of a position does not depend on the history, so a constraint set acts on the
candidate mask alone -- viterbi_ref.viterbi over an oracle whose edge_weights ANDs allow[p] into the mask IS the definition.

Not a test file: tests/test_masked_host.py pins it against an exhaustive enumeration, tests/test_gpu_masked.py holds the GPU to it."""
import numpy as np

import viterbi_ref

VALID = (0, 1, 2, 3, 5)        # A C G T - among "ACGTN-_"


class Masked:
    """`o` under the constraint set `allow` (uint8[N+1]): edge_weights offers cm(p) & allow[p], everything else is o's."""

    def __init__(self, o, allow):
        self._o = o
        self._allow = np.asarray(allow, dtype=np.uint8)

    def edge_weights(self, p, path):
        mask, w = self._o.edge_weights(p, path)
        return int(mask) & int(self._allow[p]), w

    def __getattr__(self, name):
        return getattr(self._o, name)


def viterbi_masked(o, n, allow, order="ACGT-"):
    """viterbi_ref.viterbi's dict for one constraint set: path and ll_chain None at a hole, hole_at the first p with empty cm'(p)."""
    return viterbi_ref.viterbi(Masked(o, allow), n, order)


def decode_sets(o, n, allow, order="ACGT-"):
    """Hansel.viterbi_path_masked's dict for the rows of `allow`: at a hole the row is all 6 and ll_chain NaN."""
    allow = np.asarray(allow, dtype=np.uint8).reshape(-1, n + 1)
    paths = np.full((len(allow), n + 1), 6, dtype=np.uint8)
    ll = np.full(len(allow), np.nan)
    hole = np.zeros(len(allow), dtype=np.int32)
    for q, row in enumerate(allow):
        res = viterbi_masked(o, n, row, order)
        hole[q] = res["hole_at"]
        if not res["hole_at"]:
            paths[q], ll[q] = res["path"], res["ll_chain"]
    return dict(paths=paths, ll_chain=ll, hole_at=hole)


def same_sets(got, ref):
    """Everything exact: holes, scores (NaN where there is a hole on both sides), rows."""
    assert got["hole_at"].tolist() == ref["hole_at"].tolist(), ("hole_at", got["hole_at"].tolist(), ref["hole_at"].tolist())
    assert got["paths"].dtype == np.uint8 and got["paths"].shape == ref["paths"].shape
    assert np.array_equal(got["ll_chain"], ref["ll_chain"], equal_nan=True), ("ll_chain", got["ll_chain"].tolist(), ref["ll_chain"].tolist())
    assert np.array_equal(got["paths"], ref["paths"]), ("paths", np.argwhere(got["paths"] != ref["paths"])[:4].tolist())


def masks(seed, cm, n, sets=4):
    """uint8[sets][n+1], a pure function of (seed, cm): per set and position, with probability 0.6 everything is allowed, with 0.25
    one offered candidate is pinned, with 0.15 one offered candidate is banned -- but only where at least two are offered.  So a
    generated set is infeasible only where the window itself has a hole.  cm: the candidate bits per position (index 0 unused)."""
    rng = np.random.default_rng([int(seed), 19])
    allow = np.full((sets, n + 1), 0x7F, dtype=np.uint8)
    for q in range(sets):
        for p in range(1, n + 1):
            offered = [s for s in VALID if (int(cm[p]) >> s) & 1]
            u = rng.random()
            pick = int(rng.integers(0, max(1, len(offered))))
            if u < 0.6 or not offered:
                continue
            if u < 0.85:
                allow[q, p] = 1 << offered[pick]
            elif len(offered) >= 2:
                allow[q, p] = 0x7F & ~(1 << offered[pick])
    return allow
