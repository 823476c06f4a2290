"""gh_score_paths at C3 (10 000 SNPs, 100 paths) and C5 (50 000 SNPs, 1 000 paths): wall time of Hansel.score_paths (paths upload,
k_score_pos + k_score_sum per slab, records home; per_position=1 also copies weight, margin and pick home), and for comparison one
100-path spin of a copy of the same handle (the recovery the scoring follows).  Then, on a 1 000-SNP window (C2), one path scored
against N calls of get_edge_weights_at, the only way to the per-position weights before.  The paths are the generator's haplotypes
and random rows over A C G T -.  argv: [reps] [noew: leave the get_edge_weights_at loop out]"""
import sys
import time

import numpy as np

from gretel_amd.hansel import Hansel
from gretel_amd.synth import make_config

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
SYMS = "ACGTN-_"


def paths_for(t, H, seed=1):
    rng = np.random.default_rng(seed)
    p = rng.choice(np.array([0, 1, 2, 3, 5], dtype=np.uint8), size=(H, t.n_snps + 1))
    p[:, 0] = 6
    lut = np.zeros(256, dtype=np.uint8)
    for q, c in enumerate(SYMS.encode()):
        lut[c] = q
    k = min(H, len(t.haplotypes))
    p[:k, 1:] = lut[t.haplotypes[:k]]
    return p


def timed(f, n):
    f()                                                       # warm-up (scratch buffers, code objects)
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    return np.median(ts), ts.min(), r


for name, H in (("C3", 100), ("C5", 1000)):
    t = make_config(name, seed=0)
    h = Hansel(t.n_snps, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases)
    h.snapshot_original()
    paths = paths_for(t, H)
    for per_position in (False, True):
        med, mn, r = timed(lambda: h.score_paths(paths, per_position=per_position), reps if not per_position else max(2, reps // 3))
        print("%s N=%d L=%d paths=%d per_position=%d  median %.3f ms  min %.3f ms  (on %.1f %%, greedy %.1f %% of on)"
              % (name, t.n_snps, h.L, H, per_position, med, mn, 100.0 * r["n_on"].sum() / (H * t.n_snps),
                 100.0 * r["n_greedy"].sum() / max(1, r["n_on"].sum())), flush=True)
    ts = []
    for _ in range(3):
        c = h.copy()
        c.snapshot_original()
        c.sync()
        t0 = time.perf_counter()
        res = c.spin(100)
        ts.append((time.perf_counter() - t0) * 1e3)
    print("%s one 100-path spin of a copy: %s ms (%d paths)" % (name, " ".join("%.3f" % x for x in ts), res["n"]), flush=True)

if "noew" not in sys.argv:
    t = make_config("C2", seed=0)
    h = Hansel(t.n_snps, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases)
    one = paths_for(t, 1)
    med, mn, r = timed(lambda: h.score_paths(one, per_position=True), reps)

    def old_way():
        return [h.get_edge_weights_at(p, one[0]) for p in range(1, t.n_snps + 1)]

    med2, mn2, ew = timed(old_way, 3)
    assert all(ew[p - 1][h.symbols[int(one[0, p])]] == r["weight"][0, p] for p in range(1, t.n_snps + 1) if r["weight"][0, p] > -np.inf)
    print("C2 N=%d one path: score_paths median %.3f ms  min %.3f ms;  %d calls of get_edge_weights_at median %.1f ms  min %.1f ms  (x%.0f)"
          % (t.n_snps, med, mn, t.n_snps, med2, mn2, med2 / med), flush=True)
