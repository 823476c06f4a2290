"""gh_viterbi_kbest timed: wall time around Hansel.viterbi_kbest(K) (k_vit_union + k_beam_table + k_vitk_walk + k_vitk_trace, the
results home; the call ends synchronised) and, on the same handle at the same L in the same loop, around Hansel.viterbi_path() --
that kernel is untouched by k-best decoding, so it is the parent's figure.  The two calls alternate, behind a warm-up of each;
median (min) of REPS; us per step = median / N.  Tables of 64, 1 024 and 4 096 slots (states * K) at K = 1, 4 and 32: C2 (1 000
SNPs, S = 4) at K = 1 (L = 3, 5, 6) and K = 4 (L = 2, 4, 5); C2 folded onto two alleles (G -> A, T -> C: S = 2) at K = 32
(L = 1, 5, 7), where 32 lists a state reach those slot counts at all.  GH_VIT_STAGE=0 in the environment reads the table blocks
from global memory instead of the LDS ring.
argv: [file to append the lines to]"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from gretel_amd.hansel import Hansel  # noqa: E402
from gretel_amd.synth import make_config  # noqa: E402

REPS = 15
out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed_pair(f, g):
    """f and g alternating: (median, min) in us of each."""
    f()                                                       # warm-up (scratch buffers, code objects)
    g()
    tf, tg = [], []
    for _ in range(REPS):
        for fn, ts in ((f, tf), (g, tg)):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    return [(float(np.median(ts)) * 1e6, float(np.min(ts)) * 1e6) for ts in (tf, tg)]


try:
    head = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
except Exception:
    head = "unknown"
say("# git HEAD %s  kernel_source_sha %s  GH_VIT_STAGE=%s  us per call: median (min) of %d, the two calls alternating; us per step = median / N" % (
    head, bench.kernel_source_sha(), os.environ.get("GH_VIT_STAGE", "unset"), REPS))
t4 = make_config("C2", seed=0)
t2 = make_config("C2", seed=0)
fold = np.arange(256, dtype=np.uint8)
fold[ord("G")], fold[ord("T")] = ord("A"), ord("C")
t2.bases = fold[t2.bases]
for name, t, k, Ls in (("C2", t4, 1, (3, 5, 6)), ("C2", t4, 4, (2, 4, 5)), ("C2 two alleles", t2, 32, (1, 5, 7))):
    h = Hansel(t.n_snps, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases)
    n = t.n_snps
    for L in Ls:
        h.L = L
        (pm, pn), (km, kn) = timed_pair(h.viterbi_path, lambda: h.viterbi_kbest(k))
        best = h.viterbi_path()["ll_chain"]
        res = h.viterbi_kbest(k)
        s, le, states, scratch = h.viterbi_info()
        assert res["n"] == k and res["ll_chain"][0] == best and (np.diff(res["ll_chain"]) <= 0).all()
        say("%s N=%d L=%d S=%d states=%d K=%d slots=%d scratch=%.1f MB  viterbi_path %9.1f (%9.1f) us %6.3f us/step  kbest %9.1f (%9.1f) us %6.3f us/step  "
            "ratio %.2f  ll[0] %.6f ll[K-1] %.6f" % (name, n, L, s, states, k, states * k, scratch / 1e6, pm, pn, pm / n, km, kn, km / n, km / pm,
                                                    res["ll_chain"][0], res["ll_chain"][-1]))
