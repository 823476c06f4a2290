"""gh_viterbi_marginals timed beside gh_viterbi_path, in one process on the same handles: wall time around
Hansel.viterbi_marginals (k_vit_union + k_beam_table + k_vit_cands + k_vit_walk<KEEP> + k_vit_back + k_vit_mm, mm and cm home;
the call ends synchronised) and around Hansel.viterbi_path, alternating, median (min) of 7 pairs behind a warm-up of each, on C2
(1 000 SNPs, L = 3: 64 states) and C3 (10 000 SNPs; L = 5: 1 024 states, L = 6: 4 096, the cap).  us per step = median / N; the
yardstick is the decoder's own step in this run.  GH_VIT_STAGE=0 in the environment reads the table blocks from global memory.
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

REPS = 7
out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed_pair(f, g):
    f()                                                       # warm-up (scratch buffers, code objects)
    g()
    tf, tg = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        f()
        t1 = time.perf_counter()
        g()
        t2 = time.perf_counter()
        tf.append(t1 - t0)
        tg.append(t2 - t1)
    return [(float(np.median(t)) * 1e6, float(np.min(t)) * 1e6) for t in (tf, tg)]


try:
    head = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
except Exception:
    head = "unknown"
say("# git HEAD %s  kernel_source_sha %s  GH_VIT_STAGE=%s  us per call: median (min) of %d; us per step = median / N" % (
    head, bench.kernel_source_sha(), os.environ.get("GH_VIT_STAGE", "unset"), REPS))
tables = {}
for name, L in (("C2", 3), ("C3", 5), ("C3", 6)):
    if name not in tables:
        tables[name] = make_config(name, seed=0)
    t = tables[name]
    h = Hansel(t.n_snps, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases)
    h.L = L
    n = t.n_snps
    tag = "%s N=%d L=%d" % (name, n, L)
    (pm, pmin), (mmed, mmin) = timed_pair(h.viterbi_path, h.viterbi_marginals)
    ll = h.viterbi_path()["ll_chain"]
    _, _, _, pscratch = h.viterbi_info()
    res = h.viterbi_marginals()
    s, le, states, scratch = h.viterbi_info()
    assert res["mm"][n].max() == ll
    say("%s viterbi_path      S=%d states=%d scratch=%.1f MB  %10.1f (%10.1f) us  %7.3f us/step  ll_chain %.6f" % (
        tag, s, states, pscratch / 1e6, pm, pmin, pm / n, ll))
    say("%s viterbi_marginals S=%d states=%d scratch=%.1f MB  %10.1f (%10.1f) us  %7.3f us/step  %.2f decoder runs  max mm[N] == ll_chain" % (
        tag, s, states, scratch / 1e6, mmed, mmin, mmed / n, mmed / pm))
