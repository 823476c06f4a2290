"""gh_viterbi_path timed: wall time around Hansel.viterbi_path (k_vit_union + k_beam_table + k_vit_walk + k_vit_trace, the
result home; the call ends synchronised), median (min) of 7 behind a warm-up, on C2 (1 000 SNPs, L = 3: 64 states), C3 (10 000
SNPs; L = 5: 1 024 states, L = 6: 4 096, the cap) and C3 with deletions at 1 % of the positions (S = 5, L = 5: 3 125 states).
Beside each, on the same handle in the same call: Hansel.generate_path(), beam_paths(1) and beam_paths(32) -- the scale, the
feature has no parent figure -- and whether the three scores differ.  GH_VIT_STAGE=0 in the environment reads the table blocks
from global memory instead of the LDS ring: run once with and once without to compare the two.
argv: [file to append the lines to]"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from gretel_amd.hansel import Hansel  # noqa: E402
from gretel_amd.synth import make_config, sprinkle_deletions  # noqa: E402

REPS = 7
out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed(f):
    f()                                                       # warm-up (scratch buffers, code objects)
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6, float(np.min(ts)) * 1e6


try:
    head = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
except Exception:
    head = "unknown"
say("# git HEAD %s  kernel_source_sha %s  GH_VIT_STAGE=%s  us per call: median (min) of %d; us per step = median / N" % (
    head, bench.kernel_source_sha(), os.environ.get("GH_VIT_STAGE", "unset"), REPS))
tables = {}
for name, dels, L in (("C2", False, 3), ("C3", False, 5), ("C3", False, 6), ("C3", True, 5)):
    if (name, dels) not in tables:
        t = make_config(name, seed=0)
        if dels:
            sprinkle_deletions(t, 0.01, seed=1)
        tables[name, dels] = t
    t = tables[name, dels]
    h = Hansel(t.n_snps, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases)
    h.L = L
    n = t.n_snps
    tag = "%s%s N=%d L=%d" % (name, "+del" if dels else "", n, L)
    med, mn = timed(h.generate_path)
    say("%s generate_path  %10.1f (%10.1f) us  %7.3f us/step" % (tag, med, mn, med / n))
    lls = {}
    for w in (1, 32):
        med, mn = timed(lambda: h.beam_paths(w))
        lls[w] = float(h.beam_paths(w)["ll_chain"][0])
        say("%s beam width %2d  %10.1f (%10.1f) us  %7.3f us/step  ll_chain %.6f" % (tag, w, med, mn, med / n, lls[w]))
    med, mn = timed(h.viterbi_path)
    ll = h.viterbi_path()["ll_chain"]
    s, le, states, scratch = h.viterbi_info()
    say("%s viterbi S=%d states=%d scratch=%.1f MB  %10.1f (%10.1f) us  %7.3f us/step  ll_chain %.6f  (exact - beam32 %.6f, exact - greedy %.6f)" % (
        tag, s, states, scratch / 1e6, med, mn, med / n, ll, ll - lls[32], ll - lls[1]))
