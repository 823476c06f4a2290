"""gh_beam_paths timed: wall time around Hansel.beam_paths (k_beam_table + k_beam_walk + k_beam_trace, the results home; the
call ends synchronised), median of 7 behind a warm-up, at the C3 shape (10 000 SNPs, L = 5) and C2 (1 000 SNPs, L = 3) for widths
1, 4, 16 and 32, and on one L = 20 window (C3's table, widths 1 and 8), whose table slice does not go through LDS.  Beside each,
Hansel.generate_path() on the same handle, for scale.  GH_BEAM_STAGE=0 in the environment sends every L through the global
loader: run once with and once without to compare the two loaders at the same L.
argv: [file to append the lines to]"""
import os
import subprocess
import sys
import time

import numpy as np

from gretel_amd.hansel import Hansel
from gretel_amd.synth import make_config

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
say("# git HEAD %s  GH_BEAM_STAGE=%s  us per call: median (min) of %d; us per step = median / N" % (
    head, os.environ.get("GH_BEAM_STAGE", "unset"), REPS))
tables = {}
for name, L, widths in (("C2", 3, (1, 4, 16, 32)), ("C3", 5, (1, 4, 16, 32)), ("C3", 20, (1, 8))):
    if name not in tables:
        tables[name] = make_config(name, seed=0)
    t = tables[name]
    h = Hansel(t.n_snps, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases)
    h.L = L
    n = t.n_snps
    med, mn = timed(h.generate_path)
    say("%s N=%d L=%d generate_path            %10.1f (%10.1f) us" % (name, n, L, med, mn))
    for w in widths:
        med, mn = timed(lambda: h.beam_paths(w))
        staged, ring, threads, scratch = h.beam_info()
        say("%s N=%d L=%d beam width %2d staged=%d ring=%d threads=%d scratch=%.1f MB  %10.1f (%10.1f) us  %7.3f us/step" % (
            name, n, L, w, staged, ring, threads, scratch / 1e6, med, mn, med / n))
