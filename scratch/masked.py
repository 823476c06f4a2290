"""Constrained exact decoding, timed: Hansel.viterbi_path_masked (gh_viterbi_path_masked: one chain table, one workgroup per
constraint set in one walk launch and one trace launch) on C2 (1 000 SNPs, four alleles) at L = 3, 5 and 6 -- 64, 1 024 and 4 096
states -- with 1, 16, 64 and 256 sets, and on C3 (10 000 SNPs) with 1 and 16 sets: a second N, so that what a set costs per CALL
and what it costs per STEP beside the unmasked decoder come apart (all rows of one N cannot tell them).  Two yardsticks on the SAME handle: for one set Hansel.viterbi_path (the unmasked decoder:
the same walk without the mask), for many sets a loop of one-set calls over the same masks (the only way without the call).  Set 0
allows everything; every other set pins a tenth of the SNPs to an allele offered there (seeded), so no set meets a hole and every
workgroup walks all N steps.  Nothing touches the tensor, so the handle is made once per L; the ways alternate in one process
behind a warm-up pair that has the scratch block reserved; median (min) of REPS, every call ending synchronised with its results
home.  Whole calls are timed (table build, mask upload, walk, trace, copies), not the walk kernel alone.  A row whose scratch the
card cannot give ends the shape there and says so.  Reads nothing outside the repository.
argv: [file to append the lines to] [comma-separated L] [comma-separated set counts for C2] [the same for C3, 0 = leave C3 out]"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from gretel_amd import _lib  # noqa: E402
from gretel_amd.hansel import Hansel  # noqa: E402
from gretel_amd.synth import make_config  # noqa: E402

REPS = 7
out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
lags = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [3, 5, 6]
counts2 = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 16, 64, 256]
counts3 = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else [1, 16]


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed(fn):
    """median and min of REPS calls of fn behind a warm-up pair, in ms"""
    fn()
    fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts)


try:
    head = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
except Exception:
    head = "unknown"
say("# git HEAD %s  kernel_source_sha %s  GH_VIT_STAGE=%s  ms per call: median (min) of %d behind a warm-up pair" % (
    head, bench.kernel_source_sha(), os.environ.get("GH_VIT_STAGE", "unset"), REPS))
for name, counts in (("C2", counts2), ("C3", counts3)):
    if counts == [0]:
        continue
    t = make_config(name, seed=0)
    n = t.n_snps
    h = Hansel(n, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases)
    for L in lags:
        h.L = L
        s, le, states = h.viterbi_states()
        cm = h.viterbi_marginals()["cm"]
        rng = np.random.default_rng(19)
        allow = np.full((max(counts), n + 1), 0x7F, dtype=np.uint8)
        for q in range(1, len(allow)):
            for p in rng.choice(np.arange(1, n + 1), size=n // 10, replace=False):
                offered = [b for b in (0, 1, 2, 3, 5) if (int(cm[p]) >> b) & 1]
                allow[q, p] = 1 << offered[int(rng.integers(0, len(offered)))]
        vp_med, vp_min = timed(h.viterbi_path)
        say("%s N=%d L=%d S=%d states=%d  viterbi_path %.3f (%.3f) ms = %.2f us per step" % (name, n, L, s, states, vp_med, vp_min, vp_med * 1e3 / n))
        one = None
        for m in counts:
            sets = allow[:m]
            try:
                res = h.viterbi_path_masked(sets)
            except _lib.GretelHipError as e:
                say("  sets=%d: %s -- the shape ends here" % (m, e))
                break
            assert not res["hole_at"].any() and res["ll_chain"][0] == h.viterbi_path()["ll_chain"]
            c_med, c_min = timed(lambda: h.viterbi_path_masked(sets))
            scratch = h.viterbi_masked_info()[3]

            def loop():
                for row in sets:
                    h.viterbi_path_masked(row)

            l_med, l_min = timed(loop)
            if m == counts[0]:
                one = c_med
            say("  sets=%3d  one call %9.3f (%9.3f) ms = %7.2f us per step, %6.2fx the call with %d set(s)   loop of one-set calls %10.3f (%10.3f) ms   "
                "loop / one call %6.2f   one call - viterbi_path %+.3f ms   scratch %.1f MB" % (m, c_med, c_min, c_med * 1e3 / n, c_med / one, counts[0], l_med, l_min, l_med / c_med, c_med - vp_med,
                                                            scratch / 1e6))
