"""gh_viterbi_path_grid timed: wall time around Hansel.viterbi_path_grid (k_vit_cands and the candidate bytes home, k_beam_table,
one k_vitg_step per SNP, k_vitg_end, k_vitg_end2, k_vitg_trace, the result home; the call ends synchronised), median (min) of 7
behind a warm-up, everything included.
First block, beside Hansel.viterbi_path() on the same handle in the same call: C2 (1 000 SNPs) at L = 3 (64 states), C3 (10 000
SNPs) at L = 5 (1 024) and L = 6 (4 096, the LDS decoder's cap).  Second block, the grid decoder alone, beyond that cap: C3 at
L = 7 and 8, the 60-SNP test table without deletion columns (tests/decode_util.py: "a4") at L = 7..10 and with them ("a") at
L = 10, the fill's own L.  us per step = median / N; bytes per step = 17 per state (a score written and read, a back-pointer
written) over the states.
argv: [file to append the lines to]"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from gretel_amd.hansel import Hansel  # noqa: E402
from gretel_amd.synth import make_config, make_support_table, sprinkle_deletions  # noqa: E402

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


def table(name):
    if name in ("C2", "C3"):
        return make_config(name, seed=0)
    t = make_support_table(60, 800, k=None, seed=5)           # tests/decode_util.py: _table("a4"), _table("a")
    if name == "a":
        sprinkle_deletions(t, 0.05, seed=6)
    return t


def grid_line(tag, h, n):
    med, mn = timed(h.viterbi_path_grid)
    res = h.viterbi_path_grid()
    s, le, states, scratch = h.viterbi_grid_info()
    say("%s grid    S=%d states=%d scratch=%.1f MB  %10.1f (%10.1f) us  %8.3f us/step  %7.1f GB/s at 17 B a state  ll_chain %.6f" % (
        tag, s, states, scratch / 1e6, med, mn, med / n, 17.0 * states * n / (med * 1e-6) / 1e9, res["ll_chain"]))
    return res


try:
    head = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
except Exception:
    head = "unknown"
say("# git HEAD %s  kernel_source_sha %s  us per call: median (min) of %d behind a warm-up; us per step = median / N" % (
    head, bench.kernel_source_sha(), REPS))
tables = {}
say("# --- beside the LDS decoder, same handle")
for name, L in (("C2", 3), ("C3", 5), ("C3", 6)):
    t = tables.setdefault(name, table(name))
    h = Hansel(t.n_snps, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases)
    h.L = L
    n = t.n_snps
    tag = "%s N=%d L=%d" % (name, n, L)
    med, mn = timed(h.viterbi_path)
    lds = h.viterbi_path()
    s, le, states, scratch = h.viterbi_info()
    say("%s viterbi S=%d states=%d scratch=%.1f MB  %10.1f (%10.1f) us  %8.3f us/step  ll_chain %.6f" % (
        tag, s, states, scratch / 1e6, med, mn, med / n, lds["ll_chain"]))
    res = grid_line(tag, h, n)
    say("%s same path %s same score %s" % (tag, bool(np.array_equal(res["path"], lds["path"])), res["ll_chain"] == lds["ll_chain"]))
say("# --- the grid decoder alone, beyond 4 096 states")
for name, L in (("C3", 7), ("C3", 8), ("a4", 7), ("a4", 8), ("a4", 9), ("a4", 10), ("a", 10)):
    t = tables.setdefault(name, table(name))
    h = Hansel(t.n_snps, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases)
    h.L = L
    n = t.n_snps
    tag = "%s N=%d L=%d" % (name, n, L)
    res = grid_line(tag, h, n)
    sc = h.score_paths([res["path"]])
    beam = h.beam_paths(32)["ll_chain"][0]
    greedy = h.score_paths([h.generate_path()[0]])["ll_chain"][0]
    say("%s score_paths agrees %s  exact - beam32 %.6f  exact - greedy %.6f" % (
        tag, sc["ll_chain"][0] == res["ll_chain"], res["ll_chain"] - beam, res["ll_chain"] - greedy))
