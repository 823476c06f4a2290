"""gh_viterbi_marginals_grid timed: wall time around Hansel.viterbi_marginals_grid (k_vit_cands and the candidate bytes home,
k_beam_table, one k_vitg_step<S, KEEP> and one k_vitgm_back per SNP, k_vitgm_mm, mm and cm home; the call ends synchronised),
median (min) of 7 behind a warm-up, everything included.
First block, beside Hansel.viterbi_marginals() and Hansel.viterbi_path_grid() on the same handle in the same call: C2 (1 000
SNPs) at L = 3 (64 states), C3 (10 000 SNPs) at L = 5 (1 024) and L = 6 (4 096, the LDS call's cap).  Second block, beside the
grid decoder alone: the 60-SNP test table without deletion columns (tests/decode_util.py: "a4") and with them ("a") at L = 10,
the fill's own L -- with the identities of tests/test_gpu_viterbi_grid_marg.py's test_the_fills_own_L as figures.  us per step =
median / N; bytes per step = 40 per state (F written and read: 16, B written and read S times over adjacent entries: counted
once each way, 16, and F read again backward: 8).
argv: [file to append the lines to]"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from gretel_amd.hansel import Hansel, margins_of  # noqa: E402
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


def handle(t, L):
    h = Hansel(t.n_snps, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases)
    h.L = L
    return h


def marg_line(tag, h, n):
    med, mn = timed(h.viterbi_marginals_grid)
    res = h.viterbi_marginals_grid()
    s, le, states, scratch = h.viterbi_grid_info()
    say("%s grid marginals S=%d states=%d scratch=%d bytes (%.1f MB)  %10.1f (%10.1f) us = %.3f ms  %8.3f us/step  %7.1f GB/s at 40 B a state" % (
        tag, s, states, scratch, scratch / 1e6, med, mn, med / 1e3, med / n, 40.0 * states * n / (med * 1e-6) / 1e9))
    return res, med


def path_line(tag, h, n):
    med, mn = timed(h.viterbi_path_grid)
    res = h.viterbi_path_grid()
    s, le, states, scratch = h.viterbi_grid_info()
    say("%s grid decoder   S=%d states=%d scratch=%.1f MB  %10.1f (%10.1f) us  %8.3f us/step" % (tag, s, states, scratch / 1e6, med, mn, med / n))
    return res, med


try:
    head = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
except Exception:
    head = "unknown"
say("# git HEAD %s + this change  kernel_source_sha %s  us per call: median (min) of %d behind a warm-up; us per step = median / N" % (
    head, bench.kernel_source_sha(), REPS))
tables = {}
say("# --- beside the LDS max-marginals and the grid decoder, same handle")
for name, L in (("C2", 3), ("C3", 5), ("C3", 6)):
    t = tables.setdefault(name, table(name))
    h = handle(t, L)
    n = t.n_snps
    tag = "%s N=%d L=%d" % (name, n, L)
    med, mn = timed(h.viterbi_marginals)
    lds = h.viterbi_marginals()
    s, le, states, scratch = h.viterbi_info()
    say("%s lds marginals  S=%d states=%d scratch=%.1f MB  %10.1f (%10.1f) us  %8.3f us/step" % (tag, s, states, scratch / 1e6, med, mn, med / n))
    res, gm = marg_line(tag, h, n)
    best, gp = path_line(tag, h, n)
    say("%s same mm %s same cm %s  mm[N].max() == the grid decoder's ll_chain %s  marginals / decoder %.2f" % (
        tag, bool(np.array_equal(res["mm"], lds["mm"])), bool(np.array_equal(res["cm"], lds["cm"])), res["mm"][n].max() == best["ll_chain"], gm / gp))
say("# --- the fill's own L = 10, beside the grid decoder alone")
for name in ("a4", "a"):
    t = tables.setdefault(name, table(name))
    h = handle(t, 10)
    n = t.n_snps
    tag = "%s N=%d L=10" % (name, n)
    res, gm = marg_line(tag, h, n)
    best, gp = path_line(tag, h, n)
    ll, path = best["ll_chain"], best["path"]
    w = h.score_paths([path], per_position=True)["weight"][0, 1:]
    b = n * 2.0 ** -52 * np.abs(w).sum()
    gap = margins_of(res["mm"], res["cm"], path.reshape(1, -1))["gap"][1:]
    through = res["mm"][np.arange(1, n + 1), path[1:]]
    say("%s marginals / decoder %.2f  mm[N].max() == ll %s  smallest gap %r  largest max_c mm[p][c] - ll %r  smallest mm[p][path[p]] - ll %r  b %.3e" % (
        tag, gm / gp, res["mm"][n].max() == ll, float(gap.min()), float((res["mm"][1:].max(axis=1) - ll).max()), float((through - ll).min()), b))
say("# not measured: windows beyond 5^10 states, 300 SNPs at the fill's own L (2.5 and 23 GB), the kernels alone (HIP events), counters")
