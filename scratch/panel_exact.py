"""Exact decoding over a panel, timed: HanselPanel.viterbi_spin (gh_panel_viterbi_spin: the decoders of a round side by side)
against the same windows through a loop of Hansel.viterbi_spin on twin handles -- the only way before it, the figure to beat.
Shapes: 1, 16, 64 and 256 equal windows of (a) C2 (1 000 SNPs) at L = 3, 64 states, and (b) C3 (10 000 SNPs, no deletion
columns) at L = 5, 1 024 states; 5 paths each.  Every window of a shape is a copy of one filled handle (the windows are equal on
purpose: the condition is stated for equal windows).  A spin reweights its tensor, so every repetition runs on fresh copies; each
copy decodes one path and scores it beforehand (neither touches the tensor), so that no repetition pays for the first allocation
of a scratch block.  The two ways alternate in one call: panel, loop, panel, loop ...; median (min) of REPS behind a warm-up
pair; per round = wall time / rounds run.  In a separate pass (gh_debug_panel_viterbi_phases: the device is waited for after
every phase) the split of the panel's rounds into table builds, union + walk + trace, gather + copies home, records + reweights.
Reads nothing outside the repository.
argv: [file to append the lines to] [shape: C2 | C3 | all] [comma-separated window counts]"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from gretel_amd import _lib  # noqa: E402
from gretel_amd.hansel import Hansel, HanselPanel  # noqa: E402
from gretel_amd.synth import make_config  # noqa: E402

REPS = 3
PATHS = 5
out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
which = sys.argv[2] if len(sys.argv) > 2 else "all"
counts = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 16, 64, 256]


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def fresh(src, n):
    hs = []
    for _ in range(n):
        h = src.copy()
        h.L = src.L
        p = h.viterbi_path()                                  # (the decoder's scratch in full; the tensor is only read)
        h.score_paths([p["path"]])
        hs.append(h)
    for h in hs:
        h.sync()
    return hs


def run_panel(hs):
    p = HanselPanel(hs)
    p._host_buffers(PATHS)                                    # (the page-locked result buffers: not a cost of a round)
    t0 = time.perf_counter()
    res = p.viterbi_spin(PATHS)
    dt = time.perf_counter() - t0
    return dt, res, p.viterbi_info()


def run_loop(hs):
    t0 = time.perf_counter()
    res = [h.viterbi_spin(PATHS) for h in hs]
    return time.perf_counter() - t0, res


try:
    head = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
except Exception:
    head = "unknown"
say("# git HEAD %s + this change  kernel_source_sha %s  %d paths a window; ms per round: median (min) of %d behind a warm-up" % (
    head, bench.kernel_source_sha(), PATHS, REPS))
lib = _lib.load()
for name, L in (("C2", 3), ("C3", 5)):
    if which not in ("all", name):
        continue
    t = make_config(name, seed=0)
    src = Hansel(t.n_snps, band=t.band)
    src.fill_from_support(t.rank, t.off, t.bases)
    src.L = L
    for W in counts:
        tp, tl = [], []
        for rep in range(REPS + 1):
            dt, rp, info = run_panel(fresh(src, W))
            rounds = info[1]
            dl, rl = run_loop(fresh(src, W))
            assert all(np.array_equal(a["paths"], b["paths"]) and a["ll_chain"].tolist() == b["ll_chain"].tolist() for a, b in zip(rp, rl))
            n_paths = sum(r["n"] for r in rp)
            if rep:                                           # (the first pair is the warm-up)
                tp.append(dt / rounds * 1e3)
                tl.append(dl / rounds * 1e3)
        s, le, states = src.viterbi_states()
        pm, lm = float(np.median(tp)), float(np.median(tl))
        say("%s N=%d L=%d states=%d windows=%3d rounds=%d paths=%d  panel %9.3f (%9.3f) ms/round  loop %9.3f (%9.3f) ms/round  loop/panel %5.2f  "
            "panel %8.1f us per window-path, loop %8.1f" % (name, t.n_snps, L, states, W, rounds, n_paths, pm, min(tp), lm, min(tl), lm / pm,
                                                              pm * 1e3 / W, lm * 1e3 / W))
        # the split, in a pass of its own
        hs = fresh(src, W)
        p = HanselPanel(hs)
        p._host_buffers(PATHS)
        ph = (C.c_double * 4)()
        lib.gh_debug_panel_viterbi_phases(1, None)
        p.viterbi_spin(PATHS)
        lib.gh_debug_panel_viterbi_phases(0, ph)
        r = p.viterbi_info()[1]
        say("    split (synchronised phases, ms/round): tables %.3f  union+walk+trace %.3f  gather+copies home %.3f  records+reweights %.3f" % tuple(
            v / r for v in ph))
