"""K-best decoding over a panel, timed: HanselPanel.viterbi_kbest (gh_panel_viterbi_kbest: every window's walk in one launch,
every trace in another) against a loop of Hansel.viterbi_kbest over the SAME handles -- the only way before it, the figure to
beat.  Shapes: 1, 16, 64 and 256 equal windows of (a) C2 (1 000 SNPs) at L = 3, K = 8: 512 slots; (b) C2 at L = 5, K = 4: 4 096
slots; (c) C2 folded onto two alleles (G -> A, T -> C) at L = 7, K = 32: 4 096 slots.  Every window of a shape is a copy of one
filled handle (the windows are equal on purpose: the condition is stated for equal windows).  Neither way touches a tensor, so the
handles are made once; the two ways alternate in one process -- panel, loop, panel, loop ... -- behind a warm-up pair that has
every scratch block reserved; median (min) of REPS, ms per call (results home in per-window arrays on both sides).  In a separate
pass (gh_debug_panel_viterbi_phases: the device is waited for after every phase) the split of the panel call.  A row whose
scratch the card cannot give ends the shape there and says so.  Reads nothing outside the repository.
argv: [file to append the lines to] [shape: a | b | c | all] [comma-separated window counts]"""
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

REPS = 7
out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
which = sys.argv[2] if len(sys.argv) > 2 else "all"
counts = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 16, 64, 256]


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


try:
    head = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
except Exception:
    head = "unknown"
say("# git HEAD %s + this change  kernel_source_sha %s  ms per call: median (min) of %d behind a warm-up pair" % (
    head, bench.kernel_source_sha(), REPS))
lib = _lib.load()
t4 = make_config("C2", seed=0)
t2 = make_config("C2", seed=0)
fold = np.arange(256, dtype=np.uint8)
fold[ord("G")], fold[ord("T")] = ord("A"), ord("C")
t2.bases = fold[t2.bases]
for tag, name, t, L, K in (("a", "C2", t4, 3, 8), ("b", "C2", t4, 5, 4), ("c", "C2 two alleles", t2, 7, 32)):
    if which not in ("all", tag):
        continue
    src = Hansel(t.n_snps, band=t.band)
    src.fill_from_support(t.rank, t.off, t.bases)
    src.L = L
    s, le, states = src.viterbi_states()
    hs = []
    for W in counts:
        while len(hs) < W:
            h = src.copy()
            h.L = L
            hs.append(h)
        for h in hs:
            h.sync()
        p = HanselPanel(hs)
        tp, tl = [], []
        try:
            for rep in range(REPS + 1):
                t0 = time.perf_counter()
                rp = p.viterbi_kbest(K)
                t1 = time.perf_counter()
                rl = [h.viterbi_kbest(K) for h in hs]
                t2_ = time.perf_counter()
                if rep == 0:                                  # (the warm-up pair; the comparison once)
                    assert all(a["n"] == b["n"] == K and np.array_equal(a["paths"], b["paths"]) and
                               a["ll_chain"].tolist() == b["ll_chain"].tolist() for a, b in zip(rp, rl))
                else:
                    tp.append((t1 - t0) * 1e3)
                    tl.append((t2_ - t1) * 1e3)
                del rp, rl
        except _lib.GretelHipError as e:
            say("%s N=%d L=%d states=%d K=%d windows=%3d  not served: %s" % (name, t.n_snps, L, states, K, W, e))
            break
        info = p.viterbi_kbest_info()
        pm, lm = float(np.median(tp)), float(np.median(tl))
        say("%s N=%d L=%d states=%d K=%d slots=%d windows=%3d walk launches=%d scratch=%.1f MB  panel %9.3f (%9.3f) ms  loop %9.3f (%9.3f) ms  "
            "loop/panel %5.2f  panel %8.1f us per window, loop %8.1f" % (name, t.n_snps, L, states, K, states * K, W, info[2], info[3] / 1e6, pm,
                                                                        min(tp), lm, min(tl), lm / pm, pm * 1e3 / W, lm * 1e3 / W))
        # the split, in a pass of its own
        ph = (C.c_double * 4)()
        lib.gh_debug_panel_viterbi_phases(1, None)
        t0 = time.perf_counter()
        p.viterbi_kbest(K)
        whole = (time.perf_counter() - t0) * 1e3
        lib.gh_debug_panel_viterbi_phases(0, ph)
        say("    split (synchronised phases, ms): preamble + tables %.3f  walks %.3f  traces %.3f  gather + copies home %.3f  "
            "(the call in that pass %.3f, the rest is the host's per-window arrays)" % (tuple(ph) + (whole,)))
        del p
