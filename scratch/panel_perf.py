"""Throughput of a panel (HanselPanel: windows of differing N, band and L) against the same windows spun one by one (Hansel.spin) and
against a uniform batch (HanselBatch) of as many windows with the same total of SNPs.  argv: [windows] [paths] [reps]
Windows: N drawn from 40..2 000, L from 3..8, reads of 4..8 SNPs (synth.make_support_table).  Prints one line per way and rep:
haplotypes/s and SNP-steps/s (paths x N summed over the windows, per second of spin); the last rep of each way is the figure."""
import sys
import time

import numpy as np
import torch

from gretel_amd.hansel import DeviceReads, Hansel, HanselBatch, HanselPanel
from gretel_amd.synth import make_support_table

nw = int(sys.argv[1]) if len(sys.argv) > 1 else 256
paths = int(sys.argv[2]) if len(sys.argv) > 2 else 100
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
rng = np.random.default_rng(2026)
Ns = rng.integers(40, 2001, nw)
Ls = rng.integers(3, 9, nw)
ks = rng.integers(4, 9, nw)


def windows(shapes):
    hs, rs = [], []
    for q, (n, L, k) in enumerate(shapes):
        t = make_support_table(int(n), 20 * int(n), k=int(k), seed=10 + q)
        h = Hansel(t.n_snps, band=t.band)
        rs.append((DeviceReads(h, t.rank, t.off, t.bases), int(L)))
        hs.append(h)
    return hs, rs


def refill(hs, rs):
    for h, (r, L) in zip(hs, rs):
        h.clear()
        h.fill_from_support(None, None, None, reads_handle=r)
        h.L = L
    torch.cuda.synchronize()


def report(way, rep, res, dt, info=""):
    n = sum(int(x["n"]) for x in res)
    steps = sum(int(x["n"]) * (x["paths"].shape[1] - 1) for x in res)
    print("%-22s rep %d: %6d haplotypes in %8.1f ms  %9.0f haplotypes/s  %11.0f SNP-steps/s %s" % (way, rep, n, dt * 1e3, n / dt, steps / dt, info),
          flush=True)


hs, rs = windows(zip(Ns, Ls, ks))
print("panel: %d windows, N %d..%d (%d SNPs in all), L %s, %d paths each" % (nw, Ns.min(), Ns.max(), Ns.sum(),
      {int(a): int(b) for a, b in zip(*np.unique(Ls, return_counts=True))}, paths), flush=True)
panel = HanselPanel(hs)
for rep in range(reps):
    refill(hs, rs)
    t0 = time.perf_counter()
    res = panel.spin(paths, copy=False)
    dt = time.perf_counter() - t0
    report("HanselPanel", rep, res, dt, str(panel.pipe_info()))
for rep in range(reps):
    refill(hs, rs)
    t0 = time.perf_counter()
    res = [h.spin(paths) for h in hs]
    dt = time.perf_counter() - t0
    report("Hansel.spin one by one", rep, res, dt)
del panel
# uniform: as many windows, each of the mean N, at the median L and band
nu = int(round(Ns.sum() / nw))
hs, rs = windows([(nu, int(np.median(Ls)), int(np.median(ks)))] * nw)
batch = HanselBatch(hs)
for rep in range(reps):
    refill(hs, rs)
    t0 = time.perf_counter()
    res = batch.spin(paths, copy=False)
    dt = time.perf_counter() - t0
    report("HanselBatch uniform", rep, res, dt, "N=%d L=%d %s" % (nu, hs[0].L, batch.pipe_info()))
