"""gh_assign_reads at C3 (1M reads of 5 SNPs, 100 haplotypes) and C5 (200k reads of 2..21 SNPs, 1 000 haplotypes): wall time of the
call (paths upload, match masks, k_assign, counters home) and, with per_read, the per-read arrays as well.  The haplotypes are random
rows over A C G T (a spin of 1 000 C5 paths would cost more than the thing measured; the kernel's work does not depend on them beyond
the share of ambiguous reads).  For comparison: one 100-path C3 spin step of bench.py is 3.4 ms.  argv: [reps]"""
import sys
import time

import numpy as np
import torch

from gretel_amd.hansel import Hansel
from gretel_amd.synth import make_config

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
for name, H in (("C3", 100), ("C5", 1000)):
    t = make_config(name, seed=0)
    h = Hansel(t.n_snps, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases, keep_reads=True)
    rng = np.random.default_rng(1)
    paths = rng.integers(0, 4, size=(H, t.n_snps + 1)).astype(np.uint8)
    paths[:, 0] = 6
    # half the haplotypes are the generator's own: realistic unique / ambiguous shares
    truth = np.frombuffer(t.haplotypes.tobytes(), dtype=np.uint8).reshape(t.haplotypes.shape)
    lut = np.zeros(256, dtype=np.uint8)
    for q, c in enumerate(b"ACGT"):
        lut[c] = q
    paths[:len(truth), 1:] = lut[truth]
    for per_read in (False, True):
        h.assign_reads(paths, per_read=per_read)                 # warm-up (scratch buffers, code objects)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = h.assign_reads(paths, per_read=per_read)
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts) * 1e3
        print("%s reads=%d H=%d per_read=%d  median %.3f ms  min %.3f ms  (unique %d ambiguous %d unexplained %d)"
              % (name, t.n_reads, H, per_read, np.median(ts), ts.min(), r["n_unique"], r["n_ambiguous"], r["n_unexplained"]), flush=True)
