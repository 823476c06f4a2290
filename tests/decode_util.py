"""What tests/test_gpu_beam.py, tests/test_gpu_viterbi.py and tests/test_gpu_decode_scratch.py share: the tables, a handle and
an oracle built from whole haplotypes, the comparison of a decoder's spin, the oracle of the CLI tests.  Not a test file."""
import functools
import os
import types

from conftest import REFDATA
from gretel_amd import util
from gretel_amd.hansel import Hansel
from gretel_amd.synth import make_config, make_support_table, sprinkle_deletions
from oracle.c_oracle import COracle
from spec_util import same

BAM = os.path.join(REFDATA, "test.bam")
VCF = os.path.join(REFDATA, "test.vcf.gz")
SYMS = "ACGTN-_"
E_MT = dict(cond_mode="E", marginal_term=True)


@functools.lru_cache(maxsize=None)
def _table(which):
    if which == "a":                                         # 60 SNPs, deletion columns: S = 5
        t = make_support_table(60, 800, k=None, seed=5)
        sprinkle_deletions(t, 0.05, seed=6)
    elif which == "a4":                                      # the same reads without the deletions: S = 4
        t = make_support_table(60, 800, k=None, seed=5)
    elif which == "b":                                       # the 300-SNP table of tests/test_gpu_score.py
        t = make_support_table(300, 6000, k=None, seed=31)
        sprinkle_deletions(t, 0.05, seed=32)
    else:
        t = make_config("C2", seed=6)
    return t


def _from_haps(haps, band, L, skip=(), **kw):
    """A device Hansel and the C oracle built cell by cell from whole haplotypes: every pair (i, i + d), d <= band, of
    '_' + hap + '_' except the cells (i, i + 1) with i in `skip` -- position i then has no candidate."""
    n = len(haps[0])
    h = Hansel(n, band=band, **kw)
    o = COracle(n, band, **kw)
    for hap in haps:
        full = "_" + hap + "_"
        for i in range(n + 1):
            for d in range(1, band + 1):
                if i + d <= n + 1 and not (d == 1 and i in skip):
                    h.add_observation(full[i], full[i + d], i, i + d)
                    o.add(SYMS.index(full[i]), SYMS.index(full[i + d]), i, i + d)
    h.L = o.L = L
    return h, o


def _same_spin(res, ref):
    same(res, ref)
    assert res["ll_chain"].tolist() == ref["ll_chain"].tolist()
    assert res["min_marginal"].tolist() == ref["min_marginal"].tolist()


def _cli_oracle():
    """What `BAM VCF hoot -s 1 -e 20` loads: (the VCF's dict, N, the handle filled from the BAM, the C oracle filled alike)."""
    v = util.process_vcf(VCF, "hoot", 1, 20)
    n = v["N"]
    h = util.load_from_bam(BAM, "hoot", 1, 20, v)
    rank, off, bases = util.support_table_from_bam(BAM, "hoot", 1, 20, v)
    o = COracle(n, h.band)
    o.fill(types.SimpleNamespace(rank=rank, off=off, bases=bases))
    o.L = h.L
    return v, n, h, o
