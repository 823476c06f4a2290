"""Read assignment on the host: the numpy statement of the definition (tests/assign_ref.py) on hand-built cases, the
gretel.support renderer, and the command-line options of gretel_amd.cmd / gretel_amd.panel (defaults, refusals before any
BAM read or GPU call)."""
import os

import numpy as np
import pytest

from assign_ref import assign, path_indices, render, table
from conftest import REFDATA
from gretel_amd import cmd, panel

BAM = os.path.join(REFDATA, "test.bam")
VCF = os.path.join(REFDATA, "test.vcf.gz")


def _run(reads, paths, n, **kw):
    rank, off, bases = table(reads)
    P = np.array([path_indices(p) for p in paths], dtype=np.uint8).reshape(len(paths), n + 1)
    return assign(rank, off, bases, P, n, **kw)


def test_unique_ambiguous_uninformative():
    paths = ["_ACGT", "_ACGA", "_TTTT"]
    reads = [(0, "ACGT"),       # hap 0, 4 of 4
             (0, "ACG"),        # 0 and 1 tie at 3: ambiguous
             (2, "GA"),         # hap 1 (SNPs 3, 4)
             (1, "T"),          # one column: uninformative
             (0, "TTTA"),       # hap 2 with 3 of 4 (1 mismatch)
             (3, "C")]          # one column: uninformative
    r = _run(reads, paths, 4)
    assert r["hap"].tolist() == [0, -2, 1, -1, 2, -1]
    assert r["best"].tolist() == [4, 3, 2, 1, 3, 0]
    assert r["informative"].tolist() == [4, 3, 2, 1, 4, 1]
    assert r["unique"].tolist() == [1, 1, 1]
    assert r["shared"].tolist() == [1, 1, 0]
    assert r["mismatches"].tolist() == [0, 0, 1]
    assert (r["n_reads"], r["n_informative"], r["n_unique"], r["n_ambiguous"], r["n_unexplained"]) == (6, 4, 3, 1, 0)


def test_unsymbols_deletions_and_columns_past_n():
    paths = ["_A-CG", "_AACG"]
    # N and _ are skipped; '-' is informative and matches a '-' in the path; columns past SNP 4 are skipped
    reads = [(0, "N-_G"),       # informative: '-' at 2, G at 4 -> hap 0 (2 of 2)
             (0, "A-"),         # hap 0
             (2, "CGTTTT"),     # SNPs 3, 4 and four columns past N: 2 informative, 0 and 1 tie
             (3, "GA"),         # SNP 4 and one past N: 1 informative: uninformative
             (4, "AC"),         # everything past N
             (0, "NN_N")]
    r = _run(reads, paths, 4)
    assert r["informative"].tolist() == [2, 2, 2, 1, 0, 0]
    assert r["hap"].tolist() == [0, 0, -2, -1, -1, -1]
    assert r["unique"].tolist() == [2, 0] and r["shared"].tolist() == [1, 1] and r["mismatches"].tolist() == [0, 0]
    # the path's own N / _ never match anything
    r = _run([(0, "AN")], ["_NN"], 2, min_snps=1)
    assert r["informative"].tolist() == [1] and r["best"].tolist() == [0] and r["hap"].tolist() == [0]


def test_min_snps_and_max_mismatch():
    paths = ["_AAAA", "_CCCC"]
    reads = [(0, "AAAC"), (0, "ACGT"), (0, "A"), (1, "GG")]
    r = _run(reads, paths, 4, min_snps=1)
    assert r["hap"].tolist() == [0, -2, 0, -2]
    assert r["mismatches"].tolist() == [1 + 0, 0]
    r = _run(reads, paths, 4, min_snps=3)
    assert r["hap"].tolist() == [0, -2, -1, -1] and r["n_informative"] == 2
    r = _run(reads, paths, 4, min_snps=1, max_mismatch=0)
    assert r["hap"].tolist() == [-3, -3, 0, -3] and r["n_unexplained"] == 3
    r = _run(reads, paths, 4, min_snps=1, max_mismatch=2)
    assert r["hap"].tolist() == [0, -3, 0, -2]          # ACGT: 1 of 4 at best, 3 mismatches; GG: none of 2, a tie at 0
    # the order: uninformative before unexplained before ambiguous
    r = _run([(0, "G")], paths, 4, min_snps=2, max_mismatch=0)
    assert r["hap"].tolist() == [-1]


def test_no_haplotypes():
    reads = [(0, "AC"), (0, "A"), (1, "NN")]
    r = _run(reads, [], 3)
    assert r["hap"].tolist() == [-3, -1, -1] and r["best"].tolist() == [0, 0, 0]
    assert len(r["unique"]) == len(r["shared"]) == len(r["mismatches"]) == 0
    assert (r["n_informative"], r["n_unique"], r["n_ambiguous"], r["n_unexplained"]) == (1, 0, 0, 1)


def test_tie_between_haplotype_0_and_64():
    n = 6
    paths = ["_" + "T" * n] * 130
    paths[0] = "_ACGTAC"
    paths[64] = "_ACGTAC"
    paths[100] = "_ACGTAA"
    reads = [(0, "ACGTAC"), (0, "ACGTAA"), (3, "TA")]        # 0 and 64 tie; 100 alone; 0, 64 and 100 tie
    r = _run(reads, paths, n)
    assert r["hap"].tolist() == [-2, 100, -2]
    assert r["shared"][0] == 2 and r["shared"][64] == 2 and r["shared"][100] == 1 and r["shared"].sum() == 5
    assert r["unique"][100] == 1 and r["unique"].sum() == 1


def test_bad_symbol_is_refused():
    with pytest.raises(ValueError):
        _run([(0, "AX")], ["_AA"], 2)


def test_chunking_does_not_change_the_result():
    from gretel_amd.synth import make_support_table
    t = make_support_table(300, 4000, k=None, seed=3)
    rng = np.random.default_rng(1)
    P = np.concatenate([np.full((7, 1), 6), rng.choice([0, 1, 2, 3, 5], size=(7, 300))], axis=1).astype(np.uint8)
    a = assign(t.rank, t.off, t.bases, P, 300)
    b = assign(t.rank, t.off, t.bases, P, 300, col_budget=500)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_support_renderer():
    res = dict(n_reads=10, n_informative=8, n_unique=5, n_ambiguous=2, n_unexplained=1,
               unique=np.array([3, 2, 0]), shared=np.array([2, 1, 1]), mismatches=np.array([4, 0, 0]))
    want = "# 10\t8\t5\t2\t1\n0\t3\t2\t4\t0.6000\n3\t2\t1\t0\t0.4000\n7\t0\t1\t0\t0.0000\n"
    assert cmd.support_text([0, 3, 7], res) == want == render([0, 3, 7], res)
    res.update(n_unique=0, unique=np.zeros(3, dtype=np.int64))
    assert cmd.support_text([0, 3, 7], res).splitlines()[1] == "0\t0\t2\t4\t0.0000"
    empty = dict(res, unique=[], shared=[], mismatches=[])
    assert cmd.support_text([], empty) == "# 10\t8\t0\t2\t1\n"


def test_parser_defaults():
    a = cmd.build_parser().parse_args(["b", "v", "c"])
    assert (a.assign_reads, a.min_snps, a.max_mismatch) == (False, 2, -1)
    # every existing option keeps its default
    assert (a.start, a.end, a.paths, a.master, a.gapchar, a.delchar, a.quiet, a.out, a.threads, a.debugreads, a.debugpos,
            a.max_depth, a.debughpos, a.dumpmatrix, a.dumpsnps, a.pepper) == \
        (1, -1, 100, None, "N", "", False, ".", 1, "", "", 8000, ",", None, None, False)
    a = cmd.build_parser().parse_args(["b", "v", "c", "--assign-reads", "--min-snps", "3", "--max-mismatch", "1", "--max-depth", "5"])
    assert (a.assign_reads, a.min_snps, a.max_mismatch, a.max_depth) == (True, 3, 1, 5)
    p = panel.build_parser().parse_args(["b", "v", "r.bed"])
    assert (p.assign_reads, p.min_snps, p.max_mismatch) == (False, 2, -1)
    assert (p.out, p.paths, p.master, p.gapchar, p.delchar, p.max_depth, p.pepper) == (".", 100, None, "N", "", 8000, False)


@pytest.mark.parametrize("opts, what", [(["--min-snps", "0"], "--min-snps"), (["--max-mismatch", "-2"], "--max-mismatch")])
def test_bad_options_are_refused_first(tmp_path, capsys, opts, what):
    # (refused before the BAM or the GPU is touched: the files need not exist)
    assert cmd.main(["nope.bam", "nope.vcf", "c", "--assign-reads", "-o", str(tmp_path)] + opts) == 2
    assert what in capsys.readouterr().err
    bed = tmp_path / "r.bed"
    bed.write_text("hoot\t0\t20\n")
    assert panel.main([BAM, VCF, str(bed), "--assign-reads", "-o", str(tmp_path)] + opts) == 2
    assert what in capsys.readouterr().err
    assert not (tmp_path / "hoot:1-20").exists()
