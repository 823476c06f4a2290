"""Read assignment on the GPU (gh_assign_reads, Hansel.assign_reads, --assign-reads of gretel_amd.cmd and gretel_amd.panel)
against the numpy statement of the definition (tests/assign_ref.py): every count, total and per-read array exactly equal."""
import ctypes as C
import os

import numpy as np
import pytest

from assign_ref import assign, path_indices, render
from conftest import REFDATA
from gretel_amd import _lib, bamio, cmd, panel, util
from gretel_amd.hansel import DeviceReads, Hansel
from gretel_amd.synth import make_config, make_support_table, sprinkle_deletions

pytestmark = pytest.mark.gpu
BAM = os.path.join(REFDATA, "test.bam")
VCF = os.path.join(REFDATA, "test.vcf.gz")
KEYS = ("unique", "shared", "mismatches", "n_reads", "n_informative", "n_unique", "n_ambiguous", "n_unexplained", "hap", "best",
        "informative")


def _filled(t):
    h = Hansel(t.n_snps, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases, keep_reads=True)
    return h


def _same(h, t, paths, min_snps=2, max_mismatch=-1, reads=None):
    got = h.assign_reads(paths, reads=reads, min_snps=min_snps, max_mismatch=max_mismatch, per_read=True)
    ref = assign(t.rank, t.off, t.bases, paths, t.n_snps, min_snps=min_snps, max_mismatch=max_mismatch)
    for k in KEYS:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape and np.array_equal(g, r), (k, min_snps, max_mismatch)
    for k in ("unique", "shared", "mismatches"):
        assert got[k].dtype == np.int64
    for k in ("hap", "best", "informative"):
        assert got[k].dtype == np.int32
    return got


def _random_paths(rng, H, n, syms=(0, 1, 2, 3, 4, 5, 6)):
    p = rng.choice(np.array(syms, dtype=np.uint8), size=(H, n + 1))
    p[:, 0] = 6
    return p


def test_c2_table_with_the_paths_of_a_spin():
    t = make_config("C2", seed=4)
    h = _filled(t)
    paths = h.spin(40)["paths"].copy()
    assert len(paths) == 40
    for min_snps in (1, 2, 4):
        for mm in (-1, 0, 2):
            got = _same(h, t, paths, min_snps, mm)
    assert got["n_unique"] + got["n_ambiguous"] + got["n_unexplained"] == got["n_informative"]
    # the generator's reads carry three SNPs: with min_snps = 4 none is informative
    assert h.assign_reads(paths, min_snps=4)["n_informative"] == 0


def test_poisson_k_deletions_and_unsymbols():
    rng = np.random.default_rng(7)
    t = make_support_table(2000, 40000, k=None, seed=8)            # k up to 21 SNPs per read
    assert t.max_k == 21
    sprinkle_deletions(t, 0.05, seed=9)
    b = t.bases.copy()
    b[rng.random(len(b)) < 0.03] = ord("N")
    b[rng.random(len(b)) < 0.01] = ord("_")
    t.bases = b
    h = _filled(t)
    paths = h.spin(30)["paths"].copy()
    assert (paths == 5).any()
    for min_snps, mm in ((1, -1), (2, -1), (4, 2), (2, 0)):
        _same(h, t, paths, min_snps, mm)
    # the paths with N and '_' in them as well
    _same(h, t, np.concatenate([paths, _random_paths(rng, 20, t.n_snps)]))


def test_unsorted_table():
    t = make_support_table(800, 20000, k=None, seed=10)
    perm = np.random.default_rng(1).permutation(t.n_reads)
    rows = [t.bases[t.off[r]:t.off[r + 1]] for r in perm]
    t.rank = np.ascontiguousarray(t.rank[perm])
    t.off = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    t.bases = np.concatenate(rows).astype(np.uint8)
    h = _filled(t)
    assert not h.reads.info()["sorted"]
    paths = h.spin(12)["paths"].copy()
    for min_snps, mm in ((1, -1), (2, 2)):
        _same(h, t, paths, min_snps, mm)


@pytest.mark.parametrize("H", [0, 1, 63, 64, 65, 200, 4500])
def test_haplotype_counts_and_word_boundaries(H):
    # (4500: more haplotypes than the LDS counters take -- the kernel's global-atomic form)
    rng = np.random.default_rng(H)
    t = make_support_table(300, 6000, k=None, seed=H + 1, k_lambda=6.0)
    h = _filled(t)
    truth = np.concatenate([np.full((t.haplotypes.shape[0], 1), 6, dtype=np.uint8),
                            path_indices(t.haplotypes.tobytes().decode())[None, :].reshape(t.haplotypes.shape)], axis=1)
    paths = _random_paths(rng, H, t.n_snps, syms=(0, 1, 2, 3))
    if H >= 2:
        paths[:min(H, len(truth))] = truth[:min(H, len(truth))]
    if H > 64:
        paths[63] = paths[64] = truth[0]            # a tie across the word boundary (and with haplotype 0)
    for min_snps, mm in ((2, -1), (1, 0), (4, 2)):
        got = _same(h, t, paths, min_snps, mm)
    if H > 64:
        full = h.assign_reads(paths, per_read=True)
        assert full["shared"][63] == full["shared"][64] == full["shared"][0] > 0
    if H == 0:
        assert got["n_unexplained"] == got["n_informative"] and got["n_unique"] == got["n_ambiguous"] == 0


def test_full_c3_table_against_100_spin_paths():
    t = make_config("C3", seed=0)
    h = _filled(t)
    paths = h.spin(100)["paths"].copy()
    got = _same(h, t, paths)
    assert got["n_reads"] == 1_000_000 and got["n_informative"] == 1_000_000


def test_true_haplotypes_explain_every_read_without_errors():
    t = make_support_table(500, 20000, k=5, err=0.0, seed=12)
    h = _filled(t)
    truth = np.concatenate([np.full((t.haplotypes.shape[0], 1), 6, dtype=np.uint8),
                            path_indices(t.haplotypes.tobytes().decode()).reshape(t.haplotypes.shape)], axis=1)
    got = _same(h, t, truth)
    inf = got["informative"] >= 2
    assert np.array_equal(got["best"][inf], got["informative"][inf])
    assert got["mismatches"].sum() == 0
    strict = _same(h, t, truth, max_mismatch=0)
    assert strict["n_unexplained"] == 0 and strict["n_unique"] > 0


def test_error_codes():
    t = make_support_table(100, 500, k=4, seed=3)
    h = _filled(t)
    L = _lib.load()
    paths = np.full((2, t.n_snps + 1), 0, dtype=np.uint8)
    u, s, m = (np.zeros(2, dtype=np.int64) for _ in range(3))
    st = _lib.gh_assign_stats()

    def call(p, n, min_snps=2, mm=-1, reads=h.reads):
        return L.gh_assign_reads(h._h, reads._r, p.ctypes.data, n, min_snps, mm, u.ctypes.data, s.ctypes.data, m.ctypes.data,
                                 None, None, None, C.byref(st))

    assert call(paths, 2) == _lib.GH_OK
    assert call(paths, -1) == _lib.GH_ERR_ARG
    assert call(paths, 2, min_snps=0) == _lib.GH_ERR_ARG
    assert call(paths, 2, mm=-2) == _lib.GH_ERR_ARG
    bad = paths.copy()
    bad[1, 7] = 7
    assert call(bad, 2) == _lib.GH_ERR_ARG
    assert b"not a symbol index" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError):
        h.assign_reads(bad)
    # a byte outside ACGTN-_ in a read (a table that was never filled: gh_fill refuses it too)
    b = t.bases.copy()
    b[5] = ord("x")
    with pytest.raises(_lib.SymbolError):
        h.assign_reads(paths, reads=DeviceReads(h, t.rank, t.off, b))
    # reads on another device than the handle (the check gh_fill makes)
    if _lib.device_count() > 1:
        h1 = Hansel(t.n_snps, band=t.band, device=1)
        h1.fill_from_support(t.rank, t.off, t.bases, keep_reads=True)
        assert call(paths, 2, reads=h1.reads) == _lib.GH_ERR_ARG
    # no table on the device
    h2 = Hansel(t.n_snps, band=t.band)
    h2.fill_from_support(t.rank, t.off, t.bases)
    assert h2.reads is None
    with pytest.raises(ValueError, match="keep_reads=True"):
        h2.assign_reads(paths)
    with pytest.raises(ValueError):
        h.assign_reads(paths[:, :-1])


def test_tensor_and_spin_are_untouched():
    t = make_support_table(600, 15000, k=5, seed=14)
    a, b = _filled(t), _filled(t)
    for x in (a, b):
        x.snapshot_original()
    paths = _random_paths(np.random.default_rng(2), 30, t.n_snps)
    stats = (b.L, b.n_slices, b.n_crumbs)
    b.assign_reads(paths, per_read=True)
    assert (b.L, b.n_slices, b.n_crumbs) == stats
    assert np.array_equal(a.export_band(), b.export_band())
    ra, rb = a.spin(10), b.spin(10)
    assert ra["n"] == rb["n"] == 10 and np.array_equal(ra["paths"], rb["paths"])
    for k in ("hp_current", "hp_original", "ratio", "magnitude", "min_marginal"):
        assert ra[k].tobytes() == rb[k].tobytes(), k
    b.assign_reads(rb["paths"])
    assert np.array_equal(a.export_band(), b.export_band())


def _support_want(bam, vcf, contig, s, e, out, min_snps=2, max_mismatch=-1):
    """gretel.support from the support table util.support_table_from_bam decodes and the haplotypes of snp.fasta."""
    v = util.process_vcf(vcf, contig, s, e)
    rank, off, bases = util.support_table_from_bam(bam, contig, s, e, v)
    lines = (out / "snp.fasta").read_text().splitlines()
    i0s = [int(lines[q][1:].split("__")[0]) for q in range(0, len(lines), 2)]
    paths = np.array([path_indices("_" + lines[q + 1]) for q in range(0, len(lines), 2)], dtype=np.uint8).reshape(len(i0s), v["N"] + 1)
    return render(i0s, assign(rank, off, bases, paths, v["N"], min_snps=min_snps, max_mismatch=max_mismatch))


def _with_and_without(tmp_path, capsys, argv, extra, name):
    plain, withf = tmp_path / (name + "_plain"), tmp_path / (name + "_assign")
    plain.mkdir()
    withf.mkdir()
    assert cmd.main(argv + ["-o", str(plain)]) == 0
    cap0 = capsys.readouterr()
    assert cmd.main(argv + ["-o", str(withf), "--assign-reads"] + extra) == 0
    cap1 = capsys.readouterr()
    assert cap0.out == cap1.out and cap0.err == cap1.err
    for f in ("out.fasta", "snp.fasta", "gretel.crumbs"):
        assert (plain / f).read_bytes() == (withf / f).read_bytes(), f
    assert sorted(os.listdir(withf)) == sorted(os.listdir(plain) + ["gretel.support"])
    return withf


def test_cli_on_the_reference_fixture(tmp_path, capsys):
    out = _with_and_without(tmp_path, capsys, [BAM, VCF, "hoot", "-s", "1", "-e", "20", "-p", "12"], [], "ref")
    assert (out / "gretel.support").read_text() == _support_want(BAM, VCF, "hoot", 1, 20, out)
    out = _with_and_without(tmp_path, capsys, [BAM, VCF, "hoot", "-s", "1", "-e", "20", "-p", "3", "--quiet", "--debughpos", "2,3"],
                            ["--min-snps", "1"], "dbg")
    assert (out / "gretel.support").read_text() == _support_want(BAM, VCF, "hoot", 1, 20, out, min_snps=1)


def test_cli_on_synthetic_files(tmp_path, capsys):
    t = make_support_table(150, 3000, k=None, seed=21, k_lambda=5.0, err=0.03)
    bam, vcf = str(tmp_path / "s.bam"), str(tmp_path / "s.vcf.gz")
    contig, s, e = bamio.synth_to_files(t, bam, vcf)
    out = _with_and_without(tmp_path, capsys, [bam, vcf, contig, "-p", "20", "--quiet"], [], "syn")
    text = (out / "gretel.support").read_text()
    assert text == _support_want(bam, vcf, contig, 1, e, out)
    head = [int(x) for x in text.splitlines()[0][2:].split("\t")]
    assert head[0] == t.n_reads and head[2] > 0
    out = _with_and_without(tmp_path, capsys, [bam, vcf, contig, "-p", "20", "--quiet"], ["--min-snps", "3", "--max-mismatch", "1"], "syn2")
    assert (out / "gretel.support").read_text() == _support_want(bam, vcf, contig, 1, e, out, min_snps=3, max_mismatch=1)


def test_panel_support_equals_the_single_cli(tmp_path, capsys):
    t = make_support_table(1000, 30000, k=3, seed=77)
    bam, vcf = str(tmp_path / "c.bam"), str(tmp_path / "c.vcf.gz")
    contig, s, e = bamio.synth_to_files(t, bam, vcf)
    rng = np.random.default_rng(5)
    regions = []
    for i in range(6):
        ln = int(rng.integers(300, 3000))
        st0 = int(rng.integers(0, e - ln))
        regions.append(("g%d" % i, st0, st0 + ln))
    bed = tmp_path / "r.bed"
    bed.write_text("".join("%s\t%d\t%d\t%s\n" % (contig, a, b, n) for n, a, b in regions))
    out = tmp_path / "panel"
    opts = ["-p", "10", "--assign-reads", "--max-mismatch", "2"]
    assert panel.main([bam, vcf, str(bed), "-o", str(out)] + opts) == 0
    capsys.readouterr()
    for name, a, b in regions:
        single = tmp_path / "single" / name
        single.mkdir(parents=True)
        assert cmd.main([bam, vcf, contig, "-s", str(a + 1), "-e", str(b), "--quiet", "-o", str(single)] + opts) == 0
        for f in ("out.fasta", "snp.fasta", "gretel.crumbs", "gretel.support"):
            assert (out / name / f).read_bytes() == (single / f).read_bytes(), (name, f)
    capsys.readouterr()
