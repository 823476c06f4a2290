"""Panels (gretel_amd.panel, HanselPanel, gh_panel_*) on the host: the BED reader, the one-pass VCF reader against process_vcf,
the CLI's refusals before any GPU call, and the C ABI's declarations and exports."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REFDATA, ROOT
from gretel_amd import _lib, bamio, util

VCF = os.path.join(REFDATA, "test.vcf.gz")
BAM = os.path.join(REFDATA, "test.bam")


def _bed(tmp_path, text, name="r.bed"):
    f = tmp_path / name
    f.write_text(text)
    return str(f)


def test_read_regions_good(tmp_path):
    f = _bed(tmp_path, "# a comment\ntrack name=x\nbrowser position hoot:1-20\n\nhoot\t0\t20\tgeneA\nmeow\t4\t9\n"
                       "hoot\t9\t20\t\nhoot\t0\t1\tone base\n")
    r = util.read_regions(f)
    assert r == [dict(name="geneA", contig="hoot", start=1, end=20), dict(name="meow:5-9", contig="meow", start=5, end=9),
                 dict(name="hoot:10-20", contig="hoot", start=10, end=20), dict(name="one base", contig="hoot", start=1, end=1)]
    assert util.read_regions(_bed(tmp_path, "", "empty.bed")) == []


@pytest.mark.parametrize("text, line, what", [
    ("hoot\t0\t20\n" "hoot\t5\n", 2, "three"),
    ("hoot\t0\t20\tA\nhoot\t2\t20\tA\n", 2, "already used on line 1"),
    ("hoot\t0\t20\nhoot\t0\t20\n", 2, "already used"),                  # (the default names collide as well)
    ("#x\nhoot\t20\t20\n", 2, "empty"),
    ("hoot\t21\t20\n", 1, "empty"),
    ("hoot\t-1\t20\n", 1, "before 0"),
    ("hoot\tone\t20\n", 1, "integers"),
    ("hoot\t0\t20\ta/b\n", 1, "directory"),
    ("\t0\t20\n", 1, "three"),
])
def test_read_regions_refuses(tmp_path, text, line, what):
    f = _bed(tmp_path, text)
    with pytest.raises(ValueError) as e:
        util.read_regions(f)
    assert (":%d:" % line) in str(e.value) and what in str(e.value), str(e.value)


def _same(a, b):
    assert a["N"] == b["N"] and a["snp_fwd"] == b["snp_fwd"] and a["snp_rev"] == b["snp_rev"]
    assert np.array_equal(a["region"], b["region"]) and a["region"].dtype == b["region"].dtype


def test_process_vcf_regions_reference_fixture(tmp_path):
    regions = [("hoot", 1, 20), ("hoot", 10, 20), ("hoot", 5, 12), ("meow", 1, 20), ("hoot", 1, 1), ("hoot", 3, 3),
               ("nosuch", 1, 50), ("hoot", 2, 15), ("meow", 3, 40)]
    got = util.process_vcf_regions(VCF, regions)
    assert len(got) == len(regions)
    for (c, s, e), g in zip(regions, got):
        _same(g, util.process_vcf(VCF, c, s, e))
    assert got[0]["N"] > 0 and got[6]["N"] == 0
    # read_regions' dicts are taken as they are
    f = _bed(tmp_path, "hoot\t0\t20\tx\nmeow\t0\t20\n")
    for r, g in zip(util.read_regions(f), util.process_vcf_regions(VCF, util.read_regions(f))):
        _same(g, util.process_vcf(VCF, r["contig"], r["start"], r["end"]))


def test_process_vcf_regions_synthetic(tmp_path):
    rng = np.random.default_rng(5)
    pos = np.unique(rng.integers(1, 5000, 700)).tolist()
    f = str(tmp_path / "s.vcf.gz")
    bamio.write_vcf_gz(f, "chrS", pos)
    regions = [("chrS", 1, 5000), ("chrS", 100, 900), ("chrS", 800, 2000), ("chrS", 1500, 1600), ("chrS", 4999, 5000),
               ("chrS", 1, 1), ("chrX", 1, 5000), ("chrS", 2000, 1000 + 2000)]
    for (c, s, e), g in zip(regions, util.process_vcf_regions(f, regions)):
        _same(g, util.process_vcf(f, c, s, e))


def test_process_vcf_regions_reads_the_file_once(tmp_path, monkeypatch):
    f = str(tmp_path / "s.vcf.gz")
    bamio.write_vcf_gz(f, "chrS", [10, 20, 30])
    calls = []
    real = util._vcf_bytes
    monkeypatch.setattr(util, "_vcf_bytes", lambda p: calls.append(p) or real(p))
    out = util.process_vcf_regions(f, [("chrS", 1, 15), ("chrS", 15, 30), ("chrS", 1, 30)])
    assert [o["N"] for o in out] == [1, 2, 3] and calls == [f]


def test_cli_refuses_bad_regions_before_any_gpu_call(tmp_path, monkeypatch, capsys):
    from gretel_amd import hansel, panel

    def boom(*a, **k):
        raise AssertionError("reached the BAM or the GPU")
    monkeypatch.setattr(util, "load_from_bam", boom)
    monkeypatch.setattr(util, "prefetch_bam", boom)
    monkeypatch.setattr(hansel.HanselPanel, "__init__", boom)
    for text, what in (("hoot\t0\t20\nhoot\t5\n", ":2:"), ("hoot\t0\t20\tA\nmeow\t0\t20\tA\n", "already used"),
                       ("hoot\t20\t10\n", "empty"), ("# nothing\n", "no region")):
        f = _bed(tmp_path, text)
        assert panel.main([BAM, VCF, f, "-o", str(tmp_path / "out")]) == 2
        assert what in capsys.readouterr().err
    assert panel.main([BAM, VCF, str(tmp_path / "missing.bed"), "-o", str(tmp_path / "out")]) == 2
    assert panel.main([BAM, VCF, _bed(tmp_path, "hoot\t0\t20\n"), "-p", "0", "-o", str(tmp_path / "out")]) == 2
    assert not (tmp_path / "out").exists()
    # the single-region debugging options are not offered
    for opt in (["--debughpos", "2"], ["--dumpmatrix", "x.npz"], ["--debugreads", "x"], ["--debugpos", "x"]):
        with pytest.raises(SystemExit):
            panel.main([BAM, VCF, _bed(tmp_path, "hoot\t0\t20\n")] + opt)
        capsys.readouterr()


def test_panel_abi_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "gretel_hip.h")).read()
    assert "int gh_panel_create(gh_t **handles, int n, gh_batch_t **out);" in src
    assert "int gh_panel_spin(gh_batch_t *b, int max_paths, double min_remove, uint8_t *paths_out, const int64_t *paths_off," in src
    so = ctypes.CDLL(_lib.SO_PATH)
    assert hasattr(so, "gh_panel_create") and hasattr(so, "gh_panel_spin")
    L = _lib.load()
    assert len(L.gh_panel_spin.argtypes) == 8 and len(L.gh_panel_create.argtypes) == 3
    from gretel_amd.hansel import HanselPanel, HanselBatch
    assert issubclass(HanselPanel, HanselBatch)
    with pytest.raises(ValueError):
        HanselPanel([])
