"""Panels (gh_panel_*, HanselPanel, gretel_amd.panel): windows of differing N, band and L recovered together -- one pipeline group
per lag count, gh_spin for what no group carries -- give, bit for bit, what Hansel.spin gives for every window alone."""

import numpy as np
import pytest

from gretel_amd import bamio, cmd, panel
from gretel_amd.hansel import Hansel, HanselBatch, HanselPanel
from gretel_amd.synth import make_support_table, sprinkle_deletions

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_pipeline(monkeypatch):
    for v in ("GH_PIPE", "GH_PIPE_MIN", "GH_PIPE_NT", "GH_PIPE_MAX_L", "GH_PIPE_WIDE"):
        monkeypatch.delenv(v, raising=False)


def _cut(t, p):
    """Drop every read that covers both SNP p and SNP p + 1 (1-based): no evidence across that pair -- a hole."""
    ks = np.diff(t.off)
    first = t.rank.astype(np.int64) + 1
    last = first + ks - 1
    keep = ~((first <= p) & (last >= p + 1))
    rows = [t.bases[t.off[r]:t.off[r + 1]] for r in np.flatnonzero(keep)]
    t.rank = np.ascontiguousarray(t.rank[keep])
    t.off = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    t.bases = np.concatenate(rows).astype(np.uint8)
    return t


def _twins(t, L=None, **spec):
    """Two Hansels filled independently from the same table: one for the panel, one for Hansel.spin."""
    hs = []
    for _ in range(2):
        h = Hansel(t.n_snps, band=t.band, **spec)
        h.fill_from_support(t.rank, t.off, t.bases)
        if L is not None:
            h.L = L
        hs.append(h)
    assert hs[0].L == hs[1].L
    return hs


def _same(r, ref):
    assert r["n"] == ref["n"] and r["hole_at"] == ref["hole_at"], (r["n"], ref["n"], r["hole_at"], ref["hole_at"])
    assert r["paths"].dtype == ref["paths"].dtype and np.array_equal(r["paths"], ref["paths"])
    for k in ("hp_current", "hp_original", "ratio", "min_marginal"):
        assert r[k].dtype == ref[k].dtype and r[k].tobytes() == ref[k].tobytes(), k
    # the removed mass is a sum whose order is the pipeline's own (as in every batched spin: test_gpu_batch.py, test_gpu_pipe.py)
    assert r["magnitude"].dtype == ref["magnitude"].dtype and np.allclose(r["magnitude"], ref["magnitude"], rtol=1e-12, atol=0)


def _check(wins, max_paths):
    p = HanselPanel([a for a, _ in wins])
    got = p.spin(max_paths)
    assert len(got) == len(wins)
    for (a, b), r in zip(wins, got):
        _same(r, b.spin(max_paths))
        assert np.array_equal(a.export_band(), b.export_band())
    return p, got


def test_ragged_panel_equals_single_windows():
    rng = np.random.default_rng(7)
    wins, kinds = [], []
    # L = 5: two dozen windows of 40 .. 3 000 SNPs and bands 3 .. 7, four of them with deletion columns (the WIDE launch), one
    # with a hole, one that empties after its first path (its masks move: the pipeline hands it back)
    n5 = np.sort(rng.integers(40, 3001, 24))
    for i, n in enumerate(n5):
        n = int(n)
        if i == 5:
            t, kind = make_support_table(150, 1000, k=4, seed=900, n_haps=1, err=0.0), "abort"
        else:
            t, kind = make_support_table(n, 12 * n, k=4 + i % 5, seed=1000 + i), "narrow"
            if i in (2, 9, 14, 20):
                sprinkle_deletions(t, 0.02, seed=2000 + i)
                kind = "wide"
            elif i == 11:
                _cut(t, n // 2)
                kind = "hole"
        wins.append(_twins(t, L=5))
        kinds.append(kind)
    # L = 3: two dozen more (a second pipeline group)
    for i, n in enumerate(np.sort(rng.integers(40, 2001, 24))):
        t = make_support_table(int(n), 10 * int(n), k=3 + i % 4, seed=3000 + i)
        wins.append(_twins(t, L=3))
        kinds.append("narrow")
    # a few at L = 7 and L = 11: groups too small for the pipeline, gh_spin takes them
    for i, (n, L) in enumerate(((300, 7), (900, 7), (500, 11), (1200, 11))):
        t = make_support_table(n, 12 * n, k=None, seed=4000 + i, k_max=14)
        wins.append(_twins(t, L=L))
        kinds.append("alone")
    for (a, _), kind in zip(wins, kinds):
        if kind == "wide":
            assert (a.candidate_masks()[1:] == 0x2F).any()
        if kind == "hole":
            assert a.gap_check() > 0
    assert len({a.n for a, _ in wins}) > 40 and len({a._band for a, _ in wins}) >= 4
    p, got = _check(wins, 10)
    info = p.pipe_info()
    carried = sum(k in ("narrow", "wide", "abort") for k in kinds)
    assert info["windows"] == carried and info["handed_back"] >= 1, info
    assert info["threads"] in (768, 1024) and info["chunk"] > 0, info
    hole = got[kinds.index("hole")]
    assert hole["hole_at"] > 0
    ab = got[kinds.index("abort")]
    assert ab["n"] == 1 and ab["hole_at"] >= 1
    assert all(r["n"] == 10 for r, k in zip(got, kinds) if k in ("narrow", "wide"))
    # views stay valid memory after the panel has moved on
    again = p.spin(4, copy=False)
    assert [r["n"] for r in again][:3] == [4, 4, 4]


def test_uniform_panel_equals_the_batch():
    tabs = [make_support_table(800, 16000, k=5, seed=5000 + s) for s in range(26)]
    pw, bw = [], []
    for t in tabs:
        a, b = _twins(t)
        pw.append(a)
        bw.append(b)
    p = HanselPanel(pw)
    got = p.spin(12)
    b = HanselBatch(bw)
    ref = b.spin(12)
    assert p.pipe_info() == b.pipe_info()
    for r, q, x, y in zip(got, ref, pw, bw):
        _same(r, q)
        assert np.array_equal(x.export_band(), y.export_band())
    # gh_batch_spin refuses a panel (its windows need not share a shape)
    buf, recs, k = np.zeros(26 * 3 * 801, np.uint8), np.zeros(26 * 3 * 5), np.zeros(26, np.int32)
    assert p._lib.gh_batch_spin(p._b, 3, 0.01, buf.ctypes.data, recs.ctypes.data, k.ctypes.data, k.ctypes.data) != 0


@pytest.mark.parametrize("spec", [dict(cond_mode="E", marginal_term=True), dict(storage="f64")])
def test_ragged_panel_other_specs(spec, monkeypatch):
    monkeypatch.setenv("GH_PIPE_MIN", "4")
    rng = np.random.default_rng(11)
    wins = []
    for i, n in enumerate(rng.integers(40, 1500, 10)):
        t = make_support_table(int(n), 12 * int(n), k=4 + i % 3, seed=6000 + i)
        if i == 3:
            sprinkle_deletions(t, 0.02, seed=6100)
        wins.append(_twins(t, L=5 if i < 6 else 3, **spec))
    p, _ = _check(wins, 8)
    assert p.pipe_info()["windows"] == 10, p.pipe_info()


def test_panel_cli_equals_the_single_cli(tmp_path, capsys):
    t = make_support_table(1000, 50000, k=3, seed=77)                  # (C2's shape)
    bam, vcf = str(tmp_path / "c.bam"), str(tmp_path / "c.vcf.gz")
    contig, s, e = bamio.synth_to_files(t, bam, vcf)
    rng = np.random.default_rng(3)
    regions = []
    for i in range(30):
        ln = int(rng.integers(300, 4000))
        st0 = int(rng.integers(0, e - ln))
        regions.append(("g%02d" % i, st0, st0 + ln))
    regions.append(("lonely", 45, 55))          # one SNP (position 50): no read carries two
    bed = tmp_path / "r.bed"
    bed.write_text("#name\n" + "".join("%s\t%d\t%d\t%s\n" % (contig, a, b, n) for n, a, b in regions))
    out = tmp_path / "panel"
    opts = ["-p", "15", "--gapchar", "x"]
    assert panel.main([bam, vcf, str(bed), "-o", str(out)] + opts) == 1
    cap = capsys.readouterr()
    assert cap.err.count("lonely: [FAIL] Unable to recover pairwise evidence") == 1
    summary = [x.split("\t") for x in cap.out.splitlines()]
    assert [x[0] for x in summary] == [n for n, _, _ in regions[:30]]
    assert not (out / "lonely").exists()
    for (name, a, b), row in zip(regions[:30], summary):
        single = tmp_path / "single" / name
        single.mkdir(parents=True)
        assert cmd.main([bam, vcf, contig, "-s", str(a + 1), "-e", str(b), "--quiet", "-o", str(single)] + opts) == 0
        for f in ("out.fasta", "snp.fasta", "gretel.crumbs"):
            assert (out / name / f).read_bytes() == (single / f).read_bytes(), (name, f)
        n_hap = len((single / "snp.fasta").read_text().splitlines()) // 2
        assert int(row[4]) == n_hap and int(row[3]) >= n_hap
    with pytest.raises(ZeroDivisionError):
        cmd.main([bam, vcf, contig, "-s", "46", "-e", "55", "--quiet", "-o", str(tmp_path)])
    capsys.readouterr()
