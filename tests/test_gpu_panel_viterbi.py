"""Exact decoding over a panel (gh_panel_viterbi_spin, gh_panel_viterbi_info, gh_viterbi_states; HanselBatch.viterbi_spin /
viterbi_info, Hansel.viterbi_states; --exact / --score-paths of gretel_amd.panel): every window's result is gh_viterbi_spin's on
that window alone.  The reference is the plain statement of the definition (tests/viterbi_ref.py over the C oracle), compared as
decode_util._same_spin compares; windows too large for it to be quick (table a at L = 5, a4 at L = 6, C2) go against
Hansel.viterbi_spin on a twin handle, which tests/test_gpu_viterbi.py holds to that reference."""

import numpy as np
import pytest

import viterbi_ref
from decode_util import BAM, E_MT, VCF, _from_haps, _same_spin, _table
from gretel_amd import _lib, bamio, cmd, panel, util
from gretel_amd.hansel import Hansel, HanselBatch, HanselPanel
from gretel_amd.synth import make_support_table
from spec_util import make_pair, same, spec_id

pytestmark = pytest.mark.gpu
CAP = _lib.GH_VITERBI_MAX_STATES
ACGTAC = ["ACGTAC", "CGTACG", "ACTTAG", "AGTTAC"]


def _same_exact(res, ref):
    """_same_spin, and the records bit for bit (the panel's reweight is gh_reweight_path's, window by window)."""
    _same_spin(res, ref)
    for k in ("hp_current", "hp_original", "ratio"):
        assert res[k].tolist() == ref[k].tolist(), k


class Win:
    """A panel window: the handle, and what says what it must give -- the C oracle (the reference runs over it) or a twin."""

    def __init__(self, h, o=None, twin=None):
        self.h, self.o, self.twin = h, o, twin

    def expect(self, max_paths):
        if self.o is not None:
            return viterbi_ref.viterbi_spin(self.o, self.h.n, max_paths, cand_order=self.h._cfg["cand_order"])
        return self.twin.viterbi_spin(max_paths)

    def check(self, res, max_paths):
        ref = self.expect(max_paths)
        if self.o is not None:
            _same_spin(res, ref)
        if self.twin is not None:                               # (with an oracle too: for the handle's own viterbi_info)
            alone = ref if self.o is None else self.twin.viterbi_spin(max_paths)
            _same_exact(res, alone)
            assert res["magnitude"].tolist() == alone["magnitude"].tolist()
            assert self.h.viterbi_info()[:3] == self.twin.viterbi_info()[:3]
        other = self.o if self.o is not None else self.twin
        assert np.array_equal(self.h.export_band(), other.export_band())
        return ref


def _haps(haps, band, L, **kw):
    return Win(*_from_haps(haps, band=band, L=L, **kw), twin=_from_haps(haps, band=band, L=L, **kw)[0])


def _twin(t, L, **kw):
    return Win(make_pair(t, L=L, **kw)[0], twin=make_pair(t, L=L, **kw)[0])


def _biallelic(**kw):
    rng = np.random.default_rng(12)
    haps = ["".join("AG"[v] for v in rng.integers(0, 2, 16)) for _ in range(6)]
    return _haps(haps, 12, 12, **kw)


def _run(wins, max_paths, cls=HanselPanel):
    p = cls([w.h for w in wins])
    got = p.viterbi_spin(max_paths)
    assert len(got) == len(wins)
    refs = [w.check(r, max_paths) for w, r in zip(wins, got)]
    return p, got, refs


@pytest.mark.parametrize("kw", [{}, E_MT], ids=spec_id)
def test_the_ragged_panel(kw):
    wins = [
        (_haps(["A", "C", "C"], 1, 4, **kw), (2, 1, 2)),                               # N = 1
        (_haps(["AC", "CA", "AA"], 1, 5, **kw), (2, 2, 4)),                            # N = 2 < L
        (_haps(ACGTAC, 6, 9, **kw), (4, 6, 4096)),                                     # L >= N: a thread owns four states
        (_haps(["AAAAA", "AAAAA"], 4, 4, **kw), (1, 4, 1)),                            # one candidate everywhere: one state
        (_haps(["A" * 16, "A" * 16], 14, 14, **kw), (1, 14, 1)),                       # S = 1, Le > 12: the non-staged launch
        (_biallelic(**kw), (2, 12, CAP)),
        (Win(*make_pair(_table("a"), L=3, **kw)), (5, 3, 125)),
        (_twin(_table("a"), 5, **kw), (5, 5, 3125)),
        (_twin(_table("a4"), 6, **kw), (4, 6, CAP)),                                   # the cap
        (_twin(_table("C2"), 3, **kw), (4, 3, 64)),                                    # N > 512: the trace runs in chunks
        (_haps(["ACGTACGT", "CGTACGTA", "ACTTAGGT"], 3, 3, skip=(1,), **kw), None),    # holes: n = 0 while the others run on
        (_haps(["ACGTACGT", "CGTACGTA", "ACTTAGGT"], 3, 3, skip=(8,), **kw), None),
    ]
    assert wins[9][0].h.n > 512
    for w, shape in wins:
        assert shape is None or w.h.viterbi_states() == shape
    # (afterwards each handle's viterbi_info is that of its own last decoding -- of a tensor that may offer less by then: Win.check
    # holds it to the twin's)
    p, got, refs = _run([w for w, _ in wins], 4)
    for (w, shape), r in zip(wins, got):
        if shape is None:
            assert r["n"] == 0 and r["hole_at"] in (1, 8) and r["paths"].shape == (0, 9)
        elif r["hole_at"] == 0:
            assert w.h.viterbi_info()[1] == shape[1] and 0 < w.h.viterbi_info()[2] <= shape[2]
    assert [r["hole_at"] for r in got[-2:]] == [1, 8]
    assert [r["n"] for r in got[6:10]] == [4, 4, 4, 4]
    windows, rounds, most, launches = p.viterbi_info()
    # (every round a staged launch; the S = 1, Le = 14 window in a launch of its own for as long as it lives)
    assert windows == len(wins) and rounds == 4 and most == len(wins) - 1 and launches > rounds


def test_the_live_set_shrinks():
    ta = make_support_table(150, 1000, k=4, seed=900, n_haps=1, err=0.0)              # one haplotype, no errors: it empties
    wins = [Win(*make_pair(ta, L=3)), Win(*make_pair(_table("a"), L=2)), Win(*make_pair(_table("a"), L=3))]
    p, got, refs = _run(wins, 5)
    assert 1 <= refs[0]["n"] < 5 and refs[0]["hole_at"] >= 1                           # the oracle's spin ends early ...
    assert refs[1]["n"] == 5 and refs[2]["n"] == 5                                     # ... the others' do not
    assert got[0]["n"] == refs[0]["n"] and got[0]["hole_at"] == refs[0]["hole_at"] and got[1]["n"] == got[2]["n"] == 5
    windows, rounds, most, launches = p.viterbi_info()
    assert (windows, rounds, most) == (3, 5, 3) and launches == 5


@pytest.mark.parametrize("order", ["ACGT-", "T-GCA"])
def test_ties_and_order(order):
    wins = [_haps(["ACACAC", "CACACA"], 3, 3, cand_order=order), _haps(["AGTTACG", "CGTTACG"], 3, 3, cand_order=order)]
    p, got, _ = _run(wins, 2)
    first = ["".join("ACGTN-_"[int(v)] for v in r["paths"][0][1:]) for r in got]
    assert first == (["CACACA", "AGTTACG"] if order == "ACGT-" else ["ACACAC", "CGTTACG"])


def test_no_paths_and_one_window():
    w = Win(*make_pair(_table("a"), L=3))
    for cls in (HanselPanel, HanselBatch):
        p = cls([w.h])
        before = w.h.export_band()
        got = p.viterbi_spin(0)
        assert len(got) == 1 and got[0]["n"] == 0 and got[0]["hole_at"] == 0 and got[0]["paths"].shape == (0, w.h.n + 1)
        assert got[0]["ll_chain"].shape == (0,)
        assert np.array_equal(w.h.export_band(), before) and w.h.viterbi_info() == (0, 0, 0, 0)
        assert p.viterbi_info() == (1, 0, 0, 0)
    _run([w], 3, cls=HanselBatch)                              # a batch of one window equals viterbi_spin


def test_more_workgroups_than_are_resident_at_once():
    rng = np.random.default_rng(40)
    wins = []
    for i in range(40):
        t = make_support_table(int(rng.integers(30, 61)), 600, k=None, seed=5000 + i)
        wins.append(_twin(t, 2 + i % 3))
    p, got, _ = _run(wins, 3)
    assert p.viterbi_info()[2] == 40


def _state(h):
    return h.export_band().tobytes(), h.viterbi_info(), h.L, h.n_slices, h.n_crumbs


def test_refusals():
    L = _lib.load()
    t4 = _table("a4")
    big = make_pair(t4, L=7)[0]
    ok = [make_pair(_table("a"), L=3)[0], make_pair(t4, L=3)[0]]
    hs = [ok[0], big, ok[1]]
    p = HanselPanel(hs)
    ok[1].viterbi_path()                                        # (a viterbi_info to keep)
    before = [_state(h) for h in hs]
    with pytest.raises(_lib.GretelHipError, match=r"window 1: .*16384 states") as e:
        p.viterbi_spin(3)
    assert e.value.code == _lib.GH_ERR_ARG
    assert [_state(h) for h in hs] == before
    twin = make_pair(_table("a"), L=3)[0]
    assert big.viterbi_states() == (4, 7, 16384)
    big.L = 6
    assert big.viterbi_states() == (4, 6, CAP)
    got = p.viterbi_spin(2)
    assert [r["n"] for r in got] == [2, 2, 2]
    _same_exact(got[0], twin.viterbi_spin(2))
    assert make_pair(_table("a"))[0].viterbi_states() == (5, 10, 9765625)       # the fill's own L
    fresh = Hansel(t4.n_snps, band=t4.band)
    with pytest.raises(_lib.GretelHipError, match="before any fill") as e:
        fresh.viterbi_states()
    assert e.value.code == _lib.GH_ERR_STATE
    with pytest.raises(_lib.GretelHipError, match="window 1: .*before any fill") as e:
        HanselPanel([ok[1], fresh]).viterbi_spin(2)
    assert e.value.code == _lib.GH_ERR_STATE
    hz = [make_pair(t4, L=3, offer_zero=True)[0] for _ in range(2)]
    with pytest.raises(_lib.GretelHipError, match="window 0: .*offer_zero") as e:
        HanselPanel(hz).viterbi_spin(2)
    assert e.value.code == _lib.GH_ERR_ARG
    # null arguments and max_paths = -1 through ctypes
    n = len(hs)
    paths = np.zeros(sum(h.n + 1 for h in hs) * 2, dtype=np.uint8)
    off = np.zeros(n, dtype=np.int64)
    off[1:] = np.cumsum([2 * (h.n + 1) for h in hs[:-1]])
    recs, ll = np.zeros((n, 2, 5)), np.zeros((n, 2))
    n_out, hole = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    args = [p._b, 2, 0.01, paths.ctypes.data, off.ctypes.data, recs.ctypes.data, ll.ctypes.data, n_out.ctypes.data, hole.ctypes.data]
    for q in (0, 3, 4, 5, 7, 8):
        a = list(args)
        a[q] = None
        assert L.gh_panel_viterbi_spin(*a) == _lib.GH_ERR_ARG, q
    a = list(args)
    a[1] = -1
    assert L.gh_panel_viterbi_spin(*a) == _lib.GH_ERR_ARG and b"max_paths < 0" in L.gh_last_error()
    a = list(args)
    a[1] = 0
    assert L.gh_panel_viterbi_spin(*a) == _lib.GH_OK and n_out.tolist() == [0] * n and hole.tolist() == [0] * n
    a = list(args)
    a[6] = None                                                 # ll_chain may be NULL
    assert L.gh_panel_viterbi_spin(*a) == _lib.GH_OK and 0 <= n_out.min() and n_out.max() <= 2 and n_out[0] > 0
    info = np.zeros(4, dtype=np.int64)
    assert L.gh_panel_viterbi_info(None, info.ctypes.data) == _lib.GH_ERR_ARG
    assert L.gh_panel_viterbi_info(p._b, None) == _lib.GH_ERR_ARG
    st = np.zeros(3, dtype=np.int64)
    assert L.gh_viterbi_states(None, st.ctypes.data) == _lib.GH_ERR_ARG and L.gh_viterbi_states(big._h, None) == _lib.GH_ERR_ARG


def test_handles_stay_usable_alone():
    t = _table("a")
    wins = [Win(*make_pair(t, L=3)), Win(*make_pair(_table("a4"), L=2))]
    _run(wins, 3)
    h, o = wins[0].h, wins[0].o                                 # (the reference has reweighted the oracle alike)
    got = h.viterbi_path()
    ref = viterbi_ref.viterbi(o, h.n)
    assert got["hole_at"] == ref["hole_at"] == 0 and got["ll_chain"] == ref["ll_chain"] and np.array_equal(got["path"], ref["path"])
    fresh = make_pair(t, L=3)[0]
    fresh.viterbi_spin(3)
    same(h.spin(4), fresh.spin(4))
    assert np.array_equal(h.export_band(), fresh.export_band())


def test_cli_exact(tmp_path, capsys):
    regions = [("r1", 0, 20), ("r2", 0, 15), ("r3", 0, 12)]                            # (SNPs at 1, 2, 10 and 20)
    bed = tmp_path / "r.bed"
    bed.write_text("".join("hoot\t%d\t%d\t%s\n" % (a, b, n) for n, a, b in regions))
    out = tmp_path / "panel"
    opts = ["-p", "6", "--exact", "--score-paths"]
    assert panel.main([BAM, VCF, str(bed), "-o", str(out)] + opts) == 0
    cap = capsys.readouterr()
    assert [x.split("\t")[0] for x in cap.out.splitlines()] == [n for n, _, _ in regions]
    for name, a, b in regions:
        single = tmp_path / "single" / name
        single.mkdir(parents=True)
        assert cmd.main([BAM, VCF, "hoot", "-s", str(a + 1), "-e", str(b), "--quiet", "-o", str(single)] + opts) == 0
        for f in ("out.fasta", "snp.fasta", "gretel.crumbs", "gretel.scores"):
            assert (out / name / f).read_bytes() == (single / f).read_bytes(), (name, f)
    capsys.readouterr()


def test_cli_exact_leaves_out_a_region_over_the_cap(tmp_path, capsys, monkeypatch):
    # (the reference BAM's four SNPs cannot make more than 256 states: a BAM of table a4 -- 60 SNPs at 10, 20, ..., S = 4 -- whose
    # whole contig is one region, its filled L set to 7: 16384 states; the two short regions hold five and six SNPs)
    bam, vcf = str(tmp_path / "c.bam"), str(tmp_path / "c.vcf.gz")
    contig, s, e = bamio.synth_to_files(_table("a4"), bam, vcf)
    regions = [("five", 0, 55), ("whole", s - 1, e), ("six", 100, 165)]
    bed = tmp_path / "r.bed"
    bed.write_text("".join("%s\t%d\t%d\t%s\n" % (contig, a, b, n) for n, a, b in regions))
    load = util.load_from_bam

    def over(bam_, contig_, start, end, vh, **kw):
        h = load(bam_, contig_, start, end, vh, **kw)
        if vh["N"] == 60:
            h.L = 7
        return h

    monkeypatch.setattr(util, "load_from_bam", over)
    out = tmp_path / "panel"
    opts = ["-p", "4", "--exact", "--score-paths"]
    assert panel.main([bam, vcf, str(bed), "-o", str(out)] + opts) == 1
    cap = capsys.readouterr()
    assert cap.err.count("whole: [FAIL] ") == 1 and "16384 states, more than the 4096" in cap.err
    rows = [x.split("\t") for x in cap.out.splitlines()]
    assert [(x[0], x[1]) for x in rows] == [("five", "5"), ("six", "6")]
    assert not (out / "whole").exists()
    monkeypatch.setattr(util, "load_from_bam", load)
    for name, a, b in (regions[0], regions[2]):
        single = tmp_path / "single" / name
        single.mkdir(parents=True)
        assert cmd.main([bam, vcf, contig, "-s", str(a + 1), "-e", str(b), "--quiet", "-o", str(single)] + opts) == 0
        for f in ("out.fasta", "snp.fasta", "gretel.crumbs", "gretel.scores"):
            assert (out / name / f).read_bytes() == (single / f).read_bytes(), (name, f)
    capsys.readouterr()
