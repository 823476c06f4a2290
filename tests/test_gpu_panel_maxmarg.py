"""Max-marginals over a panel (gh_panel_viterbi_marginals, gh_panel_viterbi_marginals_info; HanselBatch.viterbi_marginals /
viterbi_marginals_info; --margins of gretel_amd.panel): every window's result is gh_viterbi_marginals' on that window alone, as
IEEE values.  The reference is the plain statement of the definition (tests/maxmarg_ref.py over the C oracle); the call only reads
the tensors, so Hansel.viterbi_marginals() on the same handle afterwards is each window's twin."""
import os
import subprocess
import sys

import numpy as np
import pytest

import maxmarg_ref
from decode_util import BAM, E_MT, VCF, _from_haps, _table
from gretel_amd import _lib, bamio, cmd, panel, util
from gretel_amd.hansel import Hansel, HanselBatch, HanselPanel
from gretel_amd.synth import make_support_table
from spec_util import make_pair, same, spec_id

pytestmark = pytest.mark.gpu
CAP = _lib.GH_VITERBI_MAX_STATES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGTAC = ["ACGTAC", "CGTACG", "ACTTAG", "AGTTAC"]
OCT = ["ACGTACGT", "CGTACGTA", "ACTTAGGT"]


def _biallelic(kw):
    rng = np.random.default_rng(12)
    haps = ["".join("AG"[v] for v in rng.integers(0, 2, 16)) for _ in range(6)]
    return _from_haps(haps, band=12, L=12, **kw)


# the windows by name: (handle, oracle) under a spec
WINDOWS = {
    "n1": lambda kw: _from_haps(["A", "C", "C"], band=1, L=4, **kw),
    "n2": lambda kw: _from_haps(["AC", "CA", "AA"], band=1, L=5, **kw),
    "warm": lambda kw: _from_haps(ACGTAC, band=6, L=9, **kw),
    "one4": lambda kw: _from_haps(["AAAAA", "AAAAA"], band=4, L=4, **kw),
    "one14": lambda kw: _from_haps(["A" * 16, "A" * 16], band=14, L=14, **kw),
    "bi12": _biallelic,
    "a3": lambda kw: make_pair(_table("a"), L=3, **kw),
    "a5": lambda kw: make_pair(_table("a"), L=5, **kw),
    "a4_2": lambda kw: make_pair(_table("a4"), L=2, **kw),
    "a4_6": lambda kw: make_pair(_table("a4"), L=6, **kw),
    "C2": lambda kw: make_pair(_table("C2"), L=3, **kw),
    "hole1": lambda kw: _from_haps(OCT, band=3, L=3, skip=(1,), **kw),
    "hole8": lambda kw: _from_haps(OCT, band=3, L=3, skip=(8,), **kw),
    "tie1": lambda kw: _from_haps(["ACACAC", "CACACA"], band=3, L=3, **kw),
    "tie2": lambda kw: _from_haps(["AGTTACG", "CGTTACG"], band=3, L=3, **kw),
}
# the ragged panel of tests/test_gpu_panel_viterbi.py and what viterbi_states says of each window
RAGGED = [("n1", (2, 1, 2)), ("n2", (2, 2, 4)), ("warm", (4, 6, 4096)), ("one4", (1, 4, 1)), ("one14", (1, 14, 1)), ("bi12", (2, 12, CAP)),
          ("a3", (5, 3, 125)), ("a5", (5, 5, 3125)), ("a4_6", (4, 6, CAP)), ("C2", (4, 3, 64)), ("hole1", None), ("hole8", None)]
_refs = {}


def _win(name, **kw):
    """(the handle, the reference's max-marginals of its oracle: computed once per window and spec, never changed)."""
    h, o = WINDOWS[name](kw)
    key = (name, spec_id(kw))
    if key not in _refs:
        _refs[key] = maxmarg_ref.marginals(o, h.n)
    return h, _refs[key]


def _equal(got, ref, what):
    assert got["hole_at"] == ref["hole_at"], what
    if ref["hole_at"]:
        assert got["mm"] is None and got["cm"] is None, what
        return
    assert got["mm"].dtype == np.float64 and got["cm"].dtype == np.uint8, what
    assert got["mm"].shape == ref["mm"].shape and got["cm"].shape == ref["cm"].shape, what
    assert np.array_equal(got["cm"], ref["cm"]), (what, np.argwhere(got["cm"] != ref["cm"])[:4].tolist())
    bad = np.argwhere(got["mm"] != ref["mm"])
    assert np.array_equal(got["mm"], ref["mm"]), (what, len(bad), bad[:4].tolist(), [(got["mm"][tuple(q)], ref["mm"][tuple(q)]) for q in bad[:4]])


def _alone(hs, got, what=""):
    """Every window against Hansel.viterbi_marginals() on the same handle, and the handle's viterbi_info against the single call's."""
    for w, (h, r) in enumerate(zip(hs, got)):
        info = h.viterbi_info()
        _equal(r, h.viterbi_marginals(), "%s window %d alone" % (what, w))
        assert h.viterbi_info() == info, (what, w, info, h.viterbi_info())


@pytest.mark.parametrize("kw", [{}, E_MT], ids=spec_id)
def test_the_ragged_panel(kw):
    wins = [_win(name, **kw) for name, _ in RAGGED]
    hs = [h for h, _ in wins]
    assert hs[9].n > 512
    for h, (name, shape) in zip(hs, RAGGED):
        assert shape is None or h.viterbi_states() == shape, name
    p = HanselPanel(hs)
    got = p.viterbi_marginals()
    assert len(got) == len(wins)
    for (h, ref), r, (name, shape) in zip(wins, got, RAGGED):
        _equal(r, ref, name)
        if shape is not None:
            assert h.viterbi_info()[:3] == shape and h.viterbi_info()[3] >= h.n * shape[2] * 8, name
            assert not np.isnan(r["mm"]).any(), name
    assert [r["hole_at"] for r in got[-2:]] == [1, 8]
    windows, holes, launches, scratch = p.viterbi_marginals_info()
    # (two forward launches -- the S = 1, Le = 14 window walks without the ring -- and two backward: biallelic at L = 12 does not fit)
    assert windows == len(wins) and holes == 2 and launches >= 4
    assert scratch == sum(h.viterbi_info()[3] for h in hs)
    _alone(hs, got, spec_id(kw))
    for h, r in zip(hs, got):
        if not r["hole_at"]:
            assert r["mm"][h.n].max() == h.viterbi_path()["ll_chain"]      # B_N = +0.0
    # each window got its own arrays
    got[0]["mm"][:] = 0.0
    assert got[1]["mm"].base is None and not np.shares_memory(got[0]["mm"], got[1]["mm"]) and np.isinf(got[1]["mm"][0]).all()


def test_more_windows_than_workgroups_are_resident_at_once():
    rng = np.random.default_rng(40)
    hs = []
    for i in range(300):
        t = make_support_table(int(rng.integers(30, 61)), 600, k=None, seed=5000 + i)
        hs.append(make_pair(t, L=2 + i % 3)[0])
    p = HanselPanel(hs)
    got = p.viterbi_marginals()
    assert p.viterbi_marginals_info()[:2] == (300, 0)
    _alone(hs, got)


def _stats(h):
    return h.export_band().tobytes(), h.L, h.n_slices, h.n_crumbs


@pytest.mark.parametrize("cls", [HanselPanel, HanselBatch], ids=["panel", "batch"])
def test_the_call_only_reads(cls):
    if cls is HanselPanel:
        make = lambda: [make_pair(_table("a"), L=3)[0], make_pair(_table("a4"), L=2)[0], make_pair(_table("a"), L=2)[0]]
    else:                                                       # (a batch: windows of one shape)
        make = lambda: [make_pair(_table(w), L=3)[0] for w in ("a", "a4", "a")]      # (a4: a's reads without the deletions)
    hs, fresh = make(), make()
    before = [_stats(h) for h in hs]
    p = cls(hs)
    got = p.viterbi_marginals()
    assert [_stats(h) for h in hs] == before
    _alone(hs, got)
    assert [_stats(h) for h in hs] == before
    for a, b in zip(p.spin(4), cls(fresh).spin(4)):
        same(a, b)
    for h, f in zip(hs, fresh):
        assert np.array_equal(h.export_band(), f.export_band())


@pytest.mark.parametrize("order", ["ACGT-", "T-GCA"])
def test_exact_ties(order):
    wins = [_win("tie1", cand_order=order), _win("tie2", cand_order=order)]
    hs = [h for h, _ in wins]
    got = HanselPanel(hs).viterbi_marginals()
    for (h, ref), r in zip(wins, got):
        _equal(r, ref, order)
    assert (got[0]["mm"][1:, 0] == got[0]["mm"][1:, 1]).all() and got[1]["mm"][1, 0] == got[1]["mm"][1, 1] > -np.inf
    _alone(hs, got, order)


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from decode_util import _from_haps, _table
from gretel_amd.hansel import HanselPanel
from spec_util import make_pair
hs = [make_pair(_table("a"), L=3)[0], make_pair(_table("a4"), L=2)[0], _from_haps(["A" * 16, "A" * 16], band=14, L=14)[0]]
p = HanselPanel(hs)
got = p.viterbi_marginals()
assert p.viterbi_marginals_info()[2] == 2, p.viterbi_marginals_info()      # one forward and one backward launch, neither staged
for w, r in enumerate(got):
    np.save(sys.argv[1] + "mm%%d.npy" %% w, r["mm"])
    np.save(sys.argv[1] + "cm%%d.npy" %% w, r["cm"])
"""


def test_the_tables_from_global_memory_give_the_same_bits(tmp_path):
    # GH_VIT_STAGE is read once in a process: a fresh child
    env = dict(os.environ, GH_VIT_STAGE="0")
    stem = str(tmp_path) + os.sep
    subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), stem], env=env, check=True, timeout=300)
    for w, name in enumerate(("a3", "a4_2", "one14")):
        ref = _win(name)[1]
        assert np.array_equal(np.load(stem + "mm%d.npy" % w), ref["mm"]) and np.array_equal(np.load(stem + "cm%d.npy" % w), ref["cm"]), name


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
        p.viterbi_marginals()
    assert e.value.code == _lib.GH_ERR_ARG
    assert [_state(h) for h in hs] == before
    big.L = 6                                                   # the cap itself is served
    got = p.viterbi_marginals()
    assert [r["hole_at"] for r in got] == [0, 0, 0] and big.viterbi_info()[:3] == (4, 6, CAP)
    _equal(got[0], _win("a3")[1], "a3")
    _equal(got[1], _win("a4_6")[1], "a4_6")
    fresh = Hansel(t4.n_snps, band=t4.band)
    with pytest.raises(_lib.GretelHipError, match="window 1: .*before any fill") as e:
        HanselPanel([ok[1], fresh]).viterbi_marginals()
    assert e.value.code == _lib.GH_ERR_STATE
    hz = [make_pair(t4, L=3, offer_zero=True)[0] for _ in range(2)]
    with pytest.raises(_lib.GretelHipError, match="window 0: .*offer_zero") as e:
        HanselPanel(hz).viterbi_marginals()
    assert e.value.code == _lib.GH_ERR_ARG
    # null arguments and a negative offset through ctypes
    n = len(hs)
    n1 = [h.n + 1 for h in hs]
    mm, cm = np.zeros((sum(n1), 7)), np.zeros(sum(n1), dtype=np.uint8)
    off = np.zeros(n, dtype=np.int64)
    off[1:] = np.cumsum(n1[:-1])
    hole = np.full(n, -1, dtype=np.int32)
    args = [p._b, mm.ctypes.data, cm.ctypes.data, off.ctypes.data, hole.ctypes.data]
    for q in range(5):
        a = list(args)
        a[q] = None
        assert L.gh_panel_viterbi_marginals(*a) == _lib.GH_ERR_ARG, q
    neg = off.copy()
    neg[2] = -1
    a = list(args)
    a[3] = neg.ctypes.data
    assert L.gh_panel_viterbi_marginals(*a) == _lib.GH_ERR_ARG and b"negative offset" in L.gh_last_error()
    assert hole.tolist() == [-1] * n and not mm.any()
    assert L.gh_panel_viterbi_marginals(*args) == _lib.GH_OK and hole.tolist() == [0] * n
    assert np.array_equal(mm[off[2]:], got[2]["mm"]) and np.array_equal(cm[:n1[0]], got[0]["cm"])
    info = np.zeros(4, dtype=np.int64)
    assert L.gh_panel_viterbi_marginals_info(None, info.ctypes.data) == _lib.GH_ERR_ARG
    assert L.gh_panel_viterbi_marginals_info(p._b, None) == _lib.GH_ERR_ARG
    assert L.gh_panel_viterbi_marginals_info(p._b, info.ctypes.data) == _lib.GH_OK and info[0] == n and info[1] == 0


def _files(d):
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("exact", [[], ["--exact"]], ids=["greedy", "exact"])
def test_cli_margins(exact, tmp_path, capsys):
    regions = [("r1", 0, 20), ("r2", 0, 15), ("r3", 0, 12)]                            # (SNPs at 1, 2, 10 and 20)
    bed = tmp_path / "r.bed"
    bed.write_text("".join("hoot\t%d\t%d\t%s\n" % (a, b, n) for n, a, b in regions))
    out, plain = tmp_path / "panel", tmp_path / "plain"
    opts = ["-p", "6"] + exact
    assert panel.main([BAM, VCF, str(bed), "-o", str(plain)] + opts) == 0
    assert panel.main([BAM, VCF, str(bed), "-o", str(out)] + opts + ["--margins"]) == 0
    for name, a, b in regions:
        single = tmp_path / "single" / name
        single.mkdir(parents=True)
        assert cmd.main([BAM, VCF, "hoot", "-s", str(a + 1), "-e", str(b), "--quiet", "-o", str(single)] + opts + ["--margins"]) == 0
        with_m, without = _files(out / name), _files(plain / name)
        assert with_m.pop("gretel.margins") == (single / "gretel.margins").read_bytes(), name
        assert with_m == without and "out.fasta" in without, name
    capsys.readouterr()


def test_cli_margins_leaves_a_region_over_the_cap_without_the_file(tmp_path, capsys, monkeypatch):
    # (the construction of tests/test_gpu_panel_viterbi.py: table a4's BAM, the whole contig one region with its filled L set to 7)
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
    opts = ["-p", "4"]
    assert panel.main([bam, vcf, str(bed), "-o", str(out)] + opts + ["--margins"]) == 0
    cap = capsys.readouterr()
    assert cap.err.count("whole: [NOTE] --margins:") == 1 and cap.err.count("[NOTE] --margins:") == 1
    assert "16384 states, more than the 4096" in cap.err
    assert [x.split("\t")[0] for x in cap.out.splitlines()] == ["five", "whole", "six"]
    assert "out.fasta" in os.listdir(out / "whole") and "gretel.margins" not in os.listdir(out / "whole")
    monkeypatch.setattr(util, "load_from_bam", load)
    for name, a, b in (regions[0], regions[2]):
        single = tmp_path / "single" / name
        single.mkdir(parents=True)
        assert cmd.main([bam, vcf, contig, "-s", str(a + 1), "-e", str(b), "--quiet", "-o", str(single)] + opts + ["--margins"]) == 0
        for f in ("out.fasta", "snp.fasta", "gretel.crumbs", "gretel.margins"):
            assert (out / name / f).read_bytes() == (single / f).read_bytes(), (name, f)
    capsys.readouterr()
