"""Exact decoding of the chain likelihood on the GPU (gh_viterbi_path, gh_viterbi_spin, gh_viterbi_info; Hansel.viterbi_path /
viterbi_spin / viterbi_info; --exact of gretel_amd.cmd) against the plain statement of the definition (tests/viterbi_ref.py over
the C oracle).  Paths and scores are compared exactly -- the order of every addition and every comparison is fixed; only the
removed mass of a reweight goes through spec_util.same's relative 1e-10, as everywhere."""
import ctypes as C
import io
import itertools
import types

import numpy as np
import pytest

import score_ref
import viterbi_ref
from decode_util import BAM, E_MT, SYMS, VCF, _cli_oracle, _from_haps, _same_spin, _table
from gretel_amd import _lib, cmd
from gretel_amd.hansel import Hansel
from spec_util import make_pair, same, spec_id

pytestmark = pytest.mark.gpu
CAP = _lib.GH_VITERBI_MAX_STATES


def _str(path):
    return "".join(SYMS[int(v)] for v in path[1:])


def _check(h, o):
    """viterbi_path of `h` against viterbi_ref over `o`, and against gh_score_paths on the same handle; returns the GPU's dict."""
    n = h.n
    got = h.viterbi_path()
    ref = viterbi_ref.viterbi(o, n, h._cfg["cand_order"])
    assert got["hole_at"] == ref["hole_at"]
    if ref["hole_at"]:
        assert got["path"] is None and got["ll_chain"] is None
        return got
    assert got["path"].dtype == np.uint8 and got["path"].shape == (n + 1,)
    assert got["ll_chain"] == ref["ll_chain"], (got["ll_chain"], ref["ll_chain"])
    assert np.array_equal(got["path"], ref["path"]), np.argwhere(got["path"] != ref["path"])[:4].tolist()
    sc = h.score_paths([got["path"]])
    assert sc["ll_chain"][0] == got["ll_chain"] and sc["n_on"][0] == n
    return got


def _consistent(h, t, got, spin_kw):
    """What must hold on the handle around an exact decoding: the beam never above it, nothing disturbed."""
    wide, one = h.beam_paths(32), h.beam_paths(1)
    assert got["ll_chain"] >= wide["ll_chain"][0] >= one["ll_chain"][0]
    fresh, _ = make_pair(t, **spin_kw)
    res, ref = h.spin(4), fresh.spin(4)
    same(res, ref)
    assert np.array_equal(h.export_band(), fresh.export_band())


# (table, switches, L); the fill's own L (L = None) has its own test below: on the 60-SNP table it is 10, beyond the cap
SPECS = [{}, E_MT, dict(cond_mode="C"), dict(storage="f64"), dict(cand_order="T-GCA")]
CASES = [("a", kw, L) for kw in SPECS for L in (1, 2, 3, 5)] + [
    ("a4", {}, 6), ("a4", E_MT, 6),                          # 4096 states: the cap
    ("b", {}, 1), ("b", {}, 3), ("b", E_MT, 3),
    ("C2", {}, 2), ("C2", {}, 3), ("C2", dict(cand_order="T-GCA", **E_MT), 3),
]


@pytest.mark.parametrize("which,kw,L", CASES, ids=lambda v: v if isinstance(v, str) else (spec_id(v) if isinstance(v, dict) else "L%s" % v))
def test_viterbi_path_against_the_reference(which, kw, L):
    t = _table(which)
    h, o = make_pair(t, L=L, **kw)
    before = h.export_band()
    stats = (h.L, h.n_slices, h.n_crumbs)
    got = _check(h, o)
    S = 4 if which in ("a4", "C2") else 5
    s, le, states, scratch = h.viterbi_info()
    assert (s, le, states) == (S, L, S ** L) and states <= CAP
    assert scratch >= t.n_snps * states + t.n_snps * (30 * L + 6) * 8
    if which == "C2":
        assert t.n_snps > 512                               # the trace took its back-pointers through LDS in more than one chunk
    assert np.array_equal(h.export_band(), before) and np.array_equal(before, o.export_band())
    assert (h.L, h.n_slices, h.n_crumbs) == stats
    _consistent(h, t, got, dict(L=L, **kw))


@pytest.mark.parametrize("kw", SPECS, ids=spec_id)
def test_the_fills_own_L_is_beyond_the_cap_on_the_60_snp_table(kw):
    # (L = None: the fill sets L = 10 on this table, 5^10 states -- the decoder must refuse, and say what it would have taken)
    t = _table("a")
    h, _ = make_pair(t, **kw)
    assert h.L == 10
    with pytest.raises(_lib.GretelHipError, match=r"S = 5 .* Le = min\(L, N\) = 10 make 9765625 states.*--beam") as e:
        h.viterbi_path()
    assert e.value.code == _lib.GH_ERR_ARG
    assert h.beam_paths(4)["n"] == 4                         # ... where the beam still serves


def test_the_exact_path_beats_the_greedy_walk():
    h, o = make_pair(_table("a"))
    h.L = o.L = 3
    got = _check(h, o)
    greedy = h.generate_path()[0]
    g = h.score_paths([greedy])
    assert g["n_on"][0] == h.n and got["ll_chain"] > g["ll_chain"][0]
    r = h.score_paths([got["path"]])
    assert r["n_greedy"][0] < r["n_on"][0] == h.n           # it left the greedy choice somewhere
    h.L = o.L = 5
    assert _check(h, o)["ll_chain"] > h.score_paths([h.generate_path()[0]])["ll_chain"][0]


def test_exhaustive_on_the_device():
    haps = ["ACGTACGT", "CGTTAGCA", "AGCTTCGA"]
    n = 8
    h, o = _from_haps(haps, band=3, L=3)
    every = np.array([(6,) + x for x in itertools.product((0, 1, 2, 3), repeat=n)], dtype=np.uint8)
    assert len(every) == 4 ** 8
    sc = h.score_paths(every)
    on = sc["n_on"] == n
    assert 1 < on.sum() < len(every)
    top = sc["ll_chain"][on].max()
    got = _check(h, o)
    assert got["ll_chain"] == top
    best = {x.tobytes() for x in every[on & (sc["ll_chain"] == top)]}
    assert got["path"].tobytes() in best


def test_small_windows_and_warm_up():
    h, o = _from_haps(["A", "C", "C"], band=1, L=4)              # N = 1
    assert _check(h, o)["path"].tolist() == [6, 1]
    assert h.viterbi_info()[:3] == (2, 1, 2)
    h, o = _from_haps(["AC", "CA", "AA"], band=1, L=5, **E_MT)     # N = 2 < L
    _check(h, o)
    assert h.viterbi_info()[:3] == (2, 2, 4)
    for L in (6, 7, 9):                                          # L >= N: the whole window is warm-up, the state the whole prefix
        h, o = _from_haps(["ACGTAC", "CGTACG", "ACTTAG", "AGTTAC"], band=6, L=L)
        _check(h, o)
        assert h.viterbi_info()[:3] == (4, 6, 4096)
    # one position offers a single candidate (and the window three symbols in all)
    h, o = _from_haps(["ACGTACG", "CGGTACT", "AGGAAGG", "CCGTAGT"], band=3, L=3)
    _check(h, o)
    assert h.viterbi_info()[:3] == (4, 3, 64)
    # every position offers the same single candidate: one state, whatever L is
    h, o = _from_haps(["AAAAA", "AAAAA"], band=4, L=4)
    assert _str(_check(h, o)["path"]) == "AAAAA" and h.viterbi_info()[:3] == (1, 4, 1)


def test_a_biallelic_window_at_L_12():
    rng = np.random.default_rng(12)
    n = 16
    haps = ["".join("AG"[v] for v in rng.integers(0, 2, n)) for _ in range(6)]
    h, o = _from_haps(haps, band=12, L=12)
    _check(h, o)
    assert h.viterbi_info()[:3] == (2, 12, CAP)
    h.L = o.L = 13
    with pytest.raises(_lib.GretelHipError, match="S = 2 .* = 13 make 8192 states"):
        h.viterbi_path()


@pytest.mark.parametrize("at", [1, 4, 8])
def test_a_hole(at):
    h, o = _from_haps(["ACGTACGT", "CGTACGTA", "ACTTAGGT"], band=3, L=3, skip=(at,))
    got = _check(h, o)
    assert got == dict(path=None, ll_chain=None, hole_at=at)
    assert h.generate_path()[1] == at
    res = h.viterbi_spin(5)
    assert res["n"] == 0 and res["hole_at"] == at and res["paths"].shape == (0, 9)


@pytest.mark.parametrize("order", ["ACGT-", "T-GCA"])
def test_exact_ties(order):
    # two haplotypes with identical evidence tie exactly: the end rule takes the one whose last symbols come first in the order
    h, o = _from_haps(["ACACAC", "CACACA"], band=3, L=3, cand_order=order)
    assert _str(_check(h, o)["path"]) == ("CACACA" if order == "ACGT-" else "ACACAC")
    # ... and where two tied prefixes meet in one state (they differ at SNP 1 only), the one of smaller q(x[1]) stays
    h, o = _from_haps(["AGTTACG", "CGTTACG"], band=3, L=3, cand_order=order)
    assert _str(_check(h, o)["path"]) == ("AGTTACG" if order == "ACGT-" else "CGTTACG")


def test_refusals():
    t = _table("a4")
    h, _ = make_pair(t, L=7)
    L = _lib.load()
    path = np.zeros(t.n_snps + 1, dtype=np.uint8)
    ll, n, hole = C.c_double(), C.c_int(), C.c_int()

    def call(hh, p=path, pll=C.byref(ll), ph=C.byref(hole)):
        return L.gh_viterbi_path(hh._h if hh is not None else None, p.ctypes.data if p is not None else None, pll, ph)

    assert call(h) == _lib.GH_ERR_ARG                        # L = 7 without deletion columns
    msg = L.gh_last_error()
    assert b"S = 4 " in msg and b"= 7 make 16384 states" in msg and b"--beam" in msg
    with pytest.raises(_lib.GretelHipError, match="16384 states"):
        h.viterbi_path()
    with pytest.raises(_lib.GretelHipError, match="16384 states"):
        h.viterbi_spin(3)
    hd, _ = make_pair(_table("a"), L=6)                      # L = 6 with deletion columns
    assert call(hd) == _lib.GH_ERR_ARG
    msg = L.gh_last_error()
    assert b"S = 5 " in msg and b"= 6 make 15625 states" in msg
    # the cap itself is served, and viterbi_info says what it took
    h.L = 6
    assert call(h) == _lib.GH_OK and hole.value == 0
    s, le, states, scratch = h.viterbi_info()
    assert (s, le, states) == (4, 6, CAP) and scratch >= (t.n_snps + 1) * CAP + t.n_snps * (30 * 6 + 6) * 8
    assert call(None) == _lib.GH_ERR_ARG and call(h, None) == _lib.GH_ERR_ARG
    assert call(h, pll=None) == _lib.GH_ERR_ARG and call(h, ph=None) == _lib.GH_ERR_ARG
    paths = np.zeros((4, t.n_snps + 1), dtype=np.uint8)
    recs = np.zeros((4, 5))
    spin = lambda hh, k, r=recs: L.gh_viterbi_spin(hh._h, k, 0.01, paths.ctypes.data, r.ctypes.data if r is not None else None, None,
                                                   C.byref(n), C.byref(hole))
    assert spin(h, -1) == _lib.GH_ERR_ARG and spin(h, 1, None) == _lib.GH_ERR_ARG
    assert spin(h, 0) == _lib.GH_OK and n.value == 0
    hz, _ = make_pair(t, L=3, offer_zero=True)
    assert call(hz) == _lib.GH_ERR_ARG and b"offer_zero" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="offer_zero"):
        hz.viterbi_spin(3)
    fresh = Hansel(t.n_snps, band=t.band)
    assert call(fresh) == _lib.GH_ERR_STATE and b"before any fill" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="before any fill"):
        fresh.viterbi_path()
    info = np.full(4, -1, dtype=np.int64)
    assert L.gh_viterbi_info(fresh._h, info.ctypes.data) == _lib.GH_OK and info.tolist() == [0, 0, 0, 0]
    assert L.gh_viterbi_info(None, info.ctypes.data) == _lib.GH_ERR_ARG


@pytest.mark.parametrize("snapshot", [False, True], ids=["no-snapshot", "snapshot-before"])
@pytest.mark.parametrize("kw", [{}, E_MT], ids=spec_id)
def test_viterbi_spin(kw, snapshot):
    t = _table("a")
    h, o = make_pair(t, L=3, **kw)
    original = None
    if snapshot:
        # a snapshot taken earlier, on another tensor than the one the paths are found on: hp_original reads the frozen marginals
        h.snapshot_original()
        original = score_ref.marginals(o, t.n_snps)
        same(h.spin(2), o.spin(2))
    res = h.viterbi_spin(4)
    ref = viterbi_ref.viterbi_spin(o, t.n_snps, 4, original=original)
    assert ref["n"] == 4
    _same_spin(res, ref)
    assert np.array_equal(h.export_band(), o.export_band())


def test_cli_exact(tmp_path, capsys):
    out, want = tmp_path / "out", tmp_path / "want"
    out.mkdir()
    want.mkdir()
    assert cmd.main([BAM, VCF, "hoot", "-s", "1", "-e", "20", "-p", "12", "-o", str(out), "--exact", "--score-paths"]) == 0
    capsys.readouterr()
    v, n, h, o = _cli_oracle()
    ref = viterbi_ref.viterbi_spin(o, n, 12, cmd.MIN_REMOVE)
    unweighted = h.copy()
    res = h.viterbi_spin(12, cmd.MIN_REMOVE)                 # a handle filled the same way
    _same_spin(res, ref)
    assert res["n"] > 0
    capsys.readouterr()
    paths = cmd.paths_of_spin(h, ref, log=io.StringIO())
    args = types.SimpleNamespace(out=str(want), master=None, end=20, start=1, gapchar="N", delchar="")
    cmd.write_outputs(paths, h, v, args)
    for f in ("out.fasta", "snp.fasta", "gretel.crumbs"):
        assert (out / f).read_bytes() == (want / f).read_bytes(), f
    # gretel.scores is written against the matrix as the reads filled it: every line is the chain likelihood of an exact path
    # there, and the first path -- found on that very matrix -- scores the exact maximum
    keys = sorted(paths, key=lambda x: paths[x]["i_0"])
    rec = np.array([[s.i for s in paths[k]["hansel_path"]] for k in keys], dtype=np.uint8)
    sc = unweighted.score_paths(rec)
    assert (out / "gretel.scores").read_text() == cmd.scores_text((n, h.L, "A", 0), [paths[k]["i_0"] for k in keys], sc, v["snp_rev"])
    first = keys.index(next(k for k in keys if paths[k]["i_0"] == 0))
    assert sc["ll_chain"][first] == res["ll_chain"][0] == unweighted.viterbi_path()["ll_chain"]
    assert (sc["ll_chain"] <= res["ll_chain"][0]).all()


def test_cli_exact_refusals(tmp_path, capsys):
    out = tmp_path / "out"
    assert cmd.main([str(tmp_path / "no_such.bam"), VCF, "hoot", "-s", "1", "-e", "20", "-o", str(out), "--exact", "--beam", "4"]) == 2
    assert capsys.readouterr().err.startswith("[FAIL] --exact ")
    assert not out.exists()
