"""Beam search over the chain likelihood on the GPU (gh_beam_paths, gh_beam_spin, gh_beam_info; Hansel.beam_paths / beam_spin /
beam_info; --beam of gretel_amd.cmd) against the plain statement of the definition (tests/beam_ref.py over the C oracle).  Paths
and scores are compared exactly -- the order of every addition and every comparison is fixed; only the removed mass of a reweight
goes through spec_util.same's relative 1e-10, as everywhere."""
import ctypes as C
import io
import os
import types

import numpy as np
import pytest

import beam_ref
from decode_util import BAM, E_MT, SYMS, VCF, _cli_oracle, _from_haps, _same_spin, _table
from gretel_amd import _lib, cmd
from gretel_amd.hansel import Hansel
from gretel_amd.synth import make_support_table
from spec_util import make_pair, same, spec_id

pytestmark = pytest.mark.gpu


def _check(h, o, width):
    """beam_paths of `h` against beam_ref over `o`, and against gh_score_paths on the same handle; returns the GPU's dict."""
    n = h.n
    got = h.beam_paths(width)
    ref = beam_ref.beam(o, n, width, h._cfg["cand_order"])
    assert (got["n"], got["hole_at"]) == (ref["n"], ref["hole_at"])
    if ref["hole_at"]:
        assert got["paths"].shape == (0, n + 1) and len(got["ll_chain"]) == 0
        assert got["prefix"].tolist() == ref["prefix"].tolist()
        return got
    assert got["paths"].dtype == np.uint8 and got["ll_chain"].dtype == np.float64
    assert np.array_equal(got["paths"], ref["paths"]), (width, np.argwhere(got["paths"] != ref["paths"])[:4].tolist())
    assert got["ll_chain"].tolist() == ref["ll_chain"]
    sc = h.score_paths(got["paths"])
    assert sc["ll_chain"].tolist() == got["ll_chain"].tolist() and (sc["n_on"] == n).all()
    if width == 1:
        assert np.array_equal(got["paths"][0], h.generate_path()[0])
    return got


# (table, switches, L or None = the fill's own, widths)
CASES = [
    ("b", {}, 3, (1, 2, 5, 8, 32)),
    ("b", {}, 1, (1, 8)),
    ("b", {}, None, (1, 8)),
    ("b", {}, 16, (1, 8)),
    ("b", {}, 17, (1, 8)),
    ("b", {}, 20, (1, 8, 32)),
    ("a", E_MT, None, (1, 2, 5, 8, 32)),
    ("a", dict(cond_mode="C"), 3, (1, 8)),
    ("a", dict(storage="f64"), 16, (1, 8)),
    ("a", dict(cand_order="T-GCA"), None, (1, 5, 8)),
    ("a", E_MT, 20, (1, 8)),
    ("C2", {}, None, (1, 8)),
    ("C2", dict(cand_order="T-GCA", **E_MT), 3, (2, 32)),
]


@pytest.mark.parametrize("which,kw,L,widths", CASES, ids=lambda v: v if isinstance(v, str) else (spec_id(v) if isinstance(v, dict) else str(v)))
def test_beam_paths_against_the_reference(which, kw, L, widths):
    t = _table(which)
    h, o = make_pair(t, L=L, **kw)
    before = h.export_band()
    for width in widths:
        got = _check(h, o, width)
        assert got["n"] == width
        staged, ring, threads, scratch = h.beam_info()
        assert threads == max(64, 8 * width) and scratch >= t.n_snps * (30 * min(h.L, t.n_snps) + 6) * 8
        if L == 3:
            assert staged == 1
            if which == "b":
                assert t.n_snps / ring >= 3                 # the LDS ring went round at least three times
        if L == 20:
            assert (staged, ring) == (0, 0)
    assert np.array_equal(h.export_band(), before) and np.array_equal(before, o.export_band())


def test_a_beam_finds_what_the_greedy_walk_misses():
    h, o = make_pair(_table("a"))
    greedy, wide = _check(h, o, 1), _check(h, o, 4)
    assert wide["ll_chain"][0] > greedy["ll_chain"][0]
    assert (np.diff(wide["ll_chain"]) <= 0).all()
    r = h.score_paths(wide["paths"][0])
    assert r["n_greedy"][0] < r["n_on"][0] == h.n           # it left the greedy choice somewhere


@pytest.mark.parametrize("order", ["ACGT-", "TG-CA"])
@pytest.mark.parametrize("haps", [["ACACACAC", "CACACACA"], ["ACGTACGT", "CGTACGTA", "GTACGTAC", "TACGTACG"]], ids=["two", "four"])
def test_exact_ties(haps, order):
    # haplotypes with identical evidence: their scores tie exactly, the parent rank, the weight and cand_order decide
    h, o = _from_haps(haps, band=3, L=3, cand_order=order)
    for width in (1, 2, 3, 8):
        got = _check(h, o, width)
        if width >= len(haps):
            assert len(set(got["ll_chain"][:len(haps)].tolist())) == 1
            first = [SYMS[int(x)] for x in got["paths"][:len(haps), 1]]
            assert first == sorted(first, key=order.index)


def test_small_windows():
    h, o = _from_haps(["AC", "CA", "AA"], band=1, L=5, **E_MT)     # N = 2 < L, fewer paths than the width
    got = _check(h, o, 32)
    assert 1 < got["n"] < 32
    _check(h, o, 1)
    h, o = _from_haps(["A", "C", "C"], band=1, L=4)              # N = 1
    assert _check(h, o, 8)["n"] == 2
    assert _check(h, o, 1)["paths"].tolist() == [[6, 1]]


def test_a_hole_mid_window():
    h, o = _from_haps(["ACGTACGT", "CGTACGTA", "ACTTAGGT"], band=3, L=3, skip=(4,))
    for width in (1, 4):
        got = _check(h, o, width)
        assert got["n"] == 0 and got["hole_at"] == 4 and len(got["prefix"]) == 4 and got["prefix"][0] == 6
    assert h.generate_path()[1] == 4
    res = h.beam_spin(4, 5)
    assert res["n"] == 0 and res["hole_at"] == 4 and res["paths"].shape == (0, 9)


def test_mid_recovery_and_nothing_disturbed():
    t = _table("b")
    h, o = make_pair(t)
    same(h.spin(10), o.spin(10))
    band = h.export_band()
    assert (band != np.floor(band)).any()                   # reweighted, non-integer cells
    stats = (h.L, h.n_slices, h.n_crumbs)
    for width in (4, 8):
        _check(h, o, width)
    assert np.array_equal(h.export_band(), band) and (h.L, h.n_slices, h.n_crumbs) == stats
    same(h.spin(10), o.spin(10))                            # the beam disturbed nothing
    assert np.array_equal(h.export_band(), o.export_band())


@pytest.mark.parametrize("kw", [{}, E_MT], ids=spec_id)
def test_beam_spin_width_8(kw):
    t = _table("a")
    h, o = make_pair(t, **kw)
    res = h.beam_spin(8, 10)
    ref = beam_ref.beam_spin(o, t.n_snps, 8, 10)
    assert ref["n"] == 10
    _same_spin(res, ref)
    assert np.array_equal(h.export_band(), o.export_band())


def test_beam_spin_width_1_is_spin():
    t = _table("b")
    h, o = make_pair(t)
    h2, _ = make_pair(t)
    res, ref = h.beam_spin(1, 10), h2.spin(10)
    same(res, ref)
    assert res["min_marginal"].tolist() == ref["min_marginal"].tolist()
    assert np.array_equal(h.export_band(), h2.export_band())
    # (the first path was found on the tensor as filled: its beam score is its ll_chain there)
    fresh, _ = make_pair(t)
    assert res["ll_chain"].shape == (10,) and res["ll_chain"][0] == fresh.score_paths(res["paths"][0])["ll_chain"][0]


def test_refusals():
    t = make_support_table(100, 500, k=4, seed=3)
    h, _ = make_pair(t)
    L = _lib.load()
    paths = np.zeros((32, t.n_snps + 1), dtype=np.uint8)
    ll = np.zeros(32)
    n, hole = C.c_int(), C.c_int()

    def call(hh, width, p=paths):
        return L.gh_beam_paths(hh._h if hh is not None else None, width, p.ctypes.data if p is not None else None, ll.ctypes.data,
                               C.byref(n), C.byref(hole))

    assert call(h, 2) == _lib.GH_OK and n.value == 2
    assert L.gh_beam_paths(h._h, 2, paths.ctypes.data, None, C.byref(n), C.byref(hole)) == _lib.GH_OK      # ll_chain may be NULL
    for width in (0, 33, -1):
        assert call(h, width) == _lib.GH_ERR_ARG and b"width" in L.gh_last_error()
        with pytest.raises(_lib.GretelHipError):
            h.beam_paths(width)
    assert call(None, 2) == _lib.GH_ERR_ARG and call(h, 2, None) == _lib.GH_ERR_ARG
    assert L.gh_beam_paths(h._h, 2, paths.ctypes.data, ll.ctypes.data, None, C.byref(hole)) == _lib.GH_ERR_ARG
    recs = np.zeros((4, 5))
    assert L.gh_beam_spin(h._h, 2, -1, 0.01, paths.ctypes.data, recs.ctypes.data, None, C.byref(n), C.byref(hole)) == _lib.GH_ERR_ARG
    assert L.gh_beam_spin(h._h, 0, 2, 0.01, paths.ctypes.data, recs.ctypes.data, None, C.byref(n), C.byref(hole)) == _lib.GH_ERR_ARG
    assert L.gh_beam_spin(h._h, 2, 0, 0.01, paths.ctypes.data, recs.ctypes.data, None, C.byref(n), C.byref(hole)) == _lib.GH_OK and n.value == 0
    hz, _ = make_pair(t, offer_zero=True)
    assert call(hz, 2) == _lib.GH_ERR_ARG and b"offer_zero" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError):
        hz.beam_spin(2, 3)
    fresh = Hansel(t.n_snps, band=t.band)
    assert call(fresh, 2) == _lib.GH_ERR_STATE and b"before any fill" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError):
        fresh.beam_paths(2)
    info = np.full(4, -1, dtype=np.int64)
    assert L.gh_beam_info(fresh._h, info.ctypes.data) == _lib.GH_OK and info.tolist() == [0, 0, 0, 0]
    assert L.gh_beam_info(None, info.ctypes.data) == _lib.GH_ERR_ARG


def test_cli_beam_1_writes_what_no_flag_writes(tmp_path, capsys):
    argv = [BAM, VCF, "hoot", "-s", "1", "-e", "20", "-p", "12"]
    plain, beam = tmp_path / "plain", tmp_path / "beam"
    plain.mkdir()
    beam.mkdir()
    assert cmd.main(argv + ["-o", str(plain)]) == 0
    cap0 = capsys.readouterr()
    assert cmd.main(argv + ["-o", str(beam), "--beam", "1"]) == 0
    cap1 = capsys.readouterr()
    assert cap0.out == cap1.out and cap0.err == cap1.err
    for f in ("out.fasta", "snp.fasta", "gretel.crumbs"):
        assert (plain / f).read_bytes() == (beam / f).read_bytes(), f
    assert sorted(os.listdir(beam)) == sorted(os.listdir(plain))


def test_cli_beam_8_against_the_reference(tmp_path, capsys):
    out, want = tmp_path / "out", tmp_path / "want"
    out.mkdir()
    want.mkdir()
    assert cmd.main([BAM, VCF, "hoot", "-s", "1", "-e", "20", "-p", "12", "-o", str(out), "--beam", "8", "--score-paths"]) == 0
    capsys.readouterr()
    v, n, h, o = _cli_oracle()
    ref = beam_ref.beam_spin(o, n, 8, 12, cmd.MIN_REMOVE)
    capsys.readouterr()
    paths = cmd.paths_of_spin(h, ref, log=io.StringIO())
    args = types.SimpleNamespace(out=str(want), master=None, end=20, start=1, gapchar="N", delchar="")
    cmd.write_outputs(paths, h, v, args)
    for f in ("out.fasta", "snp.fasta", "gretel.crumbs"):
        assert (out / f).read_bytes() == (want / f).read_bytes(), f
    keys = sorted(paths, key=lambda x: paths[x]["i_0"])
    rec = np.array([[s.i for s in paths[k]["hansel_path"]] for k in keys], dtype=np.uint8)
    assert (out / "gretel.scores").read_text() == cmd.scores_text((n, h.L, "A", 0), [paths[k]["i_0"] for k in keys], h.score_paths(rec), v["snp_rev"])
