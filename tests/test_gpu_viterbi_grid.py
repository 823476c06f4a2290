"""The grid decoder on the GPU (gh_viterbi_path_grid, gh_viterbi_spin_grid, gh_viterbi_grid_info; Hansel.viterbi_path_grid /
viterbi_spin_grid / viterbi_grid_info / viterbi_grid_bytes; --exact-grid of gretel_amd.cmd): exact decoding with the score rows in
device memory and a launch per SNP, for up to 2^24 states.  Where the LDS decoder serves a window the grid decoder is held to it,
beyond its cap to the plain statement of the definition (tests/viterbi_ref.py over the C oracle), and at the fill's own L = 10 --
where no plain reference is feasible -- to gh_score_paths and the beam.  Paths and scores are compared exactly."""
import ctypes as C
import functools

import numpy as np
import pytest

import decode_cases
import decode_checks
import viterbi_ref
from decode_util import BAM, E_MT, VCF, _from_haps, _same_spin, _table
from gretel_amd import _lib, cmd
from gretel_amd.hansel import Hansel
from spec_util import make_pair, same, spec_id

pytestmark = pytest.mark.gpu
CAP = _lib.GH_VITERBI_MAX_STATES
GRID_CAP = _lib.GH_VITERBI_GRID_MAX_STATES


def _same_path(got, ref):
    assert got["hole_at"] == ref["hole_at"], (got["hole_at"], ref["hole_at"])
    if ref["hole_at"]:
        assert got["path"] is None and got["ll_chain"] is None
        return
    assert got["ll_chain"] == ref["ll_chain"], (got["ll_chain"], ref["ll_chain"])
    assert got["path"].dtype == np.uint8 and np.array_equal(got["path"], ref["path"]), np.argwhere(got["path"] != ref["path"])[:4].tolist()


def _held(build):
    """build() -> a fresh handle.  The grid decoder against the LDS decoder on one handle, and what must hold around the call."""
    h = build()
    before = h.export_band()
    stats = (h.L, h.n_slices, h.n_crumbs)
    assert h.viterbi_grid_info() == (0, 0, 0, 0)
    lds = h.viterbi_path()
    got = h.viterbi_path_grid()
    _same_path(got, lds)
    assert h.viterbi_grid_info()[:3] == h.viterbi_info()[:3]
    assert np.array_equal(h.export_band(), before) and (h.L, h.n_slices, h.n_crumbs) == stats
    same(h.spin(4), build().spin(4))
    return h, got


SPECS = [{}, E_MT, dict(cond_mode="C"), dict(storage="f64"), dict(cand_order="T-GCA")]
HELD = [("a", kw, L) for kw in SPECS for L in (1, 2, 3, 5)] + [("a4", {}, 6), ("b", {}, 3), ("C2", {}, 3)]


@pytest.mark.parametrize("which,kw,L", HELD, ids=lambda v: v if isinstance(v, str) else (spec_id(v) if isinstance(v, dict) else "L%s" % v))
def test_held_to_the_lds_decoder(which, kw, L):
    t = _table(which)
    h, got = _held(lambda: make_pair(t, L=L, **kw)[0])
    S = 4 if which in ("a4", "C2") else 5
    s, le, states, scratch = h.viterbi_grid_info()
    assert (s, le, states) == (S, L, S ** L) and states <= CAP and got["hole_at"] == 0
    assert scratch == h.viterbi_grid_bytes() >= (t.n_snps + 1) * states + 16 * states + t.n_snps * (30 * L + 6) * 8
    if which == "C2":
        assert t.n_snps == 1000                              # a thousand launches on the stream, no wait between them


def test_held_to_the_lds_decoder_on_small_windows():
    # N < L: Le = N, the whole window is warm-up
    h, _ = _held(lambda: _from_haps(["ACGTAC", "CGTACG", "ACTTAG", "AGTTAC"], band=6, L=9)[0])
    assert h.viterbi_grid_info()[:3] == (4, 6, 4096)
    h, _ = _held(lambda: _from_haps(["AC", "CA", "AA"], band=1, L=5, **E_MT)[0])
    assert h.viterbi_grid_info()[:3] == (2, 2, 4)
    # one symbol: one state whatever L is, also beyond the 24 lags the mask words hold
    h, got = _held(lambda: _from_haps(["A" * 34, "A" * 34], band=4, L=30)[0])
    assert h.viterbi_grid_info()[:3] == (1, 30, 1) and got["path"].tolist() == [6] + [0] * 34


@pytest.mark.parametrize("at", [1, 4, 8])
def test_held_to_the_lds_decoder_at_a_hole(at):
    h, got = _held(lambda: _from_haps(["ACGTACGT", "CGTACGTA", "ACTTAGGT"], band=3, L=3, skip=(at,))[0])
    assert got == dict(path=None, ll_chain=None, hole_at=at)
    res = h.viterbi_spin_grid(5)
    assert res["n"] == 0 and res["hole_at"] == at and res["paths"].shape == (0, 9)


# the seeded windows -------------------------------------------------------------------------------------------------------------
BEYOND = (35, 78, 146, 155, 176, 177, 186)    # one lag beyond the LDS decoder's cap on purpose: 6 561, 16 384 or 15 625 states
BLOCK = 24


@pytest.mark.parametrize("first", range(0, len(decode_cases.CASES), BLOCK))
def test_the_seeded_windows_against_the_reference(first):
    for seed in decode_cases.CASES[first:first + BLOCK]:
        desc, t = decode_cases.case(seed)
        ref = viterbi_ref.viterbi(decode_cases.oracle_of(desc, t), desc["N"], desc["spec"]["cand_order"])
        h, _ = decode_checks.pair_of(desc, t)
        try:
            _same_path(h.viterbi_path_grid(), ref)
            s, le, states = h.viterbi_states()
            assert states <= GRID_CAP
            if seed in BEYOND:
                assert desc["beyond"] and CAP < states <= 16384, states
                with pytest.raises(_lib.GretelHipError, match="states"):
                    h.viterbi_path()
            if states:
                assert h.viterbi_grid_info()[:3] == (s, le, states)
        except AssertionError as e:
            raise AssertionError("seed %d %r: %s" % (seed, desc, e)) from e


def test_the_seeds_beyond_the_lds_cap_are_in_the_list():
    beyond = [seed for seed in decode_cases.CASES if decode_cases.case(seed)[0]["beyond"]]
    assert set(BEYOND) <= set(beyond)


# dense windows beyond the LDS cap ---------------------------------------------------------------------------------------------------
DENSE = [(2001, 16, 13, "AC", {}, 8192), (2002, 20, 14, "GT", {}, 16384), (2003, 14, 6, "ACGT-", {}, 15625), (2004, 14, 7, "ACGT", E_MT, 16384),
         (2005, 12, 9, "ACG", dict(cand_order="T-GCA"), 19683)]


def _dense_pair(seed, n, L, alpha, kw):
    rng = np.random.default_rng(seed)
    haps = ["".join(rng.choice(list(alpha), n)) for _ in range(12)]
    return _from_haps(haps, band=n, L=L, **kw)


@functools.lru_cache(maxsize=None)
def _dense_ref(seed):
    """The reference on the window as filled: computed once, shared, never changed."""
    _, n, L, alpha, kw, _ = next(c for c in DENSE if c[0] == seed)
    _, o = _dense_pair(seed, n, L, alpha, kw)
    return viterbi_ref.viterbi(o, n, kw.get("cand_order", "ACGT-"))


@pytest.mark.parametrize("seed,n,L,alpha,kw,states", DENSE, ids=lambda v: str(v) if isinstance(v, (int, str)) else spec_id(v))
def test_dense_windows_beyond_the_lds_cap(seed, n, L, alpha, kw, states):
    h, _ = _dense_pair(seed, n, L, alpha, kw)
    ref = _dense_ref(seed)
    assert ref["hole_at"] == 0 and np.isfinite(ref["ll_chain"])
    with pytest.raises(_lib.GretelHipError, match="states"):
        h.viterbi_path()
    before = h.export_band()
    got = h.viterbi_path_grid()
    print("seed %d: grid %r reference %r" % (seed, got["ll_chain"], ref["ll_chain"]))
    _same_path(got, ref)
    assert h.viterbi_grid_info()[:3] == (len(alpha), L, states) and states > CAP
    assert h.viterbi_grid_info()[3] == h.viterbi_grid_bytes()
    sc = h.score_paths([got["path"]])
    assert sc["ll_chain"][0] == got["ll_chain"] and sc["n_on"][0] == n
    assert np.array_equal(h.export_band(), before)


# the fill's own L -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,states", [("a4", 1048576), ("a", 9765625)])
def test_the_fills_own_L(which, states):
    t = _table(which)
    h, _ = make_pair(t)
    assert h.L == 10 and t.n_snps == 60
    before = h.export_band()
    want = h.viterbi_grid_bytes()
    got = h.viterbi_path_grid()
    assert got["hole_at"] == 0
    sc = h.score_paths([got["path"]])
    print("%s: grid %r score_paths %r" % (which, got["ll_chain"], sc["ll_chain"][0]))
    assert sc["ll_chain"][0] == got["ll_chain"] and sc["n_on"][0] == 60
    assert got["ll_chain"] >= h.beam_paths(32)["ll_chain"][0]
    assert np.array_equal(h.export_band(), before)
    info = h.viterbi_grid_info()
    assert info[:3] == (4 if which == "a4" else 5, 10, states) and info[3] == want
    assert abs(want / 1e9 - (0.08 if which == "a4" else 0.75)) < 0.01


# the spin -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,L", [("a", 3), ("C2", 2)])
def test_the_spin_against_the_lds_decoders(which, L):
    t = _table(which)
    res = make_pair(t, L=L)[0].viterbi_spin_grid(6)
    ref = make_pair(t, L=L)[0].viterbi_spin(6)
    assert res["n"] == 6
    for k in ("paths", "ll_chain", "min_marginal"):
        assert np.array_equal(res[k], ref[k]), k
    _same_spin(res, ref)


def test_the_spin_against_the_reference_beyond_the_lds_cap():
    seed, n, L, alpha, kw, _ = DENSE[2]
    h, o = _dense_pair(seed, n, L, alpha, kw)
    res = h.viterbi_spin_grid(3)
    ref = viterbi_ref.viterbi_spin(o, n, 3)
    assert ref["n"] == 3 and res["ll_chain"][0] == _dense_ref(seed)["ll_chain"]
    _same_spin(res, ref)
    assert np.array_equal(h.export_band(), o.export_band())


# refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    t = _table("a4")
    h, _ = make_pair(t, L=3)
    L = _lib.load()
    path = np.zeros(t.n_snps + 1, dtype=np.uint8)
    ll, n, hole = C.c_double(), C.c_int(), C.c_int()

    def call(hh, p=path, pll=C.byref(ll), ph=C.byref(hole)):
        return L.gh_viterbi_path_grid(hh._h if hh is not None else None, p.ctypes.data if p is not None else None, pll, ph)

    assert call(None) == _lib.GH_ERR_ARG and call(h, None) == _lib.GH_ERR_ARG
    assert call(h, pll=None) == _lib.GH_ERR_ARG and call(h, ph=None) == _lib.GH_ERR_ARG
    assert call(h) == _lib.GH_OK and hole.value == 0
    paths = np.zeros((4, t.n_snps + 1), dtype=np.uint8)
    recs = np.zeros((4, 5))
    spin = lambda hh, k, r=recs: L.gh_viterbi_spin_grid(hh._h, k, 0.01, paths.ctypes.data, r.ctypes.data if r is not None else None, None,
                                                        C.byref(n), C.byref(hole))
    assert spin(h, -1) == _lib.GH_ERR_ARG and b"max_paths" in L.gh_last_error()
    assert spin(h, 1, None) == _lib.GH_ERR_ARG
    assert spin(h, 0) == _lib.GH_OK and n.value == 0
    hz, _ = make_pair(t, L=3, offer_zero=True)
    assert call(hz) == _lib.GH_ERR_ARG and b"offer_zero" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="offer_zero"):
        hz.viterbi_spin_grid(3)
    fresh = Hansel(t.n_snps, band=t.band)
    assert call(fresh) == _lib.GH_ERR_STATE and b"before any fill" in L.gh_last_error()
    info = np.full(4, -1, dtype=np.int64)
    assert L.gh_viterbi_grid_info(fresh._h, info.ctypes.data) == _lib.GH_OK and info.tolist() == [0, 0, 0, 0]
    assert L.gh_viterbi_grid_info(None, info.ctypes.data) == _lib.GH_ERR_ARG
    assert L.gh_viterbi_grid_info(fresh._h, None) == _lib.GH_ERR_ARG
    # 2^25 states: one lag beyond the grid's cap
    rng = np.random.default_rng(25)
    haps = ["".join(rng.choice(list("AC"), 26)) for _ in range(4)]
    hb, _ = _from_haps(haps, band=2, L=25)
    big = np.zeros(27, dtype=np.uint8)
    assert hb.viterbi_states() == (2, 25, 1 << 25)           # (and the staged observations are on the device)
    assert call(hb, big) == _lib.GH_ERR_ARG
    msg = L.gh_last_error()
    assert b"S = 2 " in msg and b"= 25 make 33554432 states" in msg and b"16777216" in msg and b"--beam" in msg
    assert hb.viterbi_grid_info() == (0, 0, 0, 0)           # nothing was allocated for it, no call is on record
    assert hb.viterbi_grid_bytes() == 0
    with pytest.raises(_lib.GretelHipError, match="33554432 states") as e:
        hb.viterbi_spin_grid(2)
    assert e.value.code == _lib.GH_ERR_ARG
    hb.L = 24                                                # ... and viterbi_states says what the cap itself would take
    assert hb.viterbi_states() == (2, 24, GRID_CAP) and hb.viterbi_grid_bytes() > 27 * GRID_CAP


# the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_exact_grid(tmp_path, capsys):
    out, want, both = tmp_path / "out", tmp_path / "want", tmp_path / "both"
    for d in (out, want, both):
        d.mkdir()
    argv = [BAM, VCF, "hoot", "-s", "1", "-e", "20", "-p", "12", "--score-paths", "--quiet"]
    assert cmd.main(argv + ["-o", str(want), "--exact"]) == 0
    assert "--exact-grid" not in capsys.readouterr().err
    assert cmd.main(argv + ["-o", str(out), "--exact-grid"]) == 0
    err = capsys.readouterr().err
    v = cmd.util.process_vcf(VCF, "hoot", 1, 20)
    h = cmd.util.load_from_bam(BAM, "hoot", 1, 20, v)
    s, le, states = h.viterbi_states()
    assert "[NOTE] --exact-grid: S = %d candidate symbols, Le = %d: %d states, %d bytes of device scratch\n" % (s, le, states, h.viterbi_grid_bytes()) in err
    files = ("out.fasta", "snp.fasta", "gretel.crumbs", "gretel.scores")
    for f in files:
        assert (out / f).read_bytes() == (want / f).read_bytes(), f
    assert len((out / "gretel.scores").read_text().splitlines()) > 1
    assert cmd.main(argv + ["-o", str(both), "--exact", "--exact-grid"]) == 0
    assert "[NOTE] --exact-grid: " in capsys.readouterr().err
    for f in files:
        assert (both / f).read_bytes() == (want / f).read_bytes(), f


def test_cli_exact_grid_refusals(tmp_path, capsys):
    out = tmp_path / "out"
    assert cmd.main([str(tmp_path / "no_such.bam"), VCF, "hoot", "-s", "1", "-e", "20", "-o", str(out), "--exact-grid", "--beam", "4"]) == 2
    assert capsys.readouterr().err.startswith("[FAIL] --exact ")
    assert not out.exists()
