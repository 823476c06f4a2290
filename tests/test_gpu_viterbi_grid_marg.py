"""Max-marginals on the grid on the GPU (gh_viterbi_marginals_grid; Hansel.viterbi_marginals_grid / viterbi_marginals_grid_bytes;
--margins-grid of gretel_amd.cmd): gh_viterbi_marginals' definition with one kept row of F per SNP in device memory and a launch
per SNP each way, for up to 2^24 states.  Where the LDS call serves a window the grid call is held to it, beyond its cap to the
plain statement of the definition (tests/maxmarg_ref.py over the C oracle), and at the fill's own L = 10 -- where no plain
reference is feasible -- to identities against gh_viterbi_path_grid and gh_score_paths.  mm and cm are compared as IEEE values."""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest

import decode_cases
import decode_checks
import maxmarg_ref
from decode_util import BAM, E_MT, VCF, _from_haps, _table
from gretel_amd import _lib, cmd
from gretel_amd.hansel import Hansel, grid_marginals_scratch_bytes, margins_of
from spec_util import make_pair, same, spec_id

pytestmark = pytest.mark.gpu
CAP = _lib.GH_VITERBI_MAX_STATES
GRID_CAP = _lib.GH_VITERBI_GRID_MAX_STATES


def _same(got, ref, n):
    decode_checks.same_marginals(got, ref, n)
    if not ref["hole_at"]:
        assert got["cm"].dtype == np.uint8 and got["cm"].shape == (n + 1,) and got["cm"][0] == 0
        assert (got["mm"][0] == -np.inf).all()


def _held(build):
    """build() -> a fresh handle.  The grid call against the LDS call on one handle, and what must hold around it."""
    h = build()
    before = h.export_band()
    stats = (h.L, h.n_slices, h.n_crumbs)
    assert h.viterbi_grid_info() == (0, 0, 0, 0)
    lds = h.viterbi_marginals()
    info = h.viterbi_info()
    got = h.viterbi_marginals_grid()
    _same(got, lds, h.n)
    assert h.viterbi_info() == info                          # gh_viterbi_info is not touched
    assert h.viterbi_grid_info()[:3] == info[:3]
    if not lds["hole_at"]:
        assert h.viterbi_grid_info()[3] == h.viterbi_marginals_grid_bytes()
        assert got["mm"][h.n].max() == h.viterbi_path_grid()["ll_chain"]       # B_N = +0.0
    assert np.array_equal(h.export_band(), before) and (h.L, h.n_slices, h.n_crumbs) == stats
    same(h.spin(4), build().spin(4))
    return h, got


# 1. held to gh_viterbi_marginals ---------------------------------------------------------------------------------------------------
SPECS = [{}, E_MT, dict(cond_mode="C"), dict(storage="f64"), dict(cand_order="T-GCA")]      # (those of tests/test_gpu_maxmarg.py)
HELD = [("a", kw, L) for kw in SPECS for L in (1, 2, 3, 5)] + [("a4", {}, 6), ("a4", E_MT, 6), ("b", E_MT, 3), ("C2", {}, 3)]


@pytest.mark.parametrize("which,kw,L", HELD, ids=lambda v: v if isinstance(v, str) else (spec_id(v) if isinstance(v, dict) else "L%s" % v))
def test_held_to_the_lds_call(which, kw, L):
    t = _table(which)
    h, got = _held(lambda: make_pair(t, L=L, **kw)[0])
    S = 4 if which in ("a4", "C2") else 5
    s, le, states, scratch = h.viterbi_grid_info()           # (the last grid call: _held's viterbi_path_grid)
    assert (s, le, states) == (S, L, S ** L) and states <= CAP and got["hole_at"] == 0
    assert h.viterbi_marginals_grid_bytes() >= t.n_snps * states * 8 + 16 * states + t.n_snps * (30 * L + 6) * 8
    if which == "C2":
        assert t.n_snps == 1000                              # two thousand launches on the stream, no wait between them


# 2. small windows and warm-up ------------------------------------------------------------------------------------------------------
def test_small_windows_and_warm_up():
    h, got = _held(lambda: _from_haps(["A", "C", "C"], band=1, L=4)[0])              # N = 1
    assert got["cm"].tolist() == [0, 0b11] and h.viterbi_grid_info()[:3] == (2, 1, 2)
    h, _ = _held(lambda: _from_haps(["AC", "CA", "AA"], band=1, L=5, **E_MT)[0])      # N = 2 < L
    assert h.viterbi_grid_info()[:3] == (2, 2, 4)
    for L in (6, 7, 9):                                          # L >= N: the whole window is warm-up
        h, _ = _held(lambda: _from_haps(["ACGTAC", "CGTACG", "ACTTAG", "AGTTAC"], band=6, L=L)[0])
        assert h.viterbi_grid_info()[:3] == (4, 6, 4096)
    # one position offers a single candidate (and the window three symbols in all)
    h, got = _held(lambda: _from_haps(["ACGTACG", "CGGTACT", "AGGAAGG", "CCGTAGT"], band=3, L=3)[0])
    assert got["cm"][3] == 0b100 and h.viterbi_grid_info()[:3] == (4, 3, 64)
    assert margins_of(got["mm"], got["cm"], np.zeros((0, 8), dtype=np.uint8))["gap"][3] == np.inf
    # every position offers the same single candidate: one state, whatever L is -- also beyond the 24 lags the mask words hold
    h, got = _held(lambda: _from_haps(["AAAAA", "AAAAA"], band=4, L=4)[0])
    assert got["cm"].tolist() == [0, 1, 1, 1, 1, 1] and h.viterbi_grid_info()[:3] == (1, 4, 1)
    assert len(set(got["mm"][1:, 0].tolist())) == 1              # one path: every max-marginal is its score
    h, got = _held(lambda: _from_haps(["A" * 34, "A" * 34], band=4, L=30)[0])
    assert h.viterbi_grid_info()[:3] == (1, 30, 1) and len(set(got["mm"][1:, 0].tolist())) == 1


@pytest.mark.parametrize("at", [1, 4, 8])
def test_a_hole(at):
    build = lambda: _from_haps(["ACGTACGT", "CGTACGTA", "ACTTAGGT"], band=3, L=3, skip=(at,))[0]
    h = build()
    assert h.viterbi_marginals_grid() == dict(mm=None, cm=None, hole_at=at)
    # found on the host, before anything large is reserved: the vit_out and two rows of nine candidate bytes
    assert h.viterbi_grid_info()[3] == grid_marginals_scratch_bytes(8, 3, 0) == 3 * 256
    h, got = _held(build)
    assert got == dict(mm=None, cm=None, hole_at=at)


# 3. the seeded windows -------------------------------------------------------------------------------------------------------------
BEYOND = (35, 78, 146, 155, 176, 177, 186)    # one lag beyond the LDS call's cap on purpose: 6 561, 16 384 or 15 625 states
BLOCK = 24


@pytest.mark.parametrize("first", range(0, len(decode_cases.CASES), BLOCK))
def test_the_seeded_windows_against_the_reference(first):
    for seed in decode_cases.CASES[first:first + BLOCK]:
        desc, t = decode_cases.case(seed)
        ref = maxmarg_ref.marginals(decode_cases.oracle_of(desc, t), desc["N"])
        h, _ = decode_checks.pair_of(desc, t)
        try:
            _same(h.viterbi_marginals_grid(), ref, desc["N"])
            s, le, states = h.viterbi_states()
            assert states <= GRID_CAP
            if seed in BEYOND:
                assert desc["beyond"] and CAP < states <= 16384, states
                with pytest.raises(_lib.GretelHipError, match="states"):
                    h.viterbi_marginals()
            if states:
                assert h.viterbi_grid_info()[:3] == (s, le, states)
        except AssertionError as e:
            raise AssertionError("seed %d %r: %s" % (seed, desc, e)) from e


# 4. dense windows beyond the LDS cap ------------------------------------------------------------------------------------------------
DENSE = [(2001, 16, 13, "AC", {}, 8192), (2002, 20, 14, "GT", {}, 16384), (2003, 14, 6, "ACGT-", {}, 15625), (2004, 14, 7, "ACGT", E_MT, 16384),
         (2005, 12, 9, "ACG", dict(cand_order="T-GCA"), 19683)]        # (those of tests/test_gpu_viterbi_grid.py, built the same way)


def _dense_pair(seed, n, L, alpha, kw):
    rng = np.random.default_rng(seed)
    haps = ["".join(rng.choice(list(alpha), n)) for _ in range(12)]
    return _from_haps(haps, band=n, L=L, **kw)


@functools.lru_cache(maxsize=None)
def _dense_ref(seed):
    """The reference on the window as filled: computed once, shared, never changed."""
    _, n, L, alpha, kw, _ = next(c for c in DENSE if c[0] == seed)
    _, o = _dense_pair(seed, n, L, alpha, kw)
    return maxmarg_ref.marginals(o, n)


@pytest.mark.parametrize("seed,n,L,alpha,kw,states", DENSE, ids=lambda v: str(v) if isinstance(v, (int, str)) else spec_id(v))
def test_dense_windows_beyond_the_lds_cap(seed, n, L, alpha, kw, states):
    h, _ = _dense_pair(seed, n, L, alpha, kw)
    ref = _dense_ref(seed)
    assert ref["hole_at"] == 0
    with pytest.raises(_lib.GretelHipError, match="states"):
        h.viterbi_marginals()
    before = h.export_band()
    want = h.viterbi_marginals_grid_bytes()
    got = h.viterbi_marginals_grid()
    _same(got, ref, n)
    assert h.viterbi_grid_info() == (len(alpha), L, states, want) and states > CAP
    assert want == grid_marginals_scratch_bytes(n, L, states) > n * states * 8
    assert got["mm"][n].max() == h.viterbi_path_grid()["ll_chain"]       # exactly: B_N = +0.0
    assert np.array_equal(h.export_band(), before)


# 5. dirty scratch ------------------------------------------------------------------------------------------------------------------
def _longer_L(desc):
    """The longest state of the window that stays below 65 536 states, where it is longer than the case's own; else 0."""
    return max([L for L in range(desc["L"] + 1, desc["N"] + 1) if desc["S"] ** L <= 65536], default=0)


def _some_offer_fewer(seed):
    desc, t = decode_cases.case(seed)
    if desc["cut_at"] or desc["beyond"] or desc["S"] < 3 or desc["L"] < 2 or not _longer_L(desc):
        return False
    shape = decode_cases.shape_of(decode_cases.oracle_of(desc, t), desc["N"])
    return shape["S"] == desc["S"] and 0 < min(bin(m).count("1") for m in shape["cm"][1:]) < shape["S"]


def test_dirty_scratch():
    # the handle's block is never cleared: a decoding at 4 096 states leaves its rows where the next call's unreachable entries lie
    haps =["ACGTACG", "CGGTACT", "AGGAAGG", "CCGTAGT"]
    h, o = _from_haps(haps, band=3, L=6)
    assert h.viterbi_path_grid()["hole_at"] == 0 and h.viterbi_grid_info()[2] == 4096
    filled = h.viterbi_grid_info()[3]
    h.L = o.L = 3
    ref = maxmarg_ref.marginals(o, 7)
    assert ref["hole_at"] == 0 and min(bin(int(m)).count("1") for m in ref["cm"][1:]) == 1
    got = h.viterbi_marginals_grid()
    assert h.viterbi_grid_info()[:3] == (4, 3, 64) and h.viterbi_grid_info()[3] < filled     # (the block was not had anew)
    _same(got, ref, 7)
    again = h.viterbi_marginals_grid()
    assert np.array_equal(again["mm"], got["mm"]) and np.array_equal(again["cm"], got["cm"])
    # ... and a seeded window of that kind, its handle dirtied by a decoding at a longer state
    seed = next(s for s in decode_cases.CASES if _some_offer_fewer(s))
    desc, t = decode_cases.case(seed)
    o = decode_cases.oracle_of(desc, t)
    ref = maxmarg_ref.marginals(o, desc["N"])
    h, _ = decode_checks.pair_of(desc, t)
    h.L = _longer_L(desc)
    assert h.viterbi_path_grid()["hole_at"] == 0
    big = h.viterbi_grid_info()[2]
    h.L = desc["L"]
    got = h.viterbi_marginals_grid()
    assert big > h.viterbi_grid_info()[2] == desc["S"] ** desc["L"]
    print("seed %d: S = %d, dirtied at %d states, decoded at %d" % (seed, desc["S"], big, h.viterbi_grid_info()[2]))
    try:
        _same(got, ref, desc["N"])
        again = h.viterbi_marginals_grid()
        assert np.array_equal(again["mm"], got["mm"]) and np.array_equal(again["cm"], got["cm"])
    except AssertionError as e:
        raise AssertionError("seed %d %r: %s" % (seed, desc, e)) from e


# 6. the fill's own L ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,states", [("a4", 1048576), ("a", 9765625)])
def test_the_fills_own_L(which, states):
    """No plain reference reaches 4^10 or 5^10 states: identities.  The header's exactness paragraph says that M[p][c] is the
    maximum over the full paths x through (p, c) of fl(fwd_p(x) + bwd_p(x)), two summation orders of the same N weights.  For the
    grid's own best path x* with score ll (one order: the sequential sum) the other order differs from ll by at most
    b = N * 2^-52 * sum |w_t(x*)|, so mm[p][x*[p]] >= ll - b at every p; and mm[N].max() == ll exactly, since B_N = +0.0."""
    t = _table(which)
    h, _ = make_pair(t)
    n = t.n_snps
    assert h.L == 10 and n == 60
    before = h.export_band()
    want = h.viterbi_marginals_grid_bytes()
    got = h.viterbi_marginals_grid()
    assert got["hole_at"] == 0 and not np.isnan(got["mm"]).any()
    info = h.viterbi_grid_info()
    assert info == (4 if which == "a4" else 5, 10, states, want) and want == grid_marginals_scratch_bytes(60, 10, states)
    assert abs(want / 1e9 - (0.525 if which == "a4" else 4.89)) < 0.01
    best = h.viterbi_path_grid()
    ll, path = best["ll_chain"], best["path"]
    assert best["hole_at"] == 0 and np.isfinite(ll)
    w = h.score_paths([path], per_position=True)["weight"][0, 1:]
    b = n * 2.0 ** -52 * np.abs(w).sum()
    through = got["mm"][np.arange(1, n + 1), path[1:]]
    top = got["mm"][1:].max(axis=1)
    gap = margins_of(got["mm"], got["cm"], path.reshape(1, -1))["gap"][1:]
    print("%s: ll %r, smallest gap %r, largest max_c mm[p][c] - ll %r, smallest mm[p][path[p]] - ll %r, b %.3e"
          % (which, ll, gap.min(), (top - ll).max(), (through - ll).min(), b))
    assert got["mm"][n].max() == ll                          # exactly
    assert (through >= ll - b).all(), (np.argwhere(through < ll - b)[:4].tolist(), (through - ll).min(), b)
    # what the exactness paragraph implies for the other three figures: every entry is some full path's score in the other
    # summation order, and no full path scores above ll by more than its own bound -- the weights are <= 0 under the default spec,
    # so |sum| of a path that reaches ll - b is below |ll| + b and the bound of any competitor that matters is within (1 + 1e-9) b
    assert (w <= 0).all() and (top <= ll + 2 * b).all() and (gap >= 0).all()
    assert (got["mm"][~((got["cm"][:, None] >> np.arange(7)) & 1).astype(bool)] == -np.inf).all()
    assert np.array_equal(h.export_band(), before)


# 7. the command line ---------------------------------------------------------------------------------------------------------------
def test_cli_margins_grid(tmp_path, capsys):
    plain, lds, grid, both = (tmp_path / d for d in ("plain", "lds", "grid", "both"))
    for d in (plain, lds, grid, both):
        d.mkdir()
    argv = [BAM, VCF, "hoot", "-s", "1", "-e", "20", "-p", "12", "--quiet"]
    assert cmd.main(argv + ["-o", str(plain)]) == 0
    assert cmd.main(argv + ["-o", str(lds), "--margins"]) == 0
    assert "--margins-grid" not in capsys.readouterr().err
    assert cmd.main(argv + ["-o", str(grid), "--margins-grid"]) == 0
    err = capsys.readouterr().err
    v = cmd.util.process_vcf(VCF, "hoot", 1, 20)
    h = cmd.util.load_from_bam(BAM, "hoot", 1, 20, v)
    s, le, states = h.viterbi_states()
    note = "[NOTE] --margins-grid: S = %d candidate symbols, Le = %d: %d states, %d bytes of device scratch\n" % (s, le, states, h.viterbi_marginals_grid_bytes())
    assert err.count(note) == 1 and states <= CAP
    assert cmd.main(argv + ["-o", str(both), "--margins", "--margins-grid"]) == 0
    assert capsys.readouterr().err.count(note) == 1          # the grid call, once
    want = (lds / "gretel.margins").read_bytes()
    assert want.startswith(b"# 4\t3\tA\t0\t4\t64\n") and want.count(b"\nS\t") == 4 and want.count(b"\nH\t") >= 1      # four SNPs
    for d in (grid, both):
        assert (d / "gretel.margins").read_bytes() == want
        assert sorted(os.listdir(d)) == sorted(os.listdir(plain) + ["gretel.margins"])
        for f in os.listdir(plain):
            assert (d / f).read_bytes() == (plain / f).read_bytes(), f


def test_margins_grid_writes_a_file_where_margins_writes_the_note(tmp_path, capsys):
    h, _ = make_pair(_table("a4"), L=7)                      # 16 384 states
    vcf_h = dict(N=h.n, snp_rev=list(range(1, h.n + 1)))
    (tmp_path / "lds").mkdir()
    (tmp_path / "grid").mkdir()
    cmd.write_margins({}, h, vcf_h, types.SimpleNamespace(out=str(tmp_path / "lds")))
    err = capsys.readouterr().err
    assert err.startswith("[NOTE] --margins: ") and "16384 states" in err and os.listdir(tmp_path / "lds") == []
    cmd.write_margins({}, h, vcf_h, types.SimpleNamespace(out=str(tmp_path / "grid"), margins_grid=True))
    err = capsys.readouterr().err
    assert err == "[NOTE] --margins-grid: S = 4 candidate symbols, Le = 7: 16384 states, %d bytes of device scratch\n" % h.viterbi_marginals_grid_bytes()
    assert os.listdir(tmp_path / "grid") == ["gretel.margins"]
    lines = (tmp_path / "grid" / "gretel.margins").read_text().splitlines()
    assert lines[0] == "# %d\t7\tA\t0\t4\t16384" % h.n and len(lines) == 1 + h.n and all(ln.startswith("S\t") for ln in lines[1:])


# 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    t = _table("a4")
    h, _ = make_pair(t, L=7)
    L = _lib.load()
    mm = np.zeros((t.n_snps + 1, 7))
    cm = np.zeros(t.n_snps + 1, dtype=np.uint8)
    hole = C.c_int()

    def call(hh, a=mm, b=cm, ph=C.byref(hole)):
        return L.gh_viterbi_marginals_grid(hh._h if hh is not None else None, a.ctypes.data if a is not None else None,
                                           b.ctypes.data if b is not None else None, ph)

    assert call(None) == _lib.GH_ERR_ARG and call(h, None) == _lib.GH_ERR_ARG
    assert call(h, b=None) == _lib.GH_ERR_ARG and call(h, ph=None) == _lib.GH_ERR_ARG
    assert h.viterbi_grid_info() == (0, 0, 0, 0)
    assert call(h) == _lib.GH_OK and hole.value == 0         # L = 7 without deletion columns: beyond the other call's cap, served here
    assert h.viterbi_grid_info() == (4, 7, 16384, h.viterbi_marginals_grid_bytes()) and h.viterbi_info() == (0, 0, 0, 0)
    hz, _ = make_pair(t, L=3, offer_zero=True)
    assert call(hz) == _lib.GH_ERR_ARG and b"offer_zero" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="offer_zero"):
        hz.viterbi_marginals_grid()
    fresh = Hansel(t.n_snps, band=t.band)
    assert call(fresh) == _lib.GH_ERR_STATE and b"before any fill" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="before any fill"):
        fresh.viterbi_marginals_grid()
    # 2^25 states: one lag beyond the grid's cap
    rng = np.random.default_rng(25)
    haps = ["".join(rng.choice(list("AC"), 26)) for _ in range(4)]
    hb, _ = _from_haps(haps, band=2, L=25)
    bmm, bcm = np.zeros((27, 7)), np.zeros(27, dtype=np.uint8)
    assert hb.viterbi_states() == (2, 25, 1 << 25)
    assert call(hb, bmm, bcm) == _lib.GH_ERR_ARG
    msg = L.gh_last_error()
    assert msg.startswith(b"gh_viterbi_marginals_grid") and b"S = 2 " in msg and b"= 25 make 33554432 states" in msg and b"16777216" in msg
    assert hb.viterbi_grid_info() == (0, 0, 0, 0)            # nothing was allocated for it, no call is on record
    assert hb.viterbi_marginals_grid_bytes() == 0
    with pytest.raises(_lib.GretelHipError, match="33554432 states") as e:
        hb.viterbi_marginals_grid()
    assert e.value.code == _lib.GH_ERR_ARG
