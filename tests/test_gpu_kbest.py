"""K-best exact decoding of the chain likelihood on the GPU (gh_viterbi_kbest; Hansel.viterbi_kbest; --kbest of gretel_amd.cmd)
against the plain statement of the definition (tests/kbest_ref.py over the C oracle).  Everything is compared exactly: paths,
scores, n and hole_at -- the order of every addition and every comparison is fixed."""
import ctypes as C
import io
import itertools

import numpy as np
import pytest

import kbest_ref
from decode_util import BAM, E_MT, SYMS, VCF, _cli_oracle, _from_haps, _table
from gretel_amd import _lib, cmd
from gretel_amd.hansel import Hansel, kbest_of
from spec_util import make_pair, same, spec_id

pytestmark = pytest.mark.gpu
CAP = _lib.GH_VITERBI_MAX_STATES


def _str(path):
    return "".join(SYMS[int(v)] for v in path[1:])


def _check(h, o, k):
    """viterbi_kbest(k) of `h` against kbest_ref over `o`, and against gh_score_paths on the same handle; returns the GPU's dict."""
    n = h.n
    got = h.viterbi_kbest(k)
    ref = kbest_ref.kbest(o, n, k, h._cfg["cand_order"])
    assert (got["n"], got["hole_at"]) == (ref["n"], ref["hole_at"])
    assert got["paths"].dtype == np.uint8 and got["paths"].shape == (ref["n"], n + 1) and got["ll_chain"].shape == (ref["n"],)
    if ref["hole_at"]:
        return got
    assert got["ll_chain"].tolist() == ref["ll_chain"].tolist(), [
        (i, a, b) for i, (a, b) in enumerate(zip(got["ll_chain"], ref["ll_chain"])) if a != b][:4]
    assert np.array_equal(got["paths"], ref["paths"]), np.argwhere(got["paths"] != ref["paths"])[:4].tolist()
    sc = h.score_paths(got["paths"])
    assert sc["ll_chain"].tolist() == got["ll_chain"].tolist() and (sc["n_on"] == n).all()
    assert len({x.tobytes() for x in got["paths"]}) == got["n"]
    assert (np.diff(got["ll_chain"]) <= 0).all()
    return got


F64, TGCA = dict(storage="f64"), dict(cand_order="T-GCA")
# (table, switches, L, K)
CASES = [("a", kw, L, 32) for L in (1, 2) for kw in ({}, E_MT)] + [
    ("a", kw, 3, 32) for kw in ({}, E_MT, F64, TGCA)] + [             # 125 * 32 = 4000 slots: just under the cap, four a thread
    ("a", {}, 5, 1), ("a", E_MT, 5, 1),                              # 3125 states
    ("a4", {}, 3, 32), ("a4", E_MT, 3, 32),
    ("a4", {}, 5, 4), ("a4", E_MT, 5, 4),                            # 1024 * 4: exactly the cap
    ("a4", {}, 6, 1), ("a4", E_MT, 6, 1),
    ("b", {}, 3, 8), ("b", E_MT, 3, 8),
    ("C2", {}, 2, 8), ("C2", E_MT, 2, 8),                            # N > 512: the trace takes more than one chunk
]


def _id(v):
    return v if isinstance(v, str) else (spec_id(v) if isinstance(v, dict) else str(v))


@pytest.mark.parametrize("which,kw,L,k", CASES, ids=_id)
def test_kbest_against_the_reference(which, kw, L, k):
    t = _table(which)
    h, o = make_pair(t, L=L, **kw)
    got = _check(h, o, k)
    S = 4 if which in ("a4", "C2") else 5
    assert got["n"] == k
    s, le, states, scratch = h.viterbi_info()
    assert (s, le, states) == (S, L, S ** L) and states * k <= CAP
    assert scratch >= (t.n_snps + 1) * states * k + t.n_snps * (30 * L + 6) * 8
    if which == "C2":
        assert t.n_snps > 512


@pytest.mark.parametrize("which,kw,L", sorted({(c[0], tuple(sorted(c[1].items())), c[2]) for c in CASES}),
                         ids=lambda v: v if isinstance(v, str) else (spec_id(dict(v)) if isinstance(v, tuple) else "L%s" % v))
def test_k_1_is_viterbi_path(which, kw, L):
    h, _ = make_pair(_table(which), L=L, **dict(kw))
    one, best = h.viterbi_kbest(1), h.viterbi_path()
    assert one["n"] == 1 and one["hole_at"] == 0
    assert one["ll_chain"][0] == best["ll_chain"] and np.array_equal(one["paths"][0], best["path"])


def test_exhaustive_on_the_device():
    haps = ["ACGTACGT", "CGTTAGCA", "AGCTTCGA"]
    n = 8
    h, o = _from_haps(haps, band=3, L=3)
    every = np.array([(6,) + x for x in itertools.product((0, 1, 2, 3), repeat=n)], dtype=np.uint8)
    sc = h.score_paths(every)
    on = sc["n_on"] == n
    assert 32 < on.sum() < len(every)
    top = sorted(sc["ll_chain"][on].tolist(), reverse=True)[:32]
    got = _check(h, o, 32)
    assert got["ll_chain"].tolist() == top


def test_small_windows_and_warm_up():
    h, o = _from_haps(["A", "C", "C"], band=1, L=4)              # N = 1: two full paths
    got = _check(h, o, 8)
    assert got["n"] == 2 and h.viterbi_info()[:3] == (2, 1, 2)
    h, o = _from_haps(["AC", "CA", "AA"], band=1, L=5, **E_MT)     # N = 2 < L
    assert _check(h, o, 8)["n"] == 4 and h.viterbi_info()[:3] == (2, 2, 4)
    for L in (6, 7, 9):                                          # L >= N: the whole window is warm-up, the state the whole prefix
        h, o = _from_haps(["ACGTAC", "CGTACG", "ACTTAG", "AGTTAC"], band=6, L=L)
        one = _check(h, o, 1)
        assert h.viterbi_info()[:3] == (4, 6, 4096)
        assert np.array_equal(one["paths"][0], h.viterbi_path()["path"])
    # N = 3, L = 5: the state is the whole prefix, every list has one entry and only the end rule orders
    h, o = _from_haps(["ACG", "CGT", "ACT", "AGT"], band=3, L=5)
    got = _check(h, o, 8)
    assert h.viterbi_info()[1] == 3 and got["n"] == 8
    # every position offers the same single candidate: one state whatever L is, one full path
    h, o = _from_haps(["AAAAA", "AAAAA"], band=4, L=4)
    got = _check(h, o, 4)
    assert got["n"] == 1 and _str(got["paths"][0]) == "AAAAA" and h.viterbi_info()[:3] == (1, 4, 1)


def test_a_biallelic_window_at_the_cap():
    rng = np.random.default_rng(12)
    n = 16
    haps = ["".join("AG"[v] for v in rng.integers(0, 2, n)) for _ in range(6)]
    h, o = _from_haps(haps, band=12, L=7)
    assert _check(h, o, 32)["n"] == 32 and h.viterbi_info()[:3] == (2, 7, 128)      # 128 * 32 = 4096
    h.L = o.L = 12
    one = _check(h, o, 1)
    assert h.viterbi_info()[:3] == (2, 12, CAP)
    assert np.array_equal(one["paths"][0], h.viterbi_path()["path"])
    with pytest.raises(_lib.GretelHipError, match=r"S = 2 .* = 12 make 4096 states.*k = 2 .*8192 slots.*largest k this window takes is 1") as e:
        h.viterbi_kbest(2)
    assert e.value.code == _lib.GH_ERR_ARG


@pytest.mark.parametrize("order", ["ACGT-", "T-GCA"])
def test_exact_ties(order):
    # two haplotypes with identical evidence tie exactly: both come back, in the end rule's order
    h, o = _from_haps(["ACACAC", "CACACA"], band=3, L=3, cand_order=order)
    got = _check(h, o, 2)
    assert got["ll_chain"][0] == got["ll_chain"][1]
    assert [_str(x) for x in got["paths"]] == (["CACACA", "ACACAC"] if order == "ACGT-" else ["ACACAC", "CACACA"])
    # ... and where two tied prefixes meet in one state (they differ at SNP 1 only), in ascending q(x[1])
    h, o = _from_haps(["AGTTACG", "CGTTACG"], band=3, L=3, cand_order=order)
    got = _check(h, o, 2)
    assert got["ll_chain"][0] == got["ll_chain"][1]
    assert [_str(x) for x in got["paths"]] == (["AGTTACG", "CGTTACG"] if order == "ACGT-" else ["CGTTACG", "AGTTACG"])


@pytest.mark.parametrize("at", [1, 4, 8])
def test_a_hole(at):
    h, o = _from_haps(["ACGTACGT", "CGTACGTA", "ACTTAGGT"], band=3, L=3, skip=(at,))
    got = _check(h, o, 4)
    assert got["n"] == 0 and got["hole_at"] == at and got["paths"].shape == (0, 9)
    # ... and no array is written
    paths = np.full((4, 9), 0xAB, dtype=np.uint8)
    ll = np.full(4, 7.25)
    n, hole = C.c_int(-1), C.c_int(-1)
    assert _lib.load().gh_viterbi_kbest(h._h, 4, paths.ctypes.data, ll.ctypes.data, C.byref(n), C.byref(hole)) == _lib.GH_OK
    assert (n.value, hole.value) == (0, at) and (paths == 0xAB).all() and (ll == 7.25).all()


@pytest.mark.parametrize("kw", [{}, E_MT], ids=spec_id)
def test_against_the_heuristics_and_the_max_marginals(kw):
    t = _table("a")
    h, _ = make_pair(t, L=3, **kw)
    b, kb = h.beam_paths(32), h.viterbi_kbest(32)
    assert b["n"] == kb["n"] == 32
    assert all(b["ll_chain"][r] <= kb["ll_chain"][r] for r in range(32))
    assert (np.diff(kb["ll_chain"]) <= 0).all()
    assert h.viterbi_marginals()["mm"][t.n_snps].max() == kb["ll_chain"][0]


def test_nothing_is_disturbed_and_the_block_is_shared():
    t = _table("a")
    h, _ = make_pair(t, L=3)
    before = h.export_band()
    stats = (h.L, h.n_slices, h.n_crumbs)
    kb1 = h.viterbi_kbest(8)
    s, le, states, scratch = h.viterbi_info()
    assert (s, le, states) == (5, 3, 125) and scratch >= (t.n_snps + 1) * 125 * 8 + t.n_snps * (30 * 3 + 6) * 8
    vp, vm, kb2 = h.viterbi_path(), h.viterbi_marginals(), h.viterbi_kbest(8)
    assert np.array_equal(h.export_band(), before) and (h.L, h.n_slices, h.n_crumbs) == stats
    sp = h.spin(4)
    fresh = lambda: make_pair(t, L=3)[0]
    for kb in (kb1, kb2):
        want = fresh().viterbi_kbest(8)
        assert kb["n"] == want["n"] == 8 and np.array_equal(kb["paths"], want["paths"])
        assert kb["ll_chain"].tolist() == want["ll_chain"].tolist()
    want = fresh().viterbi_path()
    assert vp["ll_chain"] == want["ll_chain"] == kb1["ll_chain"][0] and np.array_equal(vp["path"], want["path"])
    want = fresh().viterbi_marginals()
    assert np.array_equal(vm["mm"], want["mm"]) and np.array_equal(vm["cm"], want["cm"])
    f = fresh()
    same(sp, f.spin(4))
    assert np.array_equal(h.export_band(), f.export_band())


def test_refusals():
    t = _table("a4")
    h, _ = make_pair(t, L=5)
    L = _lib.load()
    paths = np.zeros((32, t.n_snps + 1), dtype=np.uint8)
    ll = np.zeros(32)
    n, hole = C.c_int(), C.c_int()

    def call(hh, k, p=paths, pll=ll, pn=C.byref(n), ph=C.byref(hole)):
        return L.gh_viterbi_kbest(hh._h if hh is not None else None, k, p.ctypes.data if p is not None else None,
                                  pll.ctypes.data if pll is not None else None, pn, ph)

    for k in (0, 33, -1):
        assert call(h, k) == _lib.GH_ERR_ARG
        assert b"outside 1..32" in L.gh_last_error()
    assert call(h, 4) == _lib.GH_OK and (n.value, hole.value) == (4, 0)           # 1024 * 4: the cap itself is served
    assert call(h, 5) == _lib.GH_ERR_ARG                                          # ... one more list a state is not
    msg = L.gh_last_error()
    assert b"S = 4 " in msg and b"= 5 make 1024 states" in msg and b"k = 5 " in msg and b"5120 slots" in msg
    assert b"largest k this window takes is 4" in msg
    with pytest.raises(_lib.GretelHipError, match="largest k this window takes is 4"):
        h.viterbi_kbest(32)
    h.L = 7                                                                       # more states than the decoder holds
    assert call(h, 1) == _lib.GH_ERR_ARG
    msg = L.gh_last_error()
    assert b"gh_viterbi_kbest: S = 4 " in msg and b"= 7 make 16384 states" in msg and b"--beam" in msg
    h.L = 3
    assert call(None, 2) == _lib.GH_ERR_ARG and call(h, 2, p=None) == _lib.GH_ERR_ARG and call(h, 2, pll=None) == _lib.GH_ERR_ARG
    assert call(h, 2, pn=None) == _lib.GH_ERR_ARG and call(h, 2, ph=None) == _lib.GH_ERR_ARG
    assert b"null argument" in L.gh_last_error()
    hz, _ = make_pair(t, L=3, offer_zero=True)
    assert call(hz, 2) == _lib.GH_ERR_ARG and b"offer_zero" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="offer_zero"):
        hz.viterbi_kbest(2)
    fresh = Hansel(t.n_snps, band=t.band)
    assert call(fresh, 2) == _lib.GH_ERR_STATE and b"before any fill" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="before any fill"):
        fresh.viterbi_kbest(2)


@pytest.mark.parametrize("exact", [False, True], ids=["greedy", "exact"])
def test_cli_kbest(tmp_path, capsys, exact):
    out, plain = tmp_path / "out", tmp_path / "plain"
    out.mkdir()
    plain.mkdir()
    argv = [BAM, VCF, "hoot", "-s", "1", "-e", "20", "-p", "12"] + (["--exact"] if exact else [])
    assert cmd.main(argv + ["-o", str(plain)]) == 0
    assert cmd.main(argv + ["-o", str(out), "--kbest", "8"]) == 0
    capsys.readouterr()
    assert not (plain / "gretel.kbest").exists()
    for f in ("out.fasta", "snp.fasta", "gretel.crumbs"):
        assert (out / f).read_bytes() == (plain / f).read_bytes(), f
    v, n, h, o = _cli_oracle()
    ref = kbest_ref.kbest(o, n, 8)                             # (before the spins: the matrix as the reads filled it)
    s, _, states = h.viterbi_states()
    res = h.viterbi_spin(12, cmd.MIN_REMOVE) if exact else h.spin(12, cmd.MIN_REMOVE)
    paths = cmd.paths_of_spin(h, res, log=io.StringIO())
    keys = sorted(paths, key=lambda x: paths[x]["i_0"])
    rec = np.array([[q.i for q in paths[k]["hansel_path"]] for k in keys], dtype=np.uint8)
    want = cmd.kbest_text((n, h.L, "A", 0, s, states, 8, ref["n"]), ref, kbest_of(ref, rec), [paths[k]["i_0"] for k in keys])
    text = (out / "gretel.kbest").read_text()
    assert text == want
    assert ref["n"] == 6 and len(text.splitlines()) == 7     # (the window has six full paths: n < K, and the header says so)
    assert text.splitlines()[0].split("\t")[-2:] == ["8", "6"]
    if exact:                                                  # rank 0 is the first recovered haplotype
        first = text.splitlines()[1].split("\t")
        assert first[0] == "0" and first[3:6] == ["0", "0", "0"]
