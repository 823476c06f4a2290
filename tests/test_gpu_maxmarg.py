"""Max-marginals of the chain likelihood on the GPU (gh_viterbi_marginals; Hansel.viterbi_marginals, margins_of; --margins of
gretel_amd.cmd) against the plain statement of the definition (tests/maxmarg_ref.py over the C oracle).  mm and cm are compared as
IEEE values, -inf included: the association of every addition is fixed and a maximum does not depend on the order."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import maxmarg_ref
from decode_util import BAM, E_MT, VCF, _cli_oracle, _from_haps, _table
from gretel_amd import _lib, cmd
from gretel_amd.hansel import Hansel, margins_of
from spec_util import make_pair, same, spec_id

pytestmark = pytest.mark.gpu
CAP = _lib.GH_VITERBI_MAX_STATES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(h, o):
    """viterbi_marginals of `h` against maxmarg_ref over `o`, and the identity against viterbi_path on the same handle."""
    n = h.n
    got = h.viterbi_marginals()
    ref = maxmarg_ref.marginals(o, n)
    assert got["hole_at"] == ref["hole_at"]
    if ref["hole_at"]:
        assert got["mm"] is None and got["cm"] is None
        return got
    assert got["mm"].dtype == np.float64 and got["mm"].shape == (n + 1, 7) and got["cm"].dtype == np.uint8 and got["cm"].shape == (n + 1,)
    assert not np.isnan(got["mm"]).any()
    assert np.array_equal(got["cm"], ref["cm"]), np.argwhere(got["cm"] != ref["cm"])[:4].tolist()
    bad = np.argwhere(got["mm"] != ref["mm"])
    assert np.array_equal(got["mm"], ref["mm"]), (len(bad), bad[:4].tolist(), [(got["mm"][tuple(q)], ref["mm"][tuple(q)]) for q in bad[:4]])
    info = h.viterbi_info()
    assert info[3] >= n * info[2] * 8
    assert got["mm"][n].max() == h.viterbi_path()["ll_chain"]       # B_N = +0.0
    return got


SPECS = [{}, E_MT, dict(cond_mode="C"), dict(storage="f64"), dict(cand_order="T-GCA")]      # (those of tests/test_gpu_viterbi.py)
CASES = [("a", kw, L) for kw in SPECS for L in (1, 2, 3, 5)] + [
    ("a4", {}, 6), ("a4", E_MT, 6),                          # 4096 states: four states a thread
    ("b", E_MT, 3),
    ("C2", {}, 3),                                           # 1000 SNPs: many turns of the ring, k_vit_mm's grid more than once over
]


@pytest.mark.parametrize("which,kw,L", CASES, ids=lambda v: v if isinstance(v, str) else (spec_id(v) if isinstance(v, dict) else "L%s" % v))
def test_max_marginals_against_the_reference(which, kw, L):
    t = _table(which)
    h, o = make_pair(t, L=L, **kw)
    before = h.export_band()
    stats = (h.L, h.n_slices, h.n_crumbs)
    _check(h, o)
    S = 4 if which in ("a4", "C2") else 5
    assert h.viterbi_info()[:3] == (S, L, S ** L)
    assert np.array_equal(h.export_band(), before) and np.array_equal(before, o.export_band())
    assert (h.L, h.n_slices, h.n_crumbs) == stats
    fresh, _ = make_pair(t, L=L, **kw)
    same(h.spin(4), fresh.spin(4))
    assert np.array_equal(h.export_band(), fresh.export_band())


def test_small_windows_and_warm_up():
    h, o = _from_haps(["A", "C", "C"], band=1, L=4)              # N = 1
    got = _check(h, o)
    assert got["cm"].tolist() == [0, 0b11] and h.viterbi_info()[:3] == (2, 1, 2)
    h, o = _from_haps(["AC", "CA", "AA"], band=1, L=5, **E_MT)     # N = 2 < L
    _check(h, o)
    assert h.viterbi_info()[:3] == (2, 2, 4)
    for L in (6, 7, 9):                                          # L >= N: the whole window is warm-up
        h, o = _from_haps(["ACGTAC", "CGTACG", "ACTTAG", "AGTTAC"], band=6, L=L)
        _check(h, o)
        assert h.viterbi_info()[:3] == (4, 6, 4096)
    # one position offers a single candidate (and the window three symbols in all)
    h, o = _from_haps(["ACGTACG", "CGGTACT", "AGGAAGG", "CCGTAGT"], band=3, L=3)
    got = _check(h, o)
    assert got["cm"][3] == 0b100 and h.viterbi_info()[:3] == (4, 3, 64)
    assert margins_of(got["mm"], got["cm"], np.zeros((0, 8), dtype=np.uint8))["gap"][3] == np.inf
    # every position offers the same single candidate: one state, whatever L is
    h, o = _from_haps(["AAAAA", "AAAAA"], band=4, L=4)
    got = _check(h, o)
    assert got["cm"].tolist() == [0, 1, 1, 1, 1, 1] and h.viterbi_info()[:3] == (1, 4, 1)
    assert len(set(got["mm"][1:, 0].tolist())) == 1              # one path: every max-marginal is its score


def test_a_biallelic_window_at_L_12():
    rng = np.random.default_rng(12)
    n = 16
    haps = ["".join("AG"[v] for v in rng.integers(0, 2, n)) for _ in range(6)]
    h, o = _from_haps(haps, band=12, L=12)
    _check(h, o)
    assert h.viterbi_info()[:3] == (2, 12, CAP)


@pytest.mark.parametrize("at", [1, 4, 8])
def test_a_hole(at):
    h, o = _from_haps(["ACGTACGT", "CGTACGTA", "ACTTAGGT"], band=3, L=3, skip=(at,))
    assert _check(h, o) == dict(mm=None, cm=None, hole_at=at)


@pytest.mark.parametrize("order", ["ACGT-", "T-GCA"])
def test_exact_ties(order):
    # two haplotypes with identical evidence tie exactly: both calls have the same max-marginal at every position
    h, o = _from_haps(["ACACAC", "CACACA"], band=3, L=3, cand_order=order)
    got = _check(h, o)
    m = margins_of(got["mm"], got["cm"], np.array([[6, 0, 1, 0, 1, 0, 1], [6, 1, 0, 1, 0, 1, 0]], dtype=np.uint8), order)
    assert m["gap"][1:].tolist() == [0.0] * 6 and m["max_regret"].tolist() == [0.0, 0.0]
    assert "".join("ACGTN-_"[v] for v in m["best"][1:]) == ("A" if order == "ACGT-" else "C") * 6     # the first of cand_order
    # ... and where two tied prefixes differ at SNP 1 only
    h, o = _from_haps(["AGTTACG", "CGTTACG"], band=3, L=3, cand_order=order)
    got = _check(h, o)
    assert got["mm"][1, 0] == got["mm"][1, 1] > -np.inf


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from decode_util import _table
from spec_util import make_pair
h, _ = make_pair(_table("a"), L=3)
got = h.viterbi_marginals()
np.save(sys.argv[1], got["mm"])
np.save(sys.argv[2], got["cm"])
"""


def test_the_table_from_global_memory_gives_the_same_bits(tmp_path):
    # GH_VIT_STAGE is read once in a process: a fresh child
    env = dict(os.environ, GH_VIT_STAGE="0")
    mm, cm = str(tmp_path / "mm.npy"), str(tmp_path / "cm.npy")
    subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), mm, cm], env=env, check=True, timeout=300)
    h, o = make_pair(_table("a"), L=3)
    ref = maxmarg_ref.marginals(o, h.n)
    assert np.array_equal(np.load(mm), ref["mm"]) and np.array_equal(np.load(cm), ref["cm"])


def test_refusals():
    t = _table("a4")
    h, _ = make_pair(t, L=7)
    L = _lib.load()
    mm = np.zeros((t.n_snps + 1, 7))
    cm = np.zeros(t.n_snps + 1, dtype=np.uint8)
    hole = C.c_int()

    def call(hh, a=mm, b=cm, ph=C.byref(hole)):
        return L.gh_viterbi_marginals(hh._h if hh is not None else None, a.ctypes.data if a is not None else None,
                                      b.ctypes.data if b is not None else None, ph)

    assert call(h) == _lib.GH_ERR_ARG                        # L = 7 without deletion columns
    msg = L.gh_last_error()
    assert msg.startswith(b"gh_viterbi_marginals") and b"S = 4 " in msg and b"= 7 make 16384 states" in msg and b"--beam" in msg
    with pytest.raises(_lib.GretelHipError, match="16384 states"):
        h.viterbi_marginals()
    h.L = 6                                                  # the cap itself is served
    assert call(h) == _lib.GH_OK and hole.value == 0
    s, le, states, scratch = h.viterbi_info()
    assert (s, le, states) == (4, 6, CAP) and scratch >= t.n_snps * CAP * 8 + t.n_snps * (30 * 6 + 6) * 8
    assert call(None) == _lib.GH_ERR_ARG and call(h, None) == _lib.GH_ERR_ARG
    assert call(h, b=None) == _lib.GH_ERR_ARG and call(h, ph=None) == _lib.GH_ERR_ARG
    hz, _ = make_pair(t, L=3, offer_zero=True)
    assert call(hz) == _lib.GH_ERR_ARG and b"offer_zero" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="offer_zero"):
        hz.viterbi_marginals()
    fresh = Hansel(t.n_snps, band=t.band)
    assert call(fresh) == _lib.GH_ERR_STATE and b"before any fill" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="before any fill"):
        fresh.viterbi_marginals()


def test_margins_of_a_window_beyond_the_cap_writes_the_message_and_no_file(tmp_path, capsys):
    import types
    h, _ = make_pair(_table("a4"), L=7)
    cmd.write_margins({}, h, dict(N=h.n, snp_rev=list(range(1, h.n + 1))), types.SimpleNamespace(out=str(tmp_path)))
    err = capsys.readouterr().err
    assert err.startswith("[NOTE] --margins: ") and "16384 states" in err
    assert os.listdir(tmp_path) == []


def test_exhaustive_on_the_device():
    # the window of tests/test_gpu_viterbi.py's test_exhaustive_on_the_device: gh_score_paths of all 4^8 paths gives, per (p, c),
    # the sequentially summed maximum; mm lies within the two-summation-orders bound of it, -inf agreeing
    haps = ["ACGTACGT", "CGTTAGCA", "AGCTTCGA"]
    n = 8
    h, o = _from_haps(haps, band=3, L=3)
    every = np.array([(6,) + x for x in itertools.product((0, 1, 2, 3), repeat=n)], dtype=np.uint8)
    sc = h.score_paths(every, per_position=True)
    on = sc["n_on"] == n
    assert 1 < on.sum() < len(every)
    got = _check(h, o)
    w = sc["weight"][on][:, 1:]
    finite = np.isfinite(w).all(axis=1)
    A = np.abs(w[finite]).sum(axis=1).max()
    bound = n * 2.0 ** -52 * A
    seen = 0
    for p in range(1, n + 1):
        for c in range(7):
            through = on & (every[:, p] == c)
            if not (got["cm"][p] >> c) & 1:
                assert not through.any() and got["mm"][p, c] == -np.inf
                continue
            top = sc["ll_chain"][through].max()
            print("p=%d c=%d mm=%r sequential=%r bound=%.3e" % (p, c, got["mm"][p, c], top, bound))
            if top == -np.inf:
                assert got["mm"][p, c] == -np.inf
            else:
                assert np.isfinite(got["mm"][p, c]) and abs(got["mm"][p, c] - top) <= bound
            seen += 1
    assert seen >= 2 * n


def test_cli_margins(tmp_path, capsys):
    out, plain, exact = tmp_path / "out", tmp_path / "plain", tmp_path / "exact"
    argv = [BAM, VCF, "hoot", "-s", "1", "-e", "20", "-p", "12"]
    plain.mkdir()
    out.mkdir()
    assert cmd.main(argv + ["-o", str(plain)]) == 0
    assert cmd.main(argv + ["-o", str(out), "--margins"]) == 0
    capsys.readouterr()
    for f in ("out.fasta", "snp.fasta", "gretel.crumbs"):
        assert (out / f).read_bytes() == (plain / f).read_bytes(), f
    assert sorted(os.listdir(out)) == sorted(os.listdir(plain) + ["gretel.margins"])
    # the file: margins_text over the reference's table of the matrix as the reads filled it, for out.fasta's haplotypes
    v, n, h, o = _cli_oracle()
    ref = maxmarg_ref.marginals(o, n)
    res = h.copy().spin(12, cmd.MIN_REMOVE)
    paths = cmd.paths_of_spin(h, res, log=open(os.devnull, "w"))
    keys = sorted(paths, key=lambda x: paths[x]["i_0"])
    rec = np.array([[s.i for s in paths[k]["hansel_path"]] for k in keys], dtype=np.uint8)
    marg = margins_of(ref["mm"], ref["cm"], rec)
    S = bin(int(np.bitwise_or.reduce(ref["cm"]))).count("1")
    le = min(h.L, n)
    want = cmd.margins_text((n, h.L, "A", 0, S, S ** le), [paths[k]["i_0"] for k in keys], marg, ref["mm"], ref["cm"], v["snp_rev"])
    assert (out / "gretel.margins").read_text() == want
    # with --exact the first haplotype IS the best path of that matrix: its regret is rounding, within the bound, at every SNP
    exact.mkdir()
    assert cmd.main(argv + ["-o", str(exact), "--exact", "--margins"]) == 0
    capsys.readouterr()
    lines = (exact / "gretel.margins").read_text().splitlines()
    first = next(ln.split("\t") for ln in lines if ln.startswith("H\t0\t"))
    best = h.viterbi_path()
    w = h.score_paths([best["path"]], per_position=True)["weight"][0, 1:]
    bound = n * 2.0 ** -52 * np.abs(w).sum()
    print("max_regret of the exact path %s, bound %.3e" % (first[3], bound))
    assert abs(float(first[3])) <= bound + 0.5e-6                # (the file rounds to six decimals)
