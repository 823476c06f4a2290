"""Constrained exact decoding on the GPU (gh_viterbi_path_masked; Hansel.viterbi_path_masked; --alternatives and --pin of
gretel_amd.cmd) against the plain statement of the definition (tests/masked_ref.py: viterbi_ref over the C oracle with the
constraint set ANDed into the candidate mask).  Paths, scores and holes are compared exactly: the order of every addition and
every comparison is fixed.  The shapes are the smallest at which the kernels can go wrong."""
import functools
import io
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import decode_cases
import decode_checks
import masked_ref
import maxmarg_ref
import viterbi_ref
from decode_cases import CASES
from decode_util import BAM, E_MT, VCF, _cli_oracle, _from_haps, _table
from gretel_amd import _lib, cmd
from gretel_amd.hansel import Hansel, allow_of, alternatives_of
from masked_ref import VALID
from spec_util import make_pair, same, spec_id

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 8
CHILD_EVERY = 16


def _check(h, o, allow):
    """viterbi_path_masked(allow) of `h` against masked_ref over `o`, and against gh_score_paths on the same handle."""
    n = h.n
    allow = np.asarray(allow, dtype=np.uint8).reshape(-1, n + 1)
    got = h.viterbi_path_masked(allow)
    masked_ref.same_sets(got, masked_ref.decode_sets(o, n, allow, h._cfg["cand_order"]))
    live = got["hole_at"] == 0
    if live.any():
        sc = h.score_paths(got["paths"][live])
        assert sc["ll_chain"].tolist() == got["ll_chain"][live].tolist() and (sc["n_on"] == n).all()
        for row, x in zip(allow[live], got["paths"][live]):
            assert all((int(row[p]) >> int(x[p])) & 1 for p in range(1, n + 1))
    assert (got["paths"][~live] == 6).all() and np.isnan(got["ll_chain"][~live]).all()
    assert h.viterbi_masked_info()[:3] == (len(allow), int((~live).sum()), 1)
    return got


def _other(cm, p, best):
    """An offered candidate at p other than `best`, or `best` where it is the only one."""
    for s in VALID:
        if (int(cm[p]) >> s) & 1 and s != best:
            return s
    return int(best)


# 1. the seeded cases ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seeded(seed):
    """(desc, table, shape, the four generated sets, the reference's dict for them or None beyond the cap): computed once."""
    desc, t = decode_cases.case(seed)
    o = decode_cases.oracle_of(desc, t)
    shape = decode_cases.shape_of(o, desc["N"])
    allow = masked_ref.masks(seed, shape["cm"], desc["N"])
    over = shape["states"] > decode_cases.CAP
    return desc, t, shape, allow, None if over else masked_ref.decode_sets(o, desc["N"], allow, desc["spec"]["cand_order"])


@pytest.mark.parametrize("part", range(STRIDE))
def test_the_seeded_cases_against_the_reference(part):
    served = 0
    for seed in CASES[part::STRIDE]:
        desc, t, shape, allow, ref = _seeded(seed)
        h, _ = decode_checks.pair_of(desc, t)
        try:
            if ref is None:                                      # beyond the cap: gh_viterbi_path's refusal, word for word
                msgs = []
                for call in (h.viterbi_path, lambda: h.viterbi_path_masked(allow)):
                    with pytest.raises(_lib.GretelHipError) as e:
                        call()
                    assert e.value.code == _lib.GH_ERR_ARG
                    msgs.append(str(e.value))
                assert msgs[1] == msgs[0].replace("gh_viterbi_path:", "gh_viterbi_path_masked:") and "states" in msgs[1]
                continue
            served += 1
            got = h.viterbi_path_masked(allow)
            masked_ref.same_sets(got, ref)
            holes = int((ref["hole_at"] != 0).sum())
            assert h.viterbi_masked_info()[:2] == (4, holes)
            if holes < 4:
                assert h.viterbi_info()[:3] == (shape["S"], shape["Le"], shape["states"])
        except AssertionError as e:
            raise AssertionError("seed %d %r: %s" % (seed, desc, e)) from e
    assert served >= len(CASES) // STRIDE - 4


# 2. the cap -----------------------------------------------------------------------------------------
def test_the_cap_four_states_a_thread():
    t = _table("a4")
    h, o = make_pair(t, L=6)
    n = t.n_snps
    best = h.viterbi_path()
    cm = h.viterbi_marginals()["cm"]
    mid = n // 2
    allow = np.stack([allow_of(n), allow_of(n, pins={mid: _other(cm, mid, best["path"][mid])}), allow_of(n, bans={n: int(best["path"][n])})])
    got = _check(h, o, allow)
    assert h.viterbi_info()[:3] == (4, 6, 4096) and not got["hole_at"].any()
    assert got["ll_chain"][0] == best["ll_chain"] and np.array_equal(got["paths"][0], best["path"])
    assert got["paths"][1][mid] != best["path"][mid] and got["paths"][2][n] != best["path"][n]
    assert (got["ll_chain"][1:] <= best["ll_chain"]).all()


# 3. the trace over several chunks, and workgroups that leave early -------------------------------
def test_several_trace_chunks_and_sets_that_leave_early():
    t = _table("C2")
    h, o = make_pair(t, L=2)
    n = t.n_snps
    assert n > 512
    best = h.viterbi_path()
    cm = h.viterbi_marginals()["cm"]
    x = best["path"]
    allow = np.stack([
        allow_of(n),
        allow_of(n, pins={1: _other(cm, 1, x[1]), 2: _other(cm, 2, x[2]), n: _other(cm, n, x[n])}),
        allow_of(n, bans={300: [s for s in VALID if (int(cm[300]) >> s) & 1]}),
        allow_of(n, bans={1: [s for s in VALID if (int(cm[1]) >> s) & 1], 700: "ACGT-"}),
        np.array([0x7F] + [1 << int(v) for v in x[1:]], dtype=np.uint8)])
    got = _check(h, o, allow)
    assert got["hole_at"].tolist() == [0, 0, 300, 1, 0]
    assert np.array_equal(got["paths"][4], x) and got["ll_chain"][4] == got["ll_chain"][0] == best["ll_chain"]
    assert got["ll_chain"][1] <= best["ll_chain"] and got["paths"][1][n] != x[n]
    # the rows and scores of the sets with a hole in a caller's buffer are not written
    paths = np.full((5, n + 1), 0xAB, dtype=np.uint8)
    ll = np.full(5, 7.25)
    hole = np.full(5, -1, dtype=np.int32)
    assert _lib.load().gh_viterbi_path_masked(h._h, allow.ctypes.data, 5, paths.ctypes.data, ll.ctypes.data, hole.ctypes.data) == _lib.GH_OK
    assert hole.tolist() == [0, 0, 300, 1, 0]
    assert (paths[2:4] == 0xAB).all() and ll[2:4].tolist() == [7.25, 7.25]
    assert np.array_equal(paths[[0, 1, 4]], got["paths"][[0, 1, 4]]) and ll[[0, 1, 4]].tolist() == got["ll_chain"][[0, 1, 4]].tolist()


# 4. the walk without the ring -------------------------------------------------------------------------
def test_one_symbol_and_a_state_longer_than_the_ring():
    h, o = _from_haps(["A" * 16, "A" * 16], band=14, L=14)
    got = _check(h, o, np.stack([allow_of(16), allow_of(16, bans={9: "A"}), allow_of(16, pins={p: "AC" for p in range(1, 17)})]))
    assert got["hole_at"].tolist() == [0, 9, 0] and h.viterbi_info()[:3] == (1, 14, 1)
    assert got["paths"][0].tolist() == [6] + [0] * 16 and np.array_equal(got["paths"][2], got["paths"][0])


CHILD = """
import pickle, sys
sys.path[:0] = [%r, %r]
import decode_cases, decode_checks, masked_ref
out = {}
for seed in decode_cases.CASES[::%d]:
    desc, t = decode_cases.case(seed)
    h, o = decode_checks.pair_of(desc, t)
    shape = decode_cases.shape_of(o, desc["N"])
    if shape["states"] <= decode_cases.CAP:
        out[seed] = h.viterbi_path_masked(masked_ref.masks(seed, shape["cm"], desc["N"]))
with open(sys.argv[1], "wb") as f:
    pickle.dump(out, f)
"""


def test_the_tables_from_global_memory_give_the_same_bits(tmp_path):
    # GH_VIT_STAGE is read once in a process: a fresh child decodes, the references are compared here
    out = str(tmp_path / "masked.pkl")
    subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), CHILD_EVERY), out], env=dict(os.environ, GH_VIT_STAGE="0"),
                   check=True, timeout=300)
    with open(out, "rb") as f:
        got = pickle.load(f)
    served = [seed for seed in CASES[::CHILD_EVERY] if _seeded(seed)[4] is not None]
    assert sorted(got) == served and len(served) >= len(CASES) // CHILD_EVERY - 3
    for seed in served:
        try:
            masked_ref.same_sets(got[seed], _seeded(seed)[4])
        except AssertionError as e:
            raise AssertionError("seed %d %r: %s" % (seed, _seeded(seed)[0], e)) from e


# 5. the set count -----------------------------------------------------------------------------------
def test_256_sets_in_one_call_and_the_limits():
    haps = ["ACGTACGT", "CGTTAGCA", "AGCTTCGA", "ACGTTCGA"]
    n = 8
    h, o = _from_haps(haps, band=3, L=3)
    cm = decode_cases.shape_of(o, n)["cm"]
    rng = np.random.default_rng(256)
    allow = rng.integers(0, 128, size=(256, n + 1)).astype(np.uint8)         # arbitrary bytes: many sets are infeasible
    allow[::3] = np.concatenate([masked_ref.masks(s, cm, n) for s in range(22)])[:len(allow[::3])]
    allow[0] = 0x7F
    got = _check(h, o, allow)
    assert 40 <= int((got["hole_at"] != 0).sum()) <= 216 and h.viterbi_masked_info()[2] == 1
    L = _lib.load()
    big = np.full((257, n + 1), 0x7F, dtype=np.uint8)
    paths = np.full((257, n + 1), 0xAB, dtype=np.uint8)
    ll = np.full(257, 7.25)
    hole = np.full(257, -1, dtype=np.int32)
    for m in (257, -1):
        assert L.gh_viterbi_path_masked(h._h, big.ctypes.data, m, paths.ctypes.data, ll.ctypes.data, hole.ctypes.data) == _lib.GH_ERR_ARG
        assert b"outside 0..256" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="outside 0..256"):
        h.viterbi_path_masked(big)
    assert L.gh_viterbi_path_masked(h._h, big.ctypes.data, 0, paths.ctypes.data, ll.ctypes.data, hole.ctypes.data) == _lib.GH_OK
    assert (paths == 0xAB).all() and (ll == 7.25).all() and (hole == -1).all()
    none = h.viterbi_path_masked(np.zeros((0, n + 1), dtype=np.uint8))
    assert none["paths"].shape == (0, n + 1) and none["ll_chain"].shape == (0,) and h.viterbi_masked_info()[:3] == (0, 0, 0)
    one = h.viterbi_path_masked(allow_of(n))                                 # one uint8[N+1] is one set
    assert one["paths"].shape == (1, n + 1) and np.array_equal(one["paths"][0], h.viterbi_path()["path"])


# 6. the consequences the header states -------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, dict(cand_order="T-GCA", **E_MT)], ids=spec_id)
def test_the_consequences_the_header_states(kw):
    t = _table("a")
    h, o = make_pair(t, L=3, **kw)
    n = t.n_snps
    best, kb, mres = h.viterbi_path(), h.viterbi_kbest(8), h.viterbi_marginals()
    mm, cm = mres["mm"], mres["cm"]
    x = best["path"]
    rng = np.random.default_rng(6)

    def one_hot(y, at):
        row = allow_of(n)
        for p in at:
            row[p] = 1 << int(y[p])
        return row

    subsets = [[p for p in range(1, n + 1) if rng.random() < f] for f in (0.1, 0.5, 0.9)] + [[1], [n], list(range(1, n + 1))]
    sets = [allow_of(n)] + [one_hot(x, at) for at in subsets] + [one_hot(y, range(1, n + 1)) for y in kb["paths"]]
    pins = [(p, c) for p in (1, 2, 3, n // 2, n - 1, n) for c in VALID if (int(cm[p]) >> c) & 1]
    sets += [allow_of(n, pins={p: c}) for p, c in pins]
    got = _check(h, o, np.stack(sets))
    assert not got["hole_at"].any()
    # all 0x7f, and one-hot subsets of the best path: the best path and its score
    for q in range(1 + len(subsets)):
        assert got["ll_chain"][q] == best["ll_chain"] and np.array_equal(got["paths"][q], x), q
    # one-hot of each of the k best: that path and its score
    q0 = 1 + len(subsets)
    assert kb["n"] == 8 and np.array_equal(got["paths"][q0:q0 + 8], kb["paths"]) and got["ll_chain"][q0:q0 + 8].tolist() == kb["ll_chain"].tolist()
    # a pin (N, c) is mm[N][c]; the best of the pins at any p is the best of all
    q0 += 8
    top = {}
    for q, (p, c) in enumerate(pins):
        assert got["paths"][q0 + q][p] == c
        top[p] = max(top.get(p, -np.inf), got["ll_chain"][q0 + q])
        if p == n:
            assert got["ll_chain"][q0 + q] == mm[n, c]
    assert all(v == best["ll_chain"] for v in top.values()), top
    sc = h.score_paths(got["paths"])
    assert sc["ll_chain"].tolist() == got["ll_chain"].tolist() and (sc["n_on"] == n).all()


# 7. nothing disturbed ---------------------------------------------------------------------------------
def test_nothing_is_disturbed_and_the_block_is_shared():
    t = _table("a")
    h, o = make_pair(t, L=3)
    n = t.n_snps
    before = h.export_band()
    stats = (h.L, h.n_slices, h.n_crumbs)
    assert h.viterbi_masked_info() == (0, 0, 0, 0)
    allow = masked_ref.masks(7, decode_cases.shape_of(o, n)["cm"], n, sets=5)
    m1 = _check(h, o, allow)
    s, le, states, scratch = h.viterbi_info()
    assert (s, le, states) == (5, 3, 125) and scratch == h.viterbi_masked_info()[3]
    assert scratch >= 5 * ((n + 1) * 125 + 3) // 4 * 4 + n * (30 * 3 + 6) * 8 + 5 * 125 * 9 + 2 * 5 * (n + 1)
    vp, vm, kb = h.viterbi_path(), h.viterbi_marginals(), h.viterbi_kbest(8)      # (the block changes layout between the calls)
    m2 = h.viterbi_path_masked(allow)
    masked_ref.same_sets(m2, m1)
    assert np.array_equal(h.export_band(), before) and (h.L, h.n_slices, h.n_crumbs) == stats
    sp = h.spin(4)
    fresh = lambda: make_pair(t, L=3)[0]
    decode_checks.same_path(vp, viterbi_ref.viterbi(o, n), n)
    decode_checks.same_marginals(vm, maxmarg_ref.marginals(o, n), n)
    want = fresh().viterbi_kbest(8)
    assert np.array_equal(kb["paths"], want["paths"]) and kb["ll_chain"].tolist() == want["ll_chain"].tolist()
    f = fresh()
    same(sp, f.spin(4))
    assert np.array_equal(h.export_band(), f.export_band())


# 8. refusals ----------------------------------------------------------------------------------------
def test_refusals():
    t = _table("a4")
    h, _ = make_pair(t, L=5)
    n = t.n_snps
    L = _lib.load()
    allow = np.full((2, n + 1), 0x7F, dtype=np.uint8)
    paths = np.zeros((2, n + 1), dtype=np.uint8)
    ll = np.zeros(2)
    hole = np.zeros(2, dtype=np.int32)

    def call(hh, a=allow, p=paths, pll=ll, ph=hole, m=2):
        ptr = lambda v: v.ctypes.data if v is not None else None
        return L.gh_viterbi_path_masked(hh._h if hh is not None else None, ptr(a), m, ptr(p), ptr(pll), ptr(ph))

    assert call(h) == _lib.GH_OK and hole.tolist() == [0, 0]
    assert call(None) == call(h, a=None) == call(h, p=None) == call(h, pll=None) == call(h, ph=None) == _lib.GH_ERR_ARG
    assert b"null argument" in L.gh_last_error()
    assert L.gh_viterbi_masked_info(None, hole.ctypes.data) == L.gh_viterbi_masked_info(h._h, None) == _lib.GH_ERR_ARG
    bad = allow.copy()
    bad[1, 17] = 0x81
    assert call(h, a=bad) == _lib.GH_ERR_ARG and b"allow[1][17] = 0x81 has bit 7 set" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="bit 7"):
        h.viterbi_path_masked(bad)
    with pytest.raises(ValueError):
        h.viterbi_path_masked(np.zeros((2, n), dtype=np.uint8))
    h.L = 7                                                                       # more states than the decoder holds
    assert call(h) == _lib.GH_ERR_ARG
    msg = L.gh_last_error()
    assert b"gh_viterbi_path_masked: S = 4 " in msg and b"= 7 make 16384 states" in msg and b"--beam" in msg
    assert call(h, m=0) == _lib.GH_ERR_ARG and L.gh_last_error() == msg            # ... whatever n_sets is, 0 included
    with pytest.raises(_lib.GretelHipError) as e:
        h.viterbi_path()
    assert msg.decode().replace("gh_viterbi_path_masked:", "gh_viterbi_path:") in str(e.value)
    h.L = 3
    hz, _ = make_pair(t, L=3, offer_zero=True)
    assert call(hz) == _lib.GH_ERR_ARG and b"offer_zero" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="offer_zero"):
        hz.viterbi_path_masked(allow)
    fresh = Hansel(n, band=t.band)
    assert call(fresh) == _lib.GH_ERR_STATE and b"before any fill" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError, match="before any fill"):
        fresh.viterbi_path_masked(allow)


# 9. the CLI -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True], ids=["greedy", "exact"])
def test_cli_alternatives_and_pins(tmp_path, capsys, exact):
    v, n, h, o = _cli_oracle()
    cm = decode_cases.shape_of(o, n)["cm"]
    rev = v["snp_rev"]
    free = viterbi_ref.viterbi(o, n)
    # three pins: another allele at SNP 1; four alleles at SNP 1 and another one at SNP 2; an allele SNP 3 does not offer (infeasible)
    absent = next(s for s in VALID if not (cm[3] >> s) & 1)
    pins = [{1: "ACGTN-_"[_other(cm, 1, free["path"][1])]}, {1: "ACGT", 2: "ACGTN-_"[_other(cm, 2, free["path"][2])]}, {3: "ACGTN-_"[absent]}]
    specs = [",".join("%d:%s" % (rev[p - 1], a) for p, a in pp.items()) for pp in pins]
    out, plain = tmp_path / "out", tmp_path / "plain"
    out.mkdir()
    plain.mkdir()
    argv = [BAM, VCF, "hoot", "-s", "1", "-e", "20", "-p", "12"] + (["--exact"] if exact else [])
    assert cmd.main(argv + ["-o", str(plain)]) == 0
    capsys.readouterr()
    assert cmd.main(argv + ["-o", str(out), "--alternatives", "3"] + [a for s in specs for a in ("--pin", s)]) == 0
    err = capsys.readouterr().err
    assert sorted(os.listdir(plain)) == ["gretel.crumbs", "out.fasta", "snp.fasta"]          # what a run without the flags writes
    assert sorted(os.listdir(out)) == ["gretel.alternatives", "gretel.crumbs", "out.fasta", "snp.fasta"]
    for f in ("out.fasta", "snp.fasta", "gretel.crumbs"):
        assert (out / f).read_bytes() == (plain / f).read_bytes(), f
    assert "[NOTE] --pin 3: no candidate at SNP 3 under the constraints\n" in err and "--pin 1:" not in err and "--pin 2:" not in err
    # the file rebuilt from the references, before the spins: the matrix as the reads filled it
    mres = maxmarg_ref.marginals(o, n)
    alts = alternatives_of(mres["mm"], mres["cm"], 3)
    allow = np.concatenate([allow_of(n)[None], alts["allow"]] + [allow_of(n, pins=pp)[None] for pp in pins])
    ref = masked_ref.decode_sets(o, n, allow)
    s, _, states = h.viterbi_states()
    res = h.viterbi_spin(12, cmd.MIN_REMOVE) if exact else h.spin(12, cmd.MIN_REMOVE)
    paths = cmd.paths_of_spin(h, res, log=io.StringIO())
    keys = sorted(paths, key=lambda k: paths[k]["i_0"])
    rec = np.array([[q.i for q in paths[k]["hansel_path"]] for k in keys], dtype=np.uint8)
    want = cmd.alternatives_text((n, h.L, "A", 0, s, states, 3), ref, alts, [1, 2, 1], rec, [paths[k]["i_0"] for k in keys], rev)
    text = (out / "gretel.alternatives").read_text()
    got_rows, want_rows = [l.split("\t") for l in text.splitlines()], [l.split("\t") for l in want.splitlines()]
    assert len(got_rows) == len(want_rows) == 2 + len(alts["p"]) + 3
    for a, b in zip(got_rows, want_rows):                       # field by field
        assert a == b, (a, b)
    # ... and what the fields are, spelled out on the rows themselves
    m = len(alts["p"])
    assert 1 <= m <= 3 and got_rows[0] == ["# %d" % n, str(h.L), "A", "0", str(s), str(states), "3", str(m)]
    assert got_rows[1] == ["B", "%.6f" % free["ll_chain"], "".join("ACGTN-_"[c] for c in free["path"][1:])]
    for q in range(m):
        row, p = got_rows[2 + q], int(alts["p"][q])
        x = ref["paths"][1 + q]
        differ = np.flatnonzero(x[1:] != free["path"][1:]) + 1
        assert row[:5] == ["A", str(p), str(rev[p - 1]), "ACGTN-_"[alts["best"][q]], "ACGTN-_"[x[p]]] and x[p] == alts["alt"][q]
        assert row[6] == "%.6f" % ref["ll_chain"][1 + q] and row[7] == "%.6f" % (free["ll_chain"] - ref["ll_chain"][1 + q])
        assert row[8:11] == [str(len(differ)), str(differ[0]), str(differ[-1])] and p in differ
        assert row[-1] == "".join("ACGTN-_"[c] for c in x[1:])
        if exact and q == 0:
            assert float(row[5]) >= 0.0
    assert [r[:3] for r in got_rows[2 + m:]] == [["P", "1", "1"], ["P", "2", "2"], ["P", "3", "1"]]
    assert got_rows[-1][3:] == ["infeasible", "3"] and got_rows[-3][3] == "%.6f" % ref["ll_chain"][1 + m]
    # a pin at a position that is no SNP of the window, and a run the parser refuses: status 2, nothing decoded
    not_snp = next(q for q in range(1, 21) if q not in v["snp_fwd"])
    assert cmd.main(argv + ["-o", str(out), "--pin", "%d:A" % not_snp]) == 2
    assert "is not a SNP of the window" in capsys.readouterr().err
