"""Scoring given haplotypes on the GPU (gh_score_paths, Hansel.score_paths, --score-paths / --known of gretel_amd.cmd) against
the plain statement of the definition (tests/score_ref.py over the C oracle): every record field and every per-position value
exactly equal -- the order of every addition is fixed, so there is no tolerance."""
import functools
import math
import os

import numpy as np
import pytest

import score_ref
from conftest import REFDATA
from gretel_amd import _lib, cmd, util
from gretel_amd.hansel import Hansel
from gretel_amd.synth import make_config, make_support_table, sprinkle_deletions
from oracle.c_oracle import COracle
from spec_util import make_pair, same, spec_id

pytestmark = pytest.mark.gpu
BAM = os.path.join(REFDATA, "test.bam")
VCF = os.path.join(REFDATA, "test.vcf.gz")
INF = math.inf
SYMS = "ACGTN-_"


def _truth(t):
    idx = np.array([SYMS.index(chr(c)) for c in t.haplotypes.ravel()], dtype=np.uint8).reshape(t.haplotypes.shape)
    return np.concatenate([np.full((len(idx), 1), 6, dtype=np.uint8), idx], axis=1)


def _random_paths(rng, H, n, syms=(0, 1, 2, 3, 4, 5, 6)):
    p = rng.choice(np.array(syms, dtype=np.uint8), size=(H, n + 1))
    p[:, 0] = 6
    return p


def _check(h, o, paths, original=None, per_position=True):
    """score_paths of `h` against score_ref over `o`; returns the GPU's dict."""
    got = h.score_paths(paths, per_position=per_position)
    ref = score_ref.score(o, paths, h.n, h._cfg["cand_order"], original)
    score_ref.assert_same(got, ref, per_position)
    for k in score_ref.FIELDS:
        assert got[k].dtype == (np.float64 if k in score_ref.FIELDS[:5] else np.int32) and got[k].shape == (len(ref[k]),)
    if per_position:
        assert got["pick"].dtype == np.uint8 and got["weight"].shape == got["margin"].shape == got["pick"].shape == (len(ref["pick"]), h.n + 1)
    return got


def _from_haps(haps, band, L, skip=(), **kw):
    """A device Hansel and the C oracle built cell by cell (add_observation) from whole haplotypes: every pair (i, i + d),
    d <= band, of '_' + hap + '_' except the cells (i, i + 1) with i in `skip` -- position i then has no candidate."""
    n = len(haps[0])
    h = Hansel(n, band=band, **kw)
    o = COracle(n, band, **{k: v for k, v in kw.items() if k in ("storage", "cond_mode", "marginal_term", "cand_order", "offer_zero")})
    for hap in haps:
        full = "_" + hap + "_"
        for i in range(n + 1):
            for d in range(1, band + 1):
                if i + d <= n + 1 and not (d == 1 and i in skip):
                    h.add_observation(full[i], full[i + d], i, i + d)
                    o.add(SYMS.index(full[i]), SYMS.index(full[i + d]), i, i + d)
    h.L = o.L = L
    return h, o


def _paths_of(strings):
    return np.array([[SYMS.index(c) for c in "_" + s] for s in strings], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _table300():
    t = make_support_table(300, 6000, k=None, seed=31)
    sprinkle_deletions(t, 0.05, seed=32)
    return t


# 1 -------------------------------------------------------------------------------------------------------------
def test_paths_of_a_spin_mid_recovery():
    t = make_config("C2", seed=6)
    h, o = make_pair(t)
    h.snapshot_original()
    o.snapshot_original()
    original = score_ref.marginals(o, t.n_snps)
    res, ref = h.spin(10), o.spin(10)
    same(res, ref)
    band = h.export_band()
    assert (band != np.floor(band)).any()                   # reweighted, non-integer cells
    rng = np.random.default_rng(1)
    paths = np.concatenate([res["paths"], _truth(t), _random_paths(rng, 30 - len(t.haplotypes), t.n_snps)])
    assert len(paths) == 40
    got = _check(h, o, paths, original)
    assert (got["n_on"][:10] == t.n_snps).all() and (got["n_on"][-5:] < t.n_snps).all()
    assert (got["hp_original"][:10] != got["hp_current"][:10]).all()
    assert np.array_equal(h.export_band(), band)
    same(h.spin(10), o.spin(10))                            # scoring disturbed nothing
    assert np.array_equal(h.export_band(), o.export_band())


# 2 -------------------------------------------------------------------------------------------------------------
def test_generate_path_consistency():
    t = _table300()
    h, o = make_pair(t)
    n = t.n_snps
    path, hc, ho, mn = h.generate_path()
    r = _check(h, o, path)
    assert r["n_greedy"][0] == r["n_on"][0] == n and r["first_off"][0] == 0
    assert (r["margin"][0, 1:] >= 0).all() and np.array_equal(r["pick"][0], path)
    assert (r["hp_current"][0], r["hp_original"][0], r["min_marginal"][0]) == (hc, ho, mn)
    assert r["min_margin"][0] == r["margin"][0, 1:].min() and r["argmin_margin"][0] == 1 + int(r["margin"][0, 1:].argmin())
    # another candidate at a mid-window SNP that was decided by a margin: the walk leaves the path there
    cm = h.candidate_masks()
    p = next(q for q in range(n // 2, n) if bin(int(cm[q])).count("1") >= 2 and 0 < r["margin"][0, q] < INF)
    flipped = path.copy()
    flipped[p] = next(s for s in (0, 1, 2, 3, 5) if s != path[p] and (int(cm[p]) >> s) & 1)
    r2 = _check(h, o, flipped)
    assert r2["margin"][0, p] < 0 and r2["pick"][0, p] == path[p] and r2["n_greedy"][0] < n and r2["n_on"][0] == n
    assert np.array_equal(r2["margin"][0, :p], r["margin"][0, :p])
    first_neg = 1 + int(np.flatnonzero(r2["margin"][0, 1:] < 0)[0])
    assert first_neg == p == 1 + int(np.flatnonzero(r2["pick"][0, 1:] != flipped[1:])[0])


# 3 -------------------------------------------------------------------------------------------------------------
SPECS = [dict(cond_mode=m, marginal_term=mt, storage=st) for m in "ABCDE" for mt in (False, True) for st in ("f32", "f64")]
SPECS += [dict(cand_order="G-TAC"), dict(offer_zero=True)]


@pytest.mark.parametrize("kw", SPECS, ids=spec_id)
def test_every_spec(kw):
    t = _table300()
    h, o = make_pair(t, L=4, **kw)
    n = t.n_snps
    h.snapshot_original()
    o.snapshot_original()
    original = score_ref.marginals(o, n)
    # (ragged cells, and current marginals that are no longer the kept ones)
    p0 = o.generate_path()[0]
    o.reweight_path(p0, 0.37)
    h.reweight_from_path(p0, 0.37)
    rng = np.random.default_rng(3)
    paths = np.concatenate([_truth(t), p0[None, :], _random_paths(rng, 2, n, syms=(0, 1, 2, 3, 5)), _random_paths(rng, 1, n)])
    assert len(paths) == 12
    got = _check(h, o, paths, original)
    assert ((h.candidate_masks()[1:] >> 5) & 1).any()       # '-' is offered somewhere
    if kw.get("offer_zero"):
        # an allele never seen at its position is offered, hence on
        cnt = np.array([[o.counts_at(p)[s] for s in range(7)] for p in range(n + 1)])
        q = 9
        zero_on = [p for p in range(1, n + 1) if cnt[p, paths[q, p]] == 0]
        assert zero_on and got["n_on"][q] == n and all(got["weight"][q, p] > -INF for p in zero_on)
    else:
        assert got["n_on"][9] < n


# 4 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("haps,L", [(["A", "C"], 5), (["AC", "CA", "AA"], 5), (["ACG", "CAG", "AAT"], 5)])
def test_windows_shorter_than_the_lag_count(haps, L):
    n = len(haps[0])
    h, o = _from_haps(haps, band=max(1, n - 1), L=L, cond_mode="E", marginal_term=True)
    paths = np.concatenate([_paths_of(haps), _random_paths(np.random.default_rng(n), 6, n)])
    _check(h, o, paths)


@pytest.mark.parametrize("k,L", [(3, 6), (None, 1), (None, 12), (None, 40)])
def test_lag_counts(k, L):
    # (k = 3: a band of 2 under six lags -- the lags beyond the band read zero cells)
    t = make_support_table(200, 4000, k=k, seed=41)
    h, o = make_pair(t, L=L)
    assert (t.band == 2) == (k == 3)
    top = int(np.argmax(t.abundances))                     # (the haplotype of the generator's tiling reads: seen everywhere)
    paths = np.concatenate([_truth(t)[top:top + 1], _truth(t)[:3], _random_paths(np.random.default_rng(L), 2, t.n_snps)])
    got = _check(h, o, paths)
    assert got["n_on"][0] == t.n_snps


# 5 -------------------------------------------------------------------------------------------------------------
def test_off_positions_inside_the_history():
    t = _table300()
    h, o = make_pair(t, L=4)
    n = t.n_snps
    cm = h.candidate_masks()
    base = _truth(t)[int(np.argmax(t.abundances))]         # (the haplotype of the generator's tiling reads: on everywhere)
    x = base.copy()
    x[10], x[20] = 4, 6                                     # N and '_'
    p = next(q for q in range(30, n - 5) if int(cm[q]) != 0x2F)
    x[p] = next(s for s in (0, 1, 2, 3, 5) if not (int(cm[p]) >> s) & 1)      # an allele never observed there
    all_off = np.full(n + 1, 4, dtype=np.uint8)
    got = _check(h, o, np.stack([base, x, all_off]))
    assert got["n_on"].tolist() == [n, n - 3, 0] and got["first_off"].tolist() == [0, 10, 1]
    for q in (10, 20, p):
        assert got["weight"][1, q] == got["margin"][1, q] == -INF and got["pick"][1, q] == got["pick"][0, q]
        assert not np.array_equal(got["weight"][1, q + 1:q + 5], got["weight"][0, q + 1:q + 5])
    assert (got["ll_chain"][2], got["hp_current"][2], got["hp_original"][2]) == (0.0, 0.0, 0.0)
    assert (got["min_marginal"][2], got["min_margin"][2], got["argmin_margin"][2], got["n_greedy"][2]) == (INF, INF, 0, 0)


def test_window_with_a_hole():
    haps = ["ACGTACGT", "CGTACGTA", "ACTTAGGT"]
    h, o = _from_haps(haps, band=3, L=3, skip=(4,))
    paths = np.concatenate([_paths_of(haps), _random_paths(np.random.default_rng(4), 5, 8)])
    got = _check(h, o, paths)
    assert (got["pick"][:, 4] == 255).all() and (got["weight"][:, 4] == -INF).all() and (got["margin"][:, 4] == -INF).all()
    assert got["first_off"][:3].tolist() == [4, 4, 4] and got["n_on"][:3].tolist() == [7, 7, 7]
    assert (got["weight"][:3, 5:] > -INF).all() and (got["pick"][:, 5:] != 255).all()


# 6 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,first", [("ACGT-", 0), ("CAGT-", 1), ("TG-CA", 1)])
def test_exact_ties_follow_the_candidate_order(order, first):
    haps = ["GAGT", "GCGT"]                                 # symmetric in A and C at SNP 2
    h, o = _from_haps(haps, band=2, L=2, cand_order=order)
    got = _check(h, o, _paths_of(haps))
    assert got["margin"][:, 2].tolist() == [0.0, 0.0] and got["weight"][0, 2] == got["weight"][1, 2]
    assert got["pick"][:, 2].tolist() == [first, first]
    assert got["n_greedy"].tolist() == ([4, 3] if first == 0 else [3, 4])
    assert got["min_margin"].tolist() == [0.0, 0.0] and got["argmin_margin"].tolist() == [2, 2]


# 7 -------------------------------------------------------------------------------------------------------------
def test_path_counts():
    t = _table300()
    h, o = make_pair(t, L=4)
    n = t.n_snps
    rng = np.random.default_rng(7)
    paths = np.concatenate([_truth(t), _random_paths(rng, 45, n, syms=(0, 1, 2, 3, 5)), _random_paths(rng, 12, n)])
    assert len(paths) == 65
    ref = score_ref.score(o, paths, n)
    for H in (0, 1, 63, 64, 65):
        got = h.score_paths(paths[:H], per_position=True)
        score_ref.assert_same(got, {k: v[:H] for k, v in ref.items()})
        assert got["weight"].shape == (H, n + 1) and got["n_on"].shape == (H,)
    one = h.score_paths(paths[3])                           # a single path is one row
    assert {k: v.tolist() for k, v in one.items()} == {k: ref[k][3:4] for k in score_ref.FIELDS}
    # more paths than one slab or one resident grid takes: every record is that of its source row
    got = h.score_paths(np.tile(paths[:60], (100, 1)))
    assert sorted(got) == sorted(score_ref.FIELDS)
    for k in score_ref.FIELDS:
        assert got[k].shape == (6000,) and got[k].tolist() == ref[k][:60] * 100, k


# 8 -------------------------------------------------------------------------------------------------------------
def test_handle_states():
    t = _table300()
    h, o = make_pair(t, L=4, cond_mode="E")         # (a column conditional: the to-major copy comes and goes)
    n = t.n_snps
    paths = np.concatenate([_truth(t)[:3], _random_paths(np.random.default_rng(8), 3, n)])

    def check(hh, original=None):
        before = hh.export_band()
        stats = (hh.L, hh.n_slices, hh.n_crumbs)
        got = _check(hh, o, paths, original)
        assert np.array_equal(hh.export_band(), before) and np.array_equal(before, o.export_band())
        assert (hh.L, hh.n_slices, hh.n_crumbs) == stats
        return got

    r0 = check(h)
    # single observations
    for a, b, i, j in [("A", "C", 5, 6), ("-", "G", 5, 7), ("T", "T", 150, 151), ("_", "A", 0, 1), ("G", "_", n, n + 1)]:
        h.add_observation(a, b, i, j)
        o.add(SYMS.index(a), SYMS.index(b), i, j)
    r1 = check(h)
    assert r1["ll_chain"].tolist() != r0["ll_chain"].tolist() and np.isfinite(r1["ll_chain"][:3]).all()
    # one cell reweighted
    a, b = int(paths[0, 40]), int(paths[0, 41])
    assert h.reweight_observation(a, b, 40, 41, 0.3) == o.reweight_obs(a, b, 40, 41, 0.3)
    check(h)
    # behind a snapshot and a path reweight the kept marginals are the snapshot's
    h.snapshot_original()
    original = score_ref.marginals(o, n)
    p0 = o.generate_path()[0]
    o.reweight_path(p0, 0.5)
    h.reweight_from_path(p0, 0.5)
    r3 = check(h, original)
    assert r3["hp_original"].tolist() != r3["hp_current"].tolist()
    # an exported tensor imported into a fresh handle (no snapshot there)
    f = Hansel(n, band=t.band, cond_mode="E")
    exported = h.export_band()
    _lib.check(f._lib.gh_import_band(f._h, exported.ctypes.data))
    f.L = 4
    r4 = _check(f, o, paths)
    assert r4["hp_original"].tolist() == r4["hp_current"].tolist() == r3["hp_current"].tolist()
    assert np.array_equal(f.export_band(), o.export_band())
    # a copy, scored on its own
    c = h.copy()
    r5 = _check(c, o, paths)
    assert r5["ll_chain"].tolist() == r3["ll_chain"].tolist() and np.array_equal(c.export_band(), h.export_band())


# 9 -------------------------------------------------------------------------------------------------------------
def test_refusals():
    t = make_support_table(100, 500, k=4, seed=3)
    h, _ = make_pair(t)
    L = _lib.load()
    paths = np.zeros((2, t.n_snps + 1), dtype=np.uint8)
    recs = np.zeros(2, dtype=np.dtype(_lib.gh_score_rec))

    def call(hh, p, k):
        return L.gh_score_paths(hh._h if hh is not None else None, p.ctypes.data if p is not None else None, k,
                                recs.ctypes.data, None, None, None)

    assert call(h, paths, 2) == _lib.GH_OK
    bad = paths.copy()
    bad[1, 7] = 7
    assert call(h, bad, 2) == _lib.GH_ERR_SYMBOL and b"not a symbol index" in L.gh_last_error()
    with pytest.raises(_lib.SymbolError):
        h.score_paths(bad)
    assert call(h, paths, -1) == _lib.GH_ERR_ARG and b"n_paths" in L.gh_last_error()
    assert call(h, None, 2) == _lib.GH_ERR_ARG and call(None, paths, 2) == _lib.GH_ERR_ARG
    assert L.gh_score_paths(h._h, paths.ctypes.data, 2, None, None, None, None) == _lib.GH_ERR_ARG
    recs[:] = 0
    recs["n_on"] = -7
    assert call(h, paths, 0) == _lib.GH_OK and (recs["n_on"] == -7).all()      # nothing written
    fresh = Hansel(t.n_snps, band=t.band)
    assert call(fresh, paths, 2) == _lib.GH_ERR_STATE and b"before any fill" in L.gh_last_error()
    with pytest.raises(_lib.GretelHipError):
        fresh.score_paths(paths)
    with pytest.raises(ValueError):
        h.score_paths(paths[:, :-1])


# 10 ------------------------------------------------------------------------------------------------------------
def test_cli_on_the_reference_fixture(tmp_path, capsys):
    argv = [BAM, VCF, "hoot", "-s", "1", "-e", "20", "-p", "12"]
    plain, scored = tmp_path / "plain", tmp_path / "scored"
    plain.mkdir()
    scored.mkdir()
    assert cmd.main(argv + ["-o", str(plain)]) == 0
    cap0 = capsys.readouterr()
    v = util.process_vcf(VCF, "hoot", 1, 20)
    n = v["N"]
    lines = (plain / "snp.fasta").read_text().splitlines()
    i0s = [int(lines[q][1:].split("__")[0]) for q in range(0, len(lines), 2)]
    rec = _paths_of([lines[q + 1] for q in range(0, len(lines), 2)])
    assert len(i0s) >= 1 and rec.shape == (len(i0s), n + 1)

    def contig_seq(row):
        seq = ["N"] * 20
        for j in range(n):
            seq[v["snp_rev"][j] - 1] = SYMS[row[j + 1]]
        return "".join(seq)

    have = {r.tobytes() for r in rec}
    mid = 1 + n // 2
    for s in (0, 1, 2, 3):
        altered = rec[0].copy()
        altered[mid] = s
        if altered.tobytes() not in have:
            break
    assert altered.tobytes() not in have
    known = np.stack([rec[0], rec[-1], altered])
    fa = tmp_path / "K.fasta"
    fa.write_text(">same_first\n%s\n>same_last the last one\n%s\n>altered\n%s\n" % tuple(contig_seq(r).lower() if q == 1 else contig_seq(r)
                                                                                         for q, r in enumerate(known)))
    assert cmd.main(argv + ["-o", str(scored), "--score-paths", "--known", str(fa)]) == 0
    cap1 = capsys.readouterr()
    assert cap0.out == cap1.out and cap0.err == cap1.err
    for f in ("out.fasta", "snp.fasta", "gretel.crumbs"):
        assert (plain / f).read_bytes() == (scored / f).read_bytes(), f
    assert sorted(os.listdir(scored)) == sorted(os.listdir(plain) + ["gretel.scores", "gretel.known"])
    # what Hansel.score_paths gives on a fresh fill
    h = util.load_from_bam(BAM, "hoot", 1, 20, v)
    capsys.readouterr()
    head = (n, h.L, "A", 0)
    assert (scored / "gretel.scores").read_text() == cmd.scores_text(head, i0s, h.score_paths(rec), v["snp_rev"])
    names, kp = util.known_snp_paths(str(fa), v, h)
    assert names == ["same_first", "same_last", "altered"] and np.array_equal(kp, known)
    dist = [[int((k[1:] != r[1:]).sum()) for r in rec] for k in known]
    near = [(i0s[d.index(min(d))], min(d)) for d in dist]
    assert near[0] == (i0s[0], 0) and near[1][1] == 0 and near[2][1] == 1
    text = (scored / "gretel.known").read_text()
    assert text == cmd.scores_text(head, names, h.score_paths(kp), v["snp_rev"], nearest=near)
    rows = [ln.split("\t") for ln in text.splitlines()[1:]]
    assert [r[0] for r in rows] == names and [r[-1] for r in rows] == ["0", "0", "1"] and rows[0][-2] == str(i0s[0])
    # the scores agree with what the run itself reported: hp_original of a recovered haplotype is its first hp_original
    # (and the walk follows it everywhere on the matrix it was found on)
    crumbs = {int(ln.split("\t")[0]): ln.split("\t") for ln in (plain / "gretel.crumbs").read_text().splitlines()[1:]}
    first = (scored / "gretel.scores").read_text().splitlines()[1].split("\t")
    assert int(first[0]) == i0s[0] and first[3] == first[4] == str(n) and first[5] == "0"
    assert "%.2f" % float(first[2]) == crumbs[i0s[0]][3].split(",")[0]
