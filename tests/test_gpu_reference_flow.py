"""The device Hansel driven through the reference's control flow, call by call (GPU).

Everything here compares the device with tests/golden/reference_flow.json (recorded from the reference's own
generate_path / reweight_hansel_from_path, tests/golden/make_reference_flow.py) or with the oracles computed on the spot;
nothing reads the reference tree.  Doubles are compared as float.hex() strings: exactly, -0.0 apart from 0.0, a NaN equal
to a NaN (both print as 'nan').

  (a) test_dropin_call_by_call            `from hansel import Hansel` off gretel_amd/dropin, filled by add_observation only
  (b) test_fused_twin_in_lockstep         generate_path() / reweight_from_path() / spin() against the per-cell handle
  (c) test_mirror_functions               gretel_amd.gretel's two functions: return values and stderr
  (d) test_every_spec_against_python_oracle
  (e) test_edge_weights_at_their_edges    k_edge_weights, the score kernel and the beam on one definition
  (f) test_staged_lazily_banded_tensor
  (g) test_reweight_observation_edges
"""
import contextlib
import functools
import io
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
import flow_util as F
from spec_util import make_pair
from gretel_amd import gretel
from gretel_amd._lib import SymbolError, check
from gretel_amd.hansel import Hansel, HanselSymbol, _p
from gretel_amd.synth import make_support_table
from oracle import gretel_ref as G
from oracle import hansel_ref
from oracle.hansel_ref import HanselSpec, SYMBOLS, UNSYMBOLS

pytestmark = pytest.mark.gpu

CASES = F.load_cases()
IDS = [c["name"] for c in CASES]
S = {c: i for i, c in enumerate(SYMBOLS)}
DROPIN = os.path.join(ROOT, "gretel_amd", "dropin")


@pytest.fixture
def dropin(monkeypatch):
    """The class an unmodified `from hansel import Hansel` gets with gretel_amd/dropin on the path."""
    monkeypatch.syspath_prepend(DROPIN)
    sys.modules.pop("hansel", None)
    try:
        from hansel import Hansel as cls
        assert sys.modules["hansel"].__file__.startswith(DROPIN)
        yield cls
    finally:
        sys.modules.pop("hansel", None)


def _per_cell(case, cls=Hansel):
    """Created WITHOUT a band, filled with add_observation only (staged; gh_add_batch flushes them), the attributes set as
    gretel/util.py:329-333 does."""
    return F.fill_per_cell(cls.init_matrix(SYMBOLS, UNSYMBOLS, case["n_snps"], **case["spec"]), case)


def _imported(case):
    """A handle of the case's window that never saw a per-cell call: the band built on the host, gh_import_band."""
    obs = F.case_observations(case)
    n, band = case["n_snps"], max(j - i for _, _, i, j in obs)
    arr = np.zeros((n + 2, band, 7, 7))
    for a, b, i, j in obs:
        arr[i, j - i - 1, S[a], S[b]] += 1
    h = Hansel(n, band=band, **case["spec"])
    check(h._lib.gh_import_band(h._h, _p(arr)))
    h.L = case["L"]
    return h


def _f64(dense):
    return np.asarray(dense).astype(np.float64)


# (a) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dropin_call_by_call(case, dropin):
    n = case["n_snps"]
    h = _per_cell(case, dropin)
    assert (h.n_slices, h.n_crumbs, h.L) == (case["n_slices"], case["n_crumbs"], case["L"])
    copies = []
    device_copy = h.copy
    h.copy = lambda: copies.append(device_copy()) or copies[-1]          # (keep hold of run_flow's `original`)
    log, _ = F.run_flow(G, h, n, case["paths"])
    F.assert_same_trace(log, F.unpack_trace(case["trace"]), "the drop-in Hansel against the reference's recorded flow")
    ph = F.oracle_for(case)
    untouched = _f64(ph.dense()).copy()
    F.run_flow(G, ph, n, case["paths"])
    assert np.array_equal(h.export_dense(), _f64(ph.dense()))
    assert len(copies) == 1 and np.array_equal(copies[0].export_dense(), untouched)
    assert (copies[0].n_slices, copies[0].n_crumbs, copies[0].L) == (case["n_slices"], case["n_crumbs"], case["L"])


# (b) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_twin_in_lockstep(case):
    n = case["n_snps"]
    pc = _per_cell(case)
    orig = pc.copy()
    tw, sp = _imported(case), _imported(case)
    assert tw.band == pc.band and np.array_equal(tw.export_band(), pc.export_band())
    tw.snapshot_original()
    recs, hole = [], 0
    for _ in range(case["paths"]):
        path, prob, mn = G.generate_path(n, pc, orig)                 # per-cell lookups on the per-cell handle
        fused_pc = pc.generate_path(orig)                              # the fused walk on the SAME handle, after its single-cell writes
        fused_tw = tw.generate_path()
        if path is None:
            assert fused_pc[0] is None and fused_tw[0] is None and fused_pc[1] == fused_tw[1] >= 1
            assert fused_pc[2].tolist() == fused_tw[2].tolist()
            hole = fused_tw[1]
            break
        string = "".join(str(x) for x in path)
        for what, res in (("per-cell handle", fused_pc), ("twin", fused_tw)):
            assert res[0] is not None, what
            assert (Hansel.path_str(res[0]), F.fhex(res[1]), F.fhex(res[2]), F.fhex(res[3])) == \
                (string, F.fhex(prob["hp_current"]), F.fhex(prob["hp_original"]), F.fhex(mn)), what
        ratio = max(mn, G.MIN_REMOVE)
        size = G.reweight_hansel_from_path(pc, path, ratio)           # N(N+3)/2+1 single-cell writes
        mag = tw.reweight_from_path(fused_tw[0], ratio)
        assert abs(mag - size) <= 1e-10 * abs(size)
        assert np.array_equal(tw.export_band(), pc.export_band()), "tensors differ after path %d" % len(recs)
        recs.append((string, prob["hp_current"], prob["hp_original"], mn, ratio, size))
    res = sp.spin(case["paths"])
    assert res["n"] == len(recs) and res["hole_at"] == hole
    assert [Hansel.path_str(p) for p in res["paths"]] == [r[0] for r in recs]
    for k, key in ((1, "hp_current"), (2, "hp_original"), (3, "min_marginal"), (4, "ratio")):
        assert [F.fhex(x) for x in res[key]] == [F.fhex(r[k]) for r in recs], key
    assert np.allclose(res["magnitude"], [r[5] for r in recs], rtol=1e-10, atol=0)
    assert np.array_equal(sp.export_band(), pc.export_band())
    # ... and they are the reference's records
    want = [r for r in F.path_records(F.unpack_trace(case["trace"])) if r[0] == "path"]
    assert [(r[0], F.fhex(r[1]), F.fhex(r[2]), F.fhex(r[3]), F.fhex(r[5])) for r in recs] == [r[1:] for r in want]


# (c) -----------------------------------------------------------------------------------------------------------------
_RWGT = re.compile(r"^\[RWGT\] Ratio (\S+), Removed (\S+)$")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mirror_functions(case):
    n = case["n_snps"]
    h = _per_cell(case)
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        orig = h.copy()
        for rec in F.path_records(F.unpack_trace(case["trace"])):
            path, prob, mn = gretel.generate_path(n, h, orig)
            if rec == ("hole",):
                assert (path, prob, mn) == (None, None, None)
                break
            assert len(path) == n + 1 and all(isinstance(x, HanselSymbol) for x in path) and path[0] == h.symbols_d["_"]
            assert "".join(str(x) for x in path) == rec[1] and rec[1][0] == "_"
            assert sorted(prob) == ["hp_current", "hp_original"]
            assert (F.fhex(prob["hp_current"]), F.fhex(prob["hp_original"]), F.fhex(mn)) == rec[2:5]
            size = gretel.reweight_hansel_from_path(h, path, max(mn, G.MIN_REMOVE))
            want = float.fromhex(rec[5])
            assert abs(size - want) <= 1e-10 * abs(want)
    got, want = err.getvalue().split("\n"), case["stderr"].split("\n")
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        mg, mw = _RWGT.match(g), _RWGT.match(w)
        if mw:
            # ("Removed %.1f": the fused sum is within 1e-10 of the per-cell one, which can move the last printed digit by one)
            assert mg and mg.group(1) == mw.group(1) and abs(float(mg.group(2)) - float(mw.group(2))) <= 0.1 + 1e-9, (q, g, w)
        else:
            assert g == w, (q, g, w)


# (d) -----------------------------------------------------------------------------------------------------------------
SPECS = [dict(storage=st, cond_mode=m, marginal_term=mt) for st in ("f32", "f64") for m in "ABCDE" for mt in (False, True)]
SPECS += [dict(cand_order="G-TAC"), dict(offer_zero=True)]


@functools.lru_cache(maxsize=None)
def _window16():
    """16 SNPs, reads of 2..6 SNPs with '-' and 'N' sprinkled over the bases: (reads, rank, off, bases)."""
    t = make_support_table(16, 90, k=None, seed=17, k_lambda=6.0, k_min=2, k_max=6)
    rng = np.random.default_rng(4)
    reads = []
    for r, seq in t.reads():
        u = rng.random(6)
        reads.append((r, "".join("-" if u[q] < 0.06 else "N" if u[q] < 0.10 else c for q, c in enumerate(seq[:6]))))
    assert any("-" in s for _, s in reads) and any("N" in s for _, s in reads)
    rank = np.array([r for r, _ in reads], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in reads])]).astype(np.int64)
    bases = np.frombuffer("".join(s for _, s in reads).encode(), dtype=np.uint8)
    return reads, rank, off, bases


@pytest.mark.parametrize("spec", SPECS, ids=["-".join("%s" % v for v in s.values()) for s in SPECS])
def test_every_spec_against_python_oracle(spec):
    reads, rank, off, bases = _window16()
    n = 16
    ph = hansel_ref.Hansel.init_matrix(SYMBOLS, UNSYMBOLS, n, HanselSpec(**spec))
    stats = G.fill_from_support(ph, reads, n)
    h = Hansel(n, band=5, **spec)
    assert h.fill_from_support(rank, off, bases) == stats and h.L == ph.L
    want, _ = F.run_flow(G, ph, n, 2)
    assert [e[0] for e in F.path_records(want)] == ["path", "path"]       # (the window has no hole in its first two paths)
    log, _ = F.run_flow(G, h, n, 2)
    # (offer_zero offers candidates of zero count; should a weight come out as NaN, it has to be NaN on both sides: 'nan' == 'nan')
    F.assert_same_trace(log, want, "the device against oracle.hansel_ref under %r" % (spec,))
    assert np.array_equal(h.export_dense(), _f64(ph.dense()))


# (e) -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table40():
    t = make_support_table(40, 1500, k=5, seed=3)
    assert t.band == 4
    return t


@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("mt", [False, True])
@pytest.mark.parametrize("mode", list("ABCDE"))
def test_edge_weights_at_their_edges(mode, mt, storage):
    t = _table40()
    n = t.n_snps
    h, o = make_pair(t, storage=storage, cond_mode=mode, marginal_term=mt)
    p0 = o.generate_path()[0]                                     # make the counts ragged first
    o.reweight_path(p0, 0.37)
    h.reweight_from_path(p0, 0.37)
    rng = np.random.default_rng(11)
    valid = rng.choice([0, 1, 2, 3, 5], size=n)
    holed = valid.copy()
    holed[0::3] = 4                                               # an N or a '_' inside every three positions
    holed[1::6] = 6
    # (this table has no deletions: '-' is never observed; where an allele is missing too, take that one)
    unseen = [next(s for s in (0, 1, 2, 3, 5) if o.counts_at(p)[s] == 0) for p in range(1, n + 1)]
    histories = [np.array([6] + list(x), dtype=np.uint8) for x in (valid, holed, unseen, [4] * n)]
    for L in (1, 4, 6, 64):
        h.L = o.L = L
        for x in histories:
            sc = h.score_paths(x, per_position=True)
            for p in range(1, n + 1):                             # (1, 2, L-1, L, L+1 and N are among them)
                mask, w = o.edge_weights(p, x)
                got = h.get_edge_weights_at(p, x)
                assert [s.i for s in got] == [s for s in (0, 1, 2, 3, 5) if (mask >> s) & 1], (L, p)
                assert [F.fhex(v) for v in got.values()] == [F.fhex(w[s.i]) for s in got], (L, p)
                mine = got.get(h.symbols[int(x[p])])
                if mine is None:                                  # an off position: N, '_' or an allele not offered
                    assert sc["weight"][0, p] == -math.inf, (L, p)
                else:                                             # the score kernel's weight is k_edge_weights' bit for bit
                    assert F.fhex(sc["weight"][0, p]) == F.fhex(mine), (L, p)
        res = h.generate_path()
        beam = h.beam_paths(1)
        assert res[0] is not None and beam["n"] == 1 and np.array_equal(beam["paths"][0], res[0])
        ll = 0.0
        for p in range(1, n + 1):
            ll += h.get_edge_weights_at(p, res[0])[h.symbols[int(res[0][p])]]
        assert F.fhex(beam["ll_chain"][0]) == F.fhex(ll), L


# (f) -----------------------------------------------------------------------------------------------------------------
def _lookups(hz, n, path):
    """Every lookup of the protocol over the whole window, as a trace."""
    log = []
    r = F.Recorder(hz, log)
    for p in range(n + 1):
        r.get_counts_at(p)
        for s in SYMBOLS:
            r.get_marginal_of_at(s, p)
    for p in range(1, n + 1):
        r.get_edge_weights_at(p, path)
    return log


def _same_state(h, ph, n, path, what):
    assert (h.n_slices, h.n_crumbs, h.L) == (ph.n_slices, ph.n_crumbs, ph.L), what
    assert np.array_equal(h.export_dense(), _f64(ph.dense())), what
    F.assert_same_trace(_lookups(h, n, path), _lookups(ph, n, path), what)


def _both(h, ph, method, *args):
    a, b = getattr(h, method)(*args), getattr(ph, method)(*args)
    if isinstance(b, float):
        assert F.fhex(a) == F.fhex(b), (method, args, a, b)
    return a


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_staged_lazily_banded_tensor(storage):
    n = 12
    path = list("_ACGTACGTACGT")
    obs = [('_', 'A', 0, 1), ('_', 'C', 0, 1), ('A', 'C', 1, 2), ('A', 'C', 1, 2), ('C', 'C', 1, 2), ('A', 'G', 1, 4),
           ('C', 'G', 2, 3), ('C', 'T', 2, 3), ('G', 'T', 3, 4), ('C', 'T', 2, 4), ('T', '-', 4, 5), ('-', 'N', 5, 6),
           ('T', 'A', 4, 7), ('G', '_', 12, 13), ('T', 'G', 11, 12)]

    def pair():
        return (Hansel.init_matrix(SYMBOLS, UNSYMBOLS, n, storage=storage),
                hansel_ref.Hansel.init_matrix(SYMBOLS, UNSYMBOLS, n, HanselSpec(storage=storage)))
    # the attributes before any lookup: plain attributes, as on the oracle object
    h, ph = pair()
    assert (h.n_slices, h.n_crumbs, h.L) == (ph.n_slices, ph.n_crumbs, ph.L) == (0, 0, 1)
    for ob in obs[:6]:
        _both(h, ph, "add_observation", *ob)
    assert (h.n_slices, h.n_crumbs, h.L) == (ph.n_slices, ph.n_crumbs, ph.L)
    h.L = ph.L = 3
    h.n_slices = ph.n_slices = 4
    for ob in obs[6:]:                                            # (more observations after an attribute was set)
        _both(h, ph, "add_observation", *ob)
    h.n_crumbs = ph.n_crumbs = 15
    assert (h.n_slices, h.n_crumbs, h.L) == (ph.n_slices, ph.n_crumbs, ph.L) == (4, 15, 3)
    _same_state(h, ph, n, path, "after the staged fill")
    assert h.band == 3

    # copy() of a handle that still holds staged observations: complete, and independent of what follows
    h2, ph2 = pair()
    for ob in obs:
        _both(h2, ph2, "add_observation", *ob)
    h2.L = ph2.L = 2
    c2, pc2 = h2.copy(), ph2.copy()
    _both(h2, ph2, "add_observation", 'A', 'C', 1, 2)
    _both(c2, pc2, "reweight_observation", 'C', 'T', 2, 3, 0.25)
    _same_state(c2, pc2, n, path, "the copy of a staged handle")
    _same_state(h2, ph2, n, path, "the staged handle after its copy was reweighted")

    # an observation wider than the band, after lookups and a reweight: the tensor is re-banded, nothing is lost
    _both(h, ph, "reweight_observation", 'A', 'C', 1, 2, 0.3)
    _both(h, ph, "reweight_observation", 'A', 'G', 1, 4, 0.7)
    _both(h, ph, "add_observation", 'G', 'G', 2, 9)
    _same_state(h, ph, n, path, "after re-banding")
    assert h.band == 7 and h.get_observation('A', 'C', 1, 2) != 2
    _both(h, ph, "add_observation", 'A', 'C', 1, 2)               # ... and on a non-integer cell of the re-banded tensor
    _same_state(h, ph, n, path, "an observation on a reweighted cell")

    # copy() carries L, the statistics and the tensor; the two are independent afterwards
    c, pc = h.copy(), ph.copy()
    _same_state(c, pc, n, path, "the copy")
    _both(c, pc, "reweight_observation", 'T', '-', 4, 5, 0.5)
    _same_state(h, ph, n, path, "the source after its copy was reweighted")
    _both(h, ph, "reweight_observation", 'C', 'G', 2, 3, 0.125)
    c.L = pc.L = 5
    _same_state(c, pc, n, path, "the copy after its source was reweighted")
    _same_state(h, ph, n, path, "the source")


# (g) -----------------------------------------------------------------------------------------------------------------
def _cell_by_cell(haps, band, storage, L):
    n = len(haps[0])
    h = Hansel.init_matrix(SYMBOLS, UNSYMBOLS, n, storage=storage)
    ph = hansel_ref.Hansel.init_matrix(SYMBOLS, UNSYMBOLS, n, HanselSpec(storage=storage))
    for hap in haps:
        full = "_" + hap + "_"
        for i in range(n + 1):
            for d in range(1, band + 1):
                if i + d <= n + 1:
                    _both(h, ph, "add_observation", full[i], full[i + d], i, i + d)
    h.L = ph.L = L
    return h, ph


def _candidates(h, ph, n):
    for p in range(1, n + 1):
        keys = [s.i for s in ph.get_edge_weights_at(p, ["_"] * (n + 1))]
        assert [s for s in range(7) if (int(h.candidate_masks()[p]) >> s) & 1] == sorted(keys), p


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_reweight_observation_edges(storage):
    haps = ["ACGTAC", "ACGTAC", "AGGTTC", "CGTTAG"]                 # C at SNP 1 and G at SNP 6 are seen on one haplotype only
    n, band = 6, 2
    path = list("_ACGTAC")
    h, ph = _cell_by_cell(haps, band, storage, L=2)
    _same_state(h, ph, n, path, "filled")
    before = h.export_dense()
    # ratio 0.0: nothing is removed, nothing changes
    assert _both(h, ph, "reweight_observation", 'A', 'C', 1, 2, 0.0) == 0.0
    assert np.array_equal(h.export_dense(), before)
    # cells that are not there: outside the band (also with j = N + 1, also with i = 0), on the diagonal, the wrong way round
    for a, b, i, j in [('A', 'T', 1, 4), ('T', '_', 4, n + 1), ('_', 'G', 0, 3), ('A', 'A', 1, 1), ('C', 'A', 2, 1), ('_', '_', 0, 0)]:
        assert _both(h, ph, "reweight_observation", a, b, i, j, 0.5) == 0.0
    assert np.array_equal(h.export_dense(), before)
    _same_state(h, ph, n, path, "after the reweights that touch nothing")
    # a symbol index of 7
    with pytest.raises(SymbolError):
        h.reweight_observation(7, 0, 1, 2, 0.5)
    with pytest.raises(SymbolError):
        h.reweight_observation(0, 7, 1, 2, 0.5)
    assert np.array_equal(h.export_dense(), before)
    # the same cell twice in a row, as the reference does for adjacent pairs: the second mass comes from the reduced cell
    r1 = _both(h, ph, "reweight_observation", 'A', 'C', 1, 2, 0.3)
    r2 = _both(h, ph, "reweight_observation", 'A', 'C', 1, 2, 0.3)
    assert 0.0 < r2 < r1
    # ... and the boundary cell (N, N + 1), which lies inside the band
    assert _both(h, ph, "reweight_observation", 'C', '_', n, n + 1, 0.25) == 0.75
    _same_state(h, ph, n, path, "after the same cell twice")
    # ratio 1.0 on the only cell that gives C its count at SNP 1: the candidate goes
    assert (int(h.candidate_masks()[1]) >> 1) & 1
    assert _both(h, ph, "reweight_observation", 'C', 'G', 1, 2, 1.0) == 1.0
    assert not (int(h.candidate_masks()[1]) >> 1) & 1
    _candidates(h, ph, n)
    _same_state(h, ph, n, path, "after a candidate lost its last count")
    assert h.gap_check() == G.gap_check(ph, n) == -1
    want, _ = F.run_flow(G, ph.copy(), n, 2)
    F.assert_same_trace(F.run_flow(G, h.copy(), n, 2)[0], want, "recovery after the candidate went")
    # the last candidate of a position: a gap, and generate_path finds the hole there
    for a, b in (('C', 'G'), ('G', 'G'), ('G', 'T')):                # (every cell (2, 3) the haplotypes fill)
        assert _both(h, ph, "reweight_observation", a, b, 2, 3, 1.0) > 0.0
    assert ph.get_counts_at(2)["total"] == 0.0
    _candidates(h, ph, n)
    _same_state(h, ph, n, path, "after a position lost its last candidate")
    assert h.gap_check() == G.gap_check(ph, n) == 2
    assert G.generate_path(n, ph, ph) == (None, None, None)
    res = h.generate_path()
    assert res[0] is None and res[1] == 2 and Hansel.path_str(res[2]) == "_A"
    want, _ = F.run_flow(G, ph, n, 2)
    assert want[-1] == ("hole",)
    F.assert_same_trace(F.run_flow(G, h, n, 2)[0], want, "the hole")
