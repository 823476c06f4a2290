"""Scoring given haplotypes, the parts that need no GPU: the test reference (tests/score_ref.py) over the C oracle held to the
Python oracle, util.known_snp_paths, the text of gretel.scores / gretel.known, the refusal of --known, and the ABI."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import score_ref
from conftest import ROOT
from gretel_amd import _lib, cmd, util
from gretel_amd.hansel import Hansel, SCORE_REC
from gretel_amd.synth import make_support_table
from oracle import gretel_ref as G
from oracle import hansel_ref
from oracle.c_oracle import COracle

INF = math.inf


class _PyOracle:
    """oracle.hansel_ref.Hansel behind the three names score_ref asks for: get_edge_weights_at and get_marginal_of_at called directly."""

    def __init__(self, h):
        self.h = h
        self.L = h.L

    def edge_weights(self, p, path):
        ew = self.h.get_edge_weights_at(p, [self.h.symbols[int(s)] for s in path])
        mask, w = 0, [0.0] * 7
        for s, v in ew.items():
            mask |= 1 << s.i
            w[s.i] = v
        return mask, w

    def marginal(self, s, p):
        return self.h.get_marginal_of_at(int(s), p)


@pytest.mark.parametrize("mode,mt,order", [("A", False, "ACGT-"), ("E", True, "ACGT-"), ("E", True, "T-GCA")])
def test_reference_over_c_oracle_equals_python_oracle(mode, mt, order):
    n = 12
    t = make_support_table(n, 300, k=4, n_haps=4, err=0.05, seed=3)
    b = t.bases.copy()
    b[np.random.default_rng(1).random(len(b)) < 0.05] = ord("-")
    t.bases = b
    spec = hansel_ref.HanselSpec(cond_mode=mode, marginal_term=mt, cand_order=order)
    ph = hansel_ref.Hansel.init_matrix(hansel_ref.SYMBOLS, hansel_ref.UNSYMBOLS, n, spec)
    G.fill_from_support(ph, t.reads(), n)
    co = COracle(n, t.band, "f32", mode, mt, use_libm=True, cand_order=order)
    co.fill(t)
    ph.L = co.L = 3
    original = score_ref.marginals(co, n)
    assert original == score_ref.marginals(_PyOracle(ph), n)
    # ragged cells and marginals that differ from the kept ones: one path reweighted on both
    p0 = co.generate_path()[0]
    co.reweight_path(p0, 0.37)
    G.reweight_hansel_from_path(ph, [ph.symbols[int(s)] for s in p0], 0.37)
    rng = np.random.default_rng(5)
    paths = rng.integers(0, 7, size=(12, n + 1)).astype(np.uint8)
    paths[0] = p0
    paths[1, 1:] = [hansel_ref.SYMBOLS.index(chr(c)) for c in t.haplotypes[0]]
    paths[2, 1:] = 4                                        # every position off
    a = score_ref.score(co, paths, n, order, original)
    b = score_ref.score(_PyOracle(ph), paths, n, order, original)
    assert a == b
    # ... and the definition spelt out once more for the recovered path, straight from the Python oracle's own calls
    x = [ph.symbols[6]] + [ph.symbols[int(s)] for s in p0[1:]]
    ll = hc = 0.0
    n_greedy = 0
    for p in range(1, n + 1):
        ew = ph.get_edge_weights_at(p, x)
        assert x[p] in ew
        ll += ew[x[p]]
        hc += math.log10(ph.get_marginal_of_at(x[p], p))
        others = [v for s, v in ew.items() if s != x[p]]
        assert a["weight"][0][p] == ew[x[p]]
        assert a["margin"][0][p] == (ew[x[p]] - max(others) if others else INF)
        best = None
        for s, v in ew.items():
            if best is None or v > ew[best]:
                best = s
        assert a["pick"][0][p] == best.i
        n_greedy += int(best == x[p])
    assert (a["ll_chain"][0], a["hp_current"][0], a["n_on"][0], a["n_greedy"][0], a["first_off"][0]) == (ll, hc, n, n_greedy, 0)
    assert a["hp_original"][0] != a["hp_current"][0]
    assert (a["n_on"][2], a["ll_chain"][2], a["min_margin"][2], a["min_marginal"][2], a["argmin_margin"][2], a["first_off"][2]) == \
        (0, 0.0, INF, INF, 0, 1)
    assert a["pick"][2][0] == 6 and a["weight"][2][1:] == [-INF] * n


def _vcf_h(positions):
    return {"N": len(positions), "snp_rev": dict(enumerate(positions)), "snp_fwd": {p: i for i, p in enumerate(positions)}}


def test_known_snp_paths(tmp_path):
    fa = tmp_path / "k.fasta"
    #            1234567890123456
    fa.write_text(">first some words\nACGTACGTAC\nGTACGT\n>second\nacgt-cRtacgtNcgt\n>short\nTTTTTTTT\n")
    v = _vcf_h([2, 5, 7, 8, 13, 16])
    names, paths = util.known_snp_paths(str(fa), v, Hansel(v["N"]))
    assert names == ["first", "second", "short"]
    assert paths.dtype == np.uint8 and paths.tolist() == [[6, 1, 0, 2, 3, 0, 3],
                                                          [6, 1, 5, 4, 3, 4, 3],
                                                          [6, 3, 3, 3, 3, 4, 4]]
    empty = tmp_path / "empty.fasta"
    empty.write_text("")
    with pytest.raises(ValueError):
        util.known_snp_paths(str(empty), v, Hansel(v["N"]))
    nohead = tmp_path / "nohead.fasta"
    nohead.write_text("ACGT\n")
    with pytest.raises(ValueError):
        util.known_snp_paths(str(nohead), v, Hansel(v["N"]))


def test_scores_text_and_known_text():
    res = dict(ll_chain=np.array([-12.25, 0.0, -3.0]), hp_current=np.zeros(3), hp_original=np.array([-4.5, 0.0, -1.0000004]),
               min_marginal=np.ones(3), min_margin=np.array([0.125, INF, -INF]), n_on=np.array([4, 0, 3], dtype=np.int32),
               n_greedy=np.array([4, 0, 1], dtype=np.int32), first_off=np.array([0, 1, 2], dtype=np.int32),
               argmin_margin=np.array([3, 0, 4], dtype=np.int32))
    snp_rev = {0: 11, 1: 25, 2: 40, 3: 77}
    head = (4, 3, "E", 1)
    assert cmd.scores_text(head, [0, 2, 5], res, snp_rev) == (
        "# 4\t3\tE\t1\n"
        "0\t-12.250000\t-4.500000\t4\t4\t0\t0.125000\t3\t40\n"
        "2\t0.000000\t0.000000\t0\t0\t1\tinf\t0\t0\n"
        "5\t-3.000000\t-1.000000\t1\t3\t2\t-inf\t4\t77\n")
    assert cmd.scores_text(head, ["mock_a", "mock_b", "c"], res, snp_rev, nearest=[(0, 0), (7, 2), (-1, -1)]) == (
        "# 4\t3\tE\t1\n"
        "mock_a\t-12.250000\t-4.500000\t4\t4\t0\t0.125000\t3\t40\t0\t0\n"
        "mock_b\t0.000000\t0.000000\t0\t0\t1\tinf\t0\t0\t7\t2\n"
        "c\t-3.000000\t-1.000000\t1\t3\t2\t-inf\t4\t77\t-1\t-1\n")
    assert cmd.scores_text((0, 1, "A", 0), [], {k: np.zeros(0) for k in res}, {}) == "# 0\t1\tA\t0\n"


def test_nearest_recovered():
    rec = np.array([[6, 0, 1, 2, 3], [6, 0, 1, 2, 0], [6, 3, 3, 3, 3]], dtype=np.uint8)
    known = np.array([[6, 0, 1, 2, 0], [0, 0, 1, 1, 1], [6, 3, 3, 3, 3], [6, 5, 5, 5, 5]], dtype=np.uint8)
    # (row 1 differs from both of the first two at two SNPs: the lowest i_0 wins; column 0 is no SNP)
    assert cmd.nearest_recovered(known, rec, [0, 4, 9]) == [(4, 0), (0, 2), (9, 0), (0, 4)]
    assert cmd.nearest_recovered(known, rec[:0], []) == [(-1, -1)] * 4


def test_known_without_records_is_refused_before_anything_is_read(tmp_path, capsys):
    empty = tmp_path / "empty.fasta"
    empty.write_text("\n")
    out = tmp_path / "out"
    argv = [str(tmp_path / "no_such.bam"), str(tmp_path / "no_such.vcf.gz"), "hoot", "-s", "1", "-e", "20", "-o", str(out)]
    assert cmd.main(argv + ["--known", str(empty)]) == 2
    err = capsys.readouterr().err
    assert err.startswith("[FAIL] ") and "holds no FASTA record" in err
    assert cmd.main(argv + ["--score-paths", "--known", str(tmp_path / "no_such.fasta")]) == 2
    assert capsys.readouterr().err.startswith("[FAIL] ")
    assert not out.exists()
    a = cmd.build_parser().parse_args(argv)
    assert a.score_paths is False and a.known is None and cmd.check_score_options(a) is None


def test_abi_declares_and_exports_the_entry_point():
    src = open(os.path.join(ROOT, "include", "gretel_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*gh_score_rec\s*;", src)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(typ, n.strip()) for n in names.split(",")]
    want = [("double", k) for k in ("ll_chain", "hp_current", "hp_original", "min_marginal", "min_margin")] + \
           [("int32_t", k) for k in ("n_on", "n_greedy", "first_off", "argmin_margin")]
    assert fields == want
    assert re.search(r"\bint\s+gh_score_paths\s*\(\s*gh_t\s*\*\s*h\s*,\s*const\s+uint8_t\s*\*\s*paths\s*,\s*int\s+n_paths\s*,\s*"
                     r"gh_score_rec\s*\*\s*recs\s*,\s*double\s*\*\s*weight\s*,\s*double\s*\*\s*margin\s*,\s*uint8_t\s*\*\s*pick\s*\)\s*;", src)
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), "gh_score_paths")
    assert len(_lib.load().gh_score_paths.argtypes) == 7
    # the binding's record and the numpy record Hansel.score_paths reads are that struct
    assert [(n, t) for n, t in _lib.gh_score_rec._fields_] == [(k, ctypes.c_double if t == "double" else ctypes.c_int32) for t, k in want]
    assert SCORE_REC.names == score_ref.FIELDS and SCORE_REC.itemsize == ctypes.sizeof(_lib.gh_score_rec) == 56
