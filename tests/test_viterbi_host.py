"""Exact decoding of the chain likelihood, the parts that need no GPU: the test reference (tests/viterbi_ref.py) over the C oracle
held to an exhaustive enumeration of every full path on windows of 5..7 SNPs built cell by cell -- its score is the maximum, its
path the member of the arg-max set the tie rule names -- and the refusals of --exact."""
import itertools

import numpy as np
import pytest

import score_ref
import viterbi_ref
from gretel_amd import cmd
from oracle.c_oracle import COracle

SYMS = "ACGTN-_"
E_MT = dict(cond_mode="E", marginal_term=True)


def _oracle(haps, band, L, skip=(), **kw):
    """The C oracle built cell by cell from whole haplotypes: every pair (i, i + d), d <= band, of '_' + hap + '_' except the
    cells (i, i + 1) with i in `skip` -- position i then has no candidate."""
    n = len(haps[0])
    o = COracle(n, band, **kw)
    for hap in haps:
        full = "_" + hap + "_"
        for i in range(n + 1):
            for d in range(1, band + 1):
                if i + d <= n + 1 and not (d == 1 and i in skip):
                    o.add(SYMS.index(full[i]), SYMS.index(full[i + d]), i, i + d)
    o.L = L
    return o


def _every_path(o, n, order):
    """Every full path (cm(p) does not depend on the history) and its sequentially summed score."""
    cands = []
    for p in range(1, n + 1):
        mask, _ = o.edge_weights(p, np.full(n + 1, 6, dtype=np.uint8))
        cands.append([s for s in (0, 1, 2, 3, 5) if (mask >> s) & 1])
    every = np.array([(6,) + x for x in itertools.product(*cands)], dtype=np.uint8)
    sc = score_ref.score(o, every, n, order)
    assert sc["n_on"] == [n] * len(every)
    return every, sc["ll_chain"]


def _argmax_set(every, scores):
    top = max(scores)
    return top, {"".join(SYMS[int(v)] for v in x[1:]) for x, s in zip(every, scores) if s == top}


def _str(path):
    return "".join(SYMS[int(v)] for v in path[1:])


WINDOWS = [
    (["ACGTA", "CGTAC", "ACTTA", "ACTTA", "CCGAA"], 3, 2),
    (["ACGTAC", "CGTACG", "ACTTAG", "AC-TAC", "CGT-CG", "CGTACG"], 4, 3),
    (["ACGTACG", "CGTACGT", "ACTTAGG", "AGTTACG", "CCTAAGT", "CCTAAGT"], 3, 3),
    (["ACGTACG", "CGTACGT", "ACTTAGG", "AGT-ACG", "CC-AAGT"], 5, 1),
    (["ACGTAC", "CGTACG", "ACTTAG", "AGTTAC"], 6, 5),
]


@pytest.mark.parametrize("kw", [{}, E_MT, dict(cond_mode="C"), dict(cand_order="T-GCA")], ids=lambda kw: "-".join(map(str, kw.values())) or "default")
@pytest.mark.parametrize("haps,band,L", WINDOWS, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_the_reference_finds_the_maximum_over_every_path(haps, band, L, kw):
    n = len(haps[0])
    order = kw.get("cand_order", "ACGT-")
    o = _oracle(haps, band, L, **kw)
    every, scores = _every_path(o, n, order)
    top, best = _argmax_set(every, scores)
    res = viterbi_ref.viterbi(o, n, order)
    assert res["hole_at"] == 0 and res["path"].dtype == np.uint8 and res["path"][0] == 6
    assert res["ll_chain"] == top
    assert _str(res["path"]) in best
    assert score_ref.score(o, res["path"], n, order)["ll_chain"] == [top]


def test_the_greedy_walk_is_not_always_the_maximum():
    # of these windows at least one has a greedy path below the maximum: the decoder is not the greedy walk restated
    below = 0
    for haps, band, L in WINDOWS:
        n = len(haps[0])
        o = _oracle(haps, band, L)
        greedy, _ = o.generate_path()
        g = score_ref.score(o, greedy, n)["ll_chain"][0]
        top = viterbi_ref.viterbi(o, n)["ll_chain"]
        assert top >= g
        below += int(top > g)
    assert below >= 1


@pytest.mark.parametrize("order,want", [("ACGT-", "CACACA"), ("T-GCA", "ACACAC")])
def test_a_tie_at_the_end(order, want):
    # two haplotypes with identical evidence tie exactly; at p = N the states are taken in ascending (q(x[N]), q(x[N-1]), ...):
    # the one whose LAST symbol comes first in the candidate order stays
    haps = ["ACACAC", "CACACA"]
    o = _oracle(haps, 3, 3, cand_order=order)
    every, scores = _every_path(o, 6, order)
    top, best = _argmax_set(every, scores)
    assert best == set(haps)
    res = viterbi_ref.viterbi(o, 6, order)
    assert res["ll_chain"] == top and _str(res["path"]) == want


@pytest.mark.parametrize("order,want", [("ACGT-", "AGTTACG"), ("T-GCA", "CGTTACG")])
def test_a_tie_where_two_prefixes_merge(order, want):
    # two haplotypes that differ at SNP 1 only, with identical evidence: their prefixes meet in one state at p = 1 + Le and are
    # taken in ascending q(x[1]); the first stays because the second is not strictly larger
    haps = ["AGTTACG", "CGTTACG"]
    o = _oracle(haps, 3, 3, cand_order=order)
    every, scores = _every_path(o, 7, order)
    top, best = _argmax_set(every, scores)
    assert best == set(haps)
    res = viterbi_ref.viterbi(o, 7, order)
    assert res["ll_chain"] == top and _str(res["path"]) == want


@pytest.mark.parametrize("at", [1, 4, 6])
def test_a_hole_is_reported_where_it_is(at):
    o = _oracle(["ACGTAC", "CGTACG", "ACTTAG"], 3, 3, skip=(at,))
    assert o.generate_path() == (None, at)
    res = viterbi_ref.viterbi(o, 6)
    assert res == dict(path=None, ll_chain=None, hole_at=at)
    spun = viterbi_ref.viterbi_spin(o, 6, 3)
    assert spun["n"] == 0 and spun["hole_at"] == at and spun["paths"].shape == (0, 7)


@pytest.mark.parametrize("L", [6, 9])
def test_with_L_at_least_N_the_state_is_the_whole_prefix(L):
    haps = ["ACGTAC", "CGTACG", "ACTTAG", "AGTTAC"]
    o = _oracle(haps, 6, L)
    every, scores = _every_path(o, 6, "ACGT-")
    top, best = _argmax_set(every, scores)
    res = viterbi_ref.viterbi(o, 6)
    # nothing ever competes before the end: the end rule alone picks, the first of the maximisers in its order
    q = {0: 0, 1: 1, 2: 2, 3: 3, 5: 4}
    first = min((x for x, s in zip(every, scores) if s == top), key=lambda x: [q[int(v)] for v in x[:0:-1]])
    assert res["ll_chain"] == top and np.array_equal(res["path"], first) and _str(first) in best


def test_the_spin_reweights_what_it_found():
    haps, band, L = WINDOWS[2]
    n = len(haps[0])
    o = _oracle(haps, band, L)
    first = viterbi_ref.viterbi(o, n)
    spun = viterbi_ref.viterbi_spin(o, n, 3)
    assert spun["n"] == 3 and spun["hole_at"] == 0
    assert np.array_equal(spun["paths"][0], first["path"]) and spun["ll_chain"][0] == first["ll_chain"]
    assert (spun["magnitude"] > 0).all() and (spun["ratio"] >= 0.01).all()


def test_exact_options_are_refused_before_anything_is_read(tmp_path, capsys):
    out = tmp_path / "out"
    argv = [str(tmp_path / "no_such.bam"), str(tmp_path / "no_such.vcf.gz"), "hoot", "-s", "1", "-e", "20", "-o", str(out)]
    for extra in (["--exact", "--beam", "4"], ["--exact", "--debughpos", "3,7"]):
        assert cmd.main(argv + extra) == 2
        assert capsys.readouterr().err.startswith("[FAIL] --exact ")
    assert not out.exists()
    a = cmd.build_parser().parse_args(argv)
    assert a.exact is False and cmd.check_exact_options(a) is None
    for extra in (["--exact"], ["--exact", "--debughpos", ","], ["--beam", "4"], ["--debughpos", "3"], ["--exact", "--score-paths"]):
        assert cmd.check_exact_options(cmd.build_parser().parse_args(argv + extra)) is None
