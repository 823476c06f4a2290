"""Max-marginals of the chain likelihood, the parts that need no GPU: the test reference (tests/maxmarg_ref.py) over the C oracle
held to an exhaustive enumeration of every full path on windows of 5..7 SNPs built cell by cell -- each entry EQUAL to the
brute-force maximum of fl(fwd_p + bwd_p), and within the two-summation-orders bound of the sequentially summed maximum -- then
margins_of, margins_text and the --margins flag."""
import itertools
import math

import numpy as np
import pytest

import maxmarg_ref
import score_ref
import viterbi_ref
from gretel_amd import cmd
from gretel_amd.hansel import margins_of
from oracle.c_oracle import COracle

SYMS = "ACGTN-_"
INF = math.inf
E_MT = dict(cond_mode="E", marginal_term=True)

# (the five windows of tests/test_viterbi_host.py, restated)
WINDOWS = [
    (["ACGTA", "CGTAC", "ACTTA", "ACTTA", "CCGAA"], 3, 2),
    (["ACGTAC", "CGTACG", "ACTTAG", "AC-TAC", "CGT-CG", "CGTACG"], 4, 3),
    (["ACGTACG", "CGTACGT", "ACTTAGG", "AGTTACG", "CCTAAGT", "CCTAAGT"], 3, 3),
    (["ACGTACG", "CGTACGT", "ACTTAGG", "AGT-ACG", "CC-AAGT"], 5, 1),
    (["ACGTAC", "CGTACG", "ACTTAG", "AGTTAC"], 6, 5),
]


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


def _every_path(o, n):
    """Every full path (cm(p) does not depend on the history), its weights w_1..w_N, and the candidate sets."""
    cands = []
    for p in range(1, n + 1):
        mask, _ = o.edge_weights(p, np.full(n + 1, 6, dtype=np.uint8))
        cands.append([s for s in (0, 1, 2, 3, 5) if (mask >> s) & 1])
    every = np.array([(6,) + x for x in itertools.product(*cands)], dtype=np.uint8)
    weights = []
    for x in every:
        weights.append([0.0] + [float(o.edge_weights(p, x)[1][int(x[p])]) for p in range(1, n + 1)])
    return every, weights, cands


def _brute(every, weights, cands, n):
    """mm by the sentence of the header: the maximum over the full paths through (p, c) of fl(fwd_p + bwd_p)."""
    mm = np.full((n + 1, 7), -INF)
    for x, w in zip(every, weights):
        fwd = [0.0] * (n + 1)
        for p in range(1, n + 1):
            fwd[p] = fwd[p - 1] + w[p]
        bwd = [0.0] * (n + 1)
        for p in range(n - 1, 0, -1):
            bwd[p] = w[p + 1] + bwd[p + 1]
        for p in range(1, n + 1):
            v = fwd[p] + bwd[p]
            if v > mm[p, int(x[p])]:
                mm[p, int(x[p])] = v
    return mm


@pytest.mark.parametrize("kw", [{}, E_MT, dict(cond_mode="C"), dict(cand_order="T-GCA")], ids=lambda kw: "-".join(map(str, kw.values())) or "default")
@pytest.mark.parametrize("haps,band,L", WINDOWS, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_the_reference_is_the_maximum_over_every_path_through_each_candidate(haps, band, L, kw):
    n = len(haps[0])
    order = kw.get("cand_order", "ACGT-")
    o = _oracle(haps, band, L, **kw)
    every, weights, cands = _every_path(o, n)
    res = maxmarg_ref.marginals(o, n)
    assert res["hole_at"] == 0 and res["mm"].shape == (n + 1, 7) and res["cm"].dtype == np.uint8
    assert res["cm"].tolist() == [0] + [sum(1 << s for s in c) for c in cands]
    # equal, bit for bit, to the brute-force maximum of fl(fwd_p + bwd_p); -inf where not offered and in row 0
    assert np.array_equal(res["mm"], _brute(every, weights, cands, n))
    # within N 2^-52 A of the sequentially summed maximum through (p, c), -inf exactly where that is
    seq = score_ref.score(o, every, n, order)["ll_chain"]
    finite = [sum(abs(v) for v in w) for w in weights if all(v > -INF for v in w)]
    assert finite
    bound = n * 2.0 ** -52 * max(finite)
    for p in range(1, n + 1):
        for c in cands[p - 1]:
            top = max(s for x, s in zip(every, seq) if int(x[p]) == c)
            got = float(res["mm"][p, c])
            if top == -INF:
                assert got == -INF
            else:
                assert got > -INF and abs(got - top) <= bound, (p, c, got, top, bound)
    assert res["mm"][n].max() == viterbi_ref.viterbi(o, n, order)["ll_chain"]


@pytest.mark.parametrize("at", [1, 4, 6])
def test_a_hole_is_reported_where_it_is(at):
    o = _oracle(["ACGTAC", "CGTACG", "ACTTAG"], 3, 3, skip=(at,))
    assert maxmarg_ref.marginals(o, 6) == dict(mm=None, cm=None, hole_at=at)


def _hand_table():
    # position 1: A and C offered, C larger; G holds a stray finite number but is NOT offered
    # position 2: T alone is offered
    # position 3: A, G and - offered: A and - tie at the top, G is an offered -inf
    mm = np.full((4, 7), -INF)
    cm = np.array([0, 0b000011, 0b001000, 0b100101], dtype=np.uint8)
    mm[1, 0], mm[1, 1], mm[1, 2] = -5.0, -3.5, -1.0
    mm[2, 3] = -3.5
    mm[3, 0], mm[3, 5] = -3.5, -3.5
    return mm, cm


def test_margins_of_on_a_hand_made_table():
    mm, cm = _hand_table()
    paths = np.array([[6, 1, 3, 0], [6, 0, 3, 5], [6, 2, 3, 2], [6, 1, 0, 5]], dtype=np.uint8)
    for order, best3 in (("ACGT-", 0), ("T-GCA", 5)):
        m = margins_of(mm, cm, paths, order)
        ref = maxmarg_ref.margins_of(mm, cm, paths, order)
        assert m["best"].tolist() == ref["best"] == [6, 1, 3, best3]              # the tie at 3: the first of cand_order
        assert m["gap"].tolist() == ref["gap"] == [0.0, 1.5, INF, 0.0]            # a sole candidate: +inf; a tie: 0
        assert m["regret"].tolist() == ref["regret"]
        assert m["regret"][0].tolist() == [0.0, 0.0, 0.0, 0.0]
        assert m["regret"][1].tolist() == [0.0, 1.5, 0.0, 0.0]
        assert m["regret"][2].tolist() == [0.0, INF, 0.0, INF]                     # not offered at 1; an offered -inf at 3
        assert m["regret"][3].tolist() == [0.0, 0.0, INF, 0.0]                     # not offered at 2
        assert m["max_regret"].tolist() == ref["max_regret"] == [0.0, 1.5, INF, INF]
        assert m["argmax_regret"].tolist() == ref["argmax_regret"] == [1, 1, 1, 2]
        assert m["n_best"].tolist() == ref["n_best"] == [3 if best3 == 0 else 2, 2 if best3 == 5 else 1, 1, 1 + int(best3 == 5)]
    # every entry -inf at a position: gap 0.0, and the regret of an offered allele there 0.0
    mm[2, 3] = -INF
    m = margins_of(mm, cm, paths[:1])
    assert m["gap"][2] == 0.0 and m["regret"][0, 2] == 0.0 and m["best"][2] == 3
    # the largest OTHER entry -inf beside a finite best: +inf
    mm, cm = _hand_table()
    mm[3, 5] = -INF
    assert margins_of(mm, cm, paths[:1])["gap"][3] == INF
    one = margins_of(mm, cm, paths[0])
    assert one["regret"].shape == (1, 4)


def test_margins_text_on_the_hand_made_table():
    mm, cm = _hand_table()
    paths = np.array([[6, 1, 3, 0], [6, 2, 3, 2]], dtype=np.uint8)
    m = margins_of(mm, cm, paths)
    text = cmd.margins_text((3, 2, "A", 0, 4, 16), [0, 7], m, mm, cm, [100, 205, 310])
    assert text == ("# 3\t2\tA\t0\t4\t16\n"
                    "H\t0\t3\t0.000000\t100\n"
                    "H\t7\t1\tinf\t100\n"
                    "S\t100\tC\t1.500000\t1.500000\t0.000000\t.\t.\t.\n"
                    "S\t205\tT\tinf\t.\t.\t.\t0.000000\t.\n"
                    "S\t310\tA\t0.000000\t0.000000\t.\tinf\t.\t0.000000\n")


def test_margins_parses(tmp_path):
    argv = [str(tmp_path / "no_such.bam"), str(tmp_path / "no_such.vcf.gz"), "hoot", "-s", "1", "-e", "20"]
    assert cmd.build_parser().parse_args(argv).margins is False
    for extra in (["--margins"], ["--margins", "--exact"], ["--margins", "--beam", "4"], ["--margins", "--score-paths"]):
        a = cmd.build_parser().parse_args(argv + extra)
        assert a.margins is True
        assert (cmd.check_beam_options(a) or cmd.check_exact_options(a) or cmd.check_score_options(a)) is None


def test_the_scratch_layout_is_what_the_kernels_spell_out(tmp_path):
    # vitm_layout (the function the library itself calls) against sizes and order written out by hand, under AddressSanitizer +
    # UBSan on the CPU: tests/native/vitm_layout.cpp, a stand-alone program
    import os
    import subprocess
    from conftest import ROOT
    exe = str(tmp_path / "vitm_layout")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gretel_amd", "csrc"), "-o", exe,
                         os.path.join(ROOT, "tests", "native", "vitm_layout.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert "vitm_layout done" in run.stdout
