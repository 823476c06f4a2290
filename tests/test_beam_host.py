"""Beam search over the chain likelihood, the parts that need no GPU: the test reference (tests/beam_ref.py) over the C oracle
held to the oracle's own greedy walk and recovery loop at width 1 and to an exhaustive ranking at a width that keeps every path,
and the refusals of --beam."""
import functools
import itertools

import numpy as np
import pytest

import beam_ref
import score_ref
from gretel_amd import cmd
from gretel_amd.synth import make_support_table, sprinkle_deletions
from oracle.c_oracle import COracle

SPECS = [dict(), dict(cond_mode="E", marginal_term=True), dict(storage="f64"), dict(cand_order="T-GCA")]


def _id(kw):
    return "-".join("%s=%s" % (k, v) for k, v in sorted(kw.items())) or "default"


@functools.lru_cache(maxsize=None)
def _table(which):
    if which == "a":
        t = make_support_table(60, 800, k=None, seed=5)
        sprinkle_deletions(t, 0.05, seed=6)
    else:                                                   # the 300-SNP table of tests/test_gpu_score.py
        t = make_support_table(300, 6000, k=None, seed=31)
        sprinkle_deletions(t, 0.05, seed=32)
    return t


def _oracle(t, L=None, **kw):
    o = COracle(t.n_snps, t.band, **kw)
    o.fill(t)
    if L is not None:
        o.L = L
    return o


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("kw", SPECS, ids=_id)
def test_width_one_is_the_greedy_walk(which, kw):
    t = _table(which)
    n = t.n_snps
    order = kw.get("cand_order", "ACGT-")
    o = _oracle(t, **kw)
    path, _ = o.generate_path()
    res = beam_ref.beam(o, n, 1, order)
    assert res["n"] == 1 and res["hole_at"] == 0 and np.array_equal(res["paths"][0], path)
    assert res["ll_chain"] == score_ref.score(o, path, n, order)["ll_chain"]
    # ... and the recovery loop at width 1 is the oracle's own
    spun = beam_ref.beam_spin(o, n, 1, 10, cand_order=order)
    ref = _oracle(t, **kw).spin(10)
    assert spun["n"] == ref["n"] == 10 and spun["hole_at"] == ref["hole_at"] == 0
    assert np.array_equal(spun["paths"], ref["paths"])
    for k in ("hp_current", "hp_original", "ratio", "magnitude"):
        assert spun[k].tolist() == ref[k].tolist(), k


def test_a_width_that_keeps_every_path_ranks_them_all():
    t = make_support_table(6, 200, k=None, seed=3)
    sprinkle_deletions(t, 0.1, seed=4)
    n = t.n_snps
    o = _oracle(t, L=3)
    res = beam_ref.beam(o, n, 5 ** n)
    # every valid path, scored on its own and sorted by the definition's key with the whole path standing in for the ranks
    cands = []
    for p in range(1, n + 1):
        mask, _ = o.edge_weights(p, np.full(n + 1, 6, dtype=np.uint8))
        cands.append([s for s in (0, 1, 2, 3, 5) if (mask >> s) & 1])
    every = [np.array((6,) + x, dtype=np.uint8) for x in itertools.product(*cands)]
    assert res["n"] == len(every) == 3840
    scores = score_ref.score(o, np.stack(every), n)["ll_chain"]
    assert sorted(scores, reverse=True) == res["ll_chain"]
    by_path = {x.tobytes(): s for x, s in zip(every, scores)}
    assert [by_path[x.tobytes()] for x in res["paths"]] == res["ll_chain"]
    assert len({x.tobytes() for x in res["paths"]}) == len(every)


def test_a_beam_finds_what_the_greedy_walk_misses():
    t = _table("a")
    o = _oracle(t)
    n = t.n_snps
    greedy, wide = beam_ref.beam(o, n, 1), beam_ref.beam(o, n, 4)
    print("ll_chain: width 1 %.3f, width 4 %.3f, %d SNPs differ" % (
        greedy["ll_chain"][0], wide["ll_chain"][0], int((greedy["paths"][0] != wide["paths"][0]).sum())))
    assert wide["n"] == 4 and wide["ll_chain"][0] > greedy["ll_chain"][0]
    assert wide["ll_chain"] == sorted(wide["ll_chain"], reverse=True)
    assert wide["ll_chain"] == score_ref.score(o, wide["paths"], n)["ll_chain"]


def test_a_hole_reports_where_and_the_prefix():
    haps = ["ACGTACGT", "CGTACGTA", "ACTTAGGT"]
    n, band = 8, 3
    o = COracle(n, band)
    for hap in haps:
        full = "_" + hap + "_"
        for i in range(n + 1):
            for d in range(1, band + 1):
                if i + d <= n + 1 and not (d == 1 and i == 4):          # nothing observed at SNP 4: no candidate there
                    o.add(beam_ref.SYMS.index(full[i]), beam_ref.SYMS.index(full[i + d]), i, i + d)
    o.L = 3
    assert o.generate_path() == (None, 4)
    for width in (1, 3):
        res = beam_ref.beam(o, n, width)
        assert res["n"] == 0 and res["hole_at"] == 4 and res["paths"].shape == (0, n + 1) and res["ll_chain"] == []
        assert res["prefix"].tolist() == beam_ref.beam(o, 3, width)["paths"][0].tolist() and len(res["prefix"]) == 4
    spun = beam_ref.beam_spin(o, n, 2, 5)
    assert spun["n"] == 0 and spun["hole_at"] == 4


def test_beam_options_are_refused_before_anything_is_read(tmp_path, capsys):
    out = tmp_path / "out"
    argv = [str(tmp_path / "no_such.bam"), str(tmp_path / "no_such.vcf.gz"), "hoot", "-s", "1", "-e", "20", "-o", str(out)]
    for extra in (["--beam", "33"], ["--beam", "-1"], ["--beam", "4", "--debughpos", "3,7"]):
        assert cmd.main(argv + extra) == 2
        assert capsys.readouterr().err.startswith("[FAIL] --beam ")
    assert not out.exists()
    a = cmd.build_parser().parse_args(argv)
    assert a.beam == 0 and cmd.check_beam_options(a) is None
    for extra in (["--beam", "32"], ["--beam", "1", "--debughpos", ","], ["--debughpos", "3"]):
        assert cmd.check_beam_options(cmd.build_parser().parse_args(argv + extra)) is None
