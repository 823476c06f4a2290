"""K-best exact decoding of the chain likelihood, the parts that need no GPU: the test reference (tests/kbest_ref.py) over the C
oracle held to an exhaustive enumeration of every full path on the windows of tests/test_viterbi_host.py and the two tie windows --
its scores are the sorted top K as a list, bit for bit, every path re-scores to its own score, the paths are distinct, K = 1 is
viterbi_ref -- the two tie orders, holes, kbest_of and kbest_text on hand-written inputs, the refusals of --kbest, and the scratch
layout under AddressSanitizer + UBSan on the CPU (tests/native/vitk_layout.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import kbest_ref
import score_ref
import viterbi_ref
from conftest import ROOT
from gretel_amd import cmd
from gretel_amd.hansel import kbest_of
from test_viterbi_host import E_MT, WINDOWS, _every_path, _oracle, _str

TIES = [(["ACACAC", "CACACA"], 3, 3), (["AGTTACG", "CGTTACG"], 3, 3)]


@pytest.mark.parametrize("kw", [{}, E_MT, dict(cond_mode="C"), dict(cand_order="T-GCA")], ids=lambda kw: "-".join(map(str, kw.values())) or "default")
@pytest.mark.parametrize("haps,band,L", WINDOWS + TIES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_the_reference_returns_the_k_largest_scores_of_every_path(haps, band, L, kw):
    n = len(haps[0])
    order = kw.get("cand_order", "ACGT-")
    o = _oracle(haps, band, L, **kw)
    every, scores = _every_path(o, n, order)
    srt = sorted(scores, reverse=True)
    for k in (1, 2, 3, 8, 32):
        res = kbest_ref.kbest(o, n, k, order)
        assert res["hole_at"] == 0 and res["n"] == min(k, len(every))
        assert res["paths"].dtype == np.uint8 and res["paths"].shape == (res["n"], n + 1) and (res["paths"][:, 0] == 6).all()
        assert res["ll_chain"].tolist() == srt[:k]                                     # as a list: ties as often as they occur
        assert score_ref.score(o, res["paths"], n, order)["ll_chain"] == res["ll_chain"].tolist()
        assert len({x.tobytes() for x in res["paths"]}) == res["n"]
        if k == 1:
            v = viterbi_ref.viterbi(o, n, order)
            assert np.array_equal(v["path"], res["paths"][0]) and v["ll_chain"] == res["ll_chain"][0]


def test_the_windows_are_full_of_exact_ties():
    # (the tie rules are exercised, not decorative: equal neighbours among the sorted scores of the windows above)
    most = 0
    for haps, band, L in WINDOWS:
        o = _oracle(haps, band, L)
        _, scores = _every_path(o, len(haps[0]), "ACGT-")
        srt = sorted(scores, reverse=True)
        most = max(most, sum(1 for a, b in zip(srt, srt[1:]) if a == b))
    assert most >= 32


@pytest.mark.parametrize("order,want", [("ACGT-", ["CACACA", "ACACAC"]), ("T-GCA", ["ACACAC", "CACACA"])])
def test_a_tie_at_the_end_returns_both_in_the_end_rules_order(order, want):
    o = _oracle(["ACACAC", "CACACA"], 3, 3, cand_order=order)
    res = kbest_ref.kbest(o, 6, 2, order)
    assert res["n"] == 2 and res["ll_chain"][0] == res["ll_chain"][1]
    assert [_str(x) for x in res["paths"]] == want


@pytest.mark.parametrize("order,want", [("ACGT-", ["AGTTACG", "CGTTACG"]), ("T-GCA", ["CGTTACG", "AGTTACG"])])
def test_a_tie_where_two_prefixes_merge_returns_both_in_the_order_of_the_dropped_pick(order, want):
    o = _oracle(["AGTTACG", "CGTTACG"], 3, 3, cand_order=order)
    res = kbest_ref.kbest(o, 7, 2, order)
    assert res["n"] == 2 and res["ll_chain"][0] == res["ll_chain"][1]
    assert [_str(x) for x in res["paths"]] == want


@pytest.mark.parametrize("at", [1, 4, 6])
def test_a_hole_is_reported_where_it_is(at):
    o = _oracle(["ACGTAC", "CGTACG", "ACTTAG"], 3, 3, skip=(at,))
    res = kbest_ref.kbest(o, 6, 4)
    assert res["n"] == 0 and res["hole_at"] == at and res["paths"].shape == (0, 7) and res["ll_chain"].shape == (0,)


def test_kbest_of_on_hand_written_inputs():
    paths = np.array([[6, 0, 1, 2, 3], [6, 0, 1, 2, 0], [6, 1, 0, 3, 2], [6, 0, 0, 0, 0]], dtype=np.uint8)
    res = dict(n=4, hole_at=0, paths=paths, ll_chain=np.array([-1.5, -1.5, -4.0, -np.inf]))
    got = kbest_of(res)
    assert sorted(got) == ["gap", "hamming0"]
    assert got["gap"].tolist() == [0.0, 0.0, 2.5, np.inf] and got["hamming0"].tolist() == [0, 1, 4, 3]
    assert got["hamming0"].dtype == np.int32
    rec = np.array([[6, 1, 0, 3, 2], [6, 0, 1, 2, 0], [6, 0, 1, 2, 1]], dtype=np.uint8)
    got = kbest_of(res, rec)
    # rank 0 is one SNP from rows 1 and 2: the first wins; rank 1 IS row 1; rank 2 IS row 0; rank 3 is 3, 2 and 3 SNPs from the rows
    assert got["nearest"].tolist() == [1, 1, 0, 1] and got["distance"].tolist() == [1, 0, 0, 2]
    none = kbest_of(res, np.zeros((0, 5), dtype=np.uint8))
    assert none["nearest"].tolist() == [-1] * 4 and none["distance"].tolist() == [-1] * 4
    # every score -inf: no gap; nothing returned: empty arrays
    assert kbest_of(dict(n=2, paths=paths[:2], ll_chain=np.array([-np.inf, -np.inf])))["gap"].tolist() == [0.0, 0.0]
    empty = kbest_of(dict(n=0, paths=np.zeros((0, 5), dtype=np.uint8), ll_chain=np.zeros(0)), rec)
    assert all(len(empty[k]) == 0 for k in ("gap", "hamming0", "nearest", "distance"))
    with pytest.raises(ValueError):
        kbest_of(res, np.zeros((2, 4), dtype=np.uint8))


def test_kbest_text_on_hand_written_inputs():
    paths = np.array([[6, 0, 1, 5, 3], [6, 0, 1, 2, 0]], dtype=np.uint8)
    res = dict(n=2, hole_at=0, paths=paths, ll_chain=np.array([-1.25, -3.0]))
    per_rank = dict(gap=np.array([0.0, 1.75]), hamming0=np.array([0, 2]), nearest=np.array([1, 0]), distance=np.array([0, 3]))
    text = cmd.kbest_text((4, 3, "A", 0, 5, 125, 8, 2), res, per_rank, [0, 7])
    assert text == ("# 4\t3\tA\t0\t5\t125\t8\t2\n"
                    "0\t-1.250000\t0.000000\t0\t7\t0\tAC-T\n"
                    "1\t-3.000000\t1.750000\t2\t0\t3\tACGA\n")
    # nothing recovered: -1 and -1; -inf in the formats of gretel.scores
    per_rank = dict(gap=np.array([np.inf]), hamming0=np.array([0]), nearest=np.array([-1]), distance=np.array([-1]))
    res = dict(n=1, hole_at=0, paths=paths[:1], ll_chain=np.array([-np.inf]))
    assert cmd.kbest_text((4, 3, "E", 1, 4, 64, 1, 1), res, per_rank, []) == "# 4\t3\tE\t1\t4\t64\t1\t1\n0\t-inf\tinf\t0\t-1\t-1\tAC-T\n"


def test_kbest_options_are_refused_before_anything_is_read(tmp_path, capsys):
    out = tmp_path / "out"
    argv = [str(tmp_path / "no_such.bam"), str(tmp_path / "no_such.vcf.gz"), "hoot", "-s", "1", "-e", "20", "-o", str(out)]
    for k in ("0", "33", "-1"):
        assert cmd.main(argv + ["--kbest", k]) == 2
        assert capsys.readouterr().err.startswith("[FAIL] --kbest ")
    assert not out.exists()
    a = cmd.build_parser().parse_args(argv)
    assert a.kbest is None and cmd.check_kbest_options(a) is None
    for extra in (["--kbest", "1"], ["--kbest", "32"], ["--kbest", "8", "--exact"], ["--kbest", "8", "--beam", "4"]):
        assert cmd.check_kbest_options(cmd.build_parser().parse_args(argv + extra)) is None


def test_the_kbest_scratch_layout_is_what_its_user_spelled_out(tmp_path):
    exe = str(tmp_path / "vitk_layout")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gretel_amd", "csrc"), "-o", exe,
                         os.path.join(ROOT, "tests", "native", "vitk_layout.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert "vitk_layout done" in run.stdout
