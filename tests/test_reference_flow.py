"""The reference's control flow over a Hansel, call by call (CPU).

Three statements of gretel/gretel.py:79-98,102-189 have to agree on every protocol call, its arguments and its result:
the reference's own functions (executed from the reference tree, where it is present), oracle/gretel_ref.py's
restatement, and the recorded fixture tests/golden/reference_flow.json (tests/golden/make_reference_flow.py).  The C
oracle, which every large GPU parity test compares with, has to recover the same records from the same observations."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401
import flow_util as F
from oracle import gretel_ref as G
from oracle.c_oracle import COracle, SYMS, paths_to_str

CASES = F.load_cases()
IDS = [c["name"] for c in CASES]
WANTED = ["fixture_n4", "n24_default", "n24_E_mt", "n24_C_f64", "n24_order_T-GCA", "tie_ACGT-", "tie_CAGT-", "hole_n8",
          "tiny_n3_L5", "tiny_n2", "tiny_n1"]


@pytest.fixture(scope="module")
def reference():
    if not F.reference_present():
        pytest.skip("the reference tree is not at %r (set $%s)" % (F.reference_root(), F.REFERENCE_ENV))
    return F.load_reference_gretel()


def test_fixture_holds_the_cases():
    assert IDS[:len(WANTED)] == WANTED
    by = {c["name"]: c for c in CASES}
    recs = {k: F.path_records(F.unpack_trace(c["trace"])) for k, c in by.items()}
    assert len(recs["fixture_n4"]) == 6 and all(r[0] == "path" for r in recs["fixture_n4"])
    assert by["n24_default"]["L"] == 8
    assert recs["hole_n8"] == [("hole",)]
    for k in ("tiny_n3_L5", "tiny_n2", "tiny_n1"):
        assert recs[k][0][0] == "path"
    # the exact tie: the first path is the allele offered first, nothing else differs
    assert recs["tie_ACGT-"][0][1] == "_GAGT" and recs["tie_CAGT-"][0][1] == "_GCGT"


def test_loader_leaves_sys_modules_alone(reference):
    import sys
    assert reference.__name__ == "gretel.gretel"
    for k in ("gretel", "gretel.util", "gretel.gretel", "hansel"):
        assert k not in sys.modules


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_restatement_and_fixture_agree_live(case, reference):
    want = F.unpack_trace(case["trace"])
    ref_log, ref_err = F.run_flow(reference, F.oracle_for(case), case["n_snps"], case["paths"])
    own_log, _ = F.run_flow(G, F.oracle_for(case), case["n_snps"], case["paths"])
    F.assert_same_trace(own_log, ref_log, "oracle.gretel_ref against the reference")
    F.assert_same_trace(ref_log, want, "the reference against the fixture")
    assert ref_err == case["stderr"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_the_fixture(case):
    want = F.unpack_trace(case["trace"])
    log, _ = F.run_flow(G, F.oracle_for(case), case["n_snps"], case["paths"])
    F.assert_same_trace(log, want, "oracle.gretel_ref against the fixture")
    # the reweight calls of every path: the pair enumeration of gretel.py:79-96
    n = case["n_snps"]
    seq = [(e[1][2], e[1][3]) for e in want if e[0] == "reweight_observation"]
    n_paths = sum(1 for e in want if e[0] == "path")
    per = n * (n + 3) // 2 + 1
    assert len(seq) == n_paths * per
    for q in range(n_paths):
        assert seq[q * per:(q + 1) * per] == G.reweight_call_sequence(n)
    if want[-1] == ("hole",):
        last_path = max([q for q, e in enumerate(want) if e[0] == "path"], default=0)
        assert not any(e[0] == "reweight_observation" for e in want[last_path:])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_c_oracle_recovers_the_same_records(case):
    obs = F.case_observations(case)
    n = case["n_snps"]
    band = max(j - i for _, _, i, j in obs)
    o = COracle(n, band, **case["spec"])
    for a, b, i, j in obs:
        o.add(SYMS.index(a), SYMS.index(b), i, j)
    o.L = case["L"]
    res = o.spin(case["paths"])
    want = F.path_records(F.unpack_trace(case["trace"]))
    recs = [r for r in want if r[0] == "path"]
    assert res["n"] == len(recs)
    assert (res["hole_at"] != 0) == (want[-1] == ("hole",))
    assert paths_to_str(res["paths"]) == [r[1] for r in recs] if recs else res["n"] == 0
    assert [float(x).hex() for x in res["hp_current"]] == [r[2] for r in recs]
    assert [float(x).hex() for x in res["hp_original"]] == [r[3] for r in recs]
    assert [float(x).hex() for x in res["ratio"]] == [max(float.fromhex(r[4]), G.MIN_REMOVE).hex() for r in recs]
    for got, r in zip(res["magnitude"], recs):
        size = float.fromhex(r[5])
        assert abs(got - size) <= 1e-10 * abs(size)
    # ... and leaves the tensor the Python oracle is left with
    ph = F.oracle_for(case)
    F.run_flow(G, ph, n, case["paths"])
    assert np.array_equal(o.export_band(), F.dense_to_band(ph.dense(), band))
