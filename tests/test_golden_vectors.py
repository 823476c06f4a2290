"""Committed golden vectors (tests/golden/oracle_vectors.json, made by make_golden.py with the
Python oracle).  CPU: both oracles still reproduce them.  GPU: the HIP path reproduces them."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import gretel_ref as G
from oracle.c_oracle import COracle, paths_to_str
from oracle.hansel_ref import Hansel, HanselSpec, SYMBOLS, UNSYMBOLS

VEC = json.load(open(os.path.join(GOLDEN, "oracle_vectors.json")))["cases"]


class _T:
    def __init__(self, reads):
        self.rank = np.array([r for r, _ in reads], dtype=np.int32)
        self.off = np.concatenate([[0], np.cumsum([len(s) for _, s in reads])]).astype(np.int64)
        self.bases = np.frombuffer("".join(s for _, s in reads).encode(), dtype=np.uint8).copy()
        self.band = max(1, max(len(s) for _, s in reads) - 1)


@pytest.mark.parametrize("case", VEC, ids=[c["name"] for c in VEC])
def test_python_oracle_reproduces_golden(case):
    spec = HanselSpec(**case["spec"])
    h = Hansel.init_matrix(SYMBOLS, UNSYMBOLS, case["n_snps"], spec)
    assert list(G.fill_from_support(h, [tuple(r) for r in case["reads"]], case["n_snps"])) == case["stats"]
    assert h.L == case["L"]
    for p, c in case["counts"].items():
        assert [float(x) for x in h._counts(int(p))] == c
    recs, _ = G.recover_paths(h, case["n_snps"], len(case["records"]))
    assert recs == case["records"]
    assert float(h.dense().astype("float64").sum()) == case["final_sum"]


@pytest.mark.parametrize("case", VEC, ids=[c["name"] for c in VEC])
def test_c_oracle_reproduces_golden(case):
    t = _T([tuple(r) for r in case["reads"]])
    sp = case["spec"]
    o = COracle(case["n_snps"], t.band, use_libm=True, **sp)
    assert list(o.fill(t)) == case["stats"]
    r = o.spin(len(case["records"]))
    assert paths_to_str(r["paths"]) == [x["path"] for x in case["records"]]
    assert r["hp_current"].tolist() == [x["hp_current"] for x in case["records"]]
    assert r["magnitude"].tolist() == [x["magnitude"] for x in case["records"]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", VEC, ids=[c["name"] for c in VEC])
def test_hip_reproduces_golden(case):
    from gretel_amd.hansel import Hansel as DevHansel
    t = _T([tuple(r) for r in case["reads"]])
    sp = case["spec"]
    h = DevHansel(case["n_snps"], band=t.band, **sp)
    assert list(h.fill_from_support(t.rank, t.off, t.bases)) == case["stats"]
    assert h.L == case["L"]
    for p, c in case["counts"].items():
        assert h.counts_array(int(p))[:7].tolist() == c
    res = h.spin(len(case["records"]))
    assert [DevHansel.path_str(p) for p in res["paths"]] == [x["path"] for x in case["records"]]
    # libm's log10 made the vectors, the kernels' log10 (include/gh_detlog.h) is that function: the very doubles (bar: 1e-6)
    assert np.array_equal(res["hp_current"], np.array([x["hp_current"] for x in case["records"]], dtype=float), equal_nan=True)
    assert np.array_equal(res["hp_original"], np.array([x["hp_original"] for x in case["records"]], dtype=float), equal_nan=True)
    assert res["ratio"].tolist() == [x["ratio"] for x in case["records"]]
    assert np.allclose(res["magnitude"], [x["magnitude"] for x in case["records"]], rtol=1e-12, atol=0)
    assert abs(h.export_band().sum() - case["final_sum"]) <= 1e-9 * case["final_sum"]


def _pinning_windows():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_hanselx_vectors", os.path.join(GOLDEN, "make_hanselx_vectors.py"))
    kit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kit)
    return kit.windows()


@pytest.mark.gpu
def test_hip_matches_the_oracle_on_the_pinning_windows():
    """The windows of the pinning kit (tests/golden/make_hanselx_vectors.py: the fixture, L = 4, five-candidate positions,
    L = 7 -- the candidate pools --, a band of 12), five paths each through the product path under its default spec, against
    the C oracle: bit-exact.  tests/test_hanselx_pinning.py holds the oracle to what the real hanselx answers for these very
    windows once the kit has written tests/golden/hanselx_vectors.json; with this test that carries over to the HIP path."""
    from gretel_amd.hansel import Hansel as DevHansel
    for name, n, reads in _pinning_windows():
        t = _T(reads)
        h = DevHansel(n, band=t.band)
        o = COracle(n, t.band)
        assert tuple(h.fill_from_support(t.rank, t.off, t.bases)) == tuple(o.fill(t)), name
        assert h.L == o.L, name
        res, ref = h.spin(5), o.spin(5)
        assert res["n"] == ref["n"] and res["hole_at"] == ref["hole_at"], name
        assert np.array_equal(res["paths"], ref["paths"]), name
        for k in ("hp_current", "hp_original", "ratio"):
            assert res[k].tolist() == ref[k].tolist(), (name, k)
        assert np.allclose(res["magnitude"], ref["magnitude"], rtol=1e-12, atol=0), name
        assert np.array_equal(h.export_band(), o.export_band()), name
