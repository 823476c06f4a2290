#!/usr/bin/env python3
"""Generates tests/golden/reference_flow.json: the per-cell protocol of the REFERENCE's own generate_path and
reweight_hansel_from_path (gretel/gretel.py, executed from the reference tree by tests/flow_util.load_reference_gretel)
over the Python oracle Hansel, call by call -- every argument and every returned double -- plus the stderr they wrote.

These are recorded results of the reference's program, not its text.  The Hansel arithmetic underneath is the oracle's
(oracle/hansel_ref.py: "parity unpinned"); what the fixture pins is the control flow around it: the call order, the
arg-max over the dict's iteration order, the pair enumeration of the reweight, the hole.

    python tests/golden/make_reference_flow.py        (needs the reference tree: $GRETEL_REFERENCE_ROOT)

Cases are only ever APPENDED, by name, and every case carries its own observations: gretel_amd.synth only helped to
draw them and may change later.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import flow_util as F                                                  # noqa: E402
from gretel_amd.synth import make_support_table, sprinkle_deletions    # noqa: E402
from oracle import gretel_ref as G                                     # noqa: E402
from oracle.hansel_ref import Hansel, HanselSpec, SYMBOLS, UNSYMBOLS   # noqa: E402


def _from_reads(n, reads):
    """The observations of a support table, in the fill's order (gretel/util.py:226-286), and the attributes it sets."""
    log = []
    h = F.Recorder(Hansel.init_matrix(SYMBOLS, UNSYMBOLS, n), log)
    G.fill_from_support(h, reads, n)
    return [e[1] for e in log], h.n_slices, h.n_crumbs, h.L


def _from_haps(haps, band, L, skip=()):
    """Cell by cell from whole haplotypes, as _from_haps of tests/test_gpu_score.py: every pair (i, i + d), d <= band, of
    '_' + hap + '_' except the cells (i, i + 1) with i in `skip`."""
    n = len(haps[0])
    obs = []
    for hap in haps:
        full = "_" + hap + "_"
        for i in range(n + 1):
            for d in range(1, band + 1):
                if i + d <= n + 1 and not (d == 1 and i in skip):
                    obs.append((full[i], full[i + d], i, i + d))
    return obs, len(haps), len(obs), L


def _n24():
    t = make_support_table(24, 150, k=None, seed=5, k_lambda=10.0, k_min=2, k_max=8)
    sprinkle_deletions(t, 0.15, seed=6)
    reads = [(r, seq[:8]) for r, seq in t.reads()]           # (the generator's tiling reads are k_lambda long)
    assert {len(seq) for _, seq in reads} <= set(range(2, 9)) and any("-" in seq for _, seq in reads)
    obs, s, c, L = _from_reads(24, reads)
    assert L == 8, L
    return obs, s, c, L


_TIE = ["GAGT", "GCGT"]                          # symmetric in A and C at SNP 2
_EIGHT = ["ACGTACGT", "ACGTACGT", "AGGTTCGA", "CCTTAGGA"]
CASES = [
    dict(name="fixture_n4", window=lambda: _from_reads(4, [(0, "AAA"), (0, "CCC"), (0, "TT"), (0, "TT"), (2, "GG")]), n_snps=4,
         paths=6, spec={}),
    dict(name="n24_default", window=_n24, n_snps=24, paths=3, spec={}),
    dict(name="n24_E_mt", window=_n24, n_snps=24, paths=3, spec=dict(cond_mode="E", marginal_term=True)),
    dict(name="n24_C_f64", window=_n24, n_snps=24, paths=3, spec=dict(cond_mode="C", storage="f64")),
    dict(name="n24_order_T-GCA", window=_n24, n_snps=24, paths=3, spec=dict(cand_order="T-GCA")),
    dict(name="tie_ACGT-", window=lambda: _from_haps(_TIE, 2, 2), n_snps=4, paths=3, spec=dict(cand_order="ACGT-")),
    dict(name="tie_CAGT-", window=lambda: _from_haps(_TIE, 2, 2), n_snps=4, paths=3, spec=dict(cand_order="CAGT-")),
    dict(name="hole_n8", window=lambda: _from_haps(_EIGHT, 3, 3, skip=(4,)), n_snps=8, paths=3, spec={}),
    dict(name="tiny_n3_L5", window=lambda: _from_haps(["ACG", "ACG", "ATG", "CTT"], 2, 5), n_snps=3, paths=3, spec={}),
    dict(name="tiny_n2", window=lambda: _from_haps(["AC", "AC", "GT"], 2, 2), n_snps=2, paths=3, spec={}),
    dict(name="tiny_n1", window=lambda: _from_haps(["A", "A", "C"], 1, 1), n_snps=1, paths=3, spec={}),
]


def run(case, ref):
    obs, n_slices, n_crumbs, L = case["window"]()
    cells = {}
    for ob in obs:                                   # (first-appearance order, a count per cell: integer counts add up exactly)
        cells[ob] = cells.get(ob, 0) + 1
    out = dict(name=case["name"], n_snps=case["n_snps"], spec=case["spec"], paths=case["paths"], n_slices=n_slices,
               n_crumbs=n_crumbs, L=L,
               obs=dict(syms="".join(a + b for a, b, _, _ in cells), pos=[x for (_, _, i, j), c in cells.items() for x in (i, j, c)]))
    log, err = F.run_flow(ref, F.oracle_for(out), case["n_snps"], case["paths"])
    assert log == F.unpack_trace(F.pack_trace(log))
    out["trace"] = F.pack_trace(log)
    out["stderr"] = err
    return out


def dump(doc, path):
    with open(path, "w") as fh:
        fh.write('{"note":%s,\n"cases":[\n' % json.dumps(doc["note"]))
        fh.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in doc["cases"]))
        fh.write("\n]}\n")


if __name__ == "__main__":
    path = F.FIXTURE
    doc = json.load(open(path)) if os.path.exists(path) else dict(
        note="recorded from the reference's gretel/gretel.py over oracle/hansel_ref.py; see make_reference_flow.py", cases=[])
    have = {c["name"] for c in doc["cases"]}
    todo = [c for c in CASES if c["name"] not in have]
    new = []
    if todo:
        ref = F.load_reference_gretel()
        new = [run(c, ref) for c in todo]
    doc["cases"] += new
    dump(doc, path)
    print("wrote", path, "added", [c["name"] for c in new])
