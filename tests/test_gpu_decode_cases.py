"""The decoders over the chain table on the seeded random windows of tests/decode_cases.py -- alphabets of 1..5 symbols with gaps,
positions that offer fewer candidates than the window's S, 3^k and other state counts between the powers the fixed windows have,
lags beyond the band, every cond_mode with and without the marginal term, f64, permuted candidate orders, K that is no power of
two, holes, refusals beyond the cap -- against the plain references over the C oracle, which tests/test_decode_cases_host.py holds
to each other and to an exhaustive enumeration on the same windows.  Everything is compared exactly (tests/decode_checks.py);
only the removed mass of a reweight goes through its relative 1e-10.  A failure names the seed and the window's description.

Per window (items 1-7 of decode_checks.check_case): viterbi_path and viterbi_info, viterbi_marginals, viterbi_kbest(K),
beam_paths(width), score_paths of the k best and of bent copies of them, the refusals beyond the cap, and after viterbi_spin(2)
on both sides the band and the three exact calls once more.  Then the panel forms on fresh handles, against the references and
against the single calls, and every fourth window in a child process that reads the table blocks from global memory."""
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import decode_cases
import decode_checks
import viterbi_ref
from decode_cases import CASES, PANEL, PANELS
from decode_util import _same_spin
from gretel_amd.hansel import HanselPanel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 12                 # windows a test id
CHILD_EVERY = 4


@functools.lru_cache(maxsize=None)
def _case(seed):
    """(desc, table, the references on the tensor as filled): computed once, shared, never changed."""
    desc, t = decode_cases.case(seed)
    return desc, t, decode_cases.references(desc, decode_cases.oracle_of(desc, t))


def _named(seed, desc, e):
    return AssertionError("seed %d %r: %s" % (seed, desc, e))


@pytest.mark.parametrize("first", range(0, len(CASES), BLOCK))
def test_every_decoder_against_its_reference(first):
    for seed in CASES[first:first + BLOCK]:
        desc, t, ref = _case(seed)
        try:
            decode_checks.check_case(desc, t, ref)
        except AssertionError as e:
            raise _named(seed, desc, e) from e


@pytest.mark.parametrize("q", range(PANELS))
def test_the_panel_forms_against_the_references_and_the_single_calls(q):
    # (the spec a panel runs under is chosen in decode_cases.PANEL_SPECS; tests/test_decode_cases_host.py asserts what the panels hold)
    wins = decode_cases.panel_windows(q, lambda seed: _case(seed)[2]["over"])
    pairs = [decode_checks.pair_of(desc, t) for desc, t in wins]         # fresh handles: nothing has touched them
    hs, ks = [h for h, _ in pairs], [desc["K"] for desc, _ in wins]
    refs = [decode_cases.references(desc, o) for (desc, _), (_, o) in zip(wins, pairs)]
    panel = HanselPanel(hs)
    mm, kb = panel.viterbi_marginals(), panel.viterbi_kbest(ks)
    for (desc, t), h, ref, m, k in zip(wins, hs, refs, mm, kb):
        try:
            n = desc["N"]
            decode_checks.same_marginals(m, ref["mm"], n)
            decode_checks.same_kbest(k, ref["kb"], n)
            decode_checks.same_marginals(m, h.viterbi_marginals(), n)           # ... and the single calls on the same handle
            decode_checks.same_kbest(k, h.viterbi_kbest(desc["K"]), n)
        except AssertionError as e:
            raise _named(desc["seed"], desc, e) from e
    holes = sum(1 for r in refs if r["vit"]["hole_at"])
    assert len(hs) == PANEL and 1 <= holes < PANEL
    assert panel.viterbi_marginals_info()[:2] == panel.viterbi_kbest_info()[:2] == (PANEL, holes)
    # the exact spin: the panel against the reference, and against the single call on a twin that nothing has touched
    spun = panel.viterbi_spin(2)
    for (desc, t), (h, o), res in zip(wins, pairs, spun):
        try:
            _same_spin(res, viterbi_ref.viterbi_spin(o, desc["N"], 2, cand_order=desc["spec"]["cand_order"]))
            assert np.array_equal(h.export_band(), o.export_band()), "export_band after the panel's viterbi_spin(2)"
            twin = decode_checks.pair_of(desc, t)[0]
            alone = twin.viterbi_spin(2)
            _same_spin(res, alone)
            assert res["magnitude"].tolist() == alone["magnitude"].tolist()
            assert np.array_equal(h.export_band(), twin.export_band())
        except AssertionError as e:
            raise _named(desc["seed"], desc, e) from e


CHILD = """
import pickle, sys
sys.path[:0] = [%r, %r]
import decode_cases, decode_checks
out = {}
for seed in decode_cases.CASES[::%d]:
    desc, t = decode_cases.case(seed)
    h, o = decode_checks.pair_of(desc, t)
    if decode_cases.shape_of(o, desc["N"])["states"] <= decode_cases.CAP:
        out[seed] = decode_checks.gpu_exact(h, desc["K"])
with open(sys.argv[1], "wb") as f:
    pickle.dump(out, f)
"""


def test_the_tables_from_global_memory_give_the_same_bits(tmp_path):
    # GH_VIT_STAGE is read once in a process: a fresh child runs items 1-3, the references are compared here
    env = dict(os.environ, GH_VIT_STAGE="0")
    out = str(tmp_path / "exact.pkl")
    subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), CHILD_EVERY), out], env=env, check=True, timeout=300)
    with open(out, "rb") as f:
        got = pickle.load(f)
    served = [seed for seed in CASES[::CHILD_EVERY] if not _case(seed)[2]["over"]]
    assert sorted(got) == served and len(served) >= len(CASES) // CHILD_EVERY - 8
    for seed in served:
        desc, _, ref = _case(seed)
        try:
            decode_checks.same_exact(got[seed], ref, desc["N"])
        except AssertionError as e:
            raise _named(seed, desc, e) from e


def test_a_short_run_of_the_long_form():
    # python tests/fuzz_decode_gpu.py [seconds] [first_seed]: seeds beyond the committed list, items 1-5 and 7
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_decode_gpu.py"), "3"], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0 and "fuzz ok:" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
