"""The seeded decoder windows (tests/decode_cases.py), the parts that need no GPU.

(a) On every window the plain references agree with each other, exactly: k = 1 of kbest_ref is viterbi_ref's path and score, the
    last row of maxmarg_ref's table peaks at that score, beam_ref never beats it, score_ref gives every one of the k best its own
    score with every SNP on a candidate, and where the window has at most 4096 full paths an exhaustive enumeration through
    score_ref gives the same top K scores and the same maximisers.  So a GPU mismatch on one of these windows
    (tests/test_gpu_decode_cases.py) is the kernel's.
(b) The committed list covers what it exists for: the conditions of COVERAGE, each a count over the generator's and the references'
    output alone.  `pytest -s` prints the table; a failure prints it too and names the condition.
(c) The panels of tests/test_gpu_decode_cases.py hold what makes a panel comparison worth its name: windows with finite scores at
    more than 1024 states and with K > 1 in every panel of a conditional that scores finitely, f64 and permuted orders among them.

The infinite scores are +inf, never -inf.  With offer_zero off a candidate's weight is a sum of log10((1 + obs) / den) with obs >= 0
(and of log10 of a positive marginal), so no term is -inf; den is 0 -- the term +inf -- where cond_mode C or D reads the lag that
reaches position 0 from a position beyond 1: under those two modes every full path of a window with N >= 2 and L >= 2 scores +inf
and only the tie orders decide.  600 further seeds, also after two reweighted paths, gave 174 windows with +inf and none with -inf.
So the condition on reachable infinities counts either sign, the -inf count is printed beside it, and the generator sends a share
of the C and D windows to L = 1, where their scores are finite and their arithmetic is what is compared."""
import functools
import hashlib
import itertools
import json

import numpy as np
import pytest

import decode_cases
import score_ref
from decode_cases import CAP, CASES

BLOCK = 40
EXHAUSTIVE_MAX = 4096


@functools.lru_cache(maxsize=None)
def _case(seed):
    """(desc, table, oracle, references): computed once, never changed."""
    desc, t = decode_cases.case(seed)
    o = decode_cases.oracle_of(desc, t)
    return desc, t, o, decode_cases.references(desc, o)


def _agree(seed):
    desc, t, o, ref = _case(seed)
    n, order, k = desc["N"], desc["spec"]["cand_order"], desc["K"]
    if ref["over"]:
        return
    vit, mm, kb, beam = ref["vit"], ref["mm"], ref["kb"], ref["beam"]
    hole = vit["hole_at"]
    assert mm["hole_at"] == kb["hole_at"] == beam["hole_at"] == hole
    if hole:
        assert vit["path"] is None and mm["mm"] is None and kb["n"] == 0 and beam["n"] == 0
        assert ref["shape"]["cm"][hole] == 0 and all(ref["shape"]["cm"][1:hole])
        return
    import kbest_ref
    one = kbest_ref.kbest(o, n, 1, order)
    assert one["n"] == 1 and one["ll_chain"][0] == vit["ll_chain"] and np.array_equal(one["paths"][0], vit["path"])
    assert kb["ll_chain"][0] == vit["ll_chain"] and np.array_equal(kb["paths"][0], vit["path"])
    assert mm["mm"][n].max() == vit["ll_chain"]
    assert mm["cm"].tolist() == ref["shape"]["cm"]
    assert not np.isnan(mm["mm"]).any() and not np.isnan(kb["ll_chain"]).any()
    assert beam["n"] >= 1 and beam["ll_chain"][0] <= vit["ll_chain"]
    sc = score_ref.score(o, kb["paths"], n, order)
    assert sc["ll_chain"] == kb["ll_chain"].tolist() and sc["n_on"] == [n] * kb["n"]
    assert len({x.tobytes() for x in kb["paths"]}) == kb["n"] and (kb["ll_chain"][:-1] >= kb["ll_chain"][1:]).all()
    cands = [[s for s in (0, 1, 2, 3, 5) if (m >> s) & 1] for m in ref["shape"]["cm"][1:]]
    full = 1
    for c in cands:
        full *= len(c)
    assert kb["n"] == min(k, full)
    if full <= EXHAUSTIVE_MAX:
        every = np.array([(6,) + x for x in itertools.product(*cands)], dtype=np.uint8)
        scores = score_ref.score(o, every, n, order)["ll_chain"]
        assert kb["ll_chain"].tolist() == sorted(scores, reverse=True)[:k]
        top = max(scores)
        best = {x.tobytes() for x, s in zip(every, scores) if s == top}
        assert vit["path"].tobytes() in best
        got = {x.tobytes() for x, s in zip(kb["paths"], kb["ll_chain"]) if s == top}
        assert got <= best and len(got) == min(k, len(best))


@pytest.mark.parametrize("first", range(0, len(CASES), BLOCK))
def test_the_references_agree_with_each_other(first):
    for seed in CASES[first:first + BLOCK]:
        try:
            _agree(seed)
        except AssertionError as e:
            raise AssertionError("seed %d %r: %s" % (seed, _case(seed)[0], e)) from e


def test_a_seed_names_the_same_window_every_time():
    for seed in CASES[:30]:
        (d1, t1), (d2, t2) = decode_cases.case(seed), decode_cases.case(seed)
        assert d1 == d2 and t1.rank.tobytes() == t2.rank.tobytes() and t1.off.tobytes() == t2.off.tobytes()
        assert t1.bases.tobytes() == t2.bases.tobytes()
        ks = np.diff(t1.off)
        assert (ks >= 2).all() and (np.diff(t1.rank) >= 0).all() and t1.rank[0] >= 0
        assert (t1.rank + ks <= t1.n_snps + (1 if t1.n_snps <= 2 else 0)).all()      # (N <= 2: the '_' behind the window)


# sha256 over json.dumps(desc, sort_keys=True) and the bytes of rank, off and bases, first 16 hex digits: a seed must name the same
# window under every numpy, or the coverage table and the seeds kept for a finding mean something else
DIGESTS = {0: "42cbf8a9b816c5f6", 1: "f121660791e119ad", 2: "1197c85c8041462a", 9: "cdf92bfc2ed24443", 144: "9401fed85f439584"}


def test_the_windows_are_the_ones_the_list_was_made_of():
    for seed, want in DIGESTS.items():
        desc, t = decode_cases.case(seed)
        raw = json.dumps(desc, sort_keys=True).encode() + t.rank.tobytes() + t.off.tobytes() + t.bases.tobytes()
        assert hashlib.sha256(raw).hexdigest()[:16] == want, (seed, desc)


def panel_coverage():
    """[(condition, count, bound, holds)] over the panels of tests/test_gpu_decode_cases.py (decode_cases.panel_windows): the panel
    copies of the walk statements must meet finite scores at many states, with K > 1, in f64 and under permuted orders.  The bounds
    ask every panel of a conditional with finite scores (A, B, E) for at least one window of each kind."""
    rows = []
    k_cap = 0
    for q, spec in enumerate(decode_cases.PANEL_SPECS):
        wins = decode_cases.panel_windows(q, lambda seed: _case(seed)[3]["over"])
        refs = [decode_cases.references(desc, decode_cases.oracle_of(desc, t)) for desc, t in wins]
        live = [(desc, r) for (desc, _), r in zip(wins, refs) if not r["vit"]["hole_at"]]
        finite = [(desc, r) for desc, r in live if np.isfinite(r["kb"]["ll_chain"]).all() and np.isfinite(r["mm"]["mm"][r["mm"]["mm"] > -np.inf]).all()]
        name = "panel %d (%s%s %s %s): " % (q, spec["cond_mode"], "+m" if spec["marginal_term"] else "", spec["storage"], spec["cand_order"])

        def row(what, count, bound):
            rows.append((name + what, count, bound, count >= bound))

        row("windows", len(wins), decode_cases.PANEL)
        row("holes among them", len(wins) - len(live), 1)
        if spec["cond_mode"] in "CD":
            row("windows whose scores are +inf: the tie orders alone", len(live) - len(finite), 1)
            continue
        row("windows with finite scores", len(finite), decode_cases.PANEL // 2)
        row("... at more than 1024 states", sum(1 for _, r in finite if r["shape"]["states"] > 1024), 1)
        row("... with K > 1 at 64 states or more", sum(1 for d, r in finite if d["K"] > 1 and r["shape"]["states"] >= 64), 1)
        k_cap += sum(1 for d, r in finite if d["K"] > 1 and d["K"] * r["shape"]["states"] == CAP)
    specs = [s for s in decode_cases.PANEL_SPECS if s["cond_mode"] not in "CD"]
    rows.append(("finite-score panels in f64", sum(s["storage"] == "f64" for s in specs), 2, sum(s["storage"] == "f64" for s in specs) >= 2))
    rows.append(("finite-score panels under a permuted order", sum(s["cand_order"] != "ACGT-" for s in specs), 2,
                 sum(s["cand_order"] != "ACGT-" for s in specs) >= 2))
    rows.append(("finite-score panels by conditional A / B / E", len({s["cond_mode"] for s in specs}), 3, {s["cond_mode"] for s in specs} == set("ABE")))
    rows.append(("finite panel windows with K > 1 and K * states == 4096", k_cap, 2, k_cap >= 2))
    return rows


def test_the_panels_compare_finite_scores_at_many_states():
    rows = panel_coverage()
    text = "\n".join("%-78s %5d  (bound %g)%s" % (what, count, bound, "" if ok else "   <-- FAILS") for what, count, bound, ok in rows)
    print("\n" + text)
    failed = [what for what, _, _, ok in rows if not ok]
    assert not failed, "panel conditions that do not hold: %s\n%s" % ("; ".join(failed), text)


def _facts(seed):
    """What the coverage conditions count, of one case."""
    desc, t, o, ref = _case(seed)
    sh = ref["shape"]
    f = dict(over=ref["over"], hole=False, S=sh["S"], states=sh["states"], N=desc["N"], L=desc["L"], band=desc["band"], K=desc["K"],
             spec=desc["spec"])
    if ref["over"]:
        return f
    if ref["vit"]["hole_at"]:
        f["hole"] = True
        return f
    offered = [bin(m).count("1") for m in sh["cm"][1:]]
    bits = [q for q, s in enumerate((0, 1, 2, 3, 5)) if (sh["U"] >> s) & 1]      # the union in "ACGT-" order
    mm, kb = ref["mm"]["mm"], ref["kb"]
    reach = [mm[p, s] for p in range(1, desc["N"] + 1) for s in (0, 1, 2, 3, 5) if (sh["cm"][p] >> s) & 1] + kb["ll_chain"].tolist()
    f.update(fewer=min(offered) < sh["S"], gap=bits != list(range(len(bits))), ties=bool((kb["ll_chain"][:-1] == kb["ll_chain"][1:]).any()),
             neg_inf=-np.inf in reach, pos_inf=np.inf in reach, short=kb["n"] < desc["K"])
    return f


def coverage(seeds=CASES):
    """[(condition, count, bound, holds)] over the case list."""
    fs = [_facts(seed) for seed in seeds]
    served = [f for f in fs if not f["over"] and not f["hole"]]
    holes = sum(f["hole"] for f in fs)
    rows = [("holes >= 5 % of the cases", holes, 0.05 * len(fs), holes >= 0.05 * len(fs)),
            ("holes <= 15 % of the cases", holes, 0.15 * len(fs), holes <= 0.15 * len(fs))]

    def at_least(what, bound, pred, among=served):
        count = sum(1 for f in among if pred(f))
        rows.append((what, count, bound, count >= bound))

    at_least("refusals beyond the cap", 5, lambda f: f["over"], fs)
    for s in range(1, 6):
        at_least("S = %d" % s, 10, lambda f, s=s: f["S"] == s)
    at_least("S = 3 with more than 1024 states", 3, lambda f: f["S"] == 3 and f["states"] > 1024)
    at_least("1024 < states < 4096", 5, lambda f: 1024 < f["states"] < CAP)
    at_least("states == 4096", 3, lambda f: f["states"] == CAP)
    at_least("K * states == 4096 with N >= 34", 2, lambda f: f["K"] * f["states"] == CAP and f["N"] >= 34)
    at_least("a position offers fewer candidates than S (half of the served)", (len(served) + 1) // 2, lambda f: f["fewer"])
    at_least("union alphabet with a gap in ACGT- order", 10, lambda f: f["gap"])
    at_least("L > band with N > L", 15, lambda f: f["L"] > f["band"] and f["N"] > f["L"])
    at_least("N < L", 8, lambda f: f["N"] < f["L"])
    for mode in "ABCDE":
        for mt in (False, True):
            at_least("cond_mode %s, marginal_term %s" % (mode, mt), 5,
                     lambda f, mode=mode, mt=mt: f["spec"]["cond_mode"] == mode and f["spec"]["marginal_term"] == mt)
    at_least("f64", 30, lambda f: f["spec"]["storage"] == "f64")
    at_least("permuted candidate order", 50, lambda f: f["spec"]["cand_order"] != "ACGT-")
    at_least("K not a power of two", 25, lambda f: f["K"] & (f["K"] - 1) != 0)
    at_least("equal scores among the k best", 10, lambda f: f["ties"])
    at_least("a reachable infinite score, in the k best or at an offered mm entry", 10, lambda f: f["neg_inf"] or f["pos_inf"])
    none = sum(1 for f in served if f["neg_inf"])
    rows.append(("no reachable -inf anywhere (none can be: see the module's text)", none, 0, none == 0))
    at_least("finite scores under cond_mode C or D", 5, lambda f: f["spec"]["cond_mode"] in "CD" and not f["pos_inf"])
    at_least("fewer than K full paths", 10, lambda f: f["short"])
    return rows, len(fs), len(served)


def table_text(rows, n_cases, n_served):
    lines = ["%d cases, %d served without a hole" % (n_cases, n_served)]
    lines += ["%-66s %5d  (bound %g)%s" % (what, count, bound, "" if ok else "   <-- FAILS") for what, count, bound, ok in rows]
    return "\n".join(lines)


def test_the_case_list_covers_what_it_exists_for():
    rows, n_cases, n_served = coverage()
    text = table_text(rows, n_cases, n_served)
    print("\n" + text)
    failed = [what for what, _, _, ok in rows if not ok]
    assert not failed, "coverage conditions that do not hold: %s\n%s" % ("; ".join(failed), text)
