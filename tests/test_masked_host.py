"""Constrained exact decoding (gh_viterbi_path_masked), the parts that need no GPU.

(a) The masked reference (tests/masked_ref.py: viterbi_ref over an oracle whose candidate mask is ANDed with the constraint set)
    against an exhaustive enumeration on the seeded windows of tests/decode_cases.py with N <= 8, under ARBITRARY mask bytes, so
    that masks do create holes where the window has none.
(b) The consequences the header states, on the windows with N <= 21, against viterbi_ref, maxmarg_ref, kbest_ref and score_ref.
(c) What the GPU test compares on covers what it exists for, by count: over the served windows of the committed list with four
    generated sets each, at most 15 % of the sets end in a hole and at least 300 return a path other than the unmasked best.
(d) hansel.allow_of, hansel.alternatives_of, the CLI's refusals of --alternatives and --pin, and the scratch layout under
    AddressSanitizer + UBSan on the CPU (tests/native/vitx_layout.cpp)."""
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import decode_cases
import masked_ref
import score_ref
from conftest import ROOT
from decode_cases import CASES
from gretel_amd import cmd
from gretel_amd.hansel import allow_of, alternatives_of, margins_of
from masked_ref import VALID

STRIDE = 4


@functools.lru_cache(maxsize=None)
def _case(seed):
    """(desc, oracle, dict(shape, over, vit: the unmasked reference)): computed once, never changed."""
    import viterbi_ref
    desc, t = decode_cases.case(seed)
    o = decode_cases.oracle_of(desc, t)
    shape = decode_cases.shape_of(o, desc["N"])
    if shape["states"] > decode_cases.CAP:
        return desc, o, dict(shape=shape, over=True)
    return desc, o, dict(shape=shape, over=False, vit=viterbi_ref.viterbi(o, desc["N"], desc["spec"]["cand_order"]))


@functools.lru_cache(maxsize=None)
def _more(seed):
    """(maxmarg_ref's table, kbest_ref's dict) of a served case without a hole."""
    import kbest_ref
    import maxmarg_ref
    desc, o, _ = _case(seed)
    return maxmarg_ref.marginals(o, desc["N"])["mm"], kbest_ref.kbest(o, desc["N"], desc["K"], desc["spec"]["cand_order"])


@functools.lru_cache(maxsize=None)
def _generated(seed):
    """(the four generated sets, the masked reference's dict for them) of a served case."""
    desc, o, ref = _case(seed)
    allow = masked_ref.masks(seed, ref["shape"]["cm"], desc["N"])
    return allow, masked_ref.decode_sets(o, desc["N"], allow, desc["spec"]["cand_order"])


def _named(seed, e):
    return AssertionError("seed %d %r: %s" % (seed, _case(seed)[0], e))


def _exhaustive(seed, counts):
    desc, o, ref = _case(seed)
    n, order, cm = desc["N"], desc["spec"]["cand_order"], ref["shape"]["cm"]
    rng = np.random.default_rng([seed, 23])
    for _ in range(4):
        allow = rng.integers(0, 128, size=n + 1).astype(np.uint8)
        got = masked_ref.viterbi_masked(o, n, allow, order)
        cands = [[s for s in VALID if ((cm[p] & int(allow[p])) >> s) & 1] for p in range(1, n + 1)]
        empty = [p for p in range(1, n + 1) if not cands[p - 1]]
        if empty:
            counts[1] += 1
            assert got["hole_at"] == empty[0] and got["path"] is None and got["ll_chain"] is None
            continue
        counts[0] += 1
        every = np.array([(6,) + x for x in itertools.product(*cands)], dtype=np.uint8)
        sc = score_ref.score(o, every, n, order)
        assert sc["n_on"] == [n] * len(every)
        top = max(sc["ll_chain"])
        assert got["hole_at"] == 0 and got["ll_chain"] == top
        assert got["path"].tobytes() in {x.tobytes() for x, s in zip(every, sc["ll_chain"]) if s == top}


def test_the_masked_reference_against_an_exhaustive_enumeration():
    counts = [0, 0]                                              # feasible sets, infeasible sets
    for seed in CASES:
        if decode_cases.case(seed)[0]["N"] <= 8 and not _case(seed)[2]["over"]:
            try:
                _exhaustive(seed, counts)
            except AssertionError as e:
                raise _named(seed, e) from e
    assert counts[0] >= 40 and counts[1] >= 40, counts           # masks both leave paths and create holes


def _consequences(seed):
    desc, o, ref = _case(seed)
    n, order, cm = desc["N"], desc["spec"]["cand_order"], ref["shape"]["cm"]
    free = masked_ref.viterbi_masked(o, n, allow_of(n), order)
    vit = ref["vit"]
    assert free["hole_at"] == vit["hole_at"]
    allow, res = _generated(seed)
    if vit["hole_at"]:
        # the generated sets never make a hole of their own: they stop where the window does
        assert res["hole_at"].tolist() == [vit["hole_at"]] * len(allow)
        return
    # all 0x7f is the unmasked decoder, path and score
    assert free["ll_chain"] == vit["ll_chain"] and np.array_equal(free["path"], vit["path"])
    assert not res["hole_at"].any()
    # every returned path is allowed, scores as gh_score_paths scores it, and never beats the free best
    sc = score_ref.score(o, res["paths"], n, order)
    assert sc["ll_chain"] == res["ll_chain"].tolist() and sc["n_on"] == [n] * len(allow)
    for row, x in zip(allow, res["paths"]):
        assert all((int(row[p]) >> int(x[p])) & 1 for p in range(1, n + 1))
    assert (res["ll_chain"] <= vit["ll_chain"]).all()

    def one_hot(x, at):
        row = allow_of(n)
        for p in at:
            row[p] = 1 << int(x[p])
        return row

    # one-hot masks of a full path at all positions return it and its score: the k best, and the generated sets' results
    mm, kb = _more(seed)
    for x, ll in list(zip(kb["paths"], kb["ll_chain"])) + list(zip(res["paths"], res["ll_chain"])):
        got = masked_ref.viterbi_masked(o, n, one_hot(x, range(1, n + 1)), order)
        assert got["hole_at"] == 0 and got["ll_chain"] == ll and np.array_equal(got["path"], x)
    # one-hot masks of the best path at any subset of positions return the best path
    rng = np.random.default_rng([seed, 29])
    for _ in range(3):
        at = [p for p in range(1, n + 1) if rng.random() < 0.5]
        got = masked_ref.viterbi_masked(o, n, one_hot(vit["path"], at), order)
        assert got["ll_chain"] == vit["ll_chain"] and np.array_equal(got["path"], vit["path"]), at
    # a pin (N, c) is mm[N][c]; at any p the best of the pins is the best of all; for p < N a pin and mm[p][c] agree to the
    # summation order: within N * 2^-52 * A, A the largest sum of |w_t| over the full paths (the bound of "Max-marginals"),
    # checked where the window has few enough full paths to take A from all of them
    cands = [[s for s in VALID if (m >> s) & 1] for m in cm[1:]]
    full = 1
    for c in cands:
        full *= len(c)
    big_a = None
    if full <= 256:
        every = np.array([(6,) + x for x in itertools.product(*cands)], dtype=np.uint8)
        big_a = max(np.abs(np.asarray(w[1:], dtype=np.float64)).sum() for w in score_ref.score(o, every, n, order)["weight"])
    for p in sorted({n, 1, int(rng.integers(1, n + 1))}):
        pinned = {}
        for c in VALID:
            if (cm[p] >> c) & 1:
                got = masked_ref.viterbi_masked(o, n, allow_of(n, pins={p: c}), order)
                assert got["hole_at"] == 0 and got["path"][p] == c
                pinned[c] = got["ll_chain"]
                if p == n:
                    assert got["ll_chain"] == mm[n, c]
                elif not (np.isfinite(got["ll_chain"]) and np.isfinite(mm[p, c])):
                    assert got["ll_chain"] == mm[p, c]
                elif big_a is not None and np.isfinite(big_a):
                    assert abs(got["ll_chain"] - mm[p, c]) <= n * 2.0 ** -52 * big_a, (p, c, got["ll_chain"], mm[p, c], big_a)
        assert max(pinned.values()) == vit["ll_chain"]


@pytest.mark.parametrize("part", range(STRIDE))
def test_the_consequences_the_header_states(part):
    for seed in CASES[part::STRIDE]:
        if decode_cases.case(seed)[0]["N"] <= 21 and not _case(seed)[2]["over"]:
            try:
                _consequences(seed)
            except AssertionError as e:
                raise _named(seed, e) from e


def test_the_generated_sets_cover_what_they_exist_for():
    served = [seed for seed in CASES if not _case(seed)[2]["over"]]
    sets = holes = differ = own = 0
    for seed in served:
        desc, _, ref = _case(seed)
        _, res = _generated(seed)
        for q in range(len(res["hole_at"])):
            sets += 1
            if res["hole_at"][q]:
                holes += 1
                own += res["hole_at"][q] != ref["vit"]["hole_at"]
            elif not np.array_equal(res["paths"][q], ref["vit"]["path"]):
                differ += 1
    print("\n%d served cases, %d sets, %d end in a hole (%.1f %%), %d of them not the window's own, %d return another path than the unmasked best"
          % (len(served), sets, holes, 100.0 * holes / sets, own, differ))
    assert sets == 4 * len(served) and len(served) >= 225
    assert holes <= 0.15 * sets and own == 0
    assert differ >= 300


# (d) --------------------------------------------------------------------------------------------
def test_allow_of():
    assert allow_of(3).tolist() == [0x7F] * 4 and allow_of(3).dtype == np.uint8
    a = allow_of(5, pins={2: "AC", 5: "-", 3: 2}, bans={1: "T", 2: "A", 4: [0, 5]})
    assert a.tolist() == [0x7F, 0x7F & ~8, 2, 4, 0x7F & ~(1 | 32), 32]
    assert allow_of(2, pins={1: [0, 1, 2, 3, 5]}).tolist() == [0x7F, 0x2F, 0x7F]
    for bad in (dict(pins={0: "A"}), dict(pins={4: "A"}), dict(bans={-1: "A"}), dict(pins={1: "N"}), dict(pins={1: "_"}), dict(bans={1: 4}),
                dict(pins={1: 6}), dict(pins={1: "AX"}), dict(bans={1: 7})):
        with pytest.raises(ValueError):
            allow_of(3, **bad)


def _table(rows):
    """mm, cm from {p: {symbol char: value}} over "ACGTN-_"."""
    n = max(rows)
    mm = np.full((n + 1, 7), -np.inf)
    cm = np.zeros(n + 1, dtype=np.uint8)
    for p, row in rows.items():
        for c, v in row.items():
            s = "ACGTN-_".index(c)
            mm[p, s] = v
            cm[p] |= 1 << s
    return mm, cm


def test_alternatives_of():
    ninf = -np.inf
    mm, cm = _table({1: dict(A=-1.0, C=-3.0), 2: dict(G=-1.0), 3: dict(A=-1.5, C=-1.0, T=-1.5), 4: dict(A=-1.0, T=-3.0),
                     5: dict(C=-1.0, G=ninf), 6: {"A": ninf, "-": ninf}, 7: dict(G=-1.0, T=-1.0)})
    alt = alternatives_of(mm, cm, 10)
    # SNP 2 offers one candidate: not eligible.  Gaps: 7 -> 0 (a tie: G is best, the first of the order), 6 -> 0.0 (all -inf),
    # 3 -> 0.5, 1 and 4 -> 2 (ascending p among equals), 5 -> inf
    assert alt["p"].tolist() == [6, 7, 3, 1, 4, 5] and alt["p"].dtype == np.int32
    assert alt["gap"].tolist() == [0.0, 0.0, 0.5, 2.0, 2.0, np.inf]
    assert alt["best"].tolist() == [0, 2, 1, 0, 0, 1] and alt["alt"].tolist() == [5, 3, 0, 1, 3, 2]     # (3: A and T tie, A is first)
    assert alt["allow"].shape == (6, 8) and alt["allow"].dtype == np.uint8
    for q, (p, r) in enumerate(zip(alt["p"], alt["alt"])):
        want = allow_of(7, pins={int(p): int(r)})
        assert alt["allow"][q].tolist() == want.tolist()
    assert margins_of(mm, cm, [])["best"][alt["p"]].tolist() == alt["best"].tolist()
    # the first m of them; fewer than m eligible positions give fewer sets
    two = alternatives_of(mm, cm, 2)
    assert two["p"].tolist() == [6, 7] and two["allow"].shape == (2, 8)
    # another candidate order decides the ties otherwise: T before G at 7, T before A at 3
    alt = alternatives_of(mm, cm, 3, "T-GCA")
    assert alt["p"].tolist() == [6, 7, 3] and alt["best"].tolist() == [5, 3, 1] and alt["alt"].tolist() == [0, 2, 3]
    none = alternatives_of(*_table({1: dict(A=-1.0), 2: dict(C=-2.0)}), 4)
    assert none["p"].shape == (0,) and none["allow"].shape == (0, 3) and none["gap"].shape == (0,)


def _args(*extra):
    return cmd.build_parser().parse_args(["x.bam", "x.vcf", "ctg"] + list(extra))


def test_the_cli_refuses_what_it_cannot_decode(capsys):
    assert cmd.check_masked_options(_args()) is None
    assert cmd.check_masked_options(_args("--alternatives", "1", "--pin", "12:A", "--pin", "7:AC-,9:T")) is None
    assert cmd.check_masked_options(_args("--alternatives", "255")) is None
    for m in ("0", "256", "-3"):
        assert "--alternatives must be 1..255" in cmd.check_masked_options(_args("--alternatives", m))
    for spec in ("12", "12:", ":A", "x:A", "12:N", "12:A_", "12:a", "12:A,", "12:A;13:C", "1.5:A", "-4:A"):
        assert "is not POS:ALLELES" in cmd.check_masked_options(_args("--pin=" + spec)), spec
    assert "given twice" in cmd.check_masked_options(_args("--pin", "12:A,12:C"))
    assert "more than 255" in cmd.check_masked_options(_args(*(["--alternatives", "250"] + ["--pin", "5:A"] * 6)))
    assert cmd.check_masked_options(_args(*(["--alternatives", "250"] + ["--pin", "5:A"] * 5))) is None
    assert cmd.parse_pin("7:AC-,9:T") == [(7, "AC-"), (9, "T")]
    # main() refuses before it opens anything: the files named do not exist
    assert cmd.main(["x.bam", "x.vcf", "ctg", "--alternatives", "0"]) == 2
    assert "[FAIL] --alternatives must be 1..255" in capsys.readouterr().err
    assert cmd.main(["x.bam", "x.vcf", "ctg", "--pin", "12:Z"]) == 2
    assert "[FAIL] --pin 12:Z" in capsys.readouterr().err
    # ... and after the VCF is read: a POS that is no SNP of the window
    vcf_h = dict(snp_fwd={5: 0, 9: 1, 12: 2})
    assert cmd.check_pins_in_window(_args("--pin", "5:A,12:C", "--pin", "9:-"), vcf_h) is None
    assert "position 7 is not a SNP of the window" in cmd.check_pins_in_window(_args("--pin", "5:A", "--pin", "9:C,7:T"), vcf_h)


def test_the_masked_scratch_layout_is_what_its_user_spelled_out(tmp_path):
    exe = str(tmp_path / "vitx_layout")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gretel_amd", "csrc"), "-o", exe,
                         os.path.join(ROOT, "tests", "native", "vitx_layout.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert "vitx_layout done" in run.stdout
