"""What tests/test_gpu_decode_cases.py and tests/fuzz_decode_gpu.py share: one window of tests/decode_cases.py on the GPU against the
plain references (viterbi_ref, maxmarg_ref, kbest_ref, beam_ref, score_ref over the C oracle).  Not a test file.  Everything is
compared exactly -- the order of every addition and every comparison is fixed by the definitions -- except the removed mass of a
reweight, which goes through spec_util.same's relative 1e-10, as everywhere."""
import re

import numpy as np

import decode_cases
import score_ref
import viterbi_ref
from decode_cases import CAP, KMAX
from decode_util import _same_spin
from gretel_amd import _lib
from spec_util import make_pair


def pair_of(desc, t, spec=None):
    """(a fresh handle, the C oracle) filled from the case's table under the case's spec (or `spec`), their L set."""
    return make_pair(t, L=desc["L"], **(desc["spec"] if spec is None else spec))


def gpu_exact(h, k):
    """The three exact calls on the handle as it stands, as they came back."""
    vit = h.viterbi_path()
    return dict(vit=vit, info=h.viterbi_info()[:3], mm=h.viterbi_marginals(), kb=h.viterbi_kbest(k))


def same_path(got, ref, n):
    assert got["hole_at"] == ref["hole_at"], ("viterbi_path hole_at", got["hole_at"], ref["hole_at"])
    if ref["hole_at"]:
        assert got["path"] is None and got["ll_chain"] is None
        return
    assert got["path"].dtype == np.uint8 and got["path"].shape == (n + 1,)
    assert got["ll_chain"] == ref["ll_chain"], ("viterbi_path ll_chain", got["ll_chain"], ref["ll_chain"])
    assert np.array_equal(got["path"], ref["path"]), ("viterbi_path", np.argwhere(got["path"] != ref["path"])[:4].tolist())


def same_marginals(got, ref, n):
    assert got["hole_at"] == ref["hole_at"], ("viterbi_marginals hole_at", got["hole_at"], ref["hole_at"])
    if ref["hole_at"]:
        assert got["mm"] is None and got["cm"] is None
        return
    assert got["mm"].shape == (n + 1, 7) and got["mm"].dtype == np.float64 and not np.isnan(got["mm"]).any()
    assert np.array_equal(got["cm"], ref["cm"]), ("cm", got["cm"].tolist(), ref["cm"].tolist())
    # IEEE values: an infinity equals itself, there is no NaN on either side
    assert np.array_equal(got["mm"], ref["mm"]), ("mm", [(int(p), int(s), got["mm"][p, s], ref["mm"][p, s])
                                                        for p, s in np.argwhere(got["mm"] != ref["mm"])[:4]])


def same_kbest(got, ref, n):
    assert (got["n"], got["hole_at"]) == (ref["n"], ref["hole_at"]), ("viterbi_kbest n, hole_at", got["n"], got["hole_at"], ref["n"], ref["hole_at"])
    assert got["paths"].dtype == np.uint8 and got["paths"].shape == (ref["n"], n + 1) and got["ll_chain"].shape == (ref["n"],)
    assert got["ll_chain"].tolist() == ref["ll_chain"].tolist(), ("viterbi_kbest ll_chain", [
        (i, a, b) for i, (a, b) in enumerate(zip(got["ll_chain"], ref["ll_chain"])) if a != b][:4])
    assert np.array_equal(got["paths"], ref["paths"]), ("viterbi_kbest paths", np.argwhere(got["paths"] != ref["paths"])[:4].tolist())


def same_exact(got, ref, n):
    """Items 1-3: gpu_exact()'s dict against decode_cases.references()'."""
    same_path(got["vit"], ref["vit"], n)
    if not ref["vit"]["hole_at"]:                                # (a hole gives hole_at and nothing else)
        sh = ref["shape"]
        assert tuple(got["info"]) == (sh["S"], sh["Le"], sh["states"]), ("viterbi_info", got["info"], (sh["S"], sh["Le"], sh["states"]))
    same_marginals(got["mm"], ref["mm"], n)
    same_kbest(got["kb"], ref["kb"], n)


def check_beam(h, desc, ref):
    n = desc["N"]
    got, want = h.beam_paths(desc["width"]), ref["beam"]
    assert (got["n"], got["hole_at"]) == (want["n"], want["hole_at"]), ("beam_paths n, hole_at", got["n"], got["hole_at"], want["n"], want["hole_at"])
    if want["hole_at"]:
        assert got["prefix"].tolist() == want["prefix"].tolist()
        return
    assert got["paths"].shape == (want["n"], n + 1)
    assert np.array_equal(got["paths"], want["paths"]), ("beam_paths", np.argwhere(got["paths"] != want["paths"])[:4].tolist())
    assert got["ll_chain"].tolist() == list(want["ll_chain"]), "beam_paths ll_chain"


def check_score(h, o, desc, ref):
    """Item 5: the k best, and the same paths with a few symbols replaced -- some by symbols their position does not offer."""
    n, kb = desc["N"], ref["kb"]
    if kb["n"] == 0:
        return
    rng = np.random.default_rng([desc["seed"], 5])
    bent = kb["paths"].copy()
    for x in bent:
        for p in rng.integers(1, n + 1, size=int(rng.integers(1, 4))):
            x[p] = rng.integers(0, 7)                            # any of "ACGTN-_": offered there or not
    paths = np.concatenate([kb["paths"], bent])
    got = h.score_paths(paths, per_position=True)
    score_ref.assert_same(got, score_ref.score(o, paths, n, desc["spec"]["cand_order"]))
    assert got["ll_chain"][:kb["n"]].tolist() == kb["ll_chain"].tolist() and (got["n_on"][:kb["n"]] == n).all()


def check_refusal(h, desc, shape):
    """Item 6: beyond the cap each exact call refuses and names S, Le and the states the reference counts."""
    want = r"S = %d .* Le = min\(L, N\) = %d make %d states" % (shape["S"], shape["Le"], shape["states"])
    for call in (h.viterbi_path, h.viterbi_marginals, lambda: h.viterbi_kbest(1)):
        try:
            call()
        except _lib.GretelHipError as e:
            assert e.code == _lib.GH_ERR_ARG and re.search(want, str(e)), (e.code, str(e), want)
        else:
            raise AssertionError("served beyond the cap: %s" % want)
    assert h.viterbi_kbest_max() == 0 and h.viterbi_states() == (shape["S"], shape["Le"], shape["states"])


def check_reweighted(h, o, desc):
    """Item 7: two exact paths recovered and removed on both sides, then items 1-3 once more on the tensor that leaves."""
    n, order = desc["N"], desc["spec"]["cand_order"]
    res = h.viterbi_spin(2)
    _same_spin(res, viterbi_ref.viterbi_spin(o, n, 2, cand_order=order))
    assert np.array_equal(h.export_band(), o.export_band()), "export_band after viterbi_spin(2)"
    ref = decode_cases.references(desc, o)
    assert not ref["over"]
    same_exact(gpu_exact(h, desc["K"]), ref, n)
    return ref


def check_case(desc, t, ref=None):
    """Items 1-7 on a fresh handle; `ref`: decode_cases.references() of the case where the caller has them.  Returns the references
    of the tensor as filled."""
    h, o = pair_of(desc, t)
    if ref is None:
        ref = decode_cases.references(desc, o)
    n, sh = desc["N"], ref["shape"]
    if ref["over"]:
        check_refusal(h, desc, sh)
        return ref
    assert h.viterbi_kbest_max() == min(KMAX, CAP // sh["states"])      # (4096 // states, and never more than the 32 a call takes)
    same_exact(gpu_exact(h, desc["K"]), ref, n)
    check_beam(h, desc, ref)
    check_score(h, o, desc, ref)
    check_reweighted(h, o, desc)
    return ref
