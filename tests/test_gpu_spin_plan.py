"""Which flow a spin took, stated from outside: every case spins one small window, compares with the C oracle, and asserts
Hansel.spin_plan() -- the plan the spin ran with (plan_spin of gretel_amd/csrc/gretel_hip.hip) -- against a
literal row, and the launch counts the profile shows for that flow.

The expected rows were not taken from plan_spin: they are what the commit before it printed for these very cases, from a scratch
build whose gh_spin wrote its handle flags (rws, fuse, seg6, the stride of the partial sums, the small-window decision of the
launch helpers, the lane groups, the segments and the dynamic LDS) to stderr under GH_PRINT_STATE."""
import numpy as np
import pytest

from gretel_amd import _lib
from gretel_amd.synth import make_support_table
from spec_util import make_pair, same, with_dels
from test_gpu_edges import PINNED

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(PINNED, reason="GH_WALK / GH_WALK_THREADS pin another variant")]


def row(flow, emit_small, seg6, stride, rw_lanes, S, lds, rwseg, reweight):
    """plan fields, then the profile's launches of k_rwseg and of the reweight kernels."""
    return dict(flow=flow, emit_small=emit_small, seg6=seg6, stride=stride, rw_lanes=rw_lanes, S=S, lds=lds), rwseg, reweight


def case(id, n, L, expect, reads=None, k=6, dels=False, paths=4, env=None, walk=None, seed=None, **kw):
    return pytest.param(dict(n=n, L=L, reads=reads or 30 * n, k=k, dels=dels, paths=paths, env=env or {}, walk=walk,
                             seed=100 + L if seed is None else seed, kw=kw), expect, id=id)


# (k = None: long-read-style reads, clip(Poisson(10), 2, 21) SNPs each -- the lag counts of the candidate pools)
CASES = [
    # L = 1..5 at 900 SNPs, over candidate ranks (narrow) and with 10 % '-' (five candidates at some positions)
    case("L1-narrow", 900, 1, row("rwseg", 1, 0, 113, 8, 113, 16848, 3, 1)),
    case("L1-dels", 900, 1, row("rwseg", 1, 0, 113, 8, 113, 16848, 3, 1), dels=True),
    case("L2-narrow", 900, 2, row("rwseg", 1, 0, 113, 8, 113, 29728, 3, 1)),
    case("L2-dels", 900, 2, row("rwseg", 1, 0, 113, 8, 113, 29728, 3, 1), dels=True),
    case("L3-narrow", 900, 3, row("rwseg", 1, 0, 113, 8, 113, 44928, 3, 1)),
    case("L3-dels", 900, 3, row("rwseg", 1, 0, 113, 8, 113, 44928, 3, 1), dels=True),
    case("L4-narrow", 900, 4, row("rwseg", 0, 0, 113, 8, 113, 70128, 3, 1)),
    case("L4-dels", 900, 4, row("rwseg", 0, 0, 113, 8, 113, 70128, 3, 1), dels=True),
    case("L5-narrow", 900, 5, row("rwseg", 0, 0, 113, 8, 113, 107920, 3, 1)),
    case("L5-dels", 900, 5, row("rwseg", 0, 0, 113, 8, 113, 107920, 3, 1), dels=True),
    # both sides of the small-window flip (every segment map in one workgroup's LDS)
    case("L3-small-last", 1968, 3, row("rwseg", 1, 0, 246, 8, 246, 44928, 3, 1)),
    case("L3-small-past", 1969, 3, row("rwseg", 0, 0, 247, 8, 247, 44928, 3, 1)),
    case("L5-small-last", 72, 5, row("rwseg", 1, 0, 9, 8, 9, 107920, 3, 1), reads=3000),
    case("L5-small-past", 73, 5, row("rwseg", 0, 0, 10, 8, 10, 107920, 3, 1), reads=3000),
    # the switches
    case("rwseg-off", 900, 3, row("seg", 1, 0, 29, 8, 113, 0, 0, 4), env=dict(GH_RWSEG="0")),
    case("rwseg-small-off", 900, 3, row("seg", 1, 0, 29, 8, 113, 0, 0, 4), env=dict(GH_RWSEG_SMALL="0")),
    case("fuse2-L3-narrow", 900, 3, row("fuse", 0, 0, 29, 8, 113, 2304, 0, 4), env=dict(GH_FUSE="2")),
    case("fuse2-L5-dels", 900, 5, row("rwseg", 0, 0, 113, 8, 113, 107920, 3, 1), dels=True, env=dict(GH_FUSE="2")),
    # L = 6: the enumerated states over a ranked table, else pools (reads of up to 21 SNPs: lane groups of 16, so four launches)
    case("L6-narrow", 900, 6, row("seg", 0, 1, 57, 16, 113, 0, 0, 4), reads=12000, k=None, seed=12),
    case("L6-dels", 900, 6, row("pools", 0, 0, 57, 16, 29, 0, 0, 4), reads=12000, k=None, seed=12, dels=True),
    case("L6-seg6-off", 900, 6, row("pools", 0, 0, 57, 16, 29, 0, 0, 4), reads=12000, k=None, seed=12, env=dict(GH_SEG6="0")),
    # band 9: lane groups of 16 in k_rw, which k_rwseg does not have
    case("band9-L3", 900, 3, row("seg", 1, 0, 57, 16, 113, 0, 0, 4), k=10),
    case("lt-full", 900, 3, row("seg", 1, 0, 29, 8, 113, 0, 0, 4), env=dict(GH_LT_FULL="1")),
    case("L7-pools", 900, 7, row("pools", 0, 0, 57, 16, 29, 0, 0, 4), reads=12000, k=None, seed=12),
    case("walk-spec", 900, 3, row("serial", 0, 0, 29, 8, 0, 0, 0, 4), walk="spec"),
    # k_rwseg holds a segment, the L positions in front and one more in the 128 positions of a workgroup: the five-symbol radix
    # cuts 30 500 SNPs into 250 segments of 122 (the ranked one, whose 255 segments the launches are sized for, into shorter ones)
    case("L5-seglen-last", 30500, 5, row("rwseg", 0, 0, 954, 8, 255, 107920, 2, 1), reads=6 * 30500, paths=3),
    case("L5-seglen-past", 30501, 5, row("seg", 0, 0, 954, 8, 255, 0, 0, 3), reads=6 * 30501, paths=3),
    # conditional C in binary64, reads of 9 SNPs: the band blocks k_rwseg would stage for segments of 79 positions exceed its LDS
    case("C-f64-20011", 20011, 3, row("seg", 0, 0, 626, 8, 254, 0, 0, 3), reads=6 * 20011, k=9, paths=3, seed=5,
         cond_mode="C", storage="f64"),
]


def build(c, monkeypatch):
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    t = make_support_table(c["n"], c["reads"], k=c["k"], seed=c["seed"])
    if c["dels"]:
        t = with_dels(t, 0.1, c["L"])
    return t, make_pair(t, L=c["L"], walk=c["walk"], **c["kw"])


@pytest.mark.parametrize("c,expect", CASES)
def test_the_flow_a_spin_takes(c, expect, monkeypatch):
    plan, rwseg, reweight = expect
    t, (h, o) = build(c, monkeypatch)
    assert h.spin_plan()["flow"] == "none"
    h.profile_enable(1)
    h.profile_reset()
    res, ref = h.spin(c["paths"]), o.spin(c["paths"])
    same(res, ref)
    assert res["n"] == c["paths"]
    assert np.array_equal(h.export_band(), o.export_band())
    got = h.spin_plan()
    print("plan", got)
    assert {k: got[k] for k in plan} == plan
    assert got["need_layout"] == 0
    prof = h.profile_get()
    print("profile", {k: v["launches"] for k, v in prof.items()})
    assert (prof["rwseg"]["launches"], prof["reweight"]["launches"]) == (rwseg, reweight)
    if plan["flow"] == "rwseg":
        assert (rwseg, reweight) == (c["paths"] - 1, 1)
    elif plan["flow"] in ("seg", "fuse"):
        assert (rwseg, reweight) == (0, c["paths"])


def test_the_small_window_cases_sit_on_the_flip():
    """(the lengths above, from the host query: the last small window and the first that is not)"""
    for L, n in ((3, 1968), (5, 72)):
        assert _lib.spin_plan(n, 5, L)["emit_small"] == 1 and _lib.spin_plan(n + 1, 5, L)["emit_small"] == 0
    assert _lib.spin_plan(30500, 5, 5)["flow"] == "rwseg" and _lib.spin_plan(30501, 5, 5)["flow"] == "seg"
