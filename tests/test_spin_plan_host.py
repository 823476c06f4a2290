"""Which kernels a gh_spin runs for every path is chosen once per spin by a pure host function (plan_spin of
gretel_amd/csrc/gretel_hip.hip; DESIGN.md section 4.1 has the table).  gh_debug_spin_plan asks it through the C ABI, without a
handle or a GPU.  Swept here over lag counts, window lengths (dense around every length at which a field of the plan flips: the
flips are found with the query itself), band widths, storages, conditionals, the table's layout and the GH_* switches; at every
point the plan must satisfy the conditions the flows are documented with.  The geometry (segments, groups, states) is mirrored
from gretel_amd/csrc/seg_geom.hpp."""
import ctypes as C
import itertools

import pytest

from gretel_amd import _lib

SEG_THREADS, SEG_MIN_LEN, SEG_MAX_L, SEG_MAX_L_NARROW, SEGM_L, SEGM_NS = 1024, 8, 5, 6, 5, 2048
RW_FUSE_HALO = 64
RWS_LDS_MAX = 160 * 1024 - 3 * 1024 - 512
KB64 = 64 * 1024
SWITCHES = ("rwseg", "rwseg_small", "emit_small", "fuse", "seg6", "mixed", "rw_lp16", "rw_tband")
N_MAX = 40000


# ---- seg_geom.hpp ------------------------------------------------------------------------------------------------------
def seg_geometry(N, L, R):
    """(NS, seglen, S, G1) of state class R: 4 ranks, 5 symbols, 6 mixed radix."""
    NS = SEGM_NS if R == 6 else R ** L
    g2 = max(1, min(16, (65536 if NS > 3125 else 32768) // NS))
    smax = (25 if 2048 < NS <= 3125 else 16) * g2
    seglen = max(SEG_MIN_LEN, (N + smax - 1) // smax)
    S = (N + seglen - 1) // seglen
    return NS, seglen, S, (S + g2 - 1) // g2


def classes(L):
    """The state classes the host sizes a lag count for (which one applies is decided on the device)."""
    return [4] + ([5] if L <= SEG_MAX_L else []) + ([6] if L == SEGM_L else [])


def emit_small_bytes(N, L, R):
    NS, _, S, G1 = seg_geometry(N, L, R)
    return (G1 + S) * NS * 2 + 16


def rw_fuse_lds(N, L, R, ppb, W):
    NS, seglen, S, G1 = seg_geometry(N, L, R)
    nts = min(S, (ppb + W + seglen - 1) // seglen + 1)
    return ((G1 * NS * 2 + 15) & ~15) + nts * NS * 2 + 512


def rw_lanes(W, L, col, lp16=True, tband=True):
    if not (W > 8 or L > 8):
        return 8
    return 16 if (W <= 32 and L <= 16 and lp16 and (not col or tband)) else 32


def rw_blocks(N, lanes):
    return ((N + 1) * lanes + 255) // 256


# ---- the query -----------------------------------------------------------------------------------------------------------
class Query:
    """One gh_spin_plan_in, asked again and again with another n_snps."""

    def __init__(self, **kw):
        self.lib = _lib.load()
        self.kw = kw
        sw = kw.get("sw", {})
        need_rinfo = kw.get("need_rinfo", bool(kw["mt"]) or sw.get("fuse", 0) >= 1)
        self.inp = _lib.gh_spin_plan_in(1, kw["W"], kw["L"], _lib.GH_STORAGE[kw["storage"]], _lib.GH_COND[kw["cond"]], int(kw["mt"]), 0,
                                        _lib.GH_WALK[kw.get("walk", "seg")], int(kw.get("lt_full", 0)), int(need_rinfo),
                                        int(kw.get("pools_off", 0)), kw["ranked"], *[sw.get(n, -1) for n in SWITCHES])
        self.need_rinfo = need_rinfo
        self.out = _lib.gh_spin_plan()

    def __call__(self, N):
        self.inp.n_snps = N
        rc = self.lib.gh_debug_spin_plan(C.byref(self.inp), C.byref(self.out))
        assert rc == 0, (self.kw, N)
        o = self.out
        return (o.flow, o.emit_small, o.seg6, o.stride, o.rw_lanes, o.S, o.mixed, o.need_layout, o.lds)


NONE, SERIAL, SEG, RWSEG, FUSE, POOLS = range(6)
GRID = sorted(set([1, 2, 7, 8, 9, 63, 64, 65, 72, 73, 100, 127, 128, 129, 255, 256, 257, 900, 2047, 2048, 2049, 4096, 8191, 12000, 20011,
                   25000, 30000, 31000, 32000, 32768, 35000, N_MAX]))


def shape(p):
    """What flips: everything but the figures that grow with N."""
    return (p[0], p[1], p[2], p[4], p[6])


def points(q):
    """The grid and, around every length between two grid points at which the plan's shape flips, five lengths."""
    pts = set(GRID)
    for lo, hi in zip(GRID, GRID[1:]):
        a, b = shape(q(lo)), shape(q(hi))
        while a != b and hi - lo > 1:
            mid = (lo + hi) // 2
            m = shape(q(mid))
            if m == a:
                lo = mid
            else:
                hi, b = mid, m
        if a != b:
            pts.update(n for n in range(lo - 2, hi + 3) if 1 <= n <= N_MAX)
    return sorted(pts)


def check_point(q, N, p):
    kw, sw = q.kw, q.kw.get("sw", {})
    L, W, ranked = kw["L"], kw["W"], kw["ranked"]
    col = kw["cond"] in ("C", "E")
    flow, emit_small, seg6, stride, lanes, S, mixed, need_layout, lds = p
    on = lambda name, default=1: sw.get(name, default) != 0        # noqa: E731
    where = (kw, N, p)
    assert not need_layout and flow != NONE, where          # (the layout is given at every point of the sweep)
    walk_seg = kw.get("walk", "seg") == "seg"
    # seg6 <=> L = 6, a ranked table, GH_SEG6 != 0 (and the segment-parallel extension at all)
    assert bool(seg6) == (walk_seg and L == SEG_MAX_L_NARROW and ranked == 1 and on("seg6")), where
    # L >= 7 => pools or serial; so is L = 6 without seg6; up to 5 the enumerated states (unless GH_WALK pins a serial walker)
    if L >= 7 or (L == 6 and not seg6) or not walk_seg:
        assert flow in (POOLS, SERIAL), where
        assert flow == (POOLS if walk_seg and L >= 6 and not kw.get("pools_off") else SERIAL), where
        assert not emit_small and not lds and not mixed, where
        pool_lanes = rw_lanes(W, L, col) if walk_seg and L >= 6 else 8
        assert lanes == pool_lanes and stride == rw_blocks(N, pool_lanes), where
        assert (S >= 1) == (flow == POOLS), where
        return
    assert flow in (SEG, RWSEG, FUSE), where
    cls = classes(L)
    assert S == max(seg_geometry(N, L, R)[2] for R in cls), where
    assert lanes == rw_lanes(W, L, col), where
    # the stride holds the blocks of every reweight kernel the flow may launch (k_rw with this spin's lane groups, and the 8-lane
    # k_marg<T,true>), and one partial sum per segment under k_rwseg
    assert stride >= rw_blocks(N, lanes) and stride >= rw_blocks(N, 8), where
    assert stride == (max(rw_blocks(N, lanes), S) if flow == RWSEG else rw_blocks(N, lanes)), where
    # emit_small <=> the segment maps of every class fit 64 KB and GH_EMIT_SMALL != 0 (the three-launch flow has no emit at all)
    small = max(emit_small_bytes(N, L, R) for R in cls) <= KB64 and on("emit_small")
    assert bool(emit_small) == (small and flow != FUSE), where
    longest = max(seg_geometry(N, L, R)[1] for R in cls)
    fuse_sw = sw.get("fuse", 0)
    if flow == RWSEG:
        assert lanes == 8 and longest + L + 1 <= SEG_THREADS // 8 and 0 < lds <= RWS_LDS_MAX and not kw.get("lt_full"), where
        assert on("rwseg") and (not small or on("rwseg_small")), where
    if flow == FUSE:
        R = 4 if ranked else 5
        assert q.need_rinfo and W <= RW_FUSE_HALO and lanes == 8 and fuse_sw >= 1, where
        assert 0 < lds <= KB64 and lds == rw_fuse_lds(N, L, R, 32, W), where
        assert L <= (SEG_MAX_L_NARROW if R == 4 else SEG_MAX_L), where                     # the radix is allowed at this lag count
        assert fuse_sw == 2 or not (emit_small_bytes(N, L, R) <= KB64 and on("emit_small")), where
    # ... and the other way round: a flow is taken wherever its conditions hold
    if q.need_rinfo and W <= RW_FUSE_HALO and lanes == 8 and fuse_sw >= 1:
        R = 4 if ranked else 5
        small_r = emit_small_bytes(N, L, R) <= KB64 and on("emit_small")
        fits = L <= (SEG_MAX_L_NARROW if R == 4 else SEG_MAX_L) and rw_fuse_lds(N, L, R, 32, W) <= KB64
        assert (flow == FUSE) == ((not small_r or fuse_sw == 2) and fits), where
    else:
        assert flow != FUSE, where
    if flow == SEG:
        assert not lds, where
        if not col:         # (row conditionals: the kernel's LDS does not grow with the band, only the segment length can be in the way)
            assert (kw.get("lt_full") or lanes != 8 or not on("rwseg") or (small and not on("rwseg_small")) or
                    longest + L + 1 > SEG_THREADS // 8), where
    assert bool(mixed) == (flow != FUSE and L == SEGM_L and on("mixed")), where


BANDS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 33]
SWITCH_SETS = [{}, {"rwseg": 0}, {"rwseg_small": 0}, {"emit_small": 0}, {"fuse": 1}, {"fuse": 2}, {"fuse": 2, "emit_small": 0},
               {"seg6": 0}, {"mixed": 0}]


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 6, 7])
def test_every_plan_meets_the_conditions_of_its_flow(L):
    flows = set()
    for W, storage, cond, mt, ranked, sw in itertools.product(BANDS, ("f32", "f64"), ("A", "C"), (False, True), (0, 1), SWITCH_SETS):
        q = Query(L=L, W=W, storage=storage, cond=cond, mt=mt, ranked=ranked, sw=sw)
        for N in points(q):
            p = q(N)
            check_point(q, N, p)
            flows.add(p[0])
    # (L = 6: short ranked windows fit the three-launch flow's LDS as well)
    assert flows == ({SEG, RWSEG, FUSE} if L <= 5 else {SEG, RWSEG, FUSE, POOLS} if L == 6 else {POOLS})


@pytest.mark.parametrize("extra", [dict(lt_full=1), dict(walk="spec"), dict(walk="src"), dict(pools_off=1), dict(need_rinfo=0, sw={"fuse": 2})])
def test_creation_time_switches(extra):
    for L, W, cond, ranked in itertools.product((1, 3, 5, 6, 7, 20), (4, 9), ("A", "C"), (0, 1)):
        kw = dict(L=L, W=W, storage="f32", cond=cond, mt=False, ranked=ranked)
        kw.update(extra)
        q = Query(**kw)
        for N in points(q):
            check_point(q, N, q(N))


def test_the_layout_is_asked_for_only_where_the_choice_depends_on_it():
    for L, sw, want in [(3, {}, 0), (5, {}, 0), (6, {}, 1), (6, {"seg6": 0}, 0), (7, {}, 0), (3, {"fuse": 1}, 1), (3, {"fuse": 2}, 1)]:
        q = Query(L=L, W=4, storage="f32", cond="A", mt=False, ranked=-1, sw=sw)
        p = q(900)
        assert p[7] == want, (L, sw, p)
        if want:
            assert p[:7] + p[8:] == (NONE, 0, 0, 0, 0, 0, 0, 0), p       # nothing else is chosen before the look
    # band 9: lane groups of 16, the three-launch flow is out whatever the layout -- no look
    assert Query(L=3, W=9, storage="f32", cond="A", mt=False, ranked=-1, sw={"fuse": 2})(900)[7] == 0
    # a serial walker pinned at creation never looks
    assert Query(L=6, W=4, storage="f32", cond="A", mt=False, ranked=-1, walk="spec")(900)[:3] == (SERIAL, 0, 0)


def test_known_windows():
    """The flagship shapes, from the rules above by hand: 900 SNPs at L = 3 is a small window under k_rwseg (two launches per
    path); 20 011 SNPs under conditional C in binary64 at band 9 has lane groups of 16, hence four launches."""
    d = _lib.spin_plan(900, 4, 3)
    assert (d["flow"], d["emit_small"], d["seg6"], d["rw_lanes"]) == ("rwseg", 1, 0, 8), d
    assert d["S"] == 113 and d["stride"] == max(113, rw_blocks(900, 8)), d
    d = _lib.spin_plan(20011, 9, 3, storage="f64", cond_mode="C")
    assert (d["flow"], d["emit_small"], d["rw_lanes"], d["lds"]) == ("seg", 0, 16, 0), d
    assert _lib.spin_plan(900, 4, 7)["flow"] == "pools" and _lib.spin_plan(900, 4, 7, walk="spec")["flow"] == "serial"


def test_arguments_are_checked():
    lib = _lib.load()
    out = _lib.gh_spin_plan()

    def rc(**change):
        base = dict(n_snps=100, band=4, L=3, storage=0, cond_mode=0, walk_mode=0, ranked=-1)
        base.update(change)
        inp = _lib.gh_spin_plan_in(**base)
        return lib.gh_debug_spin_plan(C.byref(inp), C.byref(out))

    assert rc() == 0
    for bad in (dict(n_snps=0), dict(band=0), dict(L=0), dict(storage=2), dict(storage=-1), dict(cond_mode=5), dict(cond_mode=-1),
                dict(walk_mode=4), dict(walk_mode=-1), dict(ranked=2), dict(ranked=-2)):
        assert rc(**bad) == _lib.GH_ERR_ARG, bad
    inp = _lib.gh_spin_plan_in(n_snps=100, band=4, L=3)
    assert lib.gh_debug_spin_plan(None, C.byref(out)) == _lib.GH_ERR_ARG
    assert lib.gh_debug_spin_plan(C.byref(inp), None) == _lib.GH_ERR_ARG
    with pytest.raises(TypeError):
        _lib.spin_plan(100, 4, 3, no_such_switch=1)
