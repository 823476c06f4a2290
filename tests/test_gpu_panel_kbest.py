"""K-best decoding over a panel (gh_panel_viterbi_kbest, gh_panel_viterbi_kbest_info; HanselBatch.viterbi_kbest /
viterbi_kbest_info; --kbest of gretel_amd.panel): every window's result is gh_viterbi_kbest's on that window alone, bit for bit and
in the same order.  The references are the plain statement of the definition (tests/kbest_ref.py over the C oracle) and, since the
call only reads the tensors, Hansel.viterbi_kbest() on the same handle afterwards: each window's twin.

What the ragged panel's shapes make of the kernels' branches (LDS of a launch = the largest need among its windows):
n1 / n2 N < L, n_out < k; warm the whole window warm-up at 4096 states; one4 / one14 S = 1, the second without the table ring
(Le = 14 > 12: the second walk launch); bi7 128 states * 32 = the cap, bi12 4096 states * 1; a3 125 * 32 = 4000 slots, four a
thread, not a multiple of 1024; a5 3125 states; a4_5 1024 * 4 = exactly the cap; C2 N > 512, more than one chunk of the trace;
hole1 / hole8 a hole at the first and at the last position."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kbest_ref
from decode_util import BAM, E_MT, SYMS, VCF, _from_haps, _table
from gretel_amd import _lib, bamio, cmd, panel, util
from gretel_amd.hansel import Hansel, HanselBatch, HanselPanel
from gretel_amd.synth import make_support_table
from spec_util import make_pair, same, spec_id

pytestmark = pytest.mark.gpu
CAP = _lib.GH_VITERBI_MAX_STATES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGTAC = ["ACGTAC", "CGTACG", "ACTTAG", "AGTTAC"]
OCT = ["ACGTACGT", "CGTACGTA", "ACTTAGGT"]


def _biallelic(L):
    def make(kw):
        rng = np.random.default_rng(12)
        haps = ["".join("AG"[v] for v in rng.integers(0, 2, 16)) for _ in range(6)]
        return _from_haps(haps, band=12, L=L, **kw)
    return make


# the windows by name: (handle, oracle) under a spec
WINDOWS = {
    "n1": lambda kw: _from_haps(["A", "C", "C"], band=1, L=4, **kw),
    "n2": lambda kw: _from_haps(["AC", "CA", "AA"], band=1, L=5, **kw),
    "warm": lambda kw: _from_haps(ACGTAC, band=6, L=9, **kw),
    "one4": lambda kw: _from_haps(["AAAAA", "AAAAA"], band=4, L=4, **kw),
    "one14": lambda kw: _from_haps(["A" * 16, "A" * 16], band=14, L=14, **kw),
    "bi7": _biallelic(7),
    "bi12": _biallelic(12),
    "a3": lambda kw: make_pair(_table("a"), L=3, **kw),
    "a5": lambda kw: make_pair(_table("a"), L=5, **kw),
    "a4_3": lambda kw: make_pair(_table("a4"), L=3, **kw),
    "a4_5": lambda kw: make_pair(_table("a4"), L=5, **kw),
    "C2": lambda kw: make_pair(_table("C2"), L=2, **kw),
    "hole1": lambda kw: _from_haps(OCT, band=3, L=3, skip=(1,), **kw),
    "hole8": lambda kw: _from_haps(OCT, band=3, L=3, skip=(8,), **kw),
    "tie1": lambda kw: _from_haps(["ACACAC", "CACACA"], band=3, L=3, **kw),
    "tie2": lambda kw: _from_haps(["AGTTACG", "CGTTACG"], band=3, L=3, **kw),
}
# the ragged panel: (window, k, what viterbi_info says of it afterwards, n_out)
RAGGED = [("n1", 8, (2, 1, 2), 2), ("n2", 8, (2, 2, 4), 4), ("warm", 1, (4, 6, 4096), 1), ("one4", 4, (1, 4, 1), 1), ("one14", 4, (1, 14, 1), 1),
          ("bi7", 32, (2, 7, 128), 32), ("bi12", 1, (2, 12, CAP), 1), ("a3", 32, (5, 3, 125), 32), ("a5", 1, (5, 5, 3125), 1),
          ("a4_5", 4, (4, 5, 1024), 4), ("C2", 8, (4, 2, 16), 8), ("hole1", 4, None, 0), ("hole8", 4, None, 0)]
_refs = {}


def _win(name, k, **kw):
    """(the handle, the reference's k best of its oracle: computed once per window, k and spec, never changed)."""
    h, o = WINDOWS[name](kw)
    key = (name, k, spec_id(kw))
    if key not in _refs:
        _refs[key] = kbest_ref.kbest(o, h.n, k, h._cfg["cand_order"])
    return h, _refs[key]


def _str(path):
    return "".join(SYMS[int(v)] for v in path[1:])


def _equal(got, ref, what):
    assert (got["n"], got["hole_at"]) == (ref["n"], ref["hole_at"]), what
    assert got["paths"].dtype == np.uint8 and got["ll_chain"].dtype == np.float64, what
    assert got["paths"].shape == ref["paths"].shape and got["ll_chain"].shape == ref["ll_chain"].shape, what
    assert got["ll_chain"].tolist() == ref["ll_chain"].tolist(), (what, [
        (i, a, b) for i, (a, b) in enumerate(zip(got["ll_chain"], ref["ll_chain"])) if a != b][:4])
    assert np.array_equal(got["paths"], ref["paths"]), (what, np.argwhere(got["paths"] != ref["paths"])[:4].tolist())


def _alone(hs, ks, got, what=""):
    """Every window against Hansel.viterbi_kbest(k_w) on the same handle, and the handle's viterbi_info against the single call's."""
    for w, (h, k, r) in enumerate(zip(hs, ks, got)):
        info = h.viterbi_info()
        _equal(r, h.viterbi_kbest(k), "%s window %d alone" % (what, w))
        assert h.viterbi_info()[:3] == info[:3], (what, w, info, h.viterbi_info())


@pytest.mark.parametrize("kw", [{}, E_MT], ids=spec_id)
def test_the_ragged_panel(kw):
    wins = [_win(name, k, **kw) for name, k, _, _ in RAGGED]
    hs, ks = [h for h, _ in wins], [k for _, k, _, _ in RAGGED]
    assert hs[10].n > 512
    p = HanselPanel(hs)
    got = p.viterbi_kbest(ks)
    assert len(got) == len(wins) == 13
    for (h, ref), r, (name, k, shape, n_out) in zip(wins, got, RAGGED):
        _equal(r, ref, name)
        assert r["n"] == n_out, name
        if shape is not None:
            assert h.viterbi_info()[:3] == shape and shape[2] * k <= CAP, name
            assert h.viterbi_info()[3] >= (h.n + 1) * shape[2] * k, name
            sc = h.score_paths(r["paths"])
            assert sc["ll_chain"].tolist() == r["ll_chain"].tolist() and (sc["n_on"] == h.n).all(), name
            assert len({x.tobytes() for x in r["paths"]}) == r["n"] and (np.diff(r["ll_chain"]) <= 0).all(), name
    assert [(r["n"], r["hole_at"], r["paths"].shape) for r in got[-2:]] == [(0, 1, (0, 9)), (0, 8, (0, 9))]
    windows, holes, launches, scratch = p.viterbi_kbest_info()
    # (two walk launches: the S = 1, Le = 14 window walks without the ring)
    assert windows == 13 and holes == 2 and launches >= 2
    assert scratch == sum(h.viterbi_info()[3] for h in hs)
    _alone(hs, ks, got, spec_id(kw))
    # each window got its own arrays
    assert all(r["paths"].base is None or not np.shares_memory(r["paths"], got[0]["paths"]) for r in got[1:])
    keep = got[1]["paths"].copy(), got[1]["ll_chain"].copy()
    got[0]["paths"][:] = 0
    got[0]["ll_chain"][:] = 0.0
    assert not np.shares_memory(got[0]["ll_chain"], got[1]["ll_chain"])
    assert np.array_equal(got[1]["paths"], keep[0]) and np.array_equal(got[1]["ll_chain"], keep[1])


def _raw(p, hs, ks, poff, loff, fill=True):
    """gh_panel_viterbi_kbest through ctypes into arrays pre-filled with 0xAB / 7.25: (rc, paths, ll, n_out, hole_at)."""
    n = len(hs)
    ka = np.asarray(ks, dtype=np.int32)
    poff, loff = np.asarray(poff, dtype=np.int64), np.asarray(loff, dtype=np.int64)
    paths = np.full(int(max(o + k * (h.n + 1) for o, k, h in zip(poff, ks, hs))), 0xAB, dtype=np.uint8)
    ll = np.full(int(max(o + k for o, k in zip(loff, ks))), 7.25)
    n_out, hole = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    rc = _lib.load().gh_panel_viterbi_kbest(p._b, ka.ctypes.data, paths.ctypes.data, poff.ctypes.data, ll.ctypes.data, loff.ctypes.data,
                                            n_out.ctypes.data, hole.ctypes.data)
    return rc, paths, ll, n_out, hole


def test_through_ctypes_nothing_beyond_n_out_is_written():
    names = ["n1", "hole1", "a3", "one4", "hole8", "bi7", "n2"]
    ks = [8, 4, 32, 4, 4, 32, 8]
    wins = [_win(name, k) for name, k in zip(names, ks)]
    hs = [h for h, _ in wins]
    n1 = [h.n + 1 for h in hs]
    p = HanselPanel(hs)
    packed_p = np.concatenate([[0], np.cumsum([k * m for k, m in zip(ks, n1)])[:-1]])
    packed_l = np.concatenate([[0], np.cumsum(ks)[:-1]])
    # ... and a layout with gaps, the windows in reverse order
    gap_p, gap_l, at_p, at_l = [0] * len(hs), [0] * len(hs), 5, 3
    for w in reversed(range(len(hs))):
        gap_p[w], gap_l[w] = at_p, at_l
        at_p += ks[w] * n1[w] + 7 + w
        at_l += ks[w] + 1 + w % 2
    for poff, loff in ((packed_p, packed_l), (gap_p, gap_l)):
        rc, paths, ll, n_out, hole = _raw(p, hs, ks, poff, loff)
        assert rc == _lib.GH_OK
        assert n_out.tolist() == [2, 0, 32, 1, 0, 32, 4] and hole.tolist() == [0, 1, 0, 0, 8, 0, 0]
        seen_p, seen_l = np.zeros(len(paths), dtype=bool), np.zeros(len(ll), dtype=bool)
        for w, (_, ref) in enumerate(wins):
            a, e, m = int(poff[w]), int(loff[w]), int(n_out[w])
            assert np.array_equal(paths[a:a + m * n1[w]].reshape(m, n1[w]), ref["paths"]), w
            assert ll[e:e + m].tolist() == ref["ll_chain"].tolist(), w
            seen_p[a:a + m * n1[w]] = True
            seen_l[e:e + m] = True
        # rows and scores beyond n_out[w], everything of the two hole windows and the gaps: untouched
        assert (paths[~seen_p] == 0xAB).all() and (ll[~seen_l] == 7.25).all()
        assert (~seen_p).sum() >= (8 - 2) * 2 + 4 * 9 * 2 + 3 * 6 + 4 * 3


def test_more_windows_than_workgroups_are_resident_at_once():
    rng = np.random.default_rng(40)
    hs, ks = [], []
    for i in range(300):
        t = make_support_table(int(rng.integers(30, 61)), 600, k=None, seed=5000 + i)
        hs.append(make_pair(t, L=2 + i % 3)[0])
        ks.append(1 + i % 8)
    p = HanselPanel(hs)
    got = p.viterbi_kbest(ks)
    assert p.viterbi_kbest_info()[:3] == (300, 0, 1)
    assert [r["n"] for r in got] == ks
    _alone(hs, ks, got)


@pytest.mark.parametrize("order", ["ACGT-", "T-GCA"])
def test_exact_ties(order):
    wins = [_win("tie1", 2, cand_order=order), _win("tie2", 2, cand_order=order)]
    hs = [h for h, _ in wins]
    got = HanselPanel(hs).viterbi_kbest(2)
    for (h, ref), r in zip(wins, got):
        _equal(r, ref, order)
        assert r["n"] == 2 and r["ll_chain"][0] == r["ll_chain"][1]
    # (the order tests/test_gpu_kbest.py::test_exact_ties states)
    assert [_str(x) for x in got[0]["paths"]] == (["CACACA", "ACACAC"] if order == "ACGT-" else ["ACACAC", "CACACA"])
    assert [_str(x) for x in got[1]["paths"]] == (["AGTTACG", "CGTTACG"] if order == "ACGT-" else ["CGTTACG", "AGTTACG"])
    _alone(hs, [2, 2], got, order)


def test_k_1_everywhere_is_the_exact_decoder():
    names = [name for name, _, _, _ in RAGGED]
    make = lambda: [WINDOWS[name]({})[0] for name in names]
    hs, twins = make(), make()
    got = HanselPanel(hs).viterbi_kbest(1)
    spun = HanselPanel(twins).viterbi_spin(1)
    for name, r, s in zip(names, got, spun):
        assert (r["n"], r["hole_at"]) == (s["n"], s["hole_at"]), name
        assert np.array_equal(r["paths"], s["paths"]) and r["ll_chain"].tolist() == s["ll_chain"].tolist(), name
    assert [r["n"] for r in got] == [1] * 11 + [0, 0]


def _stats(h):
    return h.export_band().tobytes(), h.L, h.n_slices, h.n_crumbs


@pytest.mark.parametrize("cls", [HanselPanel, HanselBatch], ids=["panel", "batch"])
def test_the_call_only_reads(cls):
    if cls is HanselPanel:
        make = lambda: [make_pair(_table("a"), L=3)[0], make_pair(_table("a4"), L=2)[0], make_pair(_table("a"), L=2)[0]]
    else:                                                       # (a batch: windows of one shape)
        make = lambda: [make_pair(_table(w), L=3)[0] for w in ("a", "a4", "a")]      # (a4: a's reads without the deletions)
    hs, fresh = make(), make()
    ks = [8, 32, 5]
    before = [_stats(h) for h in hs]
    p = cls(hs)
    got = p.viterbi_kbest(ks)
    assert [_stats(h) for h in hs] == before
    _alone(hs, ks, got)
    assert [_stats(h) for h in hs] == before
    # the block is shared with the two other panel decoders: in turn on one panel, each gives what it gives on fresh handles
    vm = p.viterbi_marginals()
    again = p.viterbi_kbest(ks)
    assert [_stats(h) for h in hs] == before
    for a, b in zip(got, again):
        _equal(a, b, "after the max-marginals")
    for a, f in zip(vm, make()):
        b = f.viterbi_marginals()
        assert np.array_equal(a["mm"], b["mm"]) and np.array_equal(a["cm"], b["cm"])
    for a, b in zip(p.spin(4), cls(fresh).spin(4)):
        same(a, b)
    for h, f in zip(hs, fresh):
        assert np.array_equal(h.export_band(), f.export_band())
    # ... and the exact spin behind a k-best call, against fresh handles that never saw one
    hs2, fresh2 = make(), make()
    p2 = cls(hs2)
    p2.viterbi_kbest(ks)
    for a, b in zip(p2.viterbi_spin(2), cls(fresh2).viterbi_spin(2)):
        same(a, b)
        assert a["ll_chain"].tolist() == b["ll_chain"].tolist()
    for h, f in zip(hs2, fresh2):
        assert np.array_equal(h.export_band(), f.export_band())
    _alone(hs2, [1, 1, 1], p2.viterbi_kbest(1), "after the exact spin")       # (the reweighted tensors: each window's twin all the same)


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from decode_util import _from_haps, _table
from gretel_amd.hansel import HanselPanel
from spec_util import make_pair
hs = [make_pair(_table("a"), L=3)[0], make_pair(_table("a4"), L=5)[0], _from_haps(["A" * 16, "A" * 16], band=14, L=14)[0]]
p = HanselPanel(hs)
got = p.viterbi_kbest([32, 4, 4])
assert p.viterbi_kbest_info()[:3] == (3, 0, 1), p.viterbi_kbest_info()      # one walk launch: no window stages the ring
for w, r in enumerate(got):
    np.save(sys.argv[1] + "paths%%d.npy" %% w, r["paths"])
    np.save(sys.argv[1] + "ll%%d.npy" %% w, r["ll_chain"])
"""


def test_the_tables_from_global_memory_give_the_same_bits(tmp_path):
    # GH_VIT_STAGE is read once in a process: a fresh child
    env = dict(os.environ, GH_VIT_STAGE="0")
    stem = str(tmp_path) + os.sep
    subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), stem], env=env, check=True, timeout=300)
    for w, (name, k) in enumerate((("a3", 32), ("a4_5", 4), ("one14", 4))):
        ref = _win(name, k)[1]
        assert np.array_equal(np.load(stem + "paths%d.npy" % w), ref["paths"]), name
        assert np.load(stem + "ll%d.npy" % w).tolist() == ref["ll_chain"].tolist(), name


def _state(h):
    return h.export_band().tobytes(), h.viterbi_info(), h.L, h.n_slices, h.n_crumbs


def test_refusals():
    L = _lib.load()
    t4 = _table("a4")
    big = make_pair(t4, L=7)[0]
    ok = [make_pair(_table("a"), L=3)[0], make_pair(t4, L=3)[0]]
    hs = [ok[0], big, ok[1]]
    p = HanselPanel(hs)
    ok[1].viterbi_path()                                        # (a viterbi_info to keep)
    before = [_state(h) for h in hs]
    with pytest.raises(_lib.GretelHipError, match=r"window 1: .*16384 states") as e:
        p.viterbi_kbest(4)
    assert e.value.code == _lib.GH_ERR_ARG
    assert [_state(h) for h in hs] == before
    big.L = 5                                                   # 1024 states: k = 4 is the most
    assert big.viterbi_kbest_max() == 4 and ok[0].viterbi_kbest_max() == 32
    before = [_state(h) for h in hs]
    with pytest.raises(_lib.GretelHipError, match=r"window 1: .*1024 states.*k = 8 .*8192 slots.*largest k this window takes is 4") as e:
        p.viterbi_kbest([4, 8, 4])
    assert e.value.code == _lib.GH_ERR_ARG
    for bad in (0, 33):
        with pytest.raises(_lib.GretelHipError, match=r"window 2: .*k = %d is outside 1\.\.32" % bad) as e:
            p.viterbi_kbest([4, 4, bad])
        assert e.value.code == _lib.GH_ERR_ARG
    with pytest.raises(ValueError):
        p.viterbi_kbest([4, 4])
    assert [_state(h) for h in hs] == before
    fresh = Hansel(t4.n_snps, band=t4.band)
    with pytest.raises(_lib.GretelHipError, match="window 1: .*before any fill") as e:
        HanselPanel([ok[1], fresh]).viterbi_kbest(2)
    assert e.value.code == _lib.GH_ERR_STATE
    hz = [make_pair(t4, L=3, offer_zero=True)[0] for _ in range(2)]
    with pytest.raises(_lib.GretelHipError, match="window 0: .*offer_zero") as e:
        HanselPanel(hz).viterbi_kbest(2)
    assert e.value.code == _lib.GH_ERR_ARG
    assert [_state(h) for h in hs] == before
    # null arguments and negative offsets through ctypes
    n = len(hs)
    ks = np.array([4, 4, 4], dtype=np.int32)
    n1 = [h.n + 1 for h in hs]
    paths, ll = np.zeros(4 * sum(n1), dtype=np.uint8), np.zeros(4 * n)
    poff = np.zeros(n, dtype=np.int64)
    poff[1:] = np.cumsum([4 * m for m in n1[:-1]])
    loff = np.arange(n, dtype=np.int64) * 4
    n_out, hole = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    args = [p._b, ks.ctypes.data, paths.ctypes.data, poff.ctypes.data, ll.ctypes.data, loff.ctypes.data, n_out.ctypes.data, hole.ctypes.data]
    for q in range(8):
        a = list(args)
        a[q] = None
        assert L.gh_panel_viterbi_kbest(*a) == _lib.GH_ERR_ARG and b"null argument" in L.gh_last_error(), q
    for q, off in ((3, poff), (5, loff)):
        neg = off.copy()
        neg[2] = -1
        a = list(args)
        a[q] = neg.ctypes.data
        assert L.gh_panel_viterbi_kbest(*a) == _lib.GH_ERR_ARG and b"negative offset" in L.gh_last_error()
    assert n_out.tolist() == [-1] * n and hole.tolist() == [-1] * n and not paths.any() and not ll.any()
    assert [_state(h) for h in hs] == before
    # after the refusals the same arguments are served
    assert L.gh_panel_viterbi_kbest(*args) == _lib.GH_OK and n_out.tolist() == [4] * n and hole.tolist() == [0] * n
    assert big.viterbi_info()[:3] == (4, 5, 1024)
    for w, (name, h) in enumerate((("a3", hs[0]), ("a4_5", hs[1]), ("a4_3", hs[2]))):
        ref = _win(name, 4)[1]
        assert np.array_equal(paths[poff[w]:poff[w] + 4 * n1[w]].reshape(4, n1[w]), ref["paths"]), name
        assert ll[4 * w:4 * w + 4].tolist() == ref["ll_chain"].tolist(), name
    info = np.zeros(4, dtype=np.int64)
    assert L.gh_panel_viterbi_kbest_info(None, info.ctypes.data) == _lib.GH_ERR_ARG
    assert L.gh_panel_viterbi_kbest_info(p._b, None) == _lib.GH_ERR_ARG
    assert L.gh_panel_viterbi_kbest_info(p._b, info.ctypes.data) == _lib.GH_OK and info.tolist()[:3] == [n, 0, 1]
    assert info[3] == sum(h.viterbi_info()[3] for h in hs)


def _files(d):
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("exact", [[], ["--exact"]], ids=["greedy", "exact"])
def test_cli_kbest(exact, tmp_path, capsys):
    regions = [("r1", 0, 20), ("r2", 0, 15), ("r3", 0, 12)]                            # (SNPs at 1, 2, 10 and 20)
    bed = tmp_path / "r.bed"
    bed.write_text("".join("hoot\t%d\t%d\t%s\n" % (a, b, n) for n, a, b in regions))
    out, both, plain = tmp_path / "panel", tmp_path / "both", tmp_path / "plain"
    opts = ["-p", "6"] + exact
    assert panel.main([BAM, VCF, str(bed), "-o", str(plain)] + opts) == 0
    assert panel.main([BAM, VCF, str(bed), "-o", str(out)] + opts + ["--kbest", "8"]) == 0
    assert panel.main([BAM, VCF, str(bed), "-o", str(both)] + opts + ["--margins", "--kbest", "8"]) == 0
    for name, a, b in regions:
        single = tmp_path / "single" / name
        single.mkdir(parents=True)
        assert cmd.main([BAM, VCF, "hoot", "-s", str(a + 1), "-e", str(b), "--quiet", "-o", str(single)] + opts + ["--margins", "--kbest", "8"]) == 0
        kbest = (single / "gretel.kbest").read_bytes()
        assert kbest.startswith(b"# ") and kbest.count(b"\n") >= 2, name
        with_k, with_both, without = _files(out / name), _files(both / name), _files(plain / name)
        assert with_k.pop("gretel.kbest") == kbest, name
        assert with_k == without and "out.fasta" in without, name
        assert with_both.pop("gretel.kbest") == kbest, name
        assert with_both.pop("gretel.margins") == (single / "gretel.margins").read_bytes(), name
        assert with_both == without, name
    capsys.readouterr()


def test_cli_kbest_leaves_a_region_over_the_cap_without_the_file(tmp_path, capsys, monkeypatch):
    # (the construction of tests/test_gpu_panel_viterbi.py: table a4's BAM, the whole contig one region with its filled L set to 7)
    bam, vcf = str(tmp_path / "c.bam"), str(tmp_path / "c.vcf.gz")
    contig, s, e = bamio.synth_to_files(_table("a4"), bam, vcf)
    regions = [("five", 0, 55), ("whole", s - 1, e), ("six", 100, 165)]
    bed = tmp_path / "r.bed"
    bed.write_text("".join("%s\t%d\t%d\t%s\n" % (contig, a, b, n) for n, a, b in regions))
    load = util.load_from_bam

    def over(bam_, contig_, start, end, vh, **kw):
        h = load(bam_, contig_, start, end, vh, **kw)
        if vh["N"] == 60:
            h.L = 7
        return h

    monkeypatch.setattr(util, "load_from_bam", over)
    out = tmp_path / "panel"
    opts = ["-p", "4"]
    assert panel.main([bam, vcf, str(bed), "-o", str(out)] + opts + ["--kbest", "8"]) == 0
    cap = capsys.readouterr()
    assert cap.err.count("whole: [NOTE] --kbest:") == 1
    assert "16384 states, more than the 4096" in cap.err
    assert [x.split("\t")[0] for x in cap.out.splitlines()] == ["five", "whole", "six"]
    assert "out.fasta" in os.listdir(out / "whole") and "gretel.kbest" not in os.listdir(out / "whole")
    monkeypatch.setattr(util, "load_from_bam", load)
    for name, a, b in (regions[0], regions[2]):
        single = tmp_path / "single" / name
        single.mkdir(parents=True)
        assert cmd.main([bam, vcf, contig, "-s", str(a + 1), "-e", str(b), "--quiet", "-o", str(single)] + opts + ["--kbest", "8"]) == 0
        note = capsys.readouterr().err.count("[NOTE] --kbest:")
        # (a region whose K lists are too many slots gets the note from both CLIs and the file from neither)
        assert cap.err.count("%s: [NOTE] --kbest:" % name) == note, name
        assert _files(out / name) == _files(single), name
        assert ("gretel.kbest" in os.listdir(single)) == (note == 0), name
    capsys.readouterr()
