"""The native decoder's depth cap at the edges of its batches (gretel_amd/csrc/bam_support.cpp).

In front of the sequential pass that applies pysam's max_depth sits a shortcut: per inflated batch the decoder SHOWS, from a
histogram of read starts, that no stretch as long as the longest read span holds max_depth reads, and sets the batch aside.
Here that check is driven as the one function it is (gio_debug_depth_shown) against its contract computed by brute force, and the
batch edges are swept end to end, native against the Python decoder, with GIO_WINDOW=65536 (one BGZF block per batch)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from gretel_amd import bamio, util

WINDOW = "65536"


# ---------------------------------------------------------------------------------------------------------------------
# 1. the window check, as a unit
# ---------------------------------------------------------------------------------------------------------------------
def _window_sums(H, jlo, jhi, k):
    """sum(H[max(0, j - k) .. j]) for every j in [jlo, jhi], in Python integers."""
    H = [int(x) for x in H]
    return [sum(H[max(0, j - k):j + 1]) for j in range(jlo, jhi + 1)]


def _contract(H, jlo, jhi, k, max_depth):
    """include/gretel_io.h: 1 exactly when 1 + sum(H[max(0, j-k) .. j]) <= max_depth for every j in [jlo, jhi]."""
    return all(1 + s <= max_depth for s in _window_sums(H, jlo, jhi, k))


def test_the_window_check_flips_exactly_at_the_edge_exhaustively():
    """Every n_buckets <= 10, every 0 <= jlo <= jhi < n_buckets, every k in 1 .. n_buckets + 2; one outstanding bucket at each of
    jlo-k-2, jlo-k-1, jlo-k, jlo, jhi, jhi+1 in turn (and none), in two magnitudes -- one far above everything else (an unsigned
    running sum that subtracts it without having added it wraps) and one below a window's sum (the sum is then silently too low);
    max_depth at the largest window sum, + 1 and + 2: shown is False, True, True."""
    wrong = {"said shown": 0, "said not shown": 0}
    first = []
    n_cases = 0
    for n in range(1, 11):
        for jlo in range(n):
            for jhi in range(jlo, n):
                for k in range(1, n + 3):
                    spots = [None] + sorted({t for t in (jlo - k - 2, jlo - k - 1, jlo - k, jlo, jhi, jhi + 1) if 0 <= t < n})
                    for base, big in ((3, 1000), (300, 350)):
                        for t in spots:
                            H = np.array([base + (5 * i + n) % 4 for i in range(n)], dtype=np.uint32)
                            if t is not None:
                                H[t] += big
                            W = max(_window_sums(H, jlo, jhi, k))
                            for md, want in ((W, False), (W + 1, True), (W + 2, True)):
                                assert _contract(H, jlo, jhi, k, md) is want
                                got = bamio.native_depth_shown(H, jlo, jhi, k, md)
                                n_cases += 1
                                if got is not want:
                                    wrong["said shown" if got else "said not shown"] += 1
                                    if len(first) < 5:
                                        first.append((H.tolist(), jlo, jhi, k, md, got))
    print("window check, exhaustive: %d cases, wrong: %r" % (n_cases, wrong))
    assert n_cases > 50000
    assert not first, "%d of %d cases wrong (%r); the first: %r" % (sum(wrong.values()), n_cases, wrong, first)


def test_the_window_check_on_random_histograms():
    """4000 random cases: zeros and empty stretches common, ranges of one bucket and empty ranges (jlo > jhi: nothing to refute),
    k from 0 to past the histogram, one bucket in six far above any window sum (up to 2^32 - 1), max_depth around the largest
    window sum, tiny, and INT32_MAX."""
    rng = np.random.default_rng(20)
    wrong = []
    for case in range(4000):
        n = int(rng.integers(1, 41))
        H = rng.integers(0, 60, size=n).astype(np.uint32)
        H[rng.random(n) < rng.choice([0.2, 0.6, 0.95])] = 0
        if rng.random() < 1 / 6:
            H[int(rng.integers(0, n))] = int(rng.choice([70000, 2 ** 31, 2 ** 32 - 1]))
        jlo = int(rng.integers(0, n))
        jhi = int(rng.integers(jlo, n)) if rng.random() < 0.9 else jlo - 1
        k = int(rng.integers(0, n + 4))
        sums = _window_sums(H, jlo, jhi, k)
        W = max(sums) if sums else 0
        md = int(rng.choice([W - 1, W, W + 1, W + 2, 1, int(rng.integers(1, 200)), 2 ** 31 - 1]))
        md = min(max(md, 1), 2 ** 31 - 1)
        want = _contract(H, jlo, jhi, k, md)
        if jlo > jhi:
            assert want is True
        got = bamio.native_depth_shown(H, jlo, jhi, k, md)
        if got is not want:
            wrong.append((H.tolist(), jlo, jhi, k, md, got))
    print("window check, random: 4000 cases, %d wrong" % len(wrong))
    assert not wrong, "%d of 4000 cases wrong; the first: %r" % (len(wrong), wrong[:3])


def test_the_window_check_refuses_what_it_cannot_index():
    H = np.array([1, 2, 3], dtype=np.uint32)
    assert bamio.native_depth_shown(H, 0, 2, 1, 6) is True and bamio.native_depth_shown(H, 0, 2, 1, 5) is False      # 1 + (2 + 3)
    for jlo, jhi, k in ((-1, 2, 1), (0, 3, 1), (0, 2, -1), (3, 3, 1)):
        with pytest.raises(ValueError):
            bamio.native_depth_shown(H, jlo, jhi, k, 7)
    assert bamio.io_lib().gio_debug_depth_shown(None, 3, 0, 2, 1, 7) == -1


# ---------------------------------------------------------------------------------------------------------------------
# 2. batch edges end to end
# ---------------------------------------------------------------------------------------------------------------------
_rng = np.random.default_rng(3)
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def _seqs(n, ln):
    """n random sequences of ln bases (so that WHICH reads of a pile were dropped shows in the table)."""
    m = _LETTERS[_rng.integers(0, 4, size=(n, ln))]
    return [row.tobytes().decode() for row in m]


def _pile(tag, n, pos0, ln, cigar=None):
    return [("%s%d" % (tag, i), 0, 0, pos0, 60, cigar or "%dM" % ln, s) for i, s in enumerate(_seqs(n, ln))]


def _three_piles():
    """330 reads of 100M at 0-based position 0, 350 at 128, 200 at 150: the first BGZF block ends inside the middle pile, whose
    batch therefore starts k + 1 = 8 buckets behind the crowded bucket 0."""
    return _pile("a", 330, 0, 100) + _pile("b", 350, 128, 100) + _pile("c", 200, 150, 100)


def _write(tmp_path, name, reads, length, snps, index=True):
    bam, vcf = str(tmp_path / (name + ".bam")), str(tmp_path / (name + ".vcf.gz"))
    bamio.write_bam(bam, [("c", length)], reads, index=index)
    bamio.write_vcf_gz(vcf, "c", snps)
    return bam, vcf


def _native(bam, s, e, v, cap):
    a = util.support_table_from_bam(bam, "c", s, e, v, decoder="native", max_depth=cap)
    return a, bamio.native_last_stats()


def _python(bam, s, e, v, cap):
    return util.support_table_from_bam(bam, "c", s, e, v, decoder="python", max_depth=cap)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _agree(bam, s, e, v, cap, n_full):
    """Native equals Python under this cap, and counts as dropped what is missing of the n_full rows without a cap (files in which
    every candidate of the cap opens a row of its own).  Returns the native decoder's stats."""
    got, st = _native(bam, s, e, v, cap)
    want = _python(bam, s, e, v, cap)
    assert _same(got, want), (cap, len(got[0]), len(want[0]), st)
    assert st["depth_dropped"] == n_full - len(got[0]), (cap, st)
    return st


_CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from gretel_amd import bamio, util
bam, vcf, s, e, cap, out = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), sys.argv[7]
v = util.process_vcf(vcf, "c", s, e)
rank, off, bases = util.support_table_from_bam(bam, "c", s, e, v, decoder="native", max_depth=cap)
np.savez(out, rank=rank, off=off, bases=bases)
print(json.dumps(bamio.native_last_stats()))
'''


def _native_in_a_fresh_process(tmp_path, bam, vcf, s, e, cap, **env):
    """The decoder reads GIO_THREADS and GIO_PART_RECORDS once per process: another setting is another process."""
    script, out = str(tmp_path / "decode_once.py"), str(tmp_path / "decoded.npz")
    with open(script, "w") as fh:
        fh.write(_CHILD)
    run = subprocess.run([sys.executable, script, ROOT, bam, vcf, str(s), str(e), str(cap), out],
                         env=dict(os.environ, GIO_WINDOW=WINDOW, **env), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    z = np.load(out)
    return (z["rank"], z["off"], z["bases"]), json.loads(run.stdout.splitlines()[-1])


def test_three_piles_with_the_middle_one_across_a_batch_boundary(tmp_path, monkeypatch):
    """max_depth = 450: the pile at 0 has expired when the pile at 128 is pushed (350 enter); of the 200 reads at 150 the first
    hundred find at most 449 in the buffer, the second hundred are dropped.  780 rows, whatever the batches and the threads."""
    monkeypatch.setenv("GIO_WINDOW", WINDOW)
    bam, vcf = _write(tmp_path, "piles", _three_piles(), 400, range(5, 400, 5))
    v = util.process_vcf(vcf, "c", 1, 400)
    want = _python(bam, 1, 400, v, 450)
    assert len(want[0]) == 780
    got, st = _native(bam, 1, 400, v, 450)
    print("three piles, cap 450: native %d rows, depth_dropped %d, blocks %d" % (len(got[0]), st["depth_dropped"], st["blocks"]))
    assert (len(got[0]), st["depth_dropped"]) == (780, 100) and st["blocks"] >= 3
    assert _same(got, want)
    for env in ({"GIO_THREADS": "1"}, {"GIO_THREADS": "4"}, {"GIO_THREADS": "4", "GIO_PART_RECORDS": "16"},
                {"GIO_THREADS": "1", "GIO_PART_RECORDS": "16"}):
        got, st = _native_in_a_fresh_process(tmp_path, bam, vcf, 1, 400, 450, **env)
        assert (len(got[0]), st["depth_dropped"], st["threads"]) == (780, 100, int(env["GIO_THREADS"])), (env, st)
        assert st["blocks"] >= 3 and _same(got, want), env
    # one batch (the default window) and no cap
    monkeypatch.delenv("GIO_WINDOW")
    got, st = _native(bam, 1, 400, v, 450)
    assert st["depth_dropped"] == 100 and _same(got, want)
    monkeypatch.setenv("GIO_WINDOW", WINDOW)
    got, st = _native(bam, 1, 400, v, 0)
    assert len(got[0]) == 880 and st["depth_dropped"] == 0 and _same(got, _python(bam, 1, 400, v, 0))


def test_a_window_that_starts_inside_the_middle_pile_through_the_index(tmp_path, monkeypatch):
    monkeypatch.setenv("GIO_WINDOW", WINDOW)
    bam, vcf = _write(tmp_path, "piles", _three_piles(), 400, range(5, 400, 5))
    # (the pile at 0 does not reach these windows: it is no candidate; from 229 on neither is the middle pile)
    for s, n_full in ((180, 550), (229, 200)):             # inside the middle pile (129 .. 228); on the first base behind it
        v = util.process_vcf(vcf, "c", s, 400)
        assert len(_python(bam, s, 400, v, 0)[0]) == n_full
        for cap in (450, 150, 8000):
            st = _agree(bam, s, 400, v, cap, n_full)
            assert st["used_index"] == 1 and st["blocks"] >= 3
            if cap == 450:
                assert st["depth_dropped"] == (100 if s == 180 else 0)
            if cap == 150:
                assert st["depth_dropped"] > 0


def test_batch_edges_swept_native_against_python(tmp_path, monkeypatch):
    """Piles of na / 350 / 200 reads at 0 / d / d + 22, d swept in steps of 6 so that the second pile's bucket passes k + 1 buckets
    behind the first one's for both read lengths, then a sparse tail so that batches follow the piles; caps around 550 = the second
    and third pile together.  312 points."""
    monkeypatch.setenv("GIO_WINDOW", WINDOW)
    snps = list(range(5, 2400, 7))
    bound = idle = points = 0
    failed = []
    for ln in (100, 60):
        for na in (200, 330, 470):
            for d in range(ln + 4, ln + 80, 6):
                reads = _pile("a", na, 0, ln) + _pile("b", 350, d, ln) + _pile("c", 200, d + 22, ln)
                reads += [("t%d" % i, 0, 0, d + 400 + 3 * i, 60, "%dM" % ln, s) for i, s in enumerate(_seqs(400, ln))]
                bam, vcf = _write(tmp_path, "sweep", reads, 2400, snps)
                v = util.process_vcf(vcf, "c", 1, 2400)
                for cap in (450, 549, 550, 551):
                    points += 1
                    want = _python(bam, 1, 2400, v, cap)
                    try:
                        got, st = _native(bam, 1, 2400, v, cap)
                    except Exception as exc:
                        failed.append((ln, na, d, cap, str(exc)[:90]))
                        continue
                    assert st["blocks"] >= 3, (ln, na, d, st)
                    if not _same(got, want):
                        failed.append((ln, na, d, cap, "%d rows against %d" % (len(got[0]), len(want[0]))))
                    bound += st["depth_dropped"] > 0
                    idle += st["depth_dropped"] == 0
    print("sweep: %d points, the cap bound at %d and was idle at %d, %d failed" % (points, bound, idle, len(failed)))
    assert points == 312
    assert not failed, "%d of %d points: %r" % (len(failed), points, failed[:6])
    assert 3 * bound >= points and 3 * idle >= points, (bound, idle)


def test_buckets_wider_than_sixteen_positions(tmp_path, monkeypatch):
    """A 40 Mb window: its start histogram has buckets of 64 positions (the width doubles while range / width + 2 > 2^20).
    600 sparse reads, then the three piles at 39 900 000 / + 256 / + 300."""
    monkeypatch.setenv("GIO_WINDOW", WINDOW)
    length, p = 40_000_000, 39_900_000
    reads = [("s%d" % i, 0, 0, 1000 + 66_000 * i, 60, "100M", s) for i, s in enumerate(_seqs(600, 100))]
    reads += _pile("a", 330, p, 100) + _pile("b", 350, p + 256, 100) + _pile("c", 200, p + 300, 100)
    bam, vcf = _write(tmp_path, "wide", reads, length, range(p + 5, p + 400, 5))
    v = util.process_vcf(vcf, "c", 1, length)
    for cap, rows, dropped in ((450, 780, 100), (8000, 880, 0)):
        got, st = _native(bam, 1, length, v, cap)
        assert (len(got[0]), st["depth_dropped"]) == (rows, dropped) and st["blocks"] >= 4, (cap, st)
        assert _same(got, _python(bam, 1, length, v, cap)), cap


def test_out_of_order_across_a_batch_boundary(tmp_path, monkeypatch):
    """700 reads at 500 .. 1199, then one at 10 as the last record, batches behind the first: with a cap both decoders say where;
    without one both take the records as they come."""
    monkeypatch.setenv("GIO_WINDOW", WINDOW)
    reads = [("r%d" % i, 0, 0, 500 + i, 60, "100M", s) for i, s in enumerate(_seqs(700, 100))] + _pile("late", 1, 10, 100)
    bam, vcf = _write(tmp_path, "ooo", reads, 1500, range(5, 1500, 5), index=False)
    v = util.process_vcf(vcf, "c", 1, 1500)
    for cap in (8000, 450, 5):
        said = []
        for dec in ("native", "python"):
            with pytest.raises((IOError, ValueError)) as ei:
                util.support_table_from_bam(bam, "c", 1, 1500, v, decoder=dec, max_depth=cap)
            said.append(str(ei.value))
        assert said[0] == said[1] and "records are not in coordinate order (a read at 10 behind one at 1199)" in said[0], said
    got, st = _native(bam, 1, 1500, v, 0)
    assert len(got[0]) == 701 and st["blocks"] >= 3 and _same(got, _python(bam, 1, 1500, v, 0))


def _record_bytes(read):
    qname, _, _, _, _, cigar, seq = read
    return 4 + 32 + len(qname) + 1 + 4 * len(bamio._parse_cigar(cigar)) + (len(seq) + 1) // 2 + len(seq)


def _block_of_each_record(reads, length):
    """The BGZF block (= batch, with GIO_WINDOW at one block) in which every record of a write_bam file starts."""
    text = "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:c\tLN:%d\n" % length
    at = 4 + 4 + len(text) + 4 + 4 + 2 + 4
    out = []
    for r in reads:
        out.append(at // bamio.BGZF_PAYLOAD)
        at += _record_bytes(r)
    return out


def test_the_longest_span_arrives_in_a_later_batch(tmp_path, monkeypatch):
    """k, the buckets a read in the buffer can lie back, grows with the longest reference span seen so far -- and that can arrive
    batches behind the start of the file, through a read with a ref-skip.

    One such read: a crowd of 300 short reads at 400, batches of sparse short reads, then ONE read 10M1300N10M at 1500 and 200
    reads at 1600.  Only through that read's span does the crowd at 400 lie inside the window sum of the bucket of 1600; with
    max_depth = 450 the check's answer turns on it (asked of the function itself below): the batches set aside are replayed, the
    pass runs and drops nothing.

    A crowd of such reads: 260 of 10M600N10M at 1000, a batch later 200 reads of 100M at 1500 -- inside their skips, so they ARE
    in the buffer, 500 positions back, where a k from the 100M reads alone would not look: 260 + 190 enter, 10 are dropped."""
    monkeypatch.setenv("GIO_WINDOW", WINDOW)
    snps = list(range(5, 3000, 5))
    # -- one read
    reads = _pile("a", 300, 400, 30)
    reads += [("f%d" % i, 0, 0, 440 + (i * 1040) // 700, 60, "30M", s) for i, s in enumerate(_seqs(700, 30))]
    reads += _pile("L", 1, 1500, 20, "10M1300N10M") + _pile("b", 200, 1600, 100)
    blk = _block_of_each_record(reads, 3000)
    assert blk[299] == 0 and blk[1000] >= 1                  # the long read starts in a later block than the crowd lies in
    starts = np.array([r[3] for r in reads])
    H = np.bincount((starts - starts[0]) // 16).astype(np.uint32)
    j = (1600 - 400) // 16
    assert bamio.native_depth_shown(H, 0, j - 1, 100 // 16 + 1, 450)             # everything in front: shown with the short spans
    assert bamio.native_depth_shown(H, j, j, 100 // 16 + 1, 450) and not bamio.native_depth_shown(H, j, j, 1320 // 16 + 1, 450)
    bam, vcf = _write(tmp_path, "one_long", reads, 3000, snps)
    v = util.process_vcf(vcf, "c", 1, 3000)
    n_full = len(_python(bam, 1, 3000, v, 0)[0])
    assert n_full == len(reads)
    # (201: the pile at 400 loses its last 99, at 1600 the last read finds 199 + the long read + the sentinel = 201; 200: one more each)
    for cap, dropped in ((450, 0), (201, 99), (200, 101), (8000, 0)):
        st = _agree(bam, 1, 3000, v, cap, n_full)
        assert st["depth_dropped"] == dropped and st["blocks"] >= 2, (cap, st)
    # -- a crowd of them
    reads = [("s%d" % i, 0, 0, 100 + i, 60, "100M", s) for i, s in enumerate(_seqs(345, 100))]       # the first block
    reads += _pile("L", 260, 1000, 20, "10M600N10M")
    pad = "x" * 200                                            # (long names: these sparse reads fill the rest of the long reads' block)
    reads += [("f%d%s" % (i, pad), 0, 0, 1100 + 2 * i, 60, "30M", s) for i, s in enumerate(_seqs(170, 30))]
    n_front = len(reads)
    reads += _pile("b", 200, 1500, 100)
    blk = _block_of_each_record(reads, 3000)
    assert blk[345] >= 1 and blk[345 + 259] < blk[n_front], (blk[345], blk[345 + 259], blk[n_front])
    bam, vcf = _write(tmp_path, "many_long", reads, 3000, snps)
    n_full = len(_python(bam, 1, 3000, v, 0)[0])
    assert n_full == len(reads)
    for cap, dropped in ((450, 10), (440, 20), (8000, 0)):
        st = _agree(bam, 1, 3000, v, cap, n_full)
        assert st["depth_dropped"] == dropped, (cap, st)
