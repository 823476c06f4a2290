"""One handle through calls whose device scratch needs go up and down -- the beam, the exact decoder, gh_score_paths and
gh_assign_reads each keep a block on the handle that only ever grows (gretel_amd/csrc/scratch_layout.hpp) -- against a fresh
handle per call: a block left over from a larger call, or laid out for another shape, must not show in any result."""
import numpy as np
import pytest

from decode_util import _table
from gretel_amd.hansel import Hansel

pytestmark = pytest.mark.gpu


def _filled(t, L):
    h = Hansel(t.n_snps, band=t.band)
    h.fill_from_support(t.rank, t.off, t.bases, keep_reads=True)
    h.L = L
    return h


def _same(got, ref):
    assert sorted(got) == sorted(ref)
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k
        else:
            assert got[k] == v, k


def test_scratch_blocks_that_grow_and_shrink_leave_no_trace():
    t = _table("a")                                          # 60 SNPs, deletion columns
    h = _filled(t, 3)
    fresh = None

    def step(L, call):
        nonlocal fresh
        h.L = L
        fresh = _filled(t, L)
        got, ref = call(h), call(fresh)
        _same(got, ref)
        return got

    wide = step(3, lambda x: x.beam_paths(32))                                   # 1
    assert wide["n"] == 32 and wide["hole_at"] == 0
    one = step(3, lambda x: x.score_paths(wide["paths"][0], per_position=True))
    assert one["weight"].shape == (1, t.n_snps + 1)
    step(16, lambda x: x.beam_paths(1))                                          # 2: a larger table, fewer back-pointers
    step(16, lambda x: x.assign_reads(wide["paths"], per_read=True))
    narrow = step(1, lambda x: x.beam_paths(8))                                  # 3: everything smaller
    assert narrow["n"] == 8
    # (a slab holds SCORE_SLAB_BYTES / ((N + 1) * 18) = 15279 rows at N = 60: two slabs)
    many = np.tile(wide["paths"], (625, 1))
    assert many.shape == (20000, t.n_snps + 1) and (16 << 20) // ((t.n_snps + 1) * 18) == 15279
    big = step(1, lambda x: x.score_paths(many, per_position=True))
    assert big["pick"].shape == many.shape
    exact = step(5, lambda x: x.viterbi_path())                                  # 4: 3125 states
    assert exact["hole_at"] == 0 and h.viterbi_info()[:3] == (5, 5, 3125)
    step(5, lambda x: x.assign_reads(narrow["paths"][:3]))                       # fewer paths, no per-read arrays
    step(1, lambda x: x.viterbi_path())                                          # 5: five states
    step(1, lambda x: x.score_paths(exact["path"], per_position=True))           # one path behind two slabs
    step(3, lambda x: x.viterbi_path())                                          # 6
    step(3, lambda x: x.assign_reads(wide["paths"][:5], per_read=True))
    assert np.array_equal(h.export_band(), fresh.export_band())
