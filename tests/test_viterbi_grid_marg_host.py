"""The host side of the max-marginals on the grid (gh_viterbi_marginals_grid; Hansel.viterbi_marginals_grid_bytes,
grid_marginals_scratch_bytes, --margins-grid of gretel_amd.cmd): the argument parser, which call the flag makes and the note it
writes first, the arithmetic of the scratch size, and vitgm_layout (gretel_amd/csrc/scratch_layout.hpp, the function the library
itself calls) against sizes written out by hand under AddressSanitizer + UBSan on the CPU."""
import os
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT
from gretel_amd import _lib, cmd
from gretel_amd.hansel import Hansel, grid_marginals_scratch_bytes


def test_margins_grid_parses_alone_and_beside_the_other_flags(tmp_path):
    argv = [str(tmp_path / "no_such.bam"), str(tmp_path / "no_such.vcf.gz"), "hoot", "-s", "1", "-e", "20", "-o", str(tmp_path / "out")]
    a = cmd.build_parser().parse_args(argv)
    assert a.margins_grid is False and a.margins is False
    for extra in ([], ["--exact"], ["--exact-grid"], ["--beam", "4"], ["--margins"], ["--kbest", "3"]):
        a = cmd.build_parser().parse_args(argv + ["--margins-grid"] + extra)
        assert a.margins_grid is True and a.margins is ("--margins" in extra)
        assert all(check(a) is None for check in (cmd.check_beam_options, cmd.check_exact_options, cmd.check_kbest_options, cmd.check_masked_options))
    # gretel_amd.panel does not get the flag
    from gretel_amd import panel
    assert panel.build_parser().parse_args(["bam", "vcf", "bed", "--margins"]).margins is True
    with pytest.raises(SystemExit):
        panel.build_parser().parse_args(["bam", "vcf", "bed", "--margins-grid"])


class Stub:
    """A handle that records which max-marginals call is made."""
    _cfg = dict(cand_order="ACGT-", cond_mode="A", marginal_term=False)

    def __init__(self, shape=(4, 10, 4 ** 10), refuse=None):
        self.calls, self.shape, self.refuse = [], shape, refuse
        self.n = self.N = 3
        self.L = shape[1]

    def viterbi_states(self):
        return self.shape

    def viterbi_marginals_grid_bytes(self):
        return 0 if self.shape[2] > cmd.GRID_MAX_STATES else 123

    def _res(self):
        mm = np.full((4, 7), -np.inf)
        mm[1:, 0] = -1.0
        mm[1:, 1] = -2.0
        return dict(mm=mm, cm=np.array([0, 3, 3, 3], dtype=np.uint8), hole_at=0)

    def viterbi_marginals_grid(self):
        self.calls.append("grid")
        if self.refuse:
            raise _lib.GretelHipError(_lib.GH_ERR_ARG, self.refuse)
        return self._res()

    def viterbi_marginals(self):
        self.calls.append("lds")
        return self._res()

    def viterbi_grid_info(self):
        return self.shape + (123,)

    def viterbi_info(self):
        return self.shape + (77,)


NOTE = "[NOTE] --margins-grid: S = 4 candidate symbols, Le = 10: 1048576 states, 123 bytes of device scratch\n"


def test_margins_grid_makes_the_grid_call_behind_its_note(capsys):
    h = Stub()
    res, info = cmd.marginals_once(h, grid=True)
    assert h.calls == ["grid"] and info == (4, 4 ** 10) and res["hole_at"] == 0
    assert capsys.readouterr().err == NOTE
    # without it the call, and the silence, are those of --margins
    res, info = cmd.marginals_once(h)
    assert h.calls == ["grid", "lds"] and info == (4, 4 ** 10)
    assert capsys.readouterr().err == ""


def test_write_margins_follows_the_flag(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(cmd, "_score_head", lambda h, v: (3, h.L, "A", 0))
    vcf_h = dict(N=3, snp_rev=[11, 12, 13])
    for ns, want in ((types.SimpleNamespace(), ["lds"]), (types.SimpleNamespace(margins_grid=False), ["lds"]),
                     (types.SimpleNamespace(margins_grid=True), ["grid"]), (types.SimpleNamespace(margins_grid=True, margins=True), ["grid"])):
        out = tmp_path / ("o%d" % len(os.listdir(tmp_path)))
        out.mkdir()
        ns.out = str(out)
        h = Stub()
        cmd.write_margins({}, h, vcf_h, ns)
        assert h.calls == want                               # one call, whichever it is
        assert capsys.readouterr().err == (NOTE if want == ["grid"] else "")
        text = (out / "gretel.margins").read_text()
        assert text.startswith("# 3\t10\tA\t0\t4\t1048576\n") and text.count("\nS\t") == 3
    # beyond the grid's cap: the library's message as a note, no sizes, no file
    out = tmp_path / "beyond"
    out.mkdir()
    h = Stub(shape=(2, 25, 1 << 25), refuse="gh_viterbi_marginals_grid: S = 2 candidate symbols ... 33554432 states, more than the 16777216")
    cmd.write_margins({}, h, vcf_h, types.SimpleNamespace(out=str(out), margins_grid=True))
    err = capsys.readouterr().err
    assert h.calls == ["grid"] and err.startswith("[NOTE] --margins-grid: ") and err.count("[NOTE]") == 1
    assert "gh_viterbi_marginals_grid: S = 2 " in err and "33554432 states" in err and err.count("\n") == 1
    assert os.listdir(out) == []


def test_the_scratch_bytes_are_the_layouts_sum():
    class Shape:
        def __init__(self, n, shape):
            self.n, self.shape = n, shape

        def viterbi_states(self):
            return self.shape

    def up(x):
        return (x + 255) // 256 * 256

    # 60 SNPs at the fill's own L = 10, without and with deletion columns: by hand, part by part
    #   out, cm5, cm0 | table | F and the +0.0 | B | partials: 5 doubles per SNP and 512 states | mm | cm
    assert grid_marginals_scratch_bytes(60, 10, 1048576) == 768 + 146944 + 503316736 + 16777216 + 4915200 + 3584 + 256 == 525160704
    assert grid_marginals_scratch_bytes(60, 10, 9765625) == 768 + 146944 + 4687500032 + 156250112 + 45777664 + 3584 + 256 == 4889679360
    for states in (1048576, 9765625):
        wgs = -(-states // 512)
        want = 256 + 256 + 256 + up(60 * 306 * 8) + up((60 * states + 1) * 8) + up(16 * states) + up(60 * wgs * 40) + up(61 * 56) + 256
        assert grid_marginals_scratch_bytes(60, 10, states) == want
        assert Hansel.viterbi_marginals_grid_bytes(Shape(60, (0, 10, states))) == want
    # the order of magnitude the header names: 0.5 and 4.7 GB at 60 SNPs (8.1 bytes per SNP and state: F, and a hundredth for the partials)
    assert 0.52e9 < grid_marginals_scratch_bytes(60, 10, 1048576) < 0.53e9 and 4.8e9 < grid_marginals_scratch_bytes(60, 10, 9765625) < 4.9e9
    assert grid_marginals_scratch_bytes(300, 10, 1048576) == 2558689024 and grid_marginals_scratch_bytes(300, 10, 9765625) == 23823391488
    # the cap is served, one state more is not; a window that offers nothing keeps the first reservation
    assert grid_marginals_scratch_bytes(30, 24, 1 << 24) == 768 + up(30 * 726 * 8) + (30 * (1 << 27) + 256) + (1 << 28) + 30 * 32768 * 40 + 1792 + 256
    assert grid_marginals_scratch_bytes(30, 24, (1 << 24) + 1) == 0
    assert Hansel.viterbi_marginals_grid_bytes(Shape(30, (2, 25, 1 << 25))) == 0
    assert Hansel.viterbi_marginals_grid_bytes(Shape(30, (5, 30, 2 ** 63 - 1))) == 0
    assert grid_marginals_scratch_bytes(300, 10, 0) == 256 + 2 * 512
    assert Hansel.viterbi_marginals_grid_bytes(Shape(300, (0, 10, 0))) == 256 + 2 * 512
    # one state (a window of one symbol): a row of F is one double
    assert grid_marginals_scratch_bytes(34, 30, 1) == 768 + up(34 * 906 * 8) + up(35 * 8) + 256 + up(34 * 40) + up(35 * 56) + 256
    # 10 000 SNPs at the cap: Python's integers, the library's size_t
    assert grid_marginals_scratch_bytes(10000, 12, 1 << 24) == (256 + 2 * 10240 + 29280000 + 1342177280256 + 268435456 + 13107200000 + 560128
                                                                + 10240) == 1355582786816


def test_the_scratch_layout_is_what_the_kernels_spell_out(tmp_path):
    # tests/native/vitgm_layout.cpp, a stand-alone program: nothing is loaded into Python
    exe = str(tmp_path / "vitgm_layout")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gretel_amd", "csrc"), "-o", exe,
                         os.path.join(ROOT, "tests", "native", "vitgm_layout.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert "vitgm_layout done" in run.stdout
