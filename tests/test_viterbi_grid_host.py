"""The host side of the grid decoder (gh_viterbi_path_grid; Hansel.viterbi_grid_bytes, --exact-grid of gretel_amd.cmd): the
argument parser and its refusals, the arithmetic of the scratch size, and vitg_layout (gretel_amd/csrc/scratch_layout.hpp, the
function the library itself calls) against sizes written out by hand under AddressSanitizer + UBSan on the CPU."""
import io
import os
import subprocess

from conftest import ROOT
from gretel_amd import _lib, cmd
from gretel_amd.hansel import Hansel, grid_scratch_bytes


def test_exact_grid_parses_and_is_refused_as_exact_is(tmp_path, capsys):
    out = tmp_path / "out"
    argv = [str(tmp_path / "no_such.bam"), str(tmp_path / "no_such.vcf.gz"), "hoot", "-s", "1", "-e", "20", "-o", str(out)]
    a = cmd.build_parser().parse_args(argv)
    assert a.exact_grid is False and cmd.check_exact_options(a) is None
    for extra in (["--exact-grid", "--beam", "4"], ["--exact-grid", "--debughpos", "3,7"], ["--exact", "--exact-grid", "--beam", "2"]):
        assert cmd.main(argv + extra) == 2
        assert capsys.readouterr().err.startswith("[FAIL] --exact ")
    assert not out.exists()
    for extra in (["--exact-grid"], ["--exact", "--exact-grid"], ["--exact-grid", "--debughpos", ","], ["--exact-grid", "--score-paths"],
                  ["--exact-grid", "--margins", "--kbest", "3"]):
        a = cmd.build_parser().parse_args(argv + extra)
        assert a.exact_grid is True and cmd.check_exact_options(a) is None
    assert cmd.GRID_MAX_STATES == _lib.GH_VITERBI_GRID_MAX_STATES == 16777216


def test_exact_with_exact_grid_means_the_grid():
    calls = []

    class Stub:
        def viterbi_states(self):
            return (4, 10, 4 ** 10)

        def viterbi_grid_bytes(self):
            return 123

        def viterbi_spin_grid(self, max_paths, min_remove):
            calls.append(("grid", max_paths, min_remove))
            return dict(n=0, hole_at=0)

        def viterbi_spin(self, max_paths, min_remove):
            calls.append(("lds", max_paths, min_remove))
            return dict(n=0, hole_at=0)

    log = io.StringIO()
    assert cmd.recover(Stub(), 60, 7, log=log, exact=True, grid=True) == {}
    assert cmd.recover(Stub(), 60, 7, log=log, grid=True) == {}
    assert calls == [("grid", 7, cmd.MIN_REMOVE)] * 2
    assert log.getvalue().count("[NOTE] --exact-grid: S = 4 candidate symbols, Le = 10: 1048576 states, 123 bytes of device scratch\n") == 2
    assert cmd.recover(Stub(), 60, 7, log=log, exact=True) == {} and calls[-1][0] == "lds"


def test_the_scratch_bytes_are_the_layouts_sum():
    class Stub:
        def __init__(self, n, shape):
            self.n, self.shape = n, shape

        def viterbi_states(self):
            return self.shape

    def up(x):
        return (x + 255) // 256 * 256

    # 60 SNPs at the fill's own L = 10, without and with deletion columns: by hand, part by part
    for s, states in ((4, 1048576), (5, 9765625)):
        parts = -(-states // 4096)
        want = 256 + 256 + 256 + up(60 * 306 * 8) + up(61 * states) + up(16 * states) + up(8 * parts) + up(4 * parts) + 256
        assert Hansel.viterbi_grid_bytes(Stub(60, (s, 10, states))) == want
    assert 0.08e9 < Hansel.viterbi_grid_bytes(Stub(60, (4, 10, 1048576))) < 0.09e9
    assert 0.75e9 < Hansel.viterbi_grid_bytes(Stub(60, (5, 10, 9765625))) < 0.76e9
    # the cap is served, one state more is not; a window that offers nothing keeps the first reservation
    assert Hansel.viterbi_grid_bytes(Stub(30, (2, 24, 1 << 24))) == 256 + 2 * 256 + up(30 * 726 * 8) + 31 * (1 << 24) + (1 << 28) + 32768 + 16384 + 256
    assert Hansel.viterbi_grid_bytes(Stub(30, (2, 25, 1 << 25))) == 0
    assert Hansel.viterbi_grid_bytes(Stub(30, (5, 30, 2 ** 63 - 1))) == 0
    assert Hansel.viterbi_grid_bytes(Stub(300, (0, 10, 0))) == 256 + 2 * 512
    # 10 000 SNPs at the cap: Python's integers, the library's size_t
    assert grid_scratch_bytes(10000, 12, 1 << 24) == 256 + 2 * 10240 + 29280000 + 167788937216 + 268435456 + 32768 + 16384 + 10240


def test_the_scratch_layout_is_what_the_kernels_spell_out(tmp_path):
    # tests/native/vitg_layout.cpp, a stand-alone program: nothing is loaded into Python
    exe = str(tmp_path / "vitg_layout")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gretel_amd", "csrc"), "-o", exe,
                         os.path.join(ROOT, "tests", "native", "vitg_layout.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert "vitg_layout done" in run.stdout
