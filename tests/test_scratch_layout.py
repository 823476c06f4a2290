"""The device scratch layouts of gh_assign_reads, gh_score_paths, the beam and the exact decoder (gretel_amd/csrc/
scratch_layout.hpp: host-only, the functions the library itself calls) against their sizes and orders written out by hand, under
AddressSanitizer + UBSan on the CPU: tests/native/scratch_layout.cpp."""
import os
import subprocess

from conftest import ROOT


def test_the_four_scratch_layouts_are_what_their_users_spelled_out(tmp_path):
    exe = str(tmp_path / "scratch_layout")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gretel_amd", "csrc"), "-o", exe,
                         os.path.join(ROOT, "tests", "native", "scratch_layout.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert "scratch_layout done" in run.stdout
