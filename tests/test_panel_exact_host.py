"""What exact decoding over a panel shows without a GPU: the panel CLI's options, the declarations of the three entry points
(gretel_amd/_lib.py against include/gretel_hip.h), and the layout of the panel decoder's block of the batch
(tests/native/vit_panel_layout.cpp, under AddressSanitizer + UBSan on the CPU)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from gretel_amd import _lib, panel


def test_the_panel_parser_takes_exact_and_score_paths():
    p = panel.build_parser()
    a = p.parse_args(["x.bam", "x.vcf", "r.bed"])
    assert a.exact is False and a.score_paths is False
    a = p.parse_args(["x.bam", "x.vcf", "r.bed", "--exact", "--score-paths", "-p", "7"])
    assert a.exact is True and a.score_paths is True and a.paths == 7


@pytest.mark.parametrize("opt", [["--beam", "4"], ["--known", "k.fasta"]], ids=["beam", "known"])
def test_beam_and_known_are_no_options_of_the_panel(opt, capsys):
    with pytest.raises(SystemExit) as e:
        panel.build_parser().parse_args(["x.bam", "x.vcf", "r.bed"] + opt)
    assert e.value.code == 2
    assert "unrecognized arguments" in capsys.readouterr().err
    assert "--beam" in panel.__doc__ and "--known" in panel.__doc__


def _header_args(name):
    """The parameter list of `name` in include/gretel_hip.h, comments removed, as a list of C declarations."""
    text = open(os.path.join(ROOT, "include", "gretel_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % re.escape(name), text, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_lib_declares_the_three_entry_points_as_the_header_does():
    want = {
        "gh_viterbi_states": ["gh_t *h", "int64_t out[3]"],
        "gh_panel_viterbi_spin": ["gh_batch_t *b", "int max_paths", "double min_remove", "uint8_t *paths_out", "const int64_t *paths_off",
                                  "gh_path_rec *recs", "double *ll_chain", "int *n_out", "int *hole_at"],
        "gh_panel_viterbi_info": ["gh_batch_t *b", "int64_t out[4]"],
    }
    lib = _lib.load()
    for name, args in want.items():
        assert _header_args(name) == args, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args), name
        for decl, ct in zip(args, fn.argtypes):
            if "*" in decl or "[" in decl:
                assert ct is C.c_void_p, (name, decl)
            elif decl.startswith("double"):
                assert ct is C.c_double, (name, decl)
            else:
                assert ct is C.c_int, (name, decl)


def test_the_panel_decoders_block_is_what_its_user_spelled_out(tmp_path):
    exe = str(tmp_path / "vit_panel_layout")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gretel_amd", "csrc"), "-o", exe,
                         os.path.join(ROOT, "tests", "native", "vit_panel_layout.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert "vit_panel_layout done" in run.stdout
    # the stand-in of the native check has the descriptor's size: viterbi_panel.hpp asserts the same figure
    src = open(os.path.join(ROOT, "gretel_amd", "csrc", "viterbi_panel.hpp")).read()
    assert "static_assert(sizeof(vit_win) == 104" in src
