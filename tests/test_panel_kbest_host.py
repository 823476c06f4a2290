"""What k-best decoding over a panel shows without a GPU: the panel CLI's --kbest, the declarations of the two entry points
(gretel_amd/_lib.py against include/gretel_hip.h), the writer that gretel_amd.cmd and gretel_amd.panel share, the arithmetic of
Hansel.viterbi_kbest_max, and the layout of the call's block of the batch (tests/native/vitk_panel_layout.cpp, under
AddressSanitizer + UBSan on the CPU)."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT
from gretel_amd import _lib, cmd, panel
from gretel_amd.hansel import Hansel, HanselBatch, HanselPanel, HanselSymbol, kbest_of


def test_the_panel_parser_takes_kbest(tmp_path, capsys):
    p = panel.build_parser()
    assert p.parse_args(["x.bam", "x.vcf", "r.bed"]).kbest is None
    a = p.parse_args(["x.bam", "x.vcf", "r.bed", "--kbest", "8"])
    assert a.kbest == 8 and a.exact is False and a.margins is False
    a = p.parse_args(["x.bam", "x.vcf", "r.bed", "--exact", "--margins", "--kbest", "32"])
    assert a.kbest == 32 and a.exact is True and a.margins is True
    # the help text of the single CLI's flag
    both = [next(x for x in q._actions if "--kbest" in x.option_strings).help for q in (p, cmd.build_parser())]
    assert both[0] == both[1] and "gretel.kbest" in both[0]
    assert "--kbest" in panel.__doc__
    # 0 and 33 are refused with cmd's message before any file but the BED is opened: the BAM and the VCF do not exist
    bed = tmp_path / "r.bed"
    bed.write_text("hoot\t0\t20\tr1\n")
    for k in (0, 33):
        ns = types.SimpleNamespace(kbest=k)
        assert panel.main([str(tmp_path / "no.bam"), str(tmp_path / "no.vcf"), str(bed), "-o", str(tmp_path / "out"), "--kbest", str(k)]) == 2
        assert capsys.readouterr().err == "[FAIL] %s\n" % cmd.check_kbest_options(ns)
        assert "--kbest must be 1..32" == cmd.check_kbest_options(ns)
    assert not (tmp_path / "out").exists()


def _header_args(name):
    """The parameter list of `name` in include/gretel_hip.h, comments removed, as a list of C declarations."""
    text = open(os.path.join(ROOT, "include", "gretel_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % re.escape(name), text, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_lib_declares_the_two_entry_points_as_the_header_does():
    want = {
        "gh_panel_viterbi_kbest": ["gh_batch_t *b", "const int *k", "uint8_t *paths_out", "const int64_t *paths_off", "double *ll_chain",
                                   "const int64_t *ll_off", "int *n_out", "int *hole_at"],
        "gh_panel_viterbi_kbest_info": ["gh_batch_t *b", "int64_t out[4]"],
    }
    lib = _lib.load()
    for name, args in want.items():
        assert _header_args(name) == args, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args), name
        assert all(ct is C.c_void_p for ct in fn.argtypes), name
    for cls in (HanselBatch, HanselPanel):
        assert callable(cls.viterbi_kbest) and callable(cls.viterbi_kbest_info)


def _hand_made():
    """Three SNPs, three ranked haplotypes (the last two tie), two recovered ones: a dict as Hansel.viterbi_kbest gives it."""
    res = dict(n=3, hole_at=0, paths=np.array([[6, 0, 1, 0], [6, 1, 0, 1], [6, 1, 1, 1]], dtype=np.uint8),
               ll_chain=np.array([-1.5, -2.25, -2.25]))
    rows = [[6, 1, 0, 1], [6, 0, 1, 0]]
    paths = {"h%d" % k: dict(i_0=k, hansel_path=[HanselSymbol("ACGTN-_"[v], v) for v in row]) for k, row in enumerate(rows)}
    return res, rows, paths


def test_the_shared_writer_gives_kbest_text(tmp_path, capsys):
    res, rows, paths = _hand_made()
    head = (3, 2, "A", 0, 2, 4, 8)
    vcf_h = dict(N=3, snp_rev=[11, 25, 40])
    ns = types.SimpleNamespace(out=str(tmp_path))
    cmd.write_kbest_result(paths, res, head, vcf_h, ns, name="geneA")
    want = cmd.kbest_text(head + (3,), res, kbest_of(res, np.array(rows, dtype=np.uint8)), [0, 1])
    text = (tmp_path / "gretel.kbest").read_text()
    assert text == want
    lines = text.splitlines()
    assert lines[0] == "# 3\t2\tA\t0\t2\t4\t8\t3" and len(lines) == 4
    # rank 0 is the second recovered haplotype, rank 1 the first; rank 2 is one SNP from the first
    assert [ln.split("\t")[4:] for ln in lines[1:]] == [["1", "0", "ACA"], ["0", "0", "CAC"], ["0", "1", "CCC"]]
    assert capsys.readouterr().err == ""
    # at a hole: cmd's note, behind the region's name where there is one, and no file
    os.remove(tmp_path / "gretel.kbest")
    hole = dict(n=0, hole_at=2, paths=np.zeros((0, 4), dtype=np.uint8), ll_chain=np.zeros(0))
    cmd.write_kbest_result(paths, hole, head, vcf_h, ns, name="geneA")
    cmd.write_kbest_result(paths, hole, head, vcf_h, ns)
    note = "[NOTE] --kbest: no candidate at SNP 2, no k-best haplotypes\n"
    assert capsys.readouterr().err == "geneA: " + note + note
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("states,want", [(1, 32), (2, 32), (125, 32), (128, 32), (129, 31), (1024, 4), (1025, 3), (2048, 2), (2049, 1),
                                         (3125, 1), (4096, 1), (4097, 0), (16384, 0), (2 ** 63 - 1, 0), (0, 0)])
def test_viterbi_kbest_max_is_host_arithmetic(states, want):
    h = Hansel.__new__(Hansel)                                  # (no handle: the one call it makes is stood in for)
    h.viterbi_states = lambda: (4, 5, states)
    assert h.viterbi_kbest_max() == want
    assert want == (min(_lib.GH_KBEST_MAX, _lib.GH_VITERBI_MAX_STATES // states) if 1 <= states <= _lib.GH_VITERBI_MAX_STATES else 0)


def test_the_panel_kbest_block_is_what_its_user_spelled_out(tmp_path):
    exe = str(tmp_path / "vitk_panel_layout")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gretel_amd", "csrc"), "-o", exe,
                         os.path.join(ROOT, "tests", "native", "vitk_panel_layout.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert "vitk_panel_layout done" in run.stdout
    # the stand-in of the native check has the descriptor's size: viterbi_kbest_panel.hpp asserts the same figure
    src = open(os.path.join(ROOT, "gretel_amd", "csrc", "viterbi_kbest_panel.hpp")).read()
    assert "static_assert(sizeof(vitk_win) == 128" in src
    assert "#define WIN_BYTES 128" in open(os.path.join(ROOT, "tests", "native", "vitk_panel_layout.cpp")).read()
