"""What the max-marginals over a panel show without a GPU: the panel CLI's --margins, the declarations of the two entry points
(gretel_amd/_lib.py against include/gretel_hip.h), the writer that gretel_amd.cmd and gretel_amd.panel share, and the layout of
the call's block of the batch (tests/native/vitm_panel_layout.cpp, under AddressSanitizer + UBSan on the CPU)."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np

from conftest import ROOT
from gretel_amd import _lib, cmd, panel
from gretel_amd.hansel import HanselBatch, HanselPanel, HanselSymbol, margins_of


def test_the_panel_parser_takes_margins():
    p = panel.build_parser()
    assert p.parse_args(["x.bam", "x.vcf", "r.bed"]).margins is False
    a = p.parse_args(["x.bam", "x.vcf", "r.bed", "--margins"])
    assert a.margins is True and a.exact is False
    a = p.parse_args(["x.bam", "x.vcf", "r.bed", "--exact", "--margins"])
    assert a.margins is True and a.exact is True
    # the help text of the single CLI's flag
    both = [next(x for x in q._actions if "--margins" in x.option_strings).help for q in (p, cmd.build_parser())]
    assert both[0] == both[1] and "gretel.margins" in both[0]
    assert "--margins" in panel.__doc__


def _header_args(name):
    """The parameter list of `name` in include/gretel_hip.h, comments removed, as a list of C declarations."""
    text = open(os.path.join(ROOT, "include", "gretel_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % re.escape(name), text, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_lib_declares_the_two_entry_points_as_the_header_does():
    want = {
        "gh_panel_viterbi_marginals": ["gh_batch_t *b", "double *mm", "uint8_t *cm", "const int64_t *pos_off", "int *hole_at"],
        "gh_panel_viterbi_marginals_info": ["gh_batch_t *b", "int64_t out[4]"],
    }
    lib = _lib.load()
    for name, args in want.items():
        assert _header_args(name) == args, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args), name
        assert all(ct is C.c_void_p for ct in fn.argtypes), name
    for cls in (HanselBatch, HanselPanel):
        assert callable(cls.viterbi_marginals) and callable(cls.viterbi_marginals_info)


def _hand_made():
    """Three SNPs over A / C (A / C / G at the second), two haplotypes: mm and cm as Hansel.viterbi_marginals gives them."""
    mm = np.full((4, 7), -np.inf)
    mm[1, :2] = [-1.5, -2.25]
    mm[2, :3] = [-2.0, -1.5, -np.inf]                          # (an offered -inf: cm tells it from "not offered")
    mm[3, :2] = [-1.5, -1.5]                                    # (an exact tie)
    cm = np.array([0, 0b11, 0b111, 0b11], dtype=np.uint8)
    rows = [[6, 0, 1, 0], [6, 1, 0, 1]]
    paths = {"h%d" % k: dict(i_0=k, hansel_path=[HanselSymbol("ACGTN-_"[v], v) for v in row]) for k, row in enumerate(rows)}
    return mm, cm, rows, paths


def test_the_shared_writer_gives_margins_text(tmp_path, capsys):
    mm, cm, rows, paths = _hand_made()
    head = (3, 2, "A", 0, 3, 9)
    vcf_h = dict(N=3, snp_rev=[11, 25, 40])
    ns = types.SimpleNamespace(out=str(tmp_path))
    cmd.write_margins_result(paths, dict(mm=mm, cm=cm, hole_at=0), head, "ACGT-", vcf_h, ns, name="geneA")
    marg = margins_of(mm, cm, np.array(rows, dtype=np.uint8), "ACGT-")
    want = cmd.margins_text(head, [0, 1], marg, mm, cm, vcf_h["snp_rev"])
    text = (tmp_path / "gretel.margins").read_text()
    assert text == want
    assert text.splitlines()[0] == "# 3\t2\tA\t0\t3\t9" and text.count("\nH\t") == 2 and text.count("\nS\t") == 3
    assert capsys.readouterr().err == ""
    # at a hole: cmd's note, behind the region's name where there is one, and no file
    os.remove(tmp_path / "gretel.margins")
    cmd.write_margins_result(paths, dict(mm=None, cm=None, hole_at=2), head, "ACGT-", vcf_h, ns, name="geneA")
    cmd.write_margins_result(paths, dict(mm=None, cm=None, hole_at=2), head, "ACGT-", vcf_h, ns)
    note = "[NOTE] --margins: no candidate at SNP 2, no max-marginals\n"
    assert capsys.readouterr().err == "geneA: " + note + note
    assert os.listdir(tmp_path) == []


def test_the_panel_max_marginals_block_is_what_its_user_spelled_out(tmp_path):
    exe = str(tmp_path / "vitm_panel_layout")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gretel_amd", "csrc"), "-o", exe,
                         os.path.join(ROOT, "tests", "native", "vitm_panel_layout.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert "vitm_panel_layout done" in run.stdout
    # the stand-in of the native check has the descriptor's size: viterbi_marg_panel.hpp asserts the same figure
    src = open(os.path.join(ROOT, "gretel_amd", "csrc", "viterbi_marg_panel.hpp")).read()
    assert "static_assert(sizeof(vitm_win) == 104" in src
