#!/usr/bin/env python3
"""Is the device code of two trees the same?  For a change that touches only the host side of gretel_hip.hip.

  device_isa_cmp.py build <tree> <out.s>      gretel_hip.hip of <tree> with the Makefile's flags + --cuda-device-only -S
  device_isa_cmp.py compare <parent.s> <new.s>

`compare`: the sets of kernel symbols, every kernel's instruction stream (comments and label numbers aside, as cwalk_isa.py's
walker_of) and its register, spill, scratch and LDS figures; the order of the symbols may differ.  Exits 1 on any difference.
"""
import os
import re
import subprocess
import sys

FLAGS = ("--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -pthread -Wall -Wno-unused-result -Wno-unused-value "
         "-Wno-int-to-pointer-cast").split()
FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
           ".group_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size")


def build(tree, out):
    src = os.path.join(tree, "gretel_amd", "csrc")
    return subprocess.call(["hipcc"] + FLAGS + ["-I" + os.path.join(tree, "include"), "--cuda-device-only", "-S", "-o", out,
                                                 os.path.join(src, "gretel_hip.hip")])


def kernels(path):
    """{symbol: (normalised instruction stream, resource figures)} of every kernel of one .s file"""
    text = open(path).read()
    meta = {}
    for ent in text.split("\n  - .agpr_count:")[1:]:
        ent = "\n    .agpr_count:" + ent
        name = re.search(r"\.name:\s+(\S+)", ent).group(1)
        meta[name] = tuple(int(re.search(r"%s:\s+(\d+)" % re.escape(k), ent).group(1)) for k in FIGURES)
    out = {}
    for sym in meta:
        m = re.search(r"^%s:" % re.escape(sym), text, re.M)
        body = text[m.end():text.index(".Lfunc_end", m.end())]
        lines = []
        for ln in body.split("\n"):
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith(".p2align") or ln.startswith("//"):
                continue
            lines.append(re.sub(r"\.L(BB|tmp|func_end)\d+_?", r".L\1_", ln))
        out[sym] = (lines, meta[sym])
    return out


def compare(a, b):
    ka, kb = kernels(a), kernels(b)
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    for s in only_a:
        print("only in the parent: %s" % s)
    for s in only_b:
        print("only in the new tree: %s" % s)
    both = sorted(set(ka) & set(kb))
    isa = [s for s in both if ka[s][0] != kb[s][0]]
    res = [s for s in both if ka[s][1] != kb[s][1]]
    for s in isa:
        print("instruction stream differs: %s (%d -> %d lines)" % (s, len(ka[s][0]), len(kb[s][0])))
    for s in res:
        print("resources differ: %s %s" % (s, "; ".join("%s %d -> %d" % (k, x, y) for k, x, y in zip(FIGURES, ka[s][1], kb[s][1]) if x != y)))
    print("%d kernels in the parent, %d in the new tree; %d of %d common instruction streams identical (%d instructions), "
          "%d with identical register / spill / scratch / LDS figures" % (len(ka), len(kb), len(both) - len(isa), len(both),
                                                                          sum(len(ka[s][0]) for s in both), len(both) - len(res)))
    return 1 if (only_a or only_b or isa or res) else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "build":
        sys.exit(build(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
