#!/usr/bin/env python3
"""The compiler's output for the 58 candidate-pool walkers of a source tree, and two trees compared.

  cwalk_isa.py build <tree> <outdir> [jobs]   <tree> holds include/ and gretel_amd/csrc/; one .s per walker into <outdir>
  cwalk_isa.py compare <parent dir> <new dir>   instruction streams (comments and label numbers aside) and resource usage

`compare` exits 1 when a walker is missing or one of its resource figures exceeds the parent's (LDS: differs).
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Wno-unused-value -Wno-int-to-pointer-cast".split()
WALKERS = ([("k_cwalk", n, 4) for n in range(6, 33)] + [("k_cwalk", n, 5) for n in range(6, 22)] +
           [("k_cwalk2", n, 5) for n in range(24, 41, 4)] + [("k_cwalk2", n, 4) for n in range(36, 65, 4)] +
           [("k_cwalkg", None, 4), ("k_cwalkg", None, 5)])
NO_MORE = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size")
SAME = (".group_segment_fixed_size",)


def tag(w):
    return "%s_%s_%d" % (w[0], w[1], w[2]) if w[1] is not None else "%s_%d" % (w[0], w[2])


def inst(w):
    return "%s<%d, %d>" % w if w[1] is not None else "%s<%d>" % (w[0], w[2])


def build(tree, out, jobs):
    os.makedirs(out, exist_ok=True)

    def one(w):
        cmd = ["hipcc"] + FLAGS + ["-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, "gretel_amd", "csrc"),
                                    "--cuda-device-only", "-S", "-DCW_ONLY=" + inst(w), "-o", os.path.join(out, tag(w) + ".s"),
                                    os.path.join(HERE, "cwalk_only.hip")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            sys.stderr.write("%s: %s\n" % (inst(w), r.stderr[-2000:]))
        return r.returncode

    # the largest first: k_cwalk2<64, 4> alone takes minutes
    order = sorted(WALKERS, key=lambda w: -(w[1] or 0) * (2 if w[0] == "k_cwalk2" else 1))
    with ThreadPoolExecutor(jobs) as ex:
        return 1 if any(list(ex.map(one, order))) else 0


def walker_of(path, w):
    """(symbol, normalised instruction stream, resource figures) of the walker in one .s file"""
    text = open(path).read()
    pat = re.compile(r"^(_Z\d+%sIL\S*):" % w[0], re.M)      # (the file's only instantiation)
    m = pat.search(text)
    if not m:
        return None
    sym = m.group(1)
    body = text[m.end():text.index(".Lfunc_end", m.end())]
    lines = []
    for ln in body.split("\n"):
        ln = ln.split(";")[0].strip()
        if not ln or ln.startswith(".p2align") or ln.startswith("//"):
            continue
        lines.append(re.sub(r"\.L(BB|tmp|func_end)\d+_?", r".L\1_", ln))
    meta = {}
    for ent in text.split("\n  - .agpr_count:")[1:]:
        ent = "\n    .agpr_count:" + ent
        if re.search(r"\.name:\s+%s\s" % re.escape(sym), ent):
            for k in NO_MORE + SAME:
                meta[k] = int(re.search(r"%s:\s+(\d+)" % re.escape(k), ent).group(1))
    return sym, lines, meta


def compare(a, b):
    bad = same = 0
    for w in WALKERS:
        ra, rb = walker_of(os.path.join(a, tag(w) + ".s"), w), walker_of(os.path.join(b, tag(w) + ".s"), w)
        if ra is None or rb is None or ra[0] != rb[0]:
            print("%-18s MISSING or another symbol" % inst(w))
            bad += 1
            continue
        ident = ra[1] == rb[1]
        same += ident
        worse = [k for k in NO_MORE if rb[2][k] > ra[2][k]] + [k for k in SAME if rb[2][k] != ra[2][k]]
        diff = ["%s %d -> %d" % (k, ra[2][k], rb[2][k]) for k in NO_MORE + SAME if ra[2][k] != rb[2][k]]
        print("%-18s %s  %5d -> %5d lines  vgpr %3d agpr %3d sgpr %3d scratch %3d lds %6d  %s%s" % (
            inst(w), "identical" if ident else "DIFFERS  ", len(ra[1]), len(rb[1]), rb[2][".vgpr_count"], rb[2][".agpr_count"],
            rb[2][".sgpr_count"], rb[2][".private_segment_fixed_size"], rb[2][".group_segment_fixed_size"], "; ".join(diff),
            "   <-- EXCEEDS" if worse else ""))
        bad += bool(worse)
    print("%d of %d instruction streams identical; %d walkers exceed the parent's resources" % (same, len(WALKERS), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "build":
        sys.exit(build(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 8))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
