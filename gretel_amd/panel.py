"""
`python -m gretel_amd.panel BAM VCF REGIONS -o OUT`: gretel over many regions (genes) of one BAM and VCF in one run.

REGIONS is a BED file (contig, 0-based start, end, optional name: gretel_amd.util.read_regions).  The VCF is read once
(util.process_vcf_regions), every region's Hansel is filled from the BAM in turn, and all of them are recovered together as one
panel (hansel.HanselPanel: the window pipeline over the regions' differing shapes).  For each region the files

    OUT/<name>/out.fasta, OUT/<name>/snp.fasta, OUT/<name>/gretel.crumbs

are byte for byte what `python -m gretel_amd.cmd BAM VCF contig -s start -e end -o OUT/<name>` writes with the same options
(with --assign-reads also OUT/<name>/gretel.support, one assignment call per region).
--exact recovers every path as the global maximum of the chain likelihood, all regions decoded together as one panel
(HanselPanel.viterbi_spin: the decoders of a round side by side); a region whose states exceed the decoder's cap gets the
library's message behind its name, is left out and counts as failed.  --score-paths writes OUT/<name>/gretel.scores, every
recovered haplotype scored against a copy of the region's matrix taken before the spins (a host loop over the regions).
--margins writes OUT/<name>/gretel.margins, the max-marginals of the region's matrix before the spins, all regions' walks side
by side (HanselPanel.viterbi_marginals); without --exact a region beyond the decoder's cap gets the library's message as a
[NOTE] behind its name and no such file, its other files are written and the exit status is unaffected.
--kbest K writes OUT/<name>/gretel.kbest, the K exactly best haplotypes of the region's matrix before the spins set beside the
recovered ones, all regions' walks side by side in one call made before the spins (HanselPanel.viterbi_kbest), with the greedy
spin or --exact, with or without --margins; a region the library would refuse (too many states, or K lists of them more slots
than the decoder holds) gets the library's message as a [NOTE] behind its name and no such file, a region that met a hole gets
the single CLI's note behind its name; the other files are written and the exit status is unaffected.
--beam and --known are the single CLI's alone: a panel offers neither.
A region gretel cannot recover (a SNP without pairwise evidence, or no read that carries two SNPs) gets gretel's [FAIL] text on
stderr behind its name and is left out; the exit status is then 1, once every other region has been written.  Stdout: one line
per recovered region -- name, SNPs, L, paths, distinct haplotypes.  The single-region debugging options (--debughpos,
--debugreads, --debugpos, --dumpmatrix) are the single CLI's alone.
"""
from __future__ import annotations

import argparse
import io
import os
import sys

from . import __version__
from . import cmd
from . import util
from ._lib import GretelHipError
from .hansel import HanselPanel


def build_parser():
    p = argparse.ArgumentParser(prog="gretel-panel", description="Gretel over many regions of one BAM / VCF, recovered as one panel.")
    p.add_argument("bam")
    p.add_argument("vcf")
    p.add_argument("regions", help="BED file: contig, 0-based start, end, optional name (one region per line)")
    p.add_argument("-o", "--out", default=".", help="output directory: one subdirectory per region name [default: .]")
    p.add_argument("-p", "--paths", type=int, default=100, help="maximum number of paths to generate per region [default: 100]")
    p.add_argument("--master", default=None, help="master FASTA used to fill the non-SNP positions (otherwise --gapchar)")
    p.add_argument("--gapchar", default="N", help="character for non-SNP positions without --master [default: N]")
    p.add_argument("--delchar", default="", help="character written for a deletion [default: nothing]")
    p.add_argument("--max-depth", type=int, default=8000, help="read-buffer cap of the pileup, as in gretel_amd.cmd [default: 8000]")
    p.add_argument("--pepper", action="store_true", help="permissive read filter (pysam stepper 'all' in the reference)")
    cmd.add_assign_options(p)
    p.add_argument("--score-paths", action="store_true", help="score every recovered haplotype against the region's unreweighted "
                   "matrix (chain likelihood, per-SNP margins) and write gretel.scores per region")
    p.add_argument("--exact", action="store_true", help="recover every path as the global maximum of the chain likelihood (exact "
                   "decoding over S^min(L, N) states, at most %d), the regions' decoders side by side, instead of the greedy walk"
                   % cmd.EXACT_MAX_STATES)
    p.add_argument("--margins", action="store_true", help=cmd.MARGINS_HELP)
    p.add_argument("--kbest", type=int, default=None, metavar="K", help=cmd.KBEST_HELP)
    p.add_argument("--version", action="version", version="%(prog)s " + __version__)
    return p


def _fail(name, text):
    sys.stderr.write("%s: %s" % (name, text))


def main(argv=None):
    args = build_parser().parse_args(argv)
    # everything that can be refused is refused before the first BAM read or GPU call
    try:
        regions = util.read_regions(args.regions)
    except (OSError, ValueError) as e:
        sys.stderr.write("[FAIL] %s\n" % e)
        return 2
    if not regions:
        sys.stderr.write("[FAIL] %s holds no region\n" % args.regions)
        return 2
    if args.paths < 1:
        sys.stderr.write("[FAIL] -p/--paths must be at least 1\n")
        return 2
    bad = cmd.check_assign_options(args) or cmd.check_kbest_options(args)
    if bad:
        sys.stderr.write("[FAIL] %s\n" % bad)
        return 2
    util.prefetch_bam(args.bam, regions[0]["contig"], regions[0]["start"], regions[0]["end"])
    vcfs = util.process_vcf_regions(args.vcf, regions)
    stepper = "all" if args.pepper else "samtools"
    kept = []                   # (region, vcf_h, hansel, the copy --score-paths scores against or None)
    served = []                 # --margins: indices into kept of the regions the max-marginals serve
    ranked = []                 # --kbest: likewise for the k-best decoding
    failed = 0
    for k, (r, vh) in enumerate(zip(regions, vcfs)):
        hansel = None
        if vh["N"] > 0:
            try:
                hansel = util.load_from_bam(args.bam, r["contig"], r["start"], r["end"], vh, max_depth=args.max_depth, stepper=stepper,
                                             keep_reads=args.assign_reads)
            except ZeroDivisionError:           # no read carries two SNPs (gretel/util.py:333)
                hansel = None
        if k + 1 < len(regions):                # (the decoder reads the next region while this one is checked)
            nx = regions[k + 1]
            util.prefetch_bam(args.bam, nx["contig"], nx["start"], nx["end"])
        if hansel is None:
            pos = vh["snp_rev"][0] if vh["N"] > 0 else 0
            _fail(r["name"], cmd.FAIL_TEXT % (1 if vh["N"] > 0 else 0, pos, 1 if vh["N"] > 0 else 0))
            failed += 1
            continue
        hansel.snapshot_original()              # (as gretel_amd.cmd: cmd.py:79)
        buf = io.StringIO()
        if cmd.gap_report(hansel, vh, out=buf):
            _fail(r["name"], buf.getvalue())
            failed += 1
            continue
        margins_ok = True
        if args.exact:                          # (asked before the spin: one region over the cap would refuse the whole panel)
            try:
                states = hansel.viterbi_states()[2]
                if states > cmd.EXACT_MAX_STATES:
                    hansel.viterbi_path()       # (raises: the library's own message)
            except GretelHipError as e:
                _fail(r["name"], "[FAIL] %s\n" % e)
                failed += 1
                continue
        elif args.margins:                      # (asked beforehand likewise; here a region over the cap only goes without the file)
            try:
                if hansel.viterbi_states()[2] > cmd.EXACT_MAX_STATES:
                    hansel.viterbi_marginals()  # (raises: the library's own message)
            except GretelHipError as e:
                _fail(r["name"], "[NOTE] --margins: %s\n" % e)
                margins_ok = False
        if args.margins and margins_ok:
            served.append(len(kept))
        if args.kbest:                          # (asked beforehand: one region the library refuses would refuse the whole call)
            kbest_ok = True
            try:
                states = hansel.viterbi_states()[2]
                if states > cmd.EXACT_MAX_STATES or states * args.kbest > cmd.EXACT_MAX_STATES:
                    hansel.viterbi_kbest(args.kbest)    # (raises: the library's own message)
            except GretelHipError as e:
                _fail(r["name"], "[NOTE] --kbest: %s\n" % e)
                kbest_ok = False
            if kbest_ok:
                ranked.append(len(kept))
        kept.append((r, vh, hansel, hansel.copy() if args.score_paths else None))       # (as gretel_amd.cmd: before the spins)
    margins = {}                # index into kept -> (viterbi_marginals' dict, the header's figures), taken before the spins
    if served:
        # (the call only reads the tensors: the live handles, no copy; S and states now -- an exact spin overwrites viterbi_info)
        hs = [kept[k][2] for k in served]
        for k, h, res in zip(served, hs, HanselPanel(hs).viterbi_marginals()):
            s, _, states, _ = h.viterbi_info()
            margins[k] = (res, cmd._score_head(h, kept[k][1]) + (s, states))
    kbest = {}                  # index into kept -> (viterbi_kbest's dict, the header's figures), likewise
    if ranked:
        hs = [kept[k][2] for k in ranked]
        for k, h, res in zip(ranked, hs, HanselPanel(hs).viterbi_kbest(args.kbest)):
            s, _, states, _ = h.viterbi_info()
            kbest[k] = (res, cmd._score_head(h, kept[k][1]) + (s, states, args.kbest))
    if kept:
        panel = HanselPanel([h for _, _, h, _ in kept])
        results = panel.viterbi_spin(args.paths, cmd.MIN_REMOVE) if args.exact else panel.spin(args.paths, cmd.MIN_REMOVE)
        with open(os.devnull, "w") as quiet:
            for k, ((r, vh, hansel, unweighted), res) in enumerate(zip(kept, results)):
                paths = cmd.paths_of_spin(hansel, res, log=quiet)
                dirn = os.path.join(args.out, r["name"])
                os.makedirs(dirn, exist_ok=True)
                ns = argparse.Namespace(out=dirn, master=args.master, start=r["start"], end=r["end"], gapchar=args.gapchar,
                                        delchar=args.delchar)
                cmd.write_outputs(paths, hansel, vh, ns)
                if args.assign_reads:
                    ns.min_snps, ns.max_mismatch = args.min_snps, args.max_mismatch
                    cmd.write_support(paths, hansel, ns)
                if args.score_paths:
                    cmd.write_scores(paths, unweighted, vh, ns)
                if k in margins:
                    cmd.write_margins_result(paths, margins[k][0], margins[k][1], hansel._cfg["cand_order"], vh, ns, name=r["name"])
                if k in kbest:
                    cmd.write_kbest_result(paths, kbest[k][0], kbest[k][1], vh, ns, name=r["name"])
                sys.stdout.write("%s\t%d\t%d\t%d\t%d\n" % (r["name"], vh["N"], hansel.L, res["n"], len(paths)))
    try:                        # (the decoder's kept working buffers: see gretel_amd.cmd)
        from . import bamio
        if getattr(bamio, "_io", None) is not None:
            bamio.native_release_buffers()
    except Exception:
        pass
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
