"""
`gretel` command line on top of the MI355X hot path: same positional arguments, options,
stdout table and output files as the reference driver (gretel/cmd.py:11-240), with the
SPINS loop (cmd.py:148-179) executed on the device by `Hansel.spin`.

Files written (formats: docs/protocol.rst:48-77):
    <out>/out.fasta       one record per distinct haplotype, in order of discovery   cmd.py:183-216
    <out>/snp.fasta       the SNP alleles only                                       cmd.py:218-219
    <out>/gretel.crumbs   "# N n_crumbs n_slices L" + one line per haplotype         cmd.py:224-240

and, with --assign-reads (no reference counterpart; INTEGRATION.md "Read assignment"):
    <out>/gretel.support  "# n_reads n_informative n_unique n_ambiguous n_unexplained" + one line per haplotype:
                          i_0, unique, shared, mismatches, unique / n_unique

and, with --beam B (INTEGRATION.md "Beam search"), the same files from paths that are each the best of a beam of B hypotheses over
the chain likelihood; --beam 1 writes what a run without the flag writes.

and, with --exact (INTEGRATION.md "Exact decoding"), the same files from paths that are each the global maximum of the chain
likelihood on the matrix at that moment; a window with more than 4096 states ends the run with the library's message, status 1.

and, with --exact-grid (INTEGRATION.md "Exact decoding on the grid"), the same through the grid decoder, which serves up to 2^24
states -- the fill's own L = 10 on a window of four or five candidate symbols -- at a kernel launch per SNP; a note on stderr says
what it is about to allocate.

and, with --margins (INTEGRATION.md "Max-marginals"), against the matrix as it was before any reweighting:
    <out>/gretel.margins  "# N L cond_mode marginal_term S states", one "H" line per recovered haplotype (i_0, n_best, max_regret and
                          the genomic position of argmax_regret) and one "S" line per SNP (genomic position, best allele, gap, the
                          regret of A C G T - with "." where an allele is not offered); nothing where the window has more than
                          4096 states (the library's message on stderr, the run goes on)

and, with --margins-grid (INTEGRATION.md "Max-marginals on the grid"), the same file through the grid call, which serves up to 2^24
states: byte for byte what --margins writes where both serve the window; a note on stderr says what it is about to allocate.

and, with --kbest K (INTEGRATION.md "K-best decoding"), against the matrix as it was before any reweighting:
    <out>/gretel.kbest    "# N L cond_mode marginal_term S states K n" + one line per rank of the K exactly best haplotypes of the
                          chain likelihood: rank, ll_chain, gap to rank 0, hamming0 (SNPs that differ from rank 0), the i_0 of the
                          nearest recovered haplotype, the number of SNPs at which they differ, and the SNP string; nothing where
                          K lists of the window's states do not fit 4096 slots or at a hole (a note on stderr, the run goes on)

and, with --alternatives M and/or --pin SPEC (INTEGRATION.md "Constrained decoding"), against the matrix as it was before any
reweighting:
    <out>/gretel.alternatives  "# N L cond_mode marginal_term S states M n", a "B" line for the free best haplotype of the chain
                          likelihood, one "A" line per alternative -- for the M SNPs of smallest max-marginal gap the exactly best
                          haplotype that carries the runner-up allele there: SNP rank, genomic position, best and alternative allele,
                          gap, its ll_chain, ll_best - ll, the SNPs at which it differs from the free best with the first and last
                          of them (how far the flip reaches), the nearest recovered haplotype and its distance, the SNP string --
                          and one "P" line per --pin (its index, the pinned sites, the same columns from ll_chain on); nothing
                          where the window has more than 4096 states or a hole (a note on stderr, the run goes on)

and, with --score-paths / --known FASTA (INTEGRATION.md "Scoring haplotypes"), against the matrix as it was before any reweighting:
    <out>/gretel.scores   "# N L cond_mode marginal_term" + one line per recovered haplotype: i_0, ll_chain, hp_original, n_greedy,
                          n_on, first_off, min_margin, argmin_margin and the genomic position of argmin_margin
    <out>/gretel.known    the same per record of FASTA (its name for i_0), then the i_0 of the nearest recovered haplotype and the
                          number of SNPs at which they differ
"""
from __future__ import annotations

import argparse
import sys

from . import __version__
from . import util
from ._lib import GretelHipError
from .hansel import Hansel

MIN_REMOVE = 0.01          # cmd.py:157
BEAM_MAX = 32              # include/gretel_hip.h: GH_BEAM_MAX
EXACT_MAX_STATES = 4096    # include/gretel_hip.h: GH_VITERBI_MAX_STATES
GRID_MAX_STATES = 1 << 24  # include/gretel_hip.h: GH_VITERBI_GRID_MAX_STATES
KBEST_MAX = 32             # include/gretel_hip.h: GH_KBEST_MAX
MASKED_MAX = 255           # include/gretel_hip.h: GH_MASKED_MAX_SETS less the free best path, which is set 0 of the call
MARGINS_HELP = ("compute the max-marginals of the chain likelihood on the unreweighted matrix (per SNP and allele the best likelihood "
                "of any haplotype that takes it; the state limit of --exact applies) and write per-SNP confidence gaps and "
                "per-haplotype regrets to gretel.margins")          # (gretel_amd.panel's --margins says the same)
KBEST_HELP = ("find the K exactly best haplotypes of the chain likelihood on the unreweighted matrix (1..%d; K times the states of "
              "--exact must not exceed %d) and write them, their gaps and the nearest recovered haplotype to gretel.kbest"
              % (KBEST_MAX, EXACT_MAX_STATES))               # (gretel_amd.panel's --kbest says the same)


def build_parser():
    p = argparse.ArgumentParser(prog="gretel", description="Gretel: A metagenomic haplotyper (MI355X hot path).")
    p.add_argument("bam")
    p.add_argument("vcf")
    p.add_argument("contig")
    p.add_argument("-s", "--start", type=int, default=1, help="1-indexed included start base position [default: 1]")
    p.add_argument("-e", "--end", type=int, default=-1, help="1-indexed included end base position [default: reference length]")
    p.add_argument("-p", "--paths", type=int, default=100, help="maximum number of paths to generate [default: 100]")
    p.add_argument("--master", default=None, help="master FASTA used to fill the non-SNP positions (otherwise --gapchar)")
    p.add_argument("--gapchar", default="N", help="character for non-SNP positions without --master [default: N]")
    p.add_argument("--delchar", default="", help="character written for a deletion [default: nothing]")
    p.add_argument("--quiet", default=False, action="store_true", help="do not print the per-SNP table")
    p.add_argument("-o", "--out", default=".", help="output directory [default: .]")
    p.add_argument("-@", "--threads", type=int, default=1, help="accepted for compatibility (the fill runs on the GPU)")
    p.add_argument("--debugreads", type=str, default="", help="A newline delimited list of read names to output debug data when parsing the BAM")
    p.add_argument("--debugpos", type=str, default="", help="A newline delimited list of 1-indexed genomic positions to output debug data when parsing the BAM")
    p.add_argument("--max-depth", type=int, default=8000, help="read-buffer cap of the pileup: reads beyond it at a position are dropped, as "
                   "the pysam pileup the reference runs on does at its default of 8000 (0 = keep every read) [default: 8000]")
    p.add_argument("--debughpos", type=str, default=",", help="comma delimited 1-indexed SNP ranks to print branch weights for")
    p.add_argument("--dumpmatrix", type=str, default=None, help="dump the Hansel tensor (.npz) to this path")
    p.add_argument("--dumpsnps", type=str, default=None, help="dump the SNP positions to this path")
    p.add_argument("--pepper", action="store_true", help="permissive read filter (pysam stepper 'all' in the reference)")
    add_assign_options(p)
    add_score_options(p)
    p.add_argument("--beam", type=int, default=0, metavar="B", help="recover every path as the best of a beam of B hypotheses over "
                   "the chain likelihood instead of the greedy walk (1..%d; 1 = the greedy walk; 0 = off) [default: 0]" % BEAM_MAX)
    p.add_argument("--exact", action="store_true", help="recover every path as the global maximum of the chain likelihood (exact "
                   "decoding over S^min(L, N) states, at most %d: L <= 6 without deletion columns, L <= 5 with them) instead of "
                   "the greedy walk" % EXACT_MAX_STATES)
    p.add_argument("--exact-grid", action="store_true", help="--exact through the grid decoder: the same paths, for up to %d states "
                   "(L <= 12 without deletion columns, L <= 10 with them) at a kernel launch per SNP and a byte of device memory per "
                   "SNP and state; with --exact it is what runs" % GRID_MAX_STATES)
    p.add_argument("--margins", action="store_true", help=MARGINS_HELP)
    p.add_argument("--margins-grid", action="store_true", help="--margins through the grid: the same gretel.margins, for up to %d states, "
                   "at two kernel launches per SNP and eight bytes of device memory per SNP and state; with --margins it is what "
                   "runs" % GRID_MAX_STATES)
    p.add_argument("--kbest", type=int, default=None, metavar="K", help=KBEST_HELP)
    p.add_argument("--alternatives", type=int, default=None, metavar="M", help="for the M SNPs whose call is least certain (smallest "
                   "max-marginal gap) decode the best haplotype that carries the runner-up allele there, exactly, on the unreweighted "
                   "matrix (1..%d; the state limit of --exact applies), and write them beside the free best haplotype to "
                   "gretel.alternatives" % MASKED_MAX)
    p.add_argument("--pin", action="append", default=None, metavar="SPEC", help="decode the best haplotype under constraints, exactly: "
                   "SPEC = POS:ALLELES[,POS:ALLELES...], POS a 1-based genomic position that is a SNP of the window, ALLELES the "
                   "alleles of ACGT- allowed there; repeatable, each use is one more line of gretel.alternatives")
    p.add_argument("--version", action="version", version="%(prog)s " + __version__)
    return p


def add_assign_options(p):
    """--assign-reads and its two settings (shared with gretel_amd.panel)."""
    p.add_argument("--assign-reads", action="store_true", help="assign every read to the recovered haplotype it matches best and "
                   "write the read support of each haplotype to gretel.support")
    p.add_argument("--min-snps", type=int, default=2, help="with --assign-reads: reads with fewer informative SNPs are left "
                   "out as uninformative [default: 2]")
    p.add_argument("--max-mismatch", type=int, default=-1, help="with --assign-reads: reads whose best haplotype differs at more "
                   "SNPs are unexplained (-1 = no limit) [default: -1]")


def add_score_options(p):
    """--score-paths and --known: haplotypes scored against the matrix as the reads filled it."""
    p.add_argument("--score-paths", action="store_true", help="score every recovered haplotype against the unreweighted matrix "
                   "(chain likelihood, per-SNP margins) and write gretel.scores")
    p.add_argument("--known", metavar="FASTA", default=None, help="score the haplotypes of FASTA (sequences in the contig's "
                   "coordinates, as --master) against the unreweighted matrix and write gretel.known")


def read_first_fasta_record(path):
    """What cmd.py:187-188 takes from pysam.FastaFile: the sequence of the first record."""
    seq = []
    seen = False
    with open(path) as fh:
        for line in fh:
            if line.startswith(">"):
                if seen:
                    break
                seen = True
                continue
            if seen:
                seq.append(line.strip())
    return "".join(seq)


FAIL_TEXT = '''[FAIL] Unable to recover pairwise evidence concerning SNP #%d at position %d
       Gretel needs every SNP to appear on a read with at least one other SNP, at least once.
       There is no read in your data set that bridges SNP #%d with any of its neighbours.

       * If you are trying to run Gretel along an entire contig or genome, please note that
       this is not the recommended usage for Gretel, as it was intended to uncover the
       variation in a metahaplome: the set of haplotypes for a specific gene.
           See our pre-print https://doi.org/10.1101/223404 for more information

       Consider running a prediction tool such as `prokka` on your assembly or reference
       and using the CDS regions in the GFF for corresponding genes of interest to
       uncover haplotypes with Gretel instead.

       * If you are already doing this, consider calling for SNPs more aggressively.
       We use `snpper` (https://github.com/SamStudio8/gretel-test/blob/master/snpper.py)
       to determine any site in a BAM that has at least one read in disagreement with
       the reference as a SNP. Although this introduces noise from alignment and sequence
       error, Gretel is fairly robust. Importantly, this naive calling method will
       likely close gaps between SNPs and permit recovery.

       * Finally, consider that the gaps are indicative that your reads do not support
       one or more parts of your assembly or reference. You could try and find or construct
       a more suitable reference, or reduce the size of the recovery window.

       Sorry :(\n'''            # the message of cmd.py:93-117, character for character

HOLE_TEXT = '''[NOTE] Unable to select next branch from SNP %d to %d
       By design, Gretel will attempt to recover haplotypes until a hole in the graph has been found.
       Recovery will intentionally terminate now.\n'''      # gretel.py:177-179


def gap_report(hansel, vcf_h, out=None):
    """cmd.py:85-118: returns True (and explains, in the reference's words) when some SNP has no pairwise evidence."""
    out = out or sys.stderr
    i = hansel.gap_check()
    if i < 0:
        return False
    pos = vcf_h["snp_rev"][i - 1] if i > 0 else 0
    out.write(FAIL_TEXT % (i, pos, i))
    return True


def print_snp_table(hansel, vcf_h, out=None):
    """cmd.py:123-145"""
    out = out or sys.stdout
    out.write("i\tpos\tgap\tA\tC\tG\tT\tN\t-\t_\ttot\n")
    last = 0
    for i in range(0, vcf_h["N"] + 1):
        c = hansel.counts_array(i)
        pos = vcf_h["snp_rev"][i - 1] if i > 0 else 0
        out.write("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
            i, pos, pos - last, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]))
        last = pos


def _add_path(paths, i, key, hansel_path, hp_current, hp_original, magnitude):
    """cmd.py:164-179"""
    if key not in paths:
        paths[key] = {"hp_current": [], "hp_original": [], "i": [], "i_0": i, "n": 0, "magnitude": 0,
                      "hansel_path": hansel_path}
    rec = paths[key]
    rec["n"] += 1
    rec["i"].append(i)
    rec["magnitude"] += magnitude
    rec["hp_current"].append(hp_current)
    rec["hp_original"].append(hp_original)


def recover(hansel, n_snps, max_paths, log=None, beam=0, exact=False, grid=False):
    """cmd.py:148-179 on the device; returns the PATHS table in order of discovery.  The spins have already
    happened when the notes are written, but the notes are the reference's, in the reference's order.
    beam >= 1 (--beam): every path is the best of a beam of that many hypotheses (Hansel.beam_spin).
    exact (--exact): every path is the global maximum of the chain likelihood (Hansel.viterbi_spin).
    grid (--exact-grid): the same through the grid decoder (Hansel.viterbi_spin_grid), behind a note of what it allocates."""
    if grid:
        s, le, states = hansel.viterbi_states()
        (log or sys.stderr).write("[NOTE] --exact-grid: S = %d candidate symbols, Le = %d: %d states, %d bytes of device scratch\n"
                                  % (s, le, states, hansel.viterbi_grid_bytes()))
        res = hansel.viterbi_spin_grid(max_paths, MIN_REMOVE)
    elif exact:
        res = hansel.viterbi_spin(max_paths, MIN_REMOVE)
    else:
        res = hansel.beam_spin(beam, max_paths, MIN_REMOVE) if beam else hansel.spin(max_paths, MIN_REMOVE)
    return paths_of_spin(hansel, res, log)


def paths_of_spin(hansel, res, log=None):
    """The PATHS table of cmd.py:148-179 from a finished spin `res` (Hansel.spin's dict, or a panel's for this window)."""
    log = log or sys.stderr
    paths = {}
    for i in range(res["n"]):
        log.write("[NOTE] *Establishing next path\n")                                   # gretel.py:142
        if res["min_marginal"][i] < MIN_REMOVE:                                          # cmd.py:158-160
            log.write("[RWGT] Ratio %.10f too small, adjusting to %.3f\n" % (res["min_marginal"][i], MIN_REMOVE))
        log.write("[RWGT] Ratio %.3f, Removed %.1f\n" % (res["ratio"][i], res["magnitude"][i]))   # gretel.py:97
        _add_path(paths, i, Hansel.path_str(res["paths"][i]), hansel.path_symbols(res["paths"][i]),
                  float(res["hp_current"][i]), float(res["hp_original"][i]), float(res["magnitude"][i]))
    if res["hole_at"]:
        log.write("[NOTE] *Establishing next path\n")
        log.write(HOLE_TEXT % (res["hole_at"] - 1, res["hole_at"]))
    return paths


def recover_with_debug(hansel, n_snps, max_paths, debug_hpos, log=None):
    """The same loop one path at a time through gretel_amd.gretel (one kernel sequence and one host round trip per
    path): what --debughpos needs, because the reference prints the branch weights of EVERY path as it walks
    (gretel.py:147-164), each against the tensor as reweighted so far."""
    from . import gretel
    log = log or sys.stderr
    paths = {}
    for i in range(max_paths):
        init_path, init_prob, init_min = gretel.generate_path(n_snps, hansel, hansel, debug_hpos=debug_hpos)
        if init_path is None:
            break
        if init_min < MIN_REMOVE:
            log.write("[RWGT] Ratio %.10f too small, adjusting to %.3f\n" % (init_min, MIN_REMOVE))
            init_min = MIN_REMOVE
        mag = gretel.reweight_hansel_from_path(hansel, init_path, init_min)
        _add_path(paths, i, "".join(str(x) for x in init_path), init_path, init_prob["hp_current"], init_prob["hp_original"], mag)
    return paths


def write_outputs(paths, hansel, vcf_h, args):
    """cmd.py:181-240, byte for byte."""
    dirn = args.out + "/"
    if args.master:
        master_seq = read_first_fasta_record(args.master)
    else:
        master_seq = [' '] * args.end
    with open(dirn + "out.fasta", "w") as fasta, open(dirn + "snp.fasta", "w") as hfasta:
        for key in sorted(paths, key=lambda x: paths[x]["i_0"]):
            p = paths[key]
            seq = list(master_seq[:])
            for j, mallele in enumerate(p["hansel_path"][1:]):
                pos = vcf_h["snp_rev"][j]
                seq[pos - 1] = args.delchar if mallele == hansel.symbols_d["-"] else mallele
            text = "".join(str(x) for x in seq[args.start - 1: args.end])
            if not args.master:
                text = text.replace(' ', args.gapchar)
            fasta.write(">%d__%.2f\n" % (p["i_0"], p["hp_current"][0]))
            fasta.write("%s\n" % text)
            hfasta.write(">%d__%.2f\n" % (p["i_0"], p["hp_current"][0]))
            hfasta.write("%s\n" % "".join(str(x) for x in p["hansel_path"][1:]))
    with open(dirn + "gretel.crumbs", "w") as crumbs:
        crumbs.write("# %d\t%d\t%d\t%.2f\n" % (vcf_h["N"], hansel.n_crumbs, hansel.n_slices, hansel.L))
        for key in sorted(paths, key=lambda x: paths[x]["hp_current"][0], reverse=True):
            p = paths[key]
            crumbs.write("%d\t%d\t%s\t%s\t%.2f\n" % (
                p["i_0"], p["n"], ",".join("%.2f" % x for x in p["hp_current"]),
                ",".join("%.2f" % x for x in p["hp_original"]), p["magnitude"]))


def support_text(i0s, res):
    """gretel.support: the totals behind "# ", then per haplotype (in the order of `i0s`, out.fasta's) its i_0, the reads
    assigned to it alone, the reads it shares a tie with, the mismatches of its unique reads and its share of the unique reads."""
    lines = ["# %d\t%d\t%d\t%d\t%d\n" % (res["n_reads"], res["n_informative"], res["n_unique"], res["n_ambiguous"],
                                          res["n_unexplained"])]
    nu = res["n_unique"]
    for q, i0 in enumerate(i0s):
        u = int(res["unique"][q])
        lines.append("%d\t%d\t%d\t%d\t%.4f\n" % (i0, u, int(res["shared"][q]), int(res["mismatches"][q]), u / nu if nu else 0.0))
    return "".join(lines)


def write_support(paths, hansel, args):
    """--assign-reads: the distinct haplotypes in out.fasta's order (by i_0) against the support table the fill kept."""
    import numpy as np
    keys = sorted(paths, key=lambda x: paths[x]["i_0"])
    arr = np.array([[s.i for s in paths[k]["hansel_path"]] for k in keys], dtype=np.uint8).reshape(len(keys), hansel.n + 1)
    res = hansel.assign_reads(arr, min_snps=args.min_snps, max_mismatch=args.max_mismatch)
    with open(args.out + "/gretel.support", "w") as fh:
        fh.write(support_text([paths[k]["i_0"] for k in keys], res))


def _path_array(paths, keys, n):
    import numpy as np
    return np.array([[s.i for s in paths[k]["hansel_path"]] for k in keys], dtype=np.uint8).reshape(len(keys), n + 1)


def scores_text(head, names, res, snp_rev, nearest=None):
    """gretel.scores / gretel.known: "# N L cond_mode marginal_term" (`head`), then per haplotype (in the order of `names`: i_0s
    or record names) its name, ll_chain, hp_original, n_greedy, n_on, first_off, min_margin, argmin_margin and the genomic
    position of argmin_margin (0 where there is none); `res` is Hansel.score_paths' dict.  nearest (gretel.known): per
    haplotype the (i_0, differing SNPs) of the nearest recovered haplotype, two more columns."""
    lines = ["# %d\t%d\t%s\t%d\n" % tuple(head)]
    for q, name in enumerate(names):
        arg = int(res["argmin_margin"][q])
        line = "%s\t%.6f\t%.6f\t%d\t%d\t%d\t%.6f\t%d\t%d" % (
            name, res["ll_chain"][q], res["hp_original"][q], int(res["n_greedy"][q]), int(res["n_on"][q]), int(res["first_off"][q]),
            res["min_margin"][q], arg, snp_rev[arg - 1] if arg > 0 else 0)
        if nearest is not None:
            line += "\t%d\t%d" % tuple(nearest[q])
        lines.append(line + "\n")
    return "".join(lines)


def nearest_recovered(known, recovered, i0s):
    """Per row of `known` the (i_0, differing SNPs) of the row of `recovered` that differs from it at the fewest SNP columns; the
    lowest i_0 wins a tie (`i0s` ascend); (-1, -1) when nothing was recovered."""
    import numpy as np
    if len(recovered) == 0:
        return [(-1, -1)] * len(known)
    d = (np.asarray(known)[:, None, 1:] != np.asarray(recovered)[None, :, 1:]).sum(axis=2)
    best = d.argmin(axis=1)
    return [(int(i0s[b]), int(d[q, b])) for q, b in enumerate(best)]


def _score_head(unweighted, vcf_h):
    return (vcf_h["N"], unweighted.L, unweighted._cfg["cond_mode"], int(unweighted._cfg["marginal_term"]))


def write_scores(paths, unweighted, vcf_h, args):
    """--score-paths: the distinct haplotypes in out.fasta's order (by i_0) against the copy taken before the spins."""
    keys = sorted(paths, key=lambda x: paths[x]["i_0"])
    res = unweighted.score_paths(_path_array(paths, keys, unweighted.n))
    with open(args.out + "/gretel.scores", "w") as fh:
        fh.write(scores_text(_score_head(unweighted, vcf_h), [paths[k]["i_0"] for k in keys], res, vcf_h["snp_rev"]))


def write_known(paths, unweighted, vcf_h, args):
    """--known: every record of the FASTA against the same copy, and the recovered haplotype nearest to it."""
    keys = sorted(paths, key=lambda x: paths[x]["i_0"])
    names, known = util.known_snp_paths(args.known, vcf_h, unweighted)
    res = unweighted.score_paths(known)
    near = nearest_recovered(known, _path_array(paths, keys, unweighted.n), [paths[k]["i_0"] for k in keys])
    with open(args.out + "/gretel.known", "w") as fh:
        fh.write(scores_text(_score_head(unweighted, vcf_h), names, res, vcf_h["snp_rev"], nearest=near))


def _margin_num(v):
    return "%.6f" % v


def margins_text(head, i0s, marg, mm, cm, snp_rev):
    """gretel.margins: "# N L cond_mode marginal_term S states" (`head`), then one line per haplotype (in the order of `i0s`,
    out.fasta's) -- "H", i_0, n_best, max_regret, the genomic position of argmax_regret -- then one line per SNP -- "S", the genomic
    position, the best allele, gap, and the regret of each allele in ACGT- order ("." where it is not offered).  `marg` is
    margins_of's dict for those haplotypes over Hansel.viterbi_marginals' `mm` and `cm`."""
    from .hansel import SYMBOLS, margins_of
    lines = ["# %d\t%d\t%s\t%d\t%d\t%d\n" % tuple(head)]
    for q, i0 in enumerate(i0s):
        arg = int(marg["argmax_regret"][q])
        lines.append("H\t%d\t%d\t%s\t%d\n" % (i0, int(marg["n_best"][q]), _margin_num(marg["max_regret"][q]), snp_rev[arg - 1] if arg > 0 else 0))
    n = len(cm) - 1
    alleles = [SYMBOLS.index(c) for c in "ACGT-"]
    # (the regret of allele s at every SNP is the regret of the constant "path" of s)
    each = margins_of(mm, cm, [[6] + [s] * n for s in alleles])["regret"]
    for p in range(1, n + 1):
        cols = [_margin_num(each[k, p]) if (int(cm[p]) >> s) & 1 else "." for k, s in enumerate(alleles)]
        lines.append("S\t%d\t%s\t%s\t%s\n" % (snp_rev[p - 1], SYMBOLS[int(marg["best"][p])], _margin_num(marg["gap"][p]), "\t".join(cols)))
    return "".join(lines)


def write_margins_result(paths, res, head, order, vcf_h, args, name=None, flag="--margins"):
    """What follows the max-marginals call, for this CLI and for gretel_amd.panel (which makes one call for all its regions): `res`
    is Hansel.viterbi_marginals' dict, `head` the header's six figures (N, L, cond_mode, marginal_term, S, states -- S and states
    as the call left them), `order` the handle's cand_order.  At a hole the note on stderr (behind `name` where there is one)
    and no file; otherwise gretel.margins for the distinct haplotypes in out.fasta's order."""
    from .hansel import margins_of
    if res["hole_at"]:
        sys.stderr.write("%s[NOTE] %s: no candidate at SNP %d, no max-marginals\n" % ("%s: " % name if name else "", flag, res["hole_at"]))
        return
    keys = sorted(paths, key=lambda x: paths[x]["i_0"])
    marg = margins_of(res["mm"], res["cm"], _path_array(paths, keys, len(res["cm"]) - 1), order)
    with open(args.out + "/gretel.margins", "w") as fh:
        fh.write(margins_text(head, [paths[k]["i_0"] for k in keys], marg, res["mm"], res["cm"], vcf_h["snp_rev"]))


def marginals_once(unweighted, grid=False):
    """The one max-marginals call --margins and --alternatives share: (Hansel.viterbi_marginals' dict, (S, states) as the call
    left them), or (None, the library's refusal).
    grid (--margins-grid): the same through Hansel.viterbi_marginals_grid, behind a note of what it allocates."""
    if grid:
        s, le, states = unweighted.viterbi_states()
        if 0 < states <= GRID_MAX_STATES:
            sys.stderr.write("[NOTE] --margins-grid: S = %d candidate symbols, Le = %d: %d states, %d bytes of device scratch\n"
                             % (s, le, states, unweighted.viterbi_marginals_grid_bytes()))
    try:
        res = unweighted.viterbi_marginals_grid() if grid else unweighted.viterbi_marginals()
    except GretelHipError as e:
        return None, e
    s, _, states, _ = unweighted.viterbi_grid_info() if grid else unweighted.viterbi_info()
    return res, (s, states)


def write_margins(paths, unweighted, vcf_h, args, call=None):
    """--margins: the max-marginals of the copy taken before the spins, read for the distinct haplotypes in out.fasta's order.
    A window beyond the exact decoder's cap: the library's message on stderr and no file.  `call`: marginals_once's pair where
    the call has been made already.  With args.margins_grid (--margins-grid) the call is the grid's, whose cap is 2^24 states."""
    grid = getattr(args, "margins_grid", False)                 # (gretel_amd.panel's parser has no --margins-grid)
    flag = "--margins-grid" if grid else "--margins"
    res, info = call if call is not None else marginals_once(unweighted, grid=True) if grid else marginals_once(unweighted)
    if res is None:
        sys.stderr.write("[NOTE] %s: %s\n" % (flag, info))
        return
    write_margins_result(paths, res, _score_head(unweighted, vcf_h) + info, unweighted._cfg["cand_order"], vcf_h, args, flag=flag)


def parse_pin(spec):
    """--pin SPEC -> [(genomic position, alleles)], or a message (a str) where the syntax is wrong."""
    out, seen = [], set()
    for part in spec.split(","):
        pos, sep, alleles = part.partition(":")
        if not sep or not pos.strip().isdigit() or not alleles or any(c not in "ACGT-" for c in alleles):
            return "--pin %s: %r is not POS:ALLELES (POS a position, ALLELES a non-empty string over ACGT-)" % (spec, part)
        if int(pos) in seen:
            return "--pin %s: position %d is given twice" % (spec, int(pos))
        seen.add(int(pos))
        out.append((int(pos), alleles))
    return out


def check_masked_options(args):
    """The refusals of --alternatives and --pin (before any BAM read or GPU call): a message, or None."""
    if args.alternatives is not None and not 1 <= args.alternatives <= MASKED_MAX:
        return "--alternatives must be 1..%d" % MASKED_MAX
    for spec in args.pin or []:
        pins = parse_pin(spec)
        if isinstance(pins, str):
            return pins
    if (args.alternatives or 0) + len(args.pin or []) > MASKED_MAX:
        return "--alternatives and --pin together may not ask for more than %d constraint sets" % MASKED_MAX
    return None


def check_pins_in_window(args, vcf_h):
    """... and the one that needs the VCF (still before any GPU call): every POS of a --pin is a SNP of the window."""
    for spec in args.pin or []:
        for pos, _ in parse_pin(spec):
            if pos not in vcf_h["snp_fwd"]:
                return "--pin %s: position %d is not a SNP of the window" % (spec, pos)
    return None


def _reach(x, x0):
    """(SNPs at which x differs from x0, the first and the last of them as SNP ranks; 0, 0, 0 where none does)."""
    import numpy as np
    d = np.flatnonzero(np.asarray(x)[1:] != np.asarray(x0)[1:]) + 1
    return (len(d), int(d[0]), int(d[-1])) if len(d) else (0, 0, 0)


def alternatives_text(head, res, alts, pinned, recovered, i0s, snp_rev):
    """gretel.alternatives: "# N L cond_mode marginal_term S states M n" (`head` the first seven, M = 0 without --alternatives; n the
    alternatives that follow), then, tab separated,
      B  ll_chain, SNP string                                      the free best haplotype (set 0 of the call)
      A  SNP rank p, genomic position, best allele, alternative allele, max-marginal gap, then the TAIL     one per alternative
      P  k (the k-th --pin, from 1), pinned sites, then the TAIL                                             one per --pin
    TAIL: ll_chain of the constrained best haplotype, ll_best - ll (0.0 where they are equal), the SNPs at which it differs from
    the free best, the first and the last of them as SNP ranks (0 0 where none: how far the constraint reaches), the i_0 of the
    nearest recovered haplotype and the SNPs at which they differ (-1 -1 where nothing was recovered), the SNP string.  An
    infeasible set has "infeasible" and the first SNP rank without a candidate in place of the TAIL.
    `res` is Hansel.viterbi_path_masked's dict over [all allowed] + alts["allow"] + the pin sets, `alts` alternatives_of's dict,
    `pinned` the pinned sites per --pin, `recovered` the recovered haplotypes in out.fasta's order and `i0s` their i_0s."""
    from .hansel import SYMBOLS
    m = len(alts["p"])
    lines = ["# %d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % (tuple(head) + (m,))]
    x0, ll0 = res["paths"][0], float(res["ll_chain"][0])
    near = nearest_recovered(res["paths"], recovered, i0s)

    def tail(q):
        if res["hole_at"][q]:
            return "infeasible\t%d" % res["hole_at"][q]
        ll = float(res["ll_chain"][q])
        return "%.6f\t%.6f\t%d\t%d\t%d\t%d\t%d\t%s" % ((ll, 0.0 if ll == ll0 else ll0 - ll) + _reach(res["paths"][q], x0) + tuple(near[q]) +
                                                      (Hansel.path_str(res["paths"][q][1:]),))

    lines.append("B\t%.6f\t%s\n" % (ll0, Hansel.path_str(x0[1:])))
    for q in range(m):
        p = int(alts["p"][q])
        lines.append("A\t%d\t%d\t%s\t%s\t%.6f\t%s\n" % (p, snp_rev[p - 1], SYMBOLS[int(alts["best"][q])], SYMBOLS[int(alts["alt"][q])],
                                                      alts["gap"][q], tail(1 + q)))
    for k, sites in enumerate(pinned):
        lines.append("P\t%d\t%d\t%s\n" % (k + 1, sites, tail(1 + m + k)))
    return "".join(lines)


def write_alternatives(paths, unweighted, vcf_h, args, call=None):
    """--alternatives / --pin: ONE constrained decoding of the copy taken before the spins -- set 0 all-allowed (the free best
    haplotype), the alternatives_of sets of --alternatives M (from the max-marginals call it shares with --margins: `call`), one
    set per --pin -- written to gretel.alternatives.  A window the decoder refuses: the library's message as a note and no file;
    a hole of the window itself likewise; an infeasible --pin: a note and a line that says so."""
    import numpy as np
    from .hansel import allow_of, alternatives_of
    n, order = unweighted.n, unweighted._cfg["cand_order"]
    alts = dict(p=np.zeros(0, dtype=np.int32), best=np.zeros(0, dtype=np.uint8), alt=np.zeros(0, dtype=np.uint8), gap=np.zeros(0),
                allow=np.zeros((0, n + 1), dtype=np.uint8))
    if args.alternatives:
        mres, info = call if call is not None else marginals_once(unweighted)
        if mres is None:
            sys.stderr.write("[NOTE] --alternatives: %s\n" % info)
            return
        if mres["hole_at"]:
            sys.stderr.write("[NOTE] --alternatives: no candidate at SNP %d, no alternatives\n" % mres["hole_at"])
            return
        alts = alternatives_of(mres["mm"], mres["cm"], args.alternatives, order)
    pins = [{vcf_h["snp_fwd"][pos] + 1: alleles for pos, alleles in parse_pin(spec)} for spec in args.pin or []]
    allow = np.concatenate([allow_of(n).reshape(1, -1), alts["allow"]] + [allow_of(n, pins=pp).reshape(1, -1) for pp in pins])
    try:
        res = unweighted.viterbi_path_masked(allow)
    except GretelHipError as e:
        sys.stderr.write("[NOTE] --alternatives: %s\n" % e)
        return
    if res["hole_at"][0]:
        sys.stderr.write("[NOTE] --alternatives: no candidate at SNP %d, no alternatives\n" % res["hole_at"][0])
        return
    m = len(alts["p"])
    for k in range(len(pins)):
        if res["hole_at"][1 + m + k]:
            sys.stderr.write("[NOTE] --pin %d: no candidate at SNP %d under the constraints\n" % (k + 1, res["hole_at"][1 + m + k]))
    s, _, states, _ = unweighted.viterbi_info()
    keys = sorted(paths, key=lambda x: paths[x]["i_0"])
    with open(args.out + "/gretel.alternatives", "w") as fh:
        fh.write(alternatives_text(_score_head(unweighted, vcf_h) + (s, states, args.alternatives or 0), res, alts, [len(pp) for pp in pins],
                                   _path_array(paths, keys, n), [paths[k]["i_0"] for k in keys], vcf_h["snp_rev"]))


def kbest_text(head, res, per_rank, i0s):
    """gretel.kbest: "# N L cond_mode marginal_term S states K n" (`head`), then one line per rank of Hansel.viterbi_kbest's dict
    `res`: the rank, ll_chain, gap, hamming0, the i_0 of the nearest recovered haplotype and the number of SNPs at which they differ
    (-1 and -1 where nothing was recovered), and the SNP string.  `per_rank` is kbest_of's dict for `res` against the recovered
    haplotypes in out.fasta's order, `i0s` their i_0s."""
    lines = ["# %d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % tuple(head)]
    for q in range(res["n"]):
        near = int(per_rank["nearest"][q])
        lines.append("%d\t%.6f\t%.6f\t%d\t%d\t%d\t%s\n" % (
            q, res["ll_chain"][q], per_rank["gap"][q], int(per_rank["hamming0"][q]), int(i0s[near]) if near >= 0 else -1,
            int(per_rank["distance"][q]), Hansel.path_str(res["paths"][q][1:])))
    return "".join(lines)


def write_kbest_result(paths, res, head, vcf_h, args, name=None):
    """What follows the k-best call, for this CLI and for gretel_amd.panel (which makes one call for all its regions): `res` is
    Hansel.viterbi_kbest's dict, `head` the header's first seven figures (N, L, cond_mode, marginal_term, S, states -- S and states
    as the call left them -- and K).  At a hole the note on stderr (behind `name` where there is one) and no file; otherwise
    gretel.kbest, the ranks set beside the distinct recovered haplotypes in out.fasta's order."""
    from .hansel import kbest_of
    if res["hole_at"]:
        sys.stderr.write("%s[NOTE] --kbest: no candidate at SNP %d, no k-best haplotypes\n" % ("%s: " % name if name else "", res["hole_at"]))
        return
    keys = sorted(paths, key=lambda x: paths[x]["i_0"])
    per_rank = kbest_of(res, _path_array(paths, keys, res["paths"].shape[1] - 1))
    with open(args.out + "/gretel.kbest", "w") as fh:
        fh.write(kbest_text(tuple(head) + (res["n"],), res, per_rank, [paths[k]["i_0"] for k in keys]))


def write_kbest(paths, unweighted, vcf_h, args):
    """--kbest: the K best haplotypes of the copy taken before the spins, set beside the distinct recovered haplotypes in
    out.fasta's order.  A window the library refuses (too many states, or K lists of them too many slots) or a hole: a note on
    stderr and no file."""
    try:
        res = unweighted.viterbi_kbest(args.kbest)
    except GretelHipError as e:
        sys.stderr.write("[NOTE] --kbest: %s\n" % e)
        return
    s, _, states, _ = unweighted.viterbi_info()
    write_kbest_result(paths, res, _score_head(unweighted, vcf_h) + (s, states, args.kbest), vcf_h, args)


def check_kbest_options(args):
    """The refusal of --kbest (before any BAM read or GPU call): a message, or None."""
    if args.kbest is not None and not 1 <= args.kbest <= KBEST_MAX:
        return "--kbest must be 1..%d" % KBEST_MAX
    return None


def check_score_options(args):
    """The refusal of --known (before any BAM read or GPU call): a message, or None."""
    if args.known is None:
        return None
    try:
        if not util.read_fasta_records(args.known):
            return "--known %s holds no FASTA record" % args.known
    except OSError as e:
        return "--known %s cannot be read: %s" % (args.known, e.strerror)
    return None


def check_assign_options(args):
    """The refusals of --min-snps / --max-mismatch (before any BAM read or GPU call): a message, or None."""
    if args.assign_reads and args.min_snps < 1:
        return "--min-snps must be at least 1"
    if args.assign_reads and args.max_mismatch < -1:
        return "--max-mismatch must be -1 (no limit) or at least 0"
    return None


def debug_hpos_of(args):
    """The SNP ranks of --debughpos (cmd.py:120-121: whatever does not parse as a number is dropped)."""
    out = []
    for x in (args.debughpos or "").split(","):
        try:
            out.append(int(x))
        except ValueError:
            pass
    return out


def check_beam_options(args):
    """The refusals of --beam (before any BAM read or GPU call): a message, or None."""
    if args.beam < 0 or args.beam > BEAM_MAX:
        return "--beam must be 0 (off) or 1..%d" % BEAM_MAX
    if args.beam and debug_hpos_of(args):
        return "--beam cannot be combined with --debughpos, which prints the branch weights of the greedy walk"
    return None


def check_exact_options(args):
    """The refusals of --exact and --exact-grid (before any BAM read or GPU call): a message, or None."""
    exact = args.exact or getattr(args, "exact_grid", False)     # (gretel_amd.panel's parser has no --exact-grid)
    if exact and args.beam:
        return "--exact cannot be combined with --beam: a path is either the global maximum or the best of a beam"
    if exact and debug_hpos_of(args):
        return "--exact cannot be combined with --debughpos, which prints the branch weights of the greedy walk"
    return None


def main(argv=None):
    args = build_parser().parse_args(argv)
    bad = check_assign_options(args) or check_score_options(args) or check_beam_options(args) or check_exact_options(args) or check_kbest_options(args) or check_masked_options(args)
    if bad:
        sys.stderr.write("[FAIL] %s\n" % bad)
        return 2
    if args.end == -1:
        args.end = util.get_ref_len_from_bam(args.bam, args.contig)               # cmd.py:53-55
        sys.stderr.write("[NOTE] Setting end_pos to %d" % args.end)
    if not (args.debugreads or args.debugpos):
        # (the BAM's blocks are read and inflated on the decoder's threads while the VCF is parsed here: include/gretel_io.h, gio_prefetch)
        util.prefetch_bam(args.bam, args.contig, args.start, args.end)
    vcf_h = util.process_vcf(args.vcf, args.contig, args.start, args.end)         # cmd.py:69
    bad = check_pins_in_window(args, vcf_h)
    if bad:
        sys.stderr.write("[FAIL] %s\n" % bad)
        return 2
    if args.dumpsnps:                                                             # cmd.py:70-74
        with open(args.dumpsnps, "w") as fh:
            for k in sorted(vcf_h["snp_fwd"].keys()):
                fh.write("%d\t%d\t%d\n" % (vcf_h["snp_fwd"][k] + 1, k, k - args.start + 1))
    debug_reads, debug_pos = set(), set()                                          # cmd.py:57-67
    if args.debugreads:
        with open(args.debugreads) as fh:
            debug_reads = {line.strip() for line in fh}
    if args.debugpos:
        with open(args.debugpos) as fh:
            debug_pos = {int(line.strip()) for line in fh if line.strip()}
    hansel = util.load_from_bam(args.bam, args.contig, args.start, args.end, vcf_h, n_threads=args.threads,
                                debug_reads=debug_reads, debug_pos=debug_pos, max_depth=args.max_depth,
                                stepper="all" if args.pepper else "samtools", keep_reads=args.assign_reads)     # cmd.py:78
    hansel.snapshot_original()                                                    # cmd.py:79 (what the copy is used for)
    # (the reference's copy of cmd.py:79, made only where something is scored against the matrix as the reads filled it)
    masked = bool(args.alternatives or args.pin)
    unweighted = hansel.copy() if (args.score_paths or args.known or args.margins or args.margins_grid or args.kbest or masked) else None
    if args.dumpmatrix:
        hansel.save_hansel_dump(args.dumpmatrix)                                  # cmd.py:81-82
    if gap_report(hansel, vcf_h):
        sys.exit(1)                                                               # cmd.py:118
    if not args.quiet:
        print_snp_table(hansel, vcf_h)
    debug_hpos = debug_hpos_of(args)
    if debug_hpos:
        paths = recover_with_debug(hansel, vcf_h["N"], args.paths, debug_hpos)
    else:
        try:
            paths = recover(hansel, vcf_h["N"], args.paths, beam=args.beam, exact=args.exact, grid=args.exact_grid)
        except GretelHipError as e:
            if not (args.exact or args.exact_grid):
                raise
            sys.stderr.write("[FAIL] %s\n" % e)                                   # (more states than the decoder holds: no fallback)
            return 1
    write_outputs(paths, hansel, vcf_h, args)
    if args.assign_reads:
        write_support(paths, hansel, args)
    if args.score_paths:
        write_scores(paths, unweighted, vcf_h, args)
    if args.known:
        write_known(paths, unweighted, vcf_h, args)
    # (one LDS call for --margins and --alternatives; with --margins-grid the file comes from the grid call, made once)
    marg = marginals_once(unweighted) if ((args.margins and not args.margins_grid) or args.alternatives) else None
    if args.margins_grid:
        write_margins(paths, unweighted, vcf_h, args)
    elif args.margins:
        write_margins(paths, unweighted, vcf_h, args, call=marg)
    if args.kbest:
        write_kbest(paths, unweighted, vcf_h, args)
    if masked:
        write_alternatives(paths, unweighted, vcf_h, args, call=marg)
    try:                       # the decoder's kept working buffers (include/gretel_io.h: GIO_KEEP_MB): a run has one decode
        from . import bamio
        if getattr(bamio, "_io", None) is not None:
            bamio.native_release_buffers()
    except Exception:
        pass
    return 0


if __name__ == "__main__":
    sys.exit(main())
