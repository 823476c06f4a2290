"""Seeded random windows for the decoders over the chain table (beam, exact path, max-marginals, k best and their panel forms).
Not a test file: tests/test_decode_cases_host.py holds the references to each other on these windows and checks that the list
covers what it exists for, tests/test_gpu_decode_cases.py and tests/fuzz_decode_gpu.py hold the GPU to the references on them.

    case(seed) -> (desc, SupportTable)

is a pure function of the seed: numpy.random.default_rng(seed) and nothing else, so that a seed names the same bytes everywhere.
What a window is drawn from, and why:

    alphabet   a subset of "ACGT-" of 1..5 symbols, three most often and mostly not a prefix of "ACGT-": the digit scheme of the
               exact decoders at 3^k states and the slot -> compact-index map under alphabets with gaps
    positions  every position draws its own non-empty subset of the alphabet for the haplotypes to take: positions that offer fewer
               candidates than the window's S are what the reachability words of the kernels are for
    reads      a tiling pass of one haplotype (every neighbouring pair bridged) and random reads of all of them, at most
               2, 3, 4, 6 or 9 SNPs long: band = max_k - 1 is often below L, lags beyond the band are the table's constants
    hole       in a capped share of the windows every read is cut between one chosen pair of neighbours
    L          1 .. the largest lag count the exact decoder serves for the alphabet, leaning to the top; a few windows lie one lag
               beyond it on purpose: the refusal is the expected result there
    spec       cond_mode A..E, the marginal term, f32 / f64 storage, a permuted candidate order; offer_zero stays off (the decoders
               refuse it).  Under C and D the lag that reaches position 0 from beyond position 1 has a zero denominator: every
               full path scores +inf once L >= 2 and only the tie orders decide, so a share of those windows takes L = 1
    K, width   1..32, K clipped to what the window's states leave and leaning to values that are no power of two

desc["S"] is the generator's count of the symbols in the reads; what the window offers (S of the decoders) is the reference's
business: a symbol that stands only where no read goes on to the next position is no candidate."""
import numpy as np

from gretel_amd.synth import SupportTable

VALID = "ACGT-"
CAP = 4096                 # include/gretel_hip.h: GH_VITERBI_MAX_STATES
KMAX = 32                  # GH_KBEST_MAX, GH_BEAM_MAX
NS = (1, 2, 3, 5, 8, 13, 21, 34, 55)
MAX_K = (2, 3, 4, 6, 9)
ERR = (0.0, 0.0, 0.05, 0.2)
L_TOP_S1 = 14              # S = 1: one state whatever L is; beyond 12 lags the walk takes its second body


def _alphabet(rng):
    size = int(rng.choice([1, 2, 3, 4, 5], p=[0.10, 0.18, 0.34, 0.24, 0.14]))
    idx = set(int(v) for v in rng.choice(5, size=size, replace=False))
    if size < 5 and 4 not in idx and rng.random() < 0.35:        # deletions more often than chance gives them
        idx.remove(sorted(idx)[int(rng.integers(0, size))])
        idx.add(4)
    return sorted(idx)


def _haplotypes(rng, alpha, n, n_haps):
    haps = np.zeros((n_haps, n), dtype=np.int64)
    for p in range(n):
        m = int(rng.integers(1, len(alpha) + 1))
        sub = rng.choice(alpha, size=m, replace=False)
        haps[:, p] = sub[rng.integers(0, m, size=n_haps)]
        if n_haps >= m:                                          # every symbol the position drew is taken by some haplotype
            haps[rng.permutation(n_haps)[:m], p] = sub
    return haps


def _reads(rng, haps, alpha, n, max_k, err, n_frac):
    """[(rank, [symbol indices into VALID, 5 = 'N', 6 = '_'])]: the tiling pass, then the random reads."""
    n_haps = haps.shape[0]
    reads = []
    if n <= 2:
        # no read of two SNPs ends inside such a window: position N gets its count from a read that goes on to the '_' behind it
        for _ in range(int(rng.integers(3, 9))):
            row = haps[int(rng.integers(0, n_haps))]
            if n == 2:
                reads.append((0, [int(row[0]), int(row[1])]))
            reads.append((n - 1, [int(row[n - 1]), 6]))
        return reads
    kt = min(max_k, n)
    step = max(1, kt // 2)
    starts = list(range(0, n - kt + 1, step))
    if starts[-1] != n - kt:
        starts.append(n - kt)
    for s in starts:
        reads.append((s, [int(v) for v in haps[0, s:s + kt]]))
    abund = rng.dirichlet(np.ones(n_haps))
    for _ in range(int(rng.integers(n, 5 * n + 6))):
        k = int(rng.integers(2, kt + 1))
        s = int(rng.integers(0, n - k + 1))
        row = haps[int(rng.choice(n_haps, p=abund))]
        seq = [int(v) for v in row[s:s + k]]
        for i in range(k):
            u = rng.random()
            if u < err and len(alpha) > 1:                       # a substitution stays within the alphabet
                seq[i] = int(rng.choice([a for a in alpha if a != seq[i]]))
            elif u > 1.0 - n_frac:
                seq[i] = 5
        reads.append((s, seq))
    return reads


def _cut(reads, at):
    """No read bridges positions `at` and `at` + 1 (1-based): every read that does is cut in two, pieces of one SNP are dropped."""
    out = []
    for s, seq in reads:
        e = s + len(seq)                                         # the read covers positions s + 1 .. e
        if s + 1 <= at and at + 1 <= e:
            for rank, part in ((s, seq[:at - s]), (at, seq[at - s:])):
                if len(part) >= 2:
                    out.append((rank, part))
        else:
            out.append((s, seq))
    return out


def _pow_le(s, le):
    v = 1
    for _ in range(le):
        v *= s
        if v > CAP:
            return CAP + 1
    return v


def _lags(rng, s, n):
    """(L, True where it lies one lag beyond the cap on purpose)."""
    if s <= 1:
        top = L_TOP_S1
    else:
        top = 1
        while _pow_le(s, top + 1) <= CAP:
            top += 1
        if n > top and rng.random() < 0.06:
            return top + 1, True
        if n <= top:                                             # the state is the whole prefix: every L is served
            top = n + 3
    u = rng.random()
    if u < 0.45:
        return top, False
    if u < 0.65:
        return max(1, top - 1), False
    return int(rng.integers(1, top + 1)), False


def _k(rng, states):
    most = max(1, min(KMAX, CAP // max(1, states)))
    u = rng.random()
    if u < 0.35:
        return most
    odd = [k for k in range(1, most + 1) if k & (k - 1)]
    if u < 0.8 and odd:
        return int(rng.choice(odd))
    return int(rng.integers(1, most + 1))


def case(seed):
    rng = np.random.default_rng(seed)
    alpha = _alphabet(rng)
    n = int(rng.choice(NS))
    n_haps = int(rng.integers(1, 5))
    err = float(rng.choice(ERR))
    n_frac = 0.03 if rng.random() < 0.08 else 0.0
    max_k = int(rng.choice(MAX_K))
    haps = _haplotypes(rng, alpha, n, n_haps)
    reads = _reads(rng, haps, alpha, n, max_k, err, n_frac)
    hole = 0
    if n >= 3 and rng.random() < 0.10:
        hole = int(rng.integers(1, n))
        reads = _cut(reads, hole)
    reads.sort(key=lambda r: r[0])                               # rank order, as the reads of a coordinate-sorted BAM (stable)
    lut = np.frombuffer(b"ACGT-N_", dtype=np.uint8)
    ks = [len(seq) for _, seq in reads]
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum(ks, out=off[1:])
    flat = np.array([v for _, seq in reads for v in seq], dtype=np.int64)
    t = SupportTable(n_snps=n, rank=np.array([r for r, _ in reads], dtype=np.int32), off=off, bases=lut[flat].astype(np.uint8),
                     haplotypes=lut[haps].astype(np.uint8), abundances=np.full(n_haps, 1.0 / n_haps))
    s = len(set(int(v) for v in flat if v < 5))
    spec = dict(cond_mode=str(rng.choice(list("ABCDE"))), marginal_term=bool(rng.random() < 0.4),
                storage="f64" if rng.random() < 0.3 else "f32",
                cand_order="".join(rng.permutation(list(VALID))) if rng.random() < 0.5 else VALID)
    L, beyond = _lags(rng, s, n)
    if spec["cond_mode"] in "CD" and not beyond and rng.random() < 0.3:
        L = 1                                                    # (the one lag count at which these two modes score finitely)
    states = _pow_le(s, min(L, n))
    desc = dict(seed=int(seed), alphabet="".join(VALID[a] for a in alpha), S=s, N=n, n_haps=n_haps, err=err, n_frac=n_frac, max_k=max_k,
                band=t.band, reads=len(reads), cut_at=hole, L=L, beyond=beyond, K=_k(rng, states), width=int(rng.integers(1, KMAX + 1)),
                spec=spec)
    return desc, t


def oracle_of(desc, t, spec=None, L=None):
    """The C oracle filled from the case's table under the case's spec (or `spec`), its L set."""
    from oracle.c_oracle import COracle
    o = COracle(t.n_snps, t.band, **(desc["spec"] if spec is None else spec))
    o.fill(t)
    o.L = desc["L"] if L is None else L
    return o


def shape_of(o, n):
    """What the window offers, read off the oracle: dict(cm: the candidate bits over "ACGTN-_" per position (index 0: 0), U their
    union, S its bits, Le = min(L, N), states = S^Le as a Python int, however large)."""
    blank = np.full(n + 1, 6, dtype=np.uint8)
    cm = [0] + [int(o.edge_weights(p, blank)[0]) & 0x2F for p in range(1, n + 1)]      # (the set does not depend on the history)
    u = 0
    for m in cm:
        u |= m
    s = bin(u).count("1")
    le = min(o.L, n)
    return dict(cm=cm, U=u, S=s, Le=le, states=s ** le)


def references(desc, o, shape=None):
    """The four references on the oracle as it stands: dict(shape, over, vit, mm, kb, beam); beyond the cap only shape and over."""
    import beam_ref
    import kbest_ref
    import maxmarg_ref
    import viterbi_ref
    n, order = desc["N"], desc["spec"]["cand_order"]
    shape = shape_of(o, n) if shape is None else shape
    if shape["states"] > CAP:
        return dict(shape=shape, over=True)
    return dict(shape=shape, over=False, vit=viterbi_ref.viterbi(o, n, order), mm=maxmarg_ref.marginals(o, n),
                kb=kbest_ref.kbest(o, n, desc["K"], order), beam=beam_ref.beam(o, n, desc["width"], order))


# the committed list: tests/test_decode_cases_host.py states what it must cover
CASES = tuple(range(240))
FUZZ_FIRST_SEED = 100000   # tests/fuzz_decode_gpu.py starts beyond the list

# The panels of tests/test_gpu_decode_cases.py.  A panel's windows agree in storage, modes and candidate order, so a panel runs its
# windows' tables, L and K under ONE spec, chosen here on purpose: the panel copies of the walk statements are held to the references
# on FINITE scores under A, B and E, both storages and permuted orders; one panel keeps C, where with L >= 2 every score is +inf and
# the tie orders are what is compared.  Panel q takes the first PANEL served windows among seeds q, q + PANELS, q + 2 PANELS, ...
PANEL = 16
PANEL_SPECS = (
    dict(cond_mode="A", marginal_term=False, storage="f32", cand_order="ACGT-"),
    dict(cond_mode="B", marginal_term=True, storage="f32", cand_order="T-GCA"),
    dict(cond_mode="E", marginal_term=True, storage="f64", cand_order="-CATG"),
    dict(cond_mode="A", marginal_term=True, storage="f64", cand_order="ACGT-"),
    dict(cond_mode="E", marginal_term=False, storage="f32", cand_order="GAT-C"),
    dict(cond_mode="C", marginal_term=True, storage="f64", cand_order="CT-AG"),
)
PANELS = len(PANEL_SPECS)


def panel_windows(q, over):
    """[(desc under PANEL_SPECS[q], table)] of panel q; over(seed) -> True where the window lies beyond the cap (a panel call
    refuses as a whole on such a window, so it takes none)."""
    wins = []
    for seed in CASES[q::PANELS]:
        if len(wins) < PANEL and not over(seed):
            desc, t = case(seed)
            wins.append((dict(desc, spec=dict(PANEL_SPECS[q])), t))
    return wins
