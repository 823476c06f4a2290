"""The read assignment of gh_assign_reads (INTEGRATION.md "Read assignment") stated in plain numpy, for the tests only.

Column j of read r lies at SNP rank[r] + j + 1.  It is informative when its symbol is one of A C G T - and the SNP lies in
1..N.  I = informative columns, m_h = those where haplotype h carries the read's symbol, best = max_h m_h (0 without
haplotypes), T = the haplotypes that reach best.  In this order: I < min_snps -> uninformative (-1); no haplotype, or
max_mismatch >= 0 and I - best > max_mismatch -> unexplained (-3); |T| > 1 -> ambiguous (-2, shared[h] += 1 for h in T);
else unique (hap = h, unique[h] += 1, mismatches[h] += I - best).
"""
import numpy as np

SYMBOLS = "ACGTN-_"
# support byte -> symbol index; -1: not a symbol
_LUT = np.full(256, -1, dtype=np.int16)
for _q, _c in enumerate(SYMBOLS):
    _LUT[ord(_c)] = _q


def path_indices(s):
    """'_ACG-' -> uint8 symbol indices (a path row: index 0 is the '_' sentinel)."""
    return np.array([SYMBOLS.index(c) for c in s], dtype=np.uint8)


def assign(rank, off, bases, paths, n_snps, min_snps=2, max_mismatch=-1, col_budget=1 << 23):
    """Returns the dict Hansel.assign_reads(..., per_read=True) returns.  Reads go in chunks of about col_budget column x haplotype
    cells, so that a million reads against a hundred haplotypes take seconds."""
    rank = np.asarray(rank, dtype=np.int64)
    off = np.asarray(off, dtype=np.int64)
    bases = np.asarray(bases, dtype=np.uint8)
    paths = np.asarray(paths, dtype=np.uint8).reshape(-1, n_snps + 1)
    H = paths.shape[0]
    n = len(rank)
    sym = _LUT[bases]
    if (sym < 0).any():
        raise ValueError("a read holds a byte outside ACGTN-_")
    cols = paths.T                                                  # [N+1][H]
    hap = np.zeros(n, dtype=np.int32)
    best = np.zeros(n, dtype=np.int32)
    inf = np.zeros(n, dtype=np.int32)
    unique = np.zeros(H, dtype=np.int64)
    shared = np.zeros(H, dtype=np.int64)
    mism = np.zeros(H, dtype=np.int64)
    a = 0
    while a < n:
        # reads [a, b): as many as keep (columns x H) under the budget, at least one
        b = a + 1
        per = max(1, H)
        lim = off[a] + max(1, col_budget // per)
        b = max(a + 1, int(np.searchsorted(off, lim, side="right")) - 1)
        b = min(b, n)
        o = off[a:b + 1] - off[a]
        k = np.diff(o)
        read_of = np.repeat(np.arange(b - a), k)
        j = np.arange(int(o[-1])) - o[read_of]
        snp = rank[a:b][read_of] + 1 + j
        s = sym[off[a]:off[b]]
        ok = np.isin(s, (0, 1, 2, 3, 5)) & (snp >= 1) & (snp <= n_snps)
        I = np.bincount(read_of[ok], minlength=b - a).astype(np.int64)
        if H:
            eq = (cols[np.where(ok, snp, 0)] == s[:, None]) & ok[:, None]          # [columns][H]
            cs = np.zeros((len(s) + 1, H), dtype=np.int32)
            np.cumsum(eq, axis=0, out=cs[1:])
            m = cs[o[1:]] - cs[o[:-1]]                                               # [reads][H] matches
            bst = m.max(axis=1)
            tie = m == bst[:, None]
            nt = tie.sum(axis=1)
            lo = np.argmax(m, axis=1)
        else:
            bst = np.zeros(b - a, dtype=np.int64)
            nt = np.zeros(b - a, dtype=np.int64)
            lo = np.zeros(b - a, dtype=np.int64)
        h = np.where(nt > 1, -2, lo)
        if H == 0:
            h[:] = -3
        elif max_mismatch >= 0:
            h = np.where(I - bst > max_mismatch, -3, h)
        h = np.where(I < min_snps, -1, h)
        u = h >= 0
        unique += np.bincount(h[u], minlength=H).astype(np.int64)
        mism += np.bincount(h[u], weights=(I - bst)[u], minlength=H).astype(np.int64)
        if H:
            shared += tie[h == -2].sum(axis=0).astype(np.int64)
        hap[a:b], best[a:b], inf[a:b] = h, bst, I
        a = b
    return dict(unique=unique, shared=shared, mismatches=mism, n_reads=n, n_informative=int((inf >= min_snps).sum()),
                n_unique=int((hap >= 0).sum()), n_ambiguous=int((hap == -2).sum()), n_unexplained=int((hap == -3).sum()),
                hap=hap, best=best, informative=inf)


def render(i0s, res):
    """gretel.support for haplotypes with ids i0s (in that order) and the result res."""
    out = "# %d\t%d\t%d\t%d\t%d\n" % (res["n_reads"], res["n_informative"], res["n_unique"], res["n_ambiguous"], res["n_unexplained"])
    for q, i0 in enumerate(i0s):
        u = int(res["unique"][q])
        frac = u / res["n_unique"] if res["n_unique"] else 0.0
        out += "%d\t%d\t%d\t%d\t%.4f\n" % (i0, u, int(res["shared"][q]), int(res["mismatches"][q]), frac)
    return out


def table(reads):
    """[(rank, 'ACG..'), ...] -> (rank int32, off int64, bases uint8)."""
    rank = np.array([r for r, _ in reads], dtype=np.int32)
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(s) for _, s in reads], out=off[1:])
    bases = np.frombuffer("".join(s for _, s in reads).encode(), dtype=np.uint8).copy()
    return rank, off, bases
