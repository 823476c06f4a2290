"""The per-cell protocol between Gretel's two hot functions and a `Hansel`, recorded call by call.

    Recorder                a proxy that logs every protocol call of a Hansel (any implementation)
    run_flow                the recovery loop of gretel/cmd.py:148-179 over recorded Hansels
    load_reference_gretel   the reference's own gretel/gretel.py, executed from its tree at run time
    first_divergence        where two traces part, for assertion messages
    pack_trace / unpack_trace, load_cases, oracle_for, fill_per_cell
                            tests/golden/reference_flow.json (written by tests/golden/make_reference_flow.py)

A trace is a list of tuples.  Doubles are `float.hex()` strings, symbols `str(symbol)`, so that traces of
`oracle.hansel_ref.Hansel` and of the device class compare equal with `==` (a NaN equals a NaN: both are 'nan'):

    ("copy", (), None)
    ("add_observation", (a, b, i, j), None)
    ("get_edge_weights_at", (pos, path string), ((symbol, weight), ...))      keys in the dict's ITERATION order
    ("get_marginal_of_at", (symbol, pos), value)
    ("get_counts_at", (pos,), ((key, value), ...))                            in iteration order, "total" included
    ("reweight_observation", (a, b, i, j, ratio), removed)
    ("path", string, hp_current, hp_original, min_marginal, size)             appended by run_flow after every path
    ("hole",)                                                                 ... or when generate_path gave None

Nothing of the reference's program text is in this file: load_reference_gretel reads it where it lies.  It serves the
fixture's generator and the live CPU test only -- no GPU test may call it.
"""
import contextlib
import importlib.util
import io
import json
import os
import re
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_flow.json")
REFERENCE_ENV = "GRETEL_REFERENCE_ROOT"

RECORDED = ("add_observation", "get_edge_weights_at", "get_marginal_of_at", "reweight_observation", "get_counts_at", "copy")


def fhex(x):
    return float(x).hex()


class Recorder:
    """Forwards everything to `hansel`; appends (method, normalised args, result) to `log` for the calls in RECORDED.
    copy() returns a Recorder over the copy that shares the log."""

    def __init__(self, hansel, log):
        object.__setattr__(self, "_rec_h", hansel)
        object.__setattr__(self, "_rec_log", log)

    def __getattr__(self, name):
        return getattr(self._rec_h, name)

    def __setattr__(self, name, value):
        setattr(self._rec_h, name, value)

    def _sym(self, s):
        if isinstance(s, int) or type(s).__name__.startswith(("int", "uint")):
            return str(self._rec_h.symbols[int(s)])
        return str(s)

    def add_observation(self, symbol_from, symbol_to, pos_from, pos_to):
        r = self._rec_h.add_observation(symbol_from, symbol_to, pos_from, pos_to)
        self._rec_log.append(("add_observation", (self._sym(symbol_from), self._sym(symbol_to), int(pos_from), int(pos_to)), None))
        return r

    def get_edge_weights_at(self, at_pos, current_path, **kw):
        r = self._rec_h.get_edge_weights_at(at_pos, current_path, **kw)
        self._rec_log.append(("get_edge_weights_at", (int(at_pos), "".join(self._sym(s) for s in current_path)),
                              tuple((str(k), fhex(v)) for k, v in r.items())))
        return r

    def get_marginal_of_at(self, of_symbol, at_pos):
        r = self._rec_h.get_marginal_of_at(of_symbol, at_pos)
        self._rec_log.append(("get_marginal_of_at", (self._sym(of_symbol), int(at_pos)), fhex(r)))
        return r

    def reweight_observation(self, symbol_from, symbol_to, pos_from, pos_to, ratio):
        r = self._rec_h.reweight_observation(symbol_from, symbol_to, pos_from, pos_to, ratio)
        self._rec_log.append(("reweight_observation", (self._sym(symbol_from), self._sym(symbol_to), int(pos_from), int(pos_to),
                                                       fhex(ratio)), fhex(r)))
        return r

    def get_counts_at(self, at_pos):
        r = self._rec_h.get_counts_at(at_pos)
        self._rec_log.append(("get_counts_at", (int(at_pos),), tuple((str(k), fhex(v)) for k, v in r.items())))
        return r

    def copy(self):
        c = self._rec_h.copy()
        self._rec_log.append(("copy", (), None))
        return Recorder(c, self._rec_log)


def run_flow(mod, hansel, n_snps, max_paths, min_remove=0.01):
    """The loop of gretel/cmd.py:148-179 -- `original = hansel.copy()` (cmd.py:79), then per path generate_path, the stop on
    None, the 1 % clamp and reweight_hansel_from_path -- with `hansel` and the copy wrapped in Recorders that share one log.
    `mod` is any module with the two functions (the reference's gretel/gretel.py, oracle.gretel_ref, ...).

    That loop lives inside the reference's main() behind pysam and cannot be executed here; this RESTATES lines 148-179
    (without the PATHS bookkeeping and the loop's own "[RWGT] Ratio ... too small" note).  Returns (log, stderr the
    functions wrote)."""
    log = []
    err = io.StringIO()
    h = Recorder(hansel, log)
    with contextlib.redirect_stderr(err):
        original = h.copy()
        for _ in range(max_paths):
            path, prob, mn = mod.generate_path(n_snps, h, original)
            if path is None:
                log.append(("hole",))
                break
            ratio = mn
            if ratio < min_remove:
                ratio = min_remove
            size = mod.reweight_hansel_from_path(h, path, ratio)
            log.append(("path", "".join(str(x) for x in path), fhex(prob["hp_current"]), fhex(prob["hp_original"]), fhex(mn),
                        fhex(size)))
    return log, err.getvalue()


def reference_root():
    """$GRETEL_REFERENCE_ROOT, or where SURVEY.md's title says the reference lies."""
    env = os.environ.get(REFERENCE_ENV)
    if env:
        return env
    with open(os.path.join(ROOT, "SURVEY.md")) as fh:
        m = re.search(r"reference at `([^`]+)`", fh.readline())
    return m.group(1) if m else ""


def reference_present(root=None):
    return os.path.isfile(os.path.join(root or reference_root(), "gretel", "gretel.py"))


def load_reference_gretel(root=None):
    """Executes <root>/gretel/gretel.py as module `gretel.gretel` and returns it.  That file imports `hansel.Hansel` (a name
    it never calls) and `from . import util` (which the two hot functions do not use; util.py needs pysam): stub modules
    stand in for `gretel`, `gretel.util` and `hansel` while it loads, and sys.modules is put back afterwards."""
    from oracle import hansel_ref
    root = root or reference_root()
    src = os.path.join(root, "gretel", "gretel.py")
    if not os.path.isfile(src):
        raise FileNotFoundError(src)
    names = ("gretel", "gretel.util", "gretel.gretel", "hansel")
    saved = {k: sys.modules.get(k) for k in names}
    pkg = types.ModuleType("gretel")
    pkg.__path__ = [os.path.join(root, "gretel")]
    util = types.ModuleType("gretel.util")
    pkg.util = util
    hz = types.ModuleType("hansel")
    hz.Hansel = hansel_ref.Hansel
    no_pyc = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        sys.modules.update({"gretel": pkg, "gretel.util": util, "hansel": hz})
        spec = importlib.util.spec_from_file_location("gretel.gretel", src)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["gretel.gretel"] = mod
        spec.loader.exec_module(mod)
    finally:
        sys.dont_write_bytecode = no_pyc
        for k in names:
            if saved[k] is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = saved[k]
    return mod


def first_divergence(a, b):
    """None if the traces are equal, else (index, a's entry, b's entry) of the first difference (None past an end)."""
    for q in range(min(len(a), len(b))):
        if a[q] != b[q]:
            return q, a[q], b[q]
    if len(a) != len(b):
        q = min(len(a), len(b))
        return q, (a[q] if q < len(a) else None), (b[q] if q < len(b) else None)
    return None


def assert_same_trace(got, want, what=""):
    d = first_divergence(got, want)
    assert d is None, "%s: traces part at call %d of %d/%d:\n  got  %r\n  want %r" % (what, d[0], len(got), len(want), d[1], d[2])


# -- the fixture ------------------------------------------------------------------------------------------------------
_CODE = {"copy": "k", "add_observation": "a", "get_edge_weights_at": "e", "get_marginal_of_at": "m", "get_counts_at": "c",
         "reweight_observation": "r", "path": "p", "hole": "h"}
_NAME = {v: k for k, v in _CODE.items()}


def pack_trace(log):
    """A trace as JSON: `ops` (one letter per entry), `vals` (every distinct hex string once) and one flat list per method."""
    vals, index = [], {}

    def v(x):
        if x not in index:
            index[x] = len(vals)
            vals.append(x)
        return index[x]

    out = dict(ops="", vals=vals, a=[], e=[], m=[], c=[], r=[], p=[])
    for ent in log:
        c = _CODE[ent[0]]
        out["ops"] += c
        if c == "a":
            out["a"] += [ent[1][0] + ent[1][1], ent[1][2], ent[1][3]]
        elif c == "e":
            out["e"] += [ent[1][0], ent[1][1], ",".join(k for k, _ in ent[2])] + [v(x) for _, x in ent[2]]
        elif c == "m":
            out["m"] += [ent[1][0], ent[1][1], v(ent[2])]
        elif c == "c":
            out["c"] += [ent[1][0], ",".join(k for k, _ in ent[2])] + [v(x) for _, x in ent[2]]
        elif c == "r":
            out["r"] += [ent[1][0] + ent[1][1], ent[1][2], ent[1][3], v(ent[1][4]), v(ent[2])]
        elif c == "p":
            out["p"] += [ent[1]] + [v(x) for x in ent[2:]]
    return out


def unpack_trace(d):
    vals = d["vals"]
    it = {k: iter(d[k]) for k in "aemcrp"}
    log = []
    for c in d["ops"]:
        name = _NAME[c]
        if c in "kh":
            log.append((name, (), None) if c == "k" else (name,))
            continue
        n = it[c]
        if c == "a":
            ab = next(n)
            log.append((name, (ab[0], ab[1], next(n), next(n)), None))
        elif c == "e":
            pos, path, keys = next(n), next(n), next(n)
            keys = keys.split(",") if keys else []
            log.append((name, (pos, path), tuple((k, vals[next(n)]) for k in keys)))
        elif c == "m":
            log.append((name, (next(n), next(n)), vals[next(n)]))
        elif c == "c":
            pos, keys = next(n), next(n)
            keys = keys.split(",") if keys else []
            log.append((name, (pos,), tuple((k, vals[next(n)]) for k in keys)))
        elif c == "r":
            ab = next(n)
            log.append((name, (ab[0], ab[1], next(n), next(n), vals[next(n)]), vals[next(n)]))
        elif c == "p":
            log.append((name, next(n)) + tuple(vals[next(n)] for _ in range(4)))
    return log


def load_cases():
    with open(FIXTURE) as fh:
        return json.load(fh)["cases"]


def case_observations(case):
    """[(a, b, i, j), ...] in the order and with the multiplicity the case's window was filled in."""
    o = case["obs"]
    out = []
    for q in range(len(o["syms"]) // 2):
        out += [(o["syms"][2 * q], o["syms"][2 * q + 1], o["pos"][3 * q], o["pos"][3 * q + 1])] * o["pos"][3 * q + 2]
    return out


def fill_per_cell(h, case):
    """add_observation only, then the attributes as gretel/util.py:329-333 sets them."""
    for ob in case_observations(case):
        h.add_observation(*ob)
    h.n_slices = case["n_slices"]
    h.n_crumbs = case["n_crumbs"]
    h.L = case["L"]
    return h


def oracle_for(case):
    """The Python oracle Hansel (dense, like the reference's) of a fixture case."""
    from oracle.hansel_ref import Hansel, HanselSpec, SYMBOLS, UNSYMBOLS
    return fill_per_cell(Hansel.init_matrix(SYMBOLS, UNSYMBOLS, case["n_snps"], HanselSpec(**case["spec"])), case)


def path_records(log):
    return [e for e in log if e[0] in ("path", "hole")]


def dense_to_band(dense, band):
    """[7][7][N+2][N+2] -> float64 [N+2][band][7][7] (export_band's layout); everything outside the band must be zero."""
    import numpy as np
    d = np.asarray(dense, dtype=np.float64)
    n2 = d.shape[2]
    out = np.zeros((n2, band, d.shape[0], d.shape[1]))
    rest = d.copy()
    for i in range(n2):
        for w in range(1, band + 1):
            if i + w < n2:
                out[i, w - 1] = d[:, :, i, i + w]
                rest[:, :, i, i + w] = 0
    assert not rest.any(), "cells outside the band of %d are set" % band
    return out
