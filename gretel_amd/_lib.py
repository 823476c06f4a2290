"""
ctypes binding of libgretel_hip.so (C ABI: include/gretel_hip.h).

There is NO CPU fallback: if the shared library is missing, or no HIP device is
visible when a handle is created, the product path raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("GH_LIB") or os.path.join(_HERE, "libgretel_hip.so")   # GH_LIB: alternative build (A/B experiments)

GH_OK = 0
GH_ERR_ARG, GH_ERR_HIP, GH_ERR_BAND, GH_ERR_SYMBOL, GH_ERR_NOMEM, GH_ERR_STATE = -1, -2, -3, -4, -5, -6
GH_STORAGE = {"f32": 0, "f64": 1}
GH_COND = {"A": 0, "B": 1, "C": 2, "D": 3, "E": 4}
GH_BEAM_MAX = 32
GH_VITERBI_MAX_STATES = 4096
GH_VITERBI_GRID_MAX_STATES = 1 << 24
GH_KBEST_MAX = 32
GH_MASKED_MAX_SETS = 256
GH_K = {"fill": 0, "marg": 1, "lt": 2, "walk": 3, "reweight": 4, "seg": 5, "rwseg": 6}
GH_FLOW = {0: "none", 1: "serial", 2: "seg", 3: "rwseg", 4: "fuse", 5: "pools"}      # gh_spin_plan.flow
GH_WALK = {"seg": 0, "spec": 1, "spec1": 2, "src": 3}                                # gh_spin_plan_in.walk_mode


class GretelHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libgretel_hip: %s (status %d)" % (msg, code))
        self.code = code


class BandError(GretelHipError, IndexError):
    pass


class SymbolError(GretelHipError, KeyError):
    pass


class gh_config(C.Structure):
    _fields_ = [("n_snps", C.c_int32), ("band", C.c_int32), ("storage", C.c_int32),
                ("cond_mode", C.c_int32), ("marginal_term", C.c_int32), ("device", C.c_int32),
                ("offer_zero", C.c_int32), ("cand_order", C.c_uint8 * 8)]


class gh_fill_stats(C.Structure):
    _fields_ = [("n_slices", C.c_int64), ("n_crumbs", C.c_int64), ("covered_snps", C.c_int64),
                ("L", C.c_int32), ("_pad", C.c_int32)]


class gh_path_rec(C.Structure):
    _fields_ = [("hp_current", C.c_double), ("hp_original", C.c_double),
                ("ratio", C.c_double), ("magnitude", C.c_double), ("min_marginal", C.c_double)]


class gh_assign_stats(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_informative", C.c_int64), ("n_unique", C.c_int64), ("n_ambiguous", C.c_int64),
                ("n_unexplained", C.c_int64)]


class gh_score_rec(C.Structure):
    _fields_ = [("ll_chain", C.c_double), ("hp_current", C.c_double), ("hp_original", C.c_double), ("min_marginal", C.c_double),
                ("min_margin", C.c_double), ("n_on", C.c_int32), ("n_greedy", C.c_int32), ("first_off", C.c_int32),
                ("argmin_margin", C.c_int32)]


class gh_spin_plan_in(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_snps", "band", "L", "storage", "cond_mode", "marginal_term", "offer_zero", "walk_mode", "lt_full", "need_rinfo",
        "pools_off", "ranked", "rwseg", "rwseg_small", "emit_small", "fuse", "seg6", "mixed", "rw_lp16", "rw_tband")]


class gh_spin_plan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("flow", "emit_small", "seg6", "stride", "rw_lanes", "S", "mixed", "need_layout")] + [
        ("lds", C.c_int64)]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n, _ in self._fields_}
        d["flow"] = GH_FLOW[d["flow"]]
        return d


_lib = None


def load():
    """Load libgretel_hip.so or raise -- never falls back to anything."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError(
            "gretel_amd: %s is missing. Build it with `make -C gretel_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback for the hot path." % SO_PATH)
    L = C.CDLL(SO_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    P = C.POINTER
    L.gh_last_error.restype = C.c_char_p
    L.gh_last_error.argtypes = []
    sigs = {
        "gh_device_count": [P(i32)],
        "gh_device_clock_khz": [i32, P(i32)],
        "gh_log10_device": [i32, vp, vp, C.c_int64],
        "gh_debug_segment_stamps": [vp, vp, i32],
        "gh_log10_host": [vp, vp, C.c_int64],
        "gh_create": [P(gh_config), P(vp)],
        "gh_destroy": [vp],
        "gh_copy": [vp, P(vp)],
        "gh_clear": [vp],
        "gh_sync": [vp],
        "gh_set_L": [vp, C.c_int32],
        "gh_get_L": [vp, P(C.c_int32)],
        "gh_get_fill_stats": [vp, P(gh_fill_stats)],
        "gh_set_fill_stats": [vp, P(gh_fill_stats)],
        "gh_reads_upload": [vp, vp, vp, vp, i64, P(vp)],
        "gh_reads_free": [vp],
        "gh_reads_max_k": [vp, P(i32)],
        "gh_reads_info": [vp, vp, vp],
        "gh_fill": [vp, vp, i32, P(gh_fill_stats)],
        "gh_add": [vp, i32, i32, i32, i32],
        "gh_add_batch": [vp, vp, vp, vp, vp, i64],
        "gh_get": [vp, i32, i32, i32, i32, P(dbl)],
        "gh_reweight_obs": [vp, i32, i32, i32, i32, dbl, P(dbl)],
        "gh_counts_at": [vp, i32, vp],
        "gh_marginal_of_at": [vp, i32, i32, P(dbl)],
        "gh_edge_weights_at": [vp, i32, vp, vp, P(i32)],
        "gh_gap_check": [vp, P(i32)],
        "gh_export_cmask": [vp, vp],
        "gh_snapshot_original": [vp],
        "gh_generate_path": [vp, vp, vp, P(dbl), P(dbl), P(dbl), P(i32)],
        "gh_reweight_path": [vp, vp, dbl, P(dbl)],
        "gh_spin": [vp, i32, dbl, vp, vp, P(i32), P(i32)],
        "gh_batch_create": [P(vp), i32, P(vp)],
        "gh_batch_destroy": [vp],
        "gh_batch_spin": [vp, i32, dbl, vp, vp, vp, vp],
        "gh_panel_create": [P(vp), i32, P(vp)],
        "gh_panel_spin": [vp, i32, dbl, vp, vp, vp, vp, vp],
        "gh_host_alloc": [C.c_size_t, P(vp)],
        "gh_host_free": [vp],
        "gh_batch_pipe_info": [vp, P(C.c_int32)],
        "gh_batch_profile_enable": [vp, i32],
        "gh_batch_profile_get": [vp, i32, P(dbl), P(i64), P(C.c_int32), P(dbl)],
        "gh_export_band": [vp, vp],
        "gh_import_band": [vp, vp],
        "gh_export_dense": [vp, vp],
        "gh_profile_enable": [vp, i32],
        "gh_profile_reset": [vp],
        "gh_profile_get": [vp, i32, P(dbl), P(i64)],
        "gh_profile_bytes": [vp, i32, P(dbl)],
        "gh_profile_overhead": [vp, i32, vp],
        "gh_debug_walk_clock": [vp, vp],
        "gh_debug_pool_geometry": [i32, i32, i32, vp],
        "gh_debug_spin_plan": [P(gh_spin_plan_in), P(gh_spin_plan)],
        "gh_debug_last_spin_plan": [vp, P(gh_spin_plan)],
        "gh_assign_reads": [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, P(gh_assign_stats)],
        "gh_score_paths": [vp, vp, i32, vp, vp, vp, vp],
        "gh_beam_paths": [vp, i32, vp, vp, P(i32), P(i32)],
        "gh_beam_spin": [vp, i32, i32, dbl, vp, vp, vp, P(i32), P(i32)],
        "gh_beam_info": [vp, vp],
        "gh_viterbi_path": [vp, vp, P(dbl), P(i32)],
        "gh_viterbi_spin": [vp, i32, dbl, vp, vp, vp, P(i32), P(i32)],
        "gh_viterbi_info": [vp, vp],
        "gh_viterbi_states": [vp, vp],
        "gh_viterbi_path_grid": [vp, vp, P(dbl), P(i32)],
        "gh_viterbi_spin_grid": [vp, i32, dbl, vp, vp, vp, P(i32), P(i32)],
        "gh_viterbi_grid_info": [vp, vp],
        "gh_viterbi_marginals": [vp, vp, vp, P(i32)],
        "gh_viterbi_marginals_grid": [vp, vp, vp, P(i32)],
        "gh_viterbi_kbest": [vp, i32, vp, vp, P(i32), P(i32)],
        "gh_viterbi_path_masked": [vp, vp, i32, vp, vp, vp],
        "gh_viterbi_masked_info": [vp, vp],
        "gh_panel_viterbi_spin": [vp, i32, dbl, vp, vp, vp, vp, vp, vp],
        "gh_panel_viterbi_info": [vp, vp],
        "gh_panel_viterbi_marginals": [vp, vp, vp, vp, vp],
        "gh_panel_viterbi_marginals_info": [vp, vp],
        "gh_panel_viterbi_kbest": [vp, vp, vp, vp, vp, vp, vp, vp],
        "gh_panel_viterbi_kbest_info": [vp, vp],
        "gh_debug_panel_viterbi_phases": [i32, vp],
        "gh_coverage_sites": [i32, vp, vp, vp, i64, C.c_int32, C.c_int32, C.c_int32, vp, vp],
    }
    for name, args in sigs.items():
        fn = getattr(L, name)          # AttributeError if the ABI drifted
        fn.restype = C.c_int
        fn.argtypes = args
    _lib = L
    return L


def check(rc):
    if rc == GH_OK:
        return
    msg = load().gh_last_error().decode("utf-8", "replace")
    if rc == GH_ERR_BAND:
        raise BandError(rc, msg)
    if rc == GH_ERR_SYMBOL:
        raise SymbolError(rc, msg)
    raise GretelHipError(rc, msg)


def spin_plan(n_snps, band, L, storage="f32", cond_mode="A", marginal_term=False, offer_zero=False, walk="seg", lt_full=False,
              need_rinfo=None, pools_off=False, ranked=-1, **switches):
    """Which kernels a gh_spin of such a window would run for every path (gh_debug_spin_plan: no handle, no GPU), as a dict.
    switches: rwseg, rwseg_small, emit_small, fuse, seg6, mixed, rw_lp16, rw_tband -- the value of GH_<NAME>, unset when left out.
    need_rinfo defaults to what gh_create makes of marginal_term and fuse."""
    names = ("rwseg", "rwseg_small", "emit_small", "fuse", "seg6", "mixed", "rw_lp16", "rw_tband")
    bad = set(switches) - set(names)
    if bad:
        raise TypeError("spin_plan: unknown switches %s" % sorted(bad))
    if need_rinfo is None:
        need_rinfo = bool(marginal_term) or switches.get("fuse", 0) >= 1
    inp = gh_spin_plan_in(int(n_snps), int(band), int(L), GH_STORAGE[storage], GH_COND[cond_mode], int(marginal_term), int(offer_zero),
                          GH_WALK[walk], int(lt_full), int(need_rinfo), int(pools_off), int(ranked),
                          *[int(switches.get(n, -1)) for n in names])
    out = gh_spin_plan()
    check(load().gh_debug_spin_plan(C.byref(inp), C.byref(out)))
    return out.as_dict()


def device_clock_khz(device=-1):
    k = C.c_int(0)
    check(load().gh_device_clock_khz(int(device), C.byref(k)))
    return k.value


def log10_many(x, device=None):
    """log10 as the kernels evaluate it (include/gh_detlog.h): on the GPU `device`, or (None) the same source on the host."""
    import numpy as np
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    if device is None:
        check(load().gh_log10_host(x.ctypes.data, y.ctypes.data, x.size))
    else:
        check(load().gh_log10_device(int(device), x.ctypes.data, y.ctypes.data, x.size))
    return y


def device_count():
    n = C.c_int(0)
    check(load().gh_device_count(C.byref(n)))
    return n.value
