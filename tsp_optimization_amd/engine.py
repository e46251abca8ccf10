"""ctypes binding of include/tsp_hip.h (libtsp_hip.so).  No fallback of any kind: if the library
is missing or no MI355X is visible the calls raise."""
import ctypes as C
import os

import numpy as np

from .build import lib_path

EUC_2D, MAX_2D, MAN_2D, CEIL_2D, GEO, ATT = 0, 1, 2, 3, 4, 5
FIRST, BEST = 0, 1
GREEDY, GRASP = 0, 1
ENGINE_AUTO, ENGINE_GRID, ENGINE_LDS, ENGINE_CLUSTER = 0, 1, 2, 3
OK, WRONG_STARTING_NODE, TIME_LIMIT_EXCEEDED = 0, 1, 2
E_ARG = -3
E_NOT_A_TOUR, E_INTERNAL = -4, -7
NL_2OPT, NL_OROPT = 1, 2
NL_3OPT = 4   # tsp_dev_nl_3opt and what builds on it, and seg_ils3
DLB_OFF, DLB_ON, DLB_CLOSE = 0, 1, 2   # don't-look bits of nl_3opt and ils
NL_BATCH_DEFAULT_ROUNDS = 2            # claim rounds of nl_3opt_batch (TSP_NL_BATCH_DEFAULT_ROUNDS)
NL_MAX_K, NL_DEFAULT_K = 16, 10
SEG_ILS_MAX_WINDOW, SEG_ILS_DEFAULT_WINDOW = 2048, 1024   # windows of seg_ils (TSP_SEG_ILS_MAX_WINDOW, _DEFAULT_WINDOW)
SEG_ILS_MAX_GROUPS = 64                                   # groups per window of seg_ils_groups (TSP_SEG_ILS_MAX_GROUPS)
NL_LK = 8                                                 # the chain kind of seg_ils_lk (TSP_NL_LK)
SEG_LK_MAX_DEPTH, SEG_LK_DEFAULT_DEPTH = 16, 16           # steps of a chain (TSP_SEG_LK_MAX_DEPTH, _DEFAULT_DEPTH)
HK_DEFAULT_ITERS, HK_DEFAULT_LAMBDA = 300, 2.0
ALPHA_DEFAULT_K = 5


class TspDeviceError(RuntimeError):
    pass


class _Stats(C.Structure):
    """What every stats structure below is: as_dict() has its fields by name, the array fields as lists."""

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        return {k: list(v) if isinstance(v, C.Array) else v for k, v in d.items()}


class Stats(_Stats):
    _fields_ = [("sweeps", C.c_int64), ("evals", C.c_int64), ("moves", C.c_int64),
                ("reversed", C.c_int64), ("pairs_scanned", C.c_int64), ("steps", C.c_int64),
                ("seconds", C.c_double), ("device_ms", C.c_double),
                ("lane_pairs", C.c_int64), ("tier1_pairs", C.c_int64), ("exact_pairs", C.c_int64),
                ("staged_recs", C.c_int64)]


class OrOptStats(_Stats):
    _fields_ = [("sweeps", C.c_int64), ("evals", C.c_int64), ("moves", C.c_int64), ("moves_by_len", C.c_int64 * 3),
                ("moves_reversed", C.c_int64), ("deltas_executed", C.c_int64), ("rounds", C.c_int64),
                ("seconds", C.c_double), ("device_ms", C.c_double)]


class NlOptStats(_Stats):
    _fields_ = [("decisions", C.c_int64), ("moves", C.c_int64), ("moves_2opt", C.c_int64), ("moves_oropt", C.c_int64),
                ("moves_by_len", C.c_int64 * 3), ("moves_reversed", C.c_int64), ("reversed", C.c_int64),
                ("deltas_executed", C.c_int64), ("seconds", C.c_double), ("device_ms", C.c_double)]


class Nl3OptStats(_Stats):
    _fields_ = NlOptStats._fields_ + [("moves_3opt", C.c_int64), ("moves_by_type", C.c_int64 * 4)]


class IlsStats(_Stats):
    _fields_ = Nl3OptStats._fields_ + [("iterations", C.c_int64), ("accepted", C.c_int64), ("last_improved", C.c_int64),
                                       ("start_cost", C.c_double)]


class NlDlbStats(_Stats):
    _fields_ = Nl3OptStats._fields_ + [("active_nodes", C.c_int64), ("closing_scans", C.c_int64)]


class IlsDlbStats(_Stats):
    _fields_ = IlsStats._fields_ + [("active_nodes", C.c_int64), ("closing_scans", C.c_int64)]


class SegIlsStats(_Stats):
    _fields_ = NlOptStats._fields_ + [("iterations", C.c_int64), ("windows", C.c_int64), ("trials", C.c_int64),
                                      ("accepted", C.c_int64), ("active_nodes", C.c_int64), ("start_cost", C.c_double)]


class SegIls3Stats(_Stats):
    _fields_ = SegIlsStats._fields_ + [("moves_3opt", C.c_int64), ("moves_by_type", C.c_int64 * 4)]


class SegIlsGroupsStats(_Stats):
    _fields_ = SegIls3Stats._fields_ + [("groups", C.c_int64), ("offers", C.c_int64), ("commits", C.c_int64)]


class SegIlsLkStats(_Stats):
    _fields_ = SegIlsGroupsStats._fields_ + [("lk_depth", C.c_int64), ("moves_lk", C.c_int64), ("lk_flips", C.c_int64),
                                             ("lk_chains", C.c_int64), ("lk_steps", C.c_int64)]


class LbStats(_Stats):
    _fields_ = [("iterations", C.c_int64), ("trees", C.c_int64), ("rounds", C.c_int64), ("dists_executed", C.c_int64),
                ("tour_found", C.c_int), ("lambda_final", C.c_double), ("seconds", C.c_double), ("device_ms", C.c_double)]


class LbSparseStats(_Stats):
    _fields_ = LbStats._fields_ + [("sparse_iterations", C.c_int64), ("sparse_trees", C.c_int64), ("sparse_rounds", C.c_int64),
                                   ("completion_rounds", C.c_int64), ("candidate_entries", C.c_int64), ("components", C.c_int64),
                                   ("weights_executed", C.c_int64), ("sparse_best", C.c_double),
                                   ("lambda_sparse_final", C.c_double), ("sparse_device_ms", C.c_double)]


class AlphaStats(_Stats):
    _fields_ = [("trees", C.c_int64), ("rounds", C.c_int64), ("pairs_executed", C.c_int64), ("tree_value", C.c_double),
                ("seconds", C.c_double), ("device_ms", C.c_double)]


class GreedyEdgeStats(_Stats):
    _fields_ = [("rounds", C.c_int64), ("edges", C.c_int64), ("rows_scanned", C.c_int64), ("dists_executed", C.c_int64),
                ("max_edges_in_round", C.c_int64), ("seconds", C.c_double), ("device_ms", C.c_double)]


class GpxStats(_Stats):
    _fields_ = [("common_edges", C.c_int64), ("components", C.c_int64), ("exchangeable", C.c_int64), ("taken", C.c_int64),
                ("stretches", C.c_int64), ("gain_q", C.c_int64), ("rounds", C.c_int64), ("base", C.c_int),
                ("cost_a", C.c_double), ("cost_b", C.c_double), ("cost_child", C.c_double),
                ("seconds", C.c_double), ("device_ms", C.c_double)]


_lib = None


def lib():
    """Loads libtsp_hip.so; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise TspDeviceError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
        L = C.CDLL(path)
        vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
        sp = C.POINTER(Stats)
        L.tsp_dev_last_error.restype = C.c_char_p
        L.tsp_dev_open.argtypes = [C.c_int, C.POINTER(vp)]
        L.tsp_dev_close.argtypes = [vp]
        L.tsp_dev_close.restype = None
        L.tsp_dev_synchronize.argtypes = [vp]
        L.tsp_dev_stream.argtypes = [vp]
        L.tsp_dev_stream.restype = vp
        L.tsp_dev_inst_create.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.tsp_dev_inst_destroy.argtypes = [vp]
        L.tsp_dev_inst_destroy.restype = None
        L.tsp_dev_inst_size.argtypes = [vp]
        L.tsp_dev_inst_reload_switches.argtypes = [vp]
        L.tsp_dev_dist_pairs.argtypes = [vp, ip, ip, C.c_int, dp]
        L.tsp_dev_selftest_raw_sqrt.argtypes = [vp, dp, C.c_int, dp]
        L.tsp_dev_dist_matrix.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_float)]
        L.tsp_dev_construct.argtypes = [vp, C.c_int, C.c_int, ip, dp, ip, C.c_int, C.c_int64, dp, ip]
        L.tsp_dev_construct_describe.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
        L.tsp_dev_extramileage.argtypes = [vp, ip, C.c_int, dp]
        L.tsp_dev_two_opt.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, C.c_int64, dp,
                                      C.c_double, sp]
        L.tsp_dev_tabu_create.argtypes = [vp, C.POINTER(vp)]
        L.tsp_dev_tabu_destroy.argtypes = [vp]
        L.tsp_dev_tabu_destroy.restype = None
        L.tsp_dev_tabu_set.argtypes = [vp, ip, ip, C.c_int]
        L.tsp_dev_tabu_get.argtypes = [vp, ip, ip, C.c_int]
        L.tsp_dev_tabu_upload.argtypes = [vp, ip]
        L.tsp_dev_tabu_download.argtypes = [vp, ip]
        L.tsp_dev_tabu_list_info.argtypes = [vp, ip, ip]
        L.tsp_dev_two_opt_tabu.argtypes = [vp, vp, C.c_int, C.c_int, ip, C.c_int, dp, ip, C.c_double, sp]
        L.tsp_dev_perm_cost.argtypes = [vp, C.c_int, ip, C.c_int64, dp]
        L.tsp_dev_tours_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
        L.tsp_dev_tours_destroy.argtypes = [vp]
        L.tsp_dev_tours_destroy.restype = None
        L.tsp_dev_tours_upload.argtypes = [vp, ip, C.c_int, C.c_int64, dp]
        L.tsp_dev_tours_reset.argtypes = [vp]
        L.tsp_dev_tours_download.argtypes = [vp, ip, C.c_int, C.c_int64, dp, sp]
        L.tsp_dev_tours_run.argtypes = [vp, C.c_int, C.c_int64, C.c_double, C.c_int, ip]
        L.tsp_dev_tours_run_engine.argtypes = [vp, C.c_int, C.c_int, C.c_int64, C.c_double, ip]
        L.tsp_dev_tours_two_opt.argtypes = [vp, C.c_int, C.c_int, C.c_double, dp]
        L.tsp_dev_tours_two_opt_tabu.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, dp]
        L.tsp_dev_tours_tabu_kick.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, ip]
        L.tsp_dev_tours_tabu_iteration.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, dp, dp, ip, ip]
        L.tsp_dev_tours_tabu_iterations.argtypes = [vp, vp, C.c_int, C.c_int, ip, ip, C.c_double, dp, dp, ip, ip, ip]
        L.tsp_dev_tours_tabu_iterations_ex.argtypes = [vp, vp, C.c_int, C.c_int, ip, C.c_int, ip, C.c_double, dp, dp, ip, ip, ip, ip]
        L.tsp_dev_tours_vns_kick.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
        L.tsp_dev_tours_snapshot.argtypes = [vp]
        L.tsp_dev_tours_restore.argtypes = [vp]
        L.tsp_dev_tours_time_scan.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)]
        L.tsp_dev_tours_describe.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
        L.tsp_dev_inst_lds_variant.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
        L.tsp_dev_tours_device_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.tsp_dev_tours_best.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
        L.tsp_dev_comm_last_error.restype = C.c_char_p
        L.tsp_dev_comm_unique_id.argtypes = [C.c_char_p]
        L.tsp_dev_comm_init_rank.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.POINTER(vp)]
        L.tsp_dev_comm_init_all.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp)]
        L.tsp_dev_comm_destroy.argtypes = [vp]
        L.tsp_dev_comm_destroy.restype = None
        L.tsp_dev_comm_info.argtypes = [vp, ip, ip, ip]
        L.tsp_dev_multistart_pack.argtypes = [C.c_double, C.c_int, C.POINTER(C.c_int64)]
        L.tsp_dev_multistart_allreduce.argtypes = [vp, C.c_int64, C.POINTER(C.c_int64)]
        L.tsp_dev_multistart_allreduce_f64.argtypes = [vp, C.c_double, C.POINTER(C.c_double)]
        L.tsp_dev_multistart_allreduce_f64_group.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.tsp_dev_multistart_bcast_tour.argtypes = [vp, C.c_int, ip, C.c_int, C.c_int]
        L.tsp_dev_multistart_allreduce_group.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.tsp_dev_multistart_bcast_tour_group.argtypes = [C.POINTER(vp), C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, ip]
        orp = C.POINTER(OrOptStats)
        L.tsp_dev_or_opt.argtypes = [vp, C.c_int, ip, C.c_int, C.c_int64, dp, C.c_int64, C.c_double, orp]
        L.tsp_dev_two_opt_or_opt.argtypes = [vp, C.c_int, C.c_int, ip, C.c_int, C.c_int64, dp, C.c_double, sp, orp]
        L.tsp_dev_inst_knn_build.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
        L.tsp_dev_inst_knn_set.argtypes = [vp, C.c_int, ip]
        L.tsp_dev_inst_knn_get.argtypes = [vp, ip, ip]
        L.tsp_dev_nl_opt.argtypes = [vp, C.c_int, C.c_int, ip, C.c_int, C.c_int64, dp, C.c_int64, C.c_double, C.POINTER(NlOptStats)]
        L.tsp_dev_nl_3opt.argtypes = [vp, C.c_int, C.c_int, ip, C.c_int, C.c_int64, dp, C.c_int64, C.c_double, C.POINTER(Nl3OptStats)]
        L.tsp_dev_ils.argtypes = [vp, C.c_int, C.c_int, ip, C.c_int, C.c_int64, dp, C.c_uint64, C.c_int64, C.c_int, C.c_int64,
                                  C.c_double, C.POINTER(IlsStats)]
        L.tsp_dev_ils_kick.argtypes = [vp, C.c_int, ip, C.c_int, C.c_int64, C.c_uint64, C.c_int64, C.c_int]
        L.tsp_dev_nl_3opt_dlb.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, C.c_int64, dp, C.POINTER(C.c_ubyte), C.c_int64,
                                          C.c_double, C.POINTER(NlDlbStats)]
        L.tsp_dev_ils_dlb.argtypes = [vp, C.c_int, C.c_int, ip, C.c_int, C.c_int64, dp, C.c_uint64, C.c_int64, C.c_int, C.c_int64,
                                      C.c_double, C.c_int, C.POINTER(IlsDlbStats)]
        L.tsp_dev_nl_3opt_batch.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int, C.c_int64, dp, C.c_int64, C.c_double,
                                            C.POINTER(Nl3OptStats)]
        L.tsp_dev_seg_ils.argtypes = [vp, C.c_int, C.c_int, ip, C.c_int, C.c_int64, dp, C.c_uint64, C.c_int64, C.c_int, C.c_int,
                                      C.c_int, C.c_int64, C.c_double, C.POINTER(SegIlsStats)]
        L.tsp_dev_seg_ils3.argtypes = L.tsp_dev_seg_ils.argtypes[:-1] + [C.POINTER(SegIls3Stats)]
        L.tsp_dev_seg_ils_groups.argtypes = ([vp, C.c_int, C.c_int] + L.tsp_dev_seg_ils.argtypes[2:-1]
                                             + [C.POINTER(SegIlsGroupsStats)])
        L.tsp_dev_seg_ils_lk.argtypes = ([vp, C.c_int, C.c_int, C.c_int] + L.tsp_dev_seg_ils.argtypes[2:-1]
                                         + [C.POINTER(SegIlsLkStats)])
        lbp = C.POINTER(LbStats)
        L.tsp_dev_one_tree.argtypes = [vp, dp, ip, ip, dp, lbp]
        L.tsp_dev_held_karp.argtypes = [vp, C.c_double, C.c_int, C.c_double, C.c_int, C.c_double, dp, dp, lbp]
        lsp = C.POINTER(LbSparseStats)
        L.tsp_dev_one_tree_sparse.argtypes = [vp, dp, ip, ip, dp, lsp]
        L.tsp_dev_held_karp_sparse.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, dp, dp, lsp]
        L.tsp_dev_inst_alpha_build.argtypes = [vp, C.c_int, dp, dp, C.POINTER(AlphaStats)]
        L.tsp_dev_alpha_rows.argtypes = [vp, dp, C.c_int, ip, dp]
        L.tsp_dev_greedy_edge.argtypes = [vp, ip, C.c_int, dp, ip, C.POINTER(GreedyEdgeStats)]
        L.tsp_dev_gpx.argtypes = [vp, C.c_int, ip, ip, C.c_int, C.c_int64, ip, dp, C.POINTER(GpxStats)]
        _lib = L
    return _lib


EXPORTED = [
    "tsp_dev_open", "tsp_dev_close", "tsp_dev_last_error", "tsp_dev_count", "tsp_dev_synchronize",
    "tsp_dev_stream", "tsp_dev_inst_create", "tsp_dev_inst_destroy", "tsp_dev_inst_size", "tsp_dev_inst_reload_switches",
    "tsp_dev_dist_pairs", "tsp_dev_selftest_raw_sqrt", "tsp_dev_dist_matrix", "tsp_dev_construct", "tsp_dev_construct_describe", "tsp_dev_extramileage", "tsp_dev_two_opt",
    "tsp_dev_tabu_create", "tsp_dev_tabu_destroy", "tsp_dev_tabu_set", "tsp_dev_tabu_get",
    "tsp_dev_tabu_upload", "tsp_dev_tabu_download", "tsp_dev_tabu_list_info", "tsp_dev_two_opt_tabu", "tsp_dev_perm_cost",
    "tsp_dev_tours_create", "tsp_dev_tours_destroy", "tsp_dev_tours_upload", "tsp_dev_tours_reset",
    "tsp_dev_tours_download", "tsp_dev_tours_run", "tsp_dev_tours_run_engine", "tsp_dev_tours_time_scan", "tsp_dev_tours_best", "tsp_dev_tours_describe", "tsp_dev_tours_device_ms",
    "tsp_dev_tours_two_opt", "tsp_dev_tours_two_opt_tabu", "tsp_dev_tours_tabu_kick", "tsp_dev_tours_tabu_iteration", "tsp_dev_tours_tabu_iterations", "tsp_dev_tours_tabu_iterations_ex", "tsp_dev_tours_vns_kick",
    "tsp_dev_tours_snapshot", "tsp_dev_tours_restore", "tsp_dev_host_register", "tsp_dev_host_unregister",
    "tsp_dev_comm_last_error", "tsp_dev_comm_available", "tsp_dev_comm_unique_id", "tsp_dev_comm_init_rank", "tsp_dev_comm_init_all", "tsp_dev_comm_destroy",
    "tsp_dev_comm_info", "tsp_dev_multistart_pack", "tsp_dev_multistart_allreduce", "tsp_dev_multistart_bcast_tour",
    "tsp_dev_multistart_allreduce_group", "tsp_dev_multistart_bcast_tour_group",
    "tsp_dev_multistart_allreduce_f64", "tsp_dev_multistart_allreduce_f64_group",
    "tsp_dev_or_opt", "tsp_dev_two_opt_or_opt",
    "tsp_dev_inst_knn_build", "tsp_dev_inst_knn_set", "tsp_dev_inst_knn_get", "tsp_dev_nl_opt", "tsp_dev_nl_3opt",
    "tsp_dev_ils", "tsp_dev_ils_kick", "tsp_dev_nl_3opt_dlb", "tsp_dev_ils_dlb",
    "tsp_dev_one_tree", "tsp_dev_held_karp",
    "tsp_dev_one_tree_sparse", "tsp_dev_held_karp_sparse",
    "tsp_dev_inst_alpha_build", "tsp_dev_alpha_rows",
    "tsp_dev_greedy_edge",
    "tsp_dev_nl_3opt_batch",
    "tsp_dev_seg_ils",
    "tsp_dev_seg_ils3",
    "tsp_dev_seg_ils_groups",
    "tsp_dev_seg_ils_lk",
    "tsp_dev_inst_lds_variant",
    "tsp_dev_gpx",
]

COMM_ID_BYTES = 128
E_COMM = -6


def _check(rc, allow=(OK,)):
    if rc in allow:
        return rc
    msg = lib().tsp_dev_last_error().decode()
    if rc == E_COMM:
        msg = lib().tsp_dev_comm_last_error().decode() + " " + msg
    raise TspDeviceError("tsp_dev call failed with %d %s" % (rc, msg))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _obj(obj, B):
    """the obj argument of a call on B tours: zeros, or the caller's value(s) as a [B] array of the call's own"""
    if obj is None:
        return np.zeros(B, dtype=np.float64)
    return np.array(np.broadcast_to(np.asarray(obj, dtype=np.float64), (B,)), copy=True)


def _result(rc, single, succ2, o, *stats):
    """-> (status, succ', obj', one list of stats dicts per stats array); for a single tour its own row of each"""
    _check(rc, allow=(OK, TIME_LIMIT_EXCEEDED))
    dicts = tuple([s.as_dict() for s in st] for st in stats)
    if single:
        return (rc, succ2[0], float(o[0])) + tuple(d[0] for d in dicts)
    return (rc, succ2, o) + dicts


def device_count():
    return lib().tsp_dev_count()


class Context:
    """One device + the engine's stream (tsp_dev_open)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(lib().tsp_dev_open(device, C.byref(self._h)))
        self.device = device

    def synchronize(self):
        _check(lib().tsp_dev_synchronize(self._h))

    def raw_sqrt(self, x):
        """The hardware's approximate v_sqrt_f64 (self-test of the integer-root variants' premise)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        _check(lib().tsp_dev_selftest_raw_sqrt(self._h, _d(x), len(x), _d(out)))
        return out

    def close(self):
        if self._h:
            lib().tsp_dev_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Instance:
    """Node coordinates resident in HBM (tsp_dev_inst_create)."""

    def __init__(self, ctx, xy, wtype, integer_cost=1):
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        assert xy.ndim == 2 and xy.shape[1] == 2
        self.ctx, self.n, self.wtype, self.integer_cost = ctx, len(xy), wtype, integer_cost
        self._h = C.c_void_p()
        _check(lib().tsp_dev_inst_create(ctx._h, _d(xy), self.n, wtype, integer_cost, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().tsp_dev_inst_destroy(self._h)
            self._h = C.c_void_p()

    def reload_switches(self):
        """Re-read the TSP_* environment switches for this instance (they are read once, at creation)."""
        _check(lib().tsp_dev_inst_reload_switches(self._h))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- calc_dist ------------------------------------------------------------------------
    def dist_pairs(self, i, j):
        i = np.ascontiguousarray(i, dtype=np.int32)
        j = np.ascontiguousarray(j, dtype=np.int32)
        out = np.empty(len(i), dtype=np.float64)
        _check(lib().tsp_dev_dist_pairs(self._h, _i(i), _i(j), len(i), _d(out)))
        return out

    def dist_matrix(self, as_int32=False, fetch=True):
        """-> (matrix or None, kernel_ms)"""
        n = self.n
        out = np.empty((n, n), dtype=np.int32 if as_int32 else np.float64) if fetch else None
        ms = C.c_float(0)
        _check(lib().tsp_dev_dist_matrix(self._h, out.ctypes.data_as(C.c_void_p) if fetch else None,
                                         1 if as_int32 else 0, C.byref(ms)))
        return out, ms.value

    # -- greedy / grasp -------------------------------------------------------------------
    def construct(self, kind, starts, urand=None):
        """-> (succ [B,n] int32, obj [B], status [B])"""
        starts = np.ascontiguousarray(starts, dtype=np.int32)
        B, n = len(starts), self.n
        succ = np.zeros((B, n), dtype=np.int32)
        obj = np.zeros(B, dtype=np.float64)
        status = np.zeros(B, dtype=np.int32)
        up = None
        if kind == GRASP:
            urand = np.ascontiguousarray(urand, dtype=np.float64)
            assert urand.shape == (B, n)
            up = _d(urand)
        _check(lib().tsp_dev_construct(self._h, kind, B, _i(starts), up, _i(succ), 1, n, _d(obj), _i(status)),
               allow=(OK, WRONG_STARTING_NODE))
        return succ, obj, status

    def construct_path(self, kind):
        """The kernel and variant that construct(kind, ...) launches for this instance, as text"""
        buf = C.create_string_buffer(256)
        _check(lib().tsp_dev_construct_describe(self._h, kind, buf, 256))
        return buf.value.decode()

    def lds_variant(self, mode):
        """The LDS engine's kernel body for this instance and `mode`, as text; TspDeviceError when the instance does not fit it"""
        buf = C.create_string_buffer(256)
        _check(lib().tsp_dev_inst_lds_variant(self._h, mode, buf, 256))
        return buf.value.decode()

    def extramileage(self):
        """HEU_extramileage -> (succ [n] int32, obj)"""
        succ = np.zeros(self.n, dtype=np.int32)
        obj = C.c_double(0)
        _check(lib().tsp_dev_extramileage(self._h, _i(succ), 1, C.byref(obj)))
        return succ, obj.value

    # -- alg_2opt / alg_2opt_tabu(NULL) ---------------------------------------------------
    def _tours(self, succ):
        succ = np.array(succ, dtype=np.int32, copy=True, order="C")
        single = succ.ndim == 1
        succ2 = succ.reshape(1, -1) if single else succ
        assert succ2.shape[1] == self.n
        return single, succ2

    def two_opt(self, succ, obj, mode=FIRST, engine=ENGINE_AUTO, time_limit=-1.0):
        """succ [n] or [B,n]; obj scalar or [B].  -> (status, succ', obj', [stats dict])"""
        single, succ2 = self._tours(succ)
        B, n = succ2.shape
        o = _obj(obj, B)
        st = (Stats * B)()
        rc = lib().tsp_dev_two_opt(self._h, mode, engine, B, _i(succ2), 1, n, _d(o), time_limit, st)
        return _result(rc, single, succ2, o, st)

    # -- Or-opt (extension) ---------------------------------------------------------------
    def or_opt(self, succ, obj=None, max_moves=-1, time_limit=-1.0):
        """Or-opt descent (tsp_dev_or_opt).  succ [n] or [B,n].  -> (status, succ', obj' (recomputed cost), stats dict(s))"""
        single, succ2 = self._tours(succ)
        B, n = succ2.shape
        o = _obj(obj, B)
        st = (OrOptStats * B)()
        rc = lib().tsp_dev_or_opt(self._h, B, _i(succ2), 1, n, _d(o), int(max_moves), time_limit, st)
        return _result(rc, single, succ2, o, st)

    def two_opt_or_opt(self, succ, obj, mode=FIRST, time_limit=-1.0):
        """2-opt + Or-opt rounds to a joint local optimum (tsp_dev_two_opt_or_opt).
        -> (status, succ', obj' (recomputed cost), 2-opt stats dict(s), Or-opt stats dict(s))"""
        single, succ2 = self._tours(succ)
        B, n = succ2.shape
        o = _obj(obj, B)
        st2 = (Stats * B)()
        sto = (OrOptStats * B)()
        rc = lib().tsp_dev_two_opt_or_opt(self._h, mode, B, _i(succ2), 1, n, _d(o), time_limit, st2, sto)
        return _result(rc, single, succ2, o, st2, sto)

    # -- candidate neighbour lists (extension) ----------------------------------------------
    def knn_build(self, K=NL_DEFAULT_K):
        """Exact K-nearest lists built on the device and kept in the handle (tsp_dev_inst_knn_build) -> kernel ms"""
        ms = C.c_float(0)
        _check(lib().tsp_dev_inst_knn_build(self._h, int(K), C.byref(ms)))
        return ms.value

    def knn_set(self, nbr):
        """The caller's own (n, K) candidate lists (tsp_dev_inst_knn_set)."""
        nbr = np.ascontiguousarray(nbr, dtype=np.int32)
        if nbr.ndim != 2 or nbr.shape[0] != self.n:
            raise TspDeviceError("tsp_dev call failed with %d (lists must be (n, K))" % E_ARG)
        _check(lib().tsp_dev_inst_knn_set(self._h, nbr.shape[1], _i(nbr)))

    def knn(self):
        """-> the handle's lists as an (n, K) int32 array, or None when it has none"""
        K = C.c_int(0)
        _check(lib().tsp_dev_inst_knn_get(self._h, C.byref(K), None))
        if K.value == 0:
            return None
        out = np.empty((self.n, K.value), dtype=np.int32)
        _check(lib().tsp_dev_inst_knn_get(self._h, C.byref(K), _i(out)))
        return out

    def nl_opt(self, succ, obj=None, kinds=NL_2OPT | NL_OROPT, max_moves=-1, time_limit=-1.0):
        """2-opt + Or-opt descent over the neighbour-list neighbourhood (tsp_dev_nl_opt).  succ [n] or [B,n].
        -> (status, succ', obj' (recomputed cost), stats dict(s))"""
        single, succ2 = self._tours(succ)
        B, n = succ2.shape
        o = _obj(obj, B)
        st = (NlOptStats * B)()
        rc = lib().tsp_dev_nl_opt(self._h, int(kinds), B, _i(succ2), 1, n, _d(o), int(max_moves), time_limit, st)
        return _result(rc, single, succ2, o, st)

    def nl_3opt(self, succ, obj=None, kinds=NL_2OPT | NL_OROPT | NL_3OPT, max_moves=-1, time_limit=-1.0, dlb=DLB_OFF, active=None):
        """The list descent with the 3-opt kind (tsp_dev_nl_3opt): kinds is any non-empty subset of NL_2OPT | NL_OROPT | NL_3OPT.
        succ [n] or [B,n].  -> (status, succ', obj' (recomputed cost), stats dict(s)) as nl_opt, the stats with moves_3opt and
        moves_by_type.  dlb = DLB_ON or DLB_CLOSE: the descent with don't-look bits (tsp_dev_nl_3opt_dlb) from the active set
        `active` ([n] or [B,n], non-zero = active; None: every node); the stats then carry active_nodes and closing_scans"""
        single, succ2 = self._tours(succ)
        B, n = succ2.shape
        o = _obj(obj, B)
        tours = (B, _i(succ2), 1, n, _d(o))
        if dlb != DLB_OFF:
            act = None
            if active is not None:
                act = np.ascontiguousarray(np.asarray(active).reshape(B, n) != 0, dtype=np.uint8)
            st = (NlDlbStats * B)()
            rc = lib().tsp_dev_nl_3opt_dlb(self._h, int(kinds), int(dlb), *tours,
                                           None if act is None else act.ctypes.data_as(C.POINTER(C.c_ubyte)), int(max_moves),
                                           time_limit, st)
        else:
            st = (Nl3OptStats * B)()
            rc = lib().tsp_dev_nl_3opt(self._h, int(kinds), *tours, int(max_moves), time_limit, st)
        return _result(rc, single, succ2, o, st)

    def nl_3opt_batch(self, succ, obj=None, kinds=NL_2OPT | NL_OROPT | NL_3OPT, max_arc=0, rounds=0, max_moves=-1, time_limit=-1.0):
        """The batched list descent (tsp_dev_nl_3opt_batch): every decision applies the improving moves of pairwise disjoint arcs
        that `rounds` claim rounds accept among the per-node candidates of an arc of at most max_arc positions (max_arc <= 0: n / 2;
        rounds <= 0: NL_BATCH_DEFAULT_ROUNDS).  succ [n] or [B,n].  -> (status, succ', obj' (recomputed cost), stats dict(s)) as
        nl_3opt"""
        single, succ2 = self._tours(succ)
        B, n = succ2.shape
        o = _obj(obj, B)
        st = (Nl3OptStats * B)()
        rc = lib().tsp_dev_nl_3opt_batch(self._h, int(kinds), int(max_arc), int(rounds), B, _i(succ2), 1, n, _d(o), int(max_moves),
                                         time_limit, st)
        return _result(rc, single, succ2, o, st)

    # -- iterated local search (extension) ---------------------------------------------------
    def ils(self, succ, iterations, seed=0, span=0, kinds=NL_2OPT | NL_OROPT | NL_3OPT, max_moves_per_descent=-1, time_limit=-1.0,
            obj=None, dlb=DLB_OFF):
        """Iterated local search (tsp_dev_ils): the list descent of nl_3opt, then `iterations` times a double-bridge kick within
        `span` nodes (0: the whole tour), the descent again and the better tour kept.  succ [n] or [B,n]: B chains, chain b with
        random stream b of `seed`.  -> (status, succ', obj' (recomputed cost of the incumbent), stats dict(s)): the nl_3opt
        counters summed over the chain's descents, iterations, accepted, last_improved, start_cost.  dlb = DLB_ON or DLB_CLOSE: every
        descent with don't-look bits (tsp_dev_ils_dlb), the stats with active_nodes and closing_scans"""
        single, succ2 = self._tours(succ)
        B, n = succ2.shape
        o = _obj(obj, B)
        args = (self._h, int(kinds), B, _i(succ2), 1, n, _d(o), int(seed) & (2 ** 64 - 1), int(iterations), int(span),
                int(max_moves_per_descent), time_limit)
        if dlb != DLB_OFF:
            st = (IlsDlbStats * B)()
            rc = lib().tsp_dev_ils_dlb(*args, int(dlb), st)
        else:
            st = (IlsStats * B)()
            rc = lib().tsp_dev_ils(*args, st)
        return _result(rc, single, succ2, o, st)

    def ils_kick(self, succ, seed, it, span=0):
        """The kick of iteration `it` of chain b applied to tour b and nothing else (tsp_dev_ils_kick).  succ [n] or [B,n]
        -> succ'"""
        single, succ2 = self._tours(succ)
        B, n = succ2.shape
        _check(lib().tsp_dev_ils_kick(self._h, B, _i(succ2), 1, n, int(seed) & (2 ** 64 - 1), int(it), int(span)))
        return succ2[0] if single else succ2

    def seg_ils(self, succ, iterations, window=0, span=0, trials=1, seed=0, kinds=NL_2OPT | NL_OROPT, max_moves_per_trial=-1,
                time_limit=-1.0, obj=None):
        """Windowed iterated local search (tsp_dev_seg_ils): per iteration the tour is cut into windows of `window` consecutive
        nodes (0: SEG_ILS_DEFAULT_WINDOW) from a random anchor, and every window runs `trials` trials of a double-bridge kick
        within `span` window nodes (0: window - 1), the repair by the 2-opt + Or-opt list moves that stay inside the window, and
        the better window kept.  There is no descent before the first iteration: pass a local optimum (nl_3opt_batch).  succ [n]
        or [B,n]: B chains, chain b with random stream b of `seed`.  -> (status, succ', obj' (recomputed cost), stats dict(s)):
        the nl_opt counters summed over all trials, iterations, windows, trials, accepted, active_nodes, start_cost"""
        single, succ2 = self._tours(succ)
        B, n = succ2.shape
        o = _obj(obj, B)
        st = (SegIlsStats * B)()
        rc = lib().tsp_dev_seg_ils(self._h, int(kinds), B, _i(succ2), 1, n, _d(o), int(seed) & (2 ** 64 - 1), int(iterations),
                                   int(window), int(span), int(trials), int(max_moves_per_trial), time_limit, st)
        return _result(rc, single, succ2, o, st)

    def seg_ils3(self, succ, iterations, window=0, span=0, trials=1, seed=0, kinds=NL_2OPT | NL_OROPT | NL_3OPT,
                 max_moves_per_trial=-1, time_limit=-1.0, obj=None):
        """seg_ils with the 3-opt kind in the repair (tsp_dev_seg_ils3): kinds is any non-empty subset of NL_2OPT | NL_OROPT |
        NL_3OPT, a window 3-opt move is a segment move all three removed edges of which are window edges.  Arguments and result as
        seg_ils, the stats with moves_3opt and moves_by_type behind them.  With kinds inside NL_2OPT | NL_OROPT it returns the bits
        of seg_ils"""
        single, succ2 = self._tours(succ)
        B, n = succ2.shape
        o = _obj(obj, B)
        st = (SegIls3Stats * B)()
        rc = lib().tsp_dev_seg_ils3(self._h, int(kinds), B, _i(succ2), 1, n, _d(o), int(seed) & (2 ** 64 - 1), int(iterations),
                                    int(window), int(span), int(trials), int(max_moves_per_trial), time_limit, st)
        return _result(rc, single, succ2, o, st)

    def seg_ils_groups(self, succ, iterations, groups=0, window=0, span=0, trials=1, seed=0, kinds=NL_2OPT | NL_OROPT | NL_3OPT,
                       max_moves_per_trial=-1, time_limit=-1.0, obj=None):
        """seg_ils3 with `groups` independent trial groups per window (tsp_dev_seg_ils_groups): every group runs its `trials`
        trials from the window as the iteration found it, with draws of its own, and the groups whose changed slot intervals
        do not meet a better one's are all written to the tour.  groups 1 .. SEG_ILS_MAX_GROUPS, 0: as many as fill the device,
        max(1, min(SEG_ILS_MAX_GROUPS, 1024 / windows)).  Everything else as seg_ils3, the stats with groups, offers and commits
        behind them and every other counter summed over all groups.  With groups=1 it returns the bits of seg_ils3"""
        single, succ2 = self._tours(succ)
        B, n = succ2.shape
        o = _obj(obj, B)
        st = (SegIlsGroupsStats * B)()
        rc = lib().tsp_dev_seg_ils_groups(self._h, int(kinds), int(groups), B, _i(succ2), 1, n, _d(o), int(seed) & (2 ** 64 - 1),
                                          int(iterations), int(window), int(span), int(trials), int(max_moves_per_trial),
                                          time_limit, st)
        return _result(rc, single, succ2, o, st)

    def seg_ils_lk(self, succ, iterations, kinds=NL_2OPT | NL_OROPT | NL_3OPT | NL_LK, depth=0, groups=1, window=0, span=0,
                   trials=1, seed=0, max_moves=-1, time_limit=-1.0, obj=None):
        """seg_ils_groups with Lin-Kernighan chains as a fourth kind of the repair (tsp_dev_seg_ils_lk): kinds is any non-empty
        subset of NL_2OPT | NL_OROPT | NL_3OPT | NL_LK.  With NL_LK every active node also runs two chains per decision, one to
        each side along the window: up to `depth` reversals (1 .. SEG_LK_MAX_DEPTH, 0: SEG_LK_DEFAULT_DEPTH) under the gain
        criterion, kept up to the best prefix.  Everything else as seg_ils_groups (max_moves is its max_moves_per_trial), the stats
        with lk_depth, moves_lk, lk_flips, lk_chains and lk_steps behind them.  Without NL_LK it returns the bits of
        seg_ils_groups"""
        single, succ2 = self._tours(succ)
        B, n = succ2.shape
        o = _obj(obj, B)
        st = (SegIlsLkStats * B)()
        rc = lib().tsp_dev_seg_ils_lk(self._h, int(kinds), int(depth), int(groups), B, _i(succ2), 1, n, _d(o),
                                      int(seed) & (2 ** 64 - 1), int(iterations), int(window), int(span), int(trials),
                                      int(max_moves), time_limit, st)
        return _result(rc, single, succ2, o, st)

    # -- Held-Karp lower bound (extension) ---------------------------------------------------
    def _pi(self, pi):
        if pi is None:
            return None
        pi = np.array(pi, dtype=np.float64, copy=True, order="C")
        if pi.shape != (self.n,):
            raise TspDeviceError("tsp_dev call failed with %d (pi must have n entries)" % E_ARG)
        return pi

    def one_tree(self, pi=None, want_stats=False):
        """Minimum 1-tree under the penalties pi (tsp_dev_one_tree) -> (edges [n,2] sorted (lo, hi), deg [n], value W(pi))
        (+ stats dict with want_stats)"""
        pi = self._pi(pi)
        edges = np.zeros((self.n, 2), dtype=np.int32)
        deg = np.zeros(self.n, dtype=np.int32)
        val = C.c_double(0)
        st = LbStats()
        _check(lib().tsp_dev_one_tree(self._h, _d(pi) if pi is not None else None, _i(edges), _i(deg), C.byref(val), C.byref(st)))
        if want_stats:
            return edges, deg, val.value, st.as_dict()
        return edges, deg, val.value

    def held_karp(self, ub, max_iters=HK_DEFAULT_ITERS, lambda0=HK_DEFAULT_LAMBDA, patience=0, time_limit=-1.0, pi=None):
        """Subgradient ascent over 1-trees (tsp_dev_held_karp) -> (bound, pi_best [n], stats dict); stats["status"] is OK or
        TIME_LIMIT_EXCEEDED (the bound is valid either way)."""
        pi = self._pi(pi)
        if pi is None:
            pi = np.zeros(self.n, dtype=np.float64)
        bound = C.c_double(0)
        st = LbStats()
        rc = lib().tsp_dev_held_karp(self._h, float(ub), int(max_iters), float(lambda0), int(patience), float(time_limit), _d(pi),
                                     C.byref(bound), C.byref(st))
        _check(rc, allow=(OK, TIME_LIMIT_EXCEEDED))
        stats = st.as_dict()
        stats["status"] = rc
        return bound.value, pi, stats

    def one_tree_sparse(self, pi=None, want_stats=False):
        """The 1-tree over the candidate graph of the handle's lists, completed over all edges where the lists leave several
        components (tsp_dev_one_tree_sparse) -> (edges [n,2] sorted (lo, hi), deg [n], value W_C(pi)) (+ stats dict with
        want_stats).  W_C is not a lower bound."""
        pi = self._pi(pi)
        edges = np.zeros((self.n, 2), dtype=np.int32)
        deg = np.zeros(self.n, dtype=np.int32)
        val = C.c_double(0)
        st = LbSparseStats()
        _check(lib().tsp_dev_one_tree_sparse(self._h, _d(pi) if pi is not None else None, _i(edges), _i(deg), C.byref(val),
                                             C.byref(st)))
        if want_stats:
            return edges, deg, val.value, st.as_dict()
        return edges, deg, val.value

    def held_karp_sparse(self, ub, sparse_iters, dense_iters=1, lambda0=HK_DEFAULT_LAMBDA, patience=0, time_limit=-1.0, pi=None):
        """The ascent over the candidate graph for sparse_iters iterations, then dense_iters iterations of held_karp from its
        pi_best and lambda (tsp_dev_held_karp_sparse) -> (bound, pi_best [n], stats dict); the bound comes from dense 1-trees
        and is valid; stats["status"] is OK or TIME_LIMIT_EXCEEDED."""
        pi = self._pi(pi)
        if pi is None:
            pi = np.zeros(self.n, dtype=np.float64)
        bound = C.c_double(0)
        st = LbSparseStats()
        rc = lib().tsp_dev_held_karp_sparse(self._h, float(ub), int(sparse_iters), int(dense_iters), float(lambda0), int(patience),
                                            float(time_limit), _d(pi), C.byref(bound), C.byref(st))
        _check(rc, allow=(OK, TIME_LIMIT_EXCEEDED))
        stats = st.as_dict()
        stats["status"] = rc
        return bound.value, pi, stats

    # -- alpha-nearness candidate lists (extension) ------------------------------------------
    def alpha_build(self, K=ALPHA_DEFAULT_K, pi=None, want_alpha=False, want_stats=False):
        """Alpha-nearness lists from the minimum 1-tree of pi, built on the device and kept in the handle
        (tsp_dev_inst_alpha_build) -> the (n, K) int32 lists (+ the (n, K) alpha values with want_alpha, + a stats dict with
        want_stats)"""
        pi = self._pi(pi)
        K = int(K)
        alpha = np.zeros((self.n, max(K, 0)), dtype=np.float64) if want_alpha else None
        st = AlphaStats()
        _check(lib().tsp_dev_inst_alpha_build(self._h, K, _d(pi) if pi is not None else None,
                                              _d(alpha) if want_alpha else None, C.byref(st)))
        out = (self.knn(),)
        if want_alpha:
            out += (alpha,)
        if want_stats:
            out += (st.as_dict(),)
        return out[0] if len(out) == 1 else out

    def alpha_rows(self, rows, pi=None):
        """Whole alpha rows (tsp_dev_alpha_rows) -> (len(rows), n) float64; the rows' own entries are 0"""
        pi = self._pi(pi)
        rows = np.ascontiguousarray(np.atleast_1d(rows), dtype=np.int32)
        out = np.zeros((len(rows), self.n), dtype=np.float64)
        _check(lib().tsp_dev_alpha_rows(self._h, _d(pi) if pi is not None else None, len(rows), _i(rows), _d(out)))
        return out

    # -- greedy-edge construction (extension) -------------------------------------------------
    def greedy_edge(self, want_edges=False, want_stats=False):
        """The greedy-edge tour (tsp_dev_greedy_edge) -> (succ [n] int32 with succ[0] the smaller of node 0's two neighbours, obj
        (recomputed cost)) (+ the n - 1 accepted edges [n-1,2] sorted (lo, hi) with want_edges, + a stats dict with want_stats)"""
        succ = np.zeros(self.n, dtype=np.int32)
        edges = np.zeros((self.n - 1, 2), dtype=np.int32) if want_edges else None
        obj = C.c_double(0)
        st = GreedyEdgeStats()
        _check(lib().tsp_dev_greedy_edge(self._h, _i(succ), 1, C.byref(obj), _i(edges) if want_edges else None, C.byref(st)))
        out = (succ, obj.value)
        if want_edges:
            out += (edges,)
        if want_stats:
            out += (st.as_dict(),)
        return out

    # -- partition crossover (extension) --------------------------------------------------------
    def gpx(self, succ_a, succ_b, want_stats=False):
        """Partition crossover of two tours (tsp_dev_gpx): succ_a, succ_b [n] or [P,n], pair k merged from row k of each, all P
        pairs in one device call.  The child is the cheaper parent (succ_a on ties of the fixed-point lengths) with every
        exchangeable component of the parents' differences taken from the other parent where that is strictly shorter: never
        longer than either parent.  -> (child [n] or [P,n] int32, obj float or [P]) (+ a stats dict, or a list of P, with
        want_stats)"""
        single, a2 = self._tours(succ_a)
        single_b, b2 = self._tours(succ_b)
        assert single == single_b and a2.shape == b2.shape
        P, n = a2.shape
        child = np.zeros_like(a2)
        obj = np.zeros(P, dtype=np.float64)
        st = (GpxStats * P)()
        _check(lib().tsp_dev_gpx(self._h, P, _i(a2), _i(b2), 1, n, _i(child), _d(obj), st))
        out = (child[0], float(obj[0])) if single else (child, obj)
        if want_stats:
            dicts = [x.as_dict() for x in st]
            out += (dicts[0] if single else dicts,)
        return out

    def gpx_tournament(self, tours):
        """Rounds of pairwise gpx over tours [T,n]: pairs (0,1), (2,3), ... in one device call per round, an odd last tour passes
        through, until one tour is left.  -> (succ [n] int32, its cost, one list of per-pair stats dicts per round).  T = 1: the
        tour itself, its cost from perm_cost's kernel, no rounds."""
        tours = np.array(tours, dtype=np.int32, copy=True, order="C")
        assert tours.ndim == 2 and tours.shape[0] >= 1 and tours.shape[1] == self.n
        rounds = []
        cost = None
        while tours.shape[0] > 1:
            P = tours.shape[0] // 2
            child, obj, st = self.gpx(tours[0:2 * P:2], tours[1:2 * P:2], want_stats=True)
            rounds.append(st)
            tours = np.concatenate([child, tours[-1:]]) if tours.shape[0] % 2 else child
            if tours.shape[0] == 1:   # the last round had one pair
                cost = float(obj[0])
        if cost is None:
            order = np.zeros(self.n, dtype=np.int32)
            v = 0
            for k in range(self.n):
                order[k] = v
                v = int(tours[0][v])
            cost = float(self.perm_cost(order)[0])
        return tours[0], cost, rounds

    def perm_cost(self, perms):
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        if perms.ndim == 1:
            perms = perms.reshape(1, -1)
        B, n = perms.shape
        cost = np.zeros(B, dtype=np.float64)
        _check(lib().tsp_dev_perm_cost(self._h, B, _i(perms), n, _d(cost)))
        return cost


class Tabu:
    """n(n-1)/2 tabu stamps resident in HBM (tabusearch.c:195)."""

    def __init__(self, inst):
        self.inst = inst
        self._h = C.c_void_p()
        _check(lib().tsp_dev_tabu_create(inst._h, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().tsp_dev_tabu_destroy(self._h)
            self._h = C.c_void_p()

    def set(self, idx, value):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        value = np.ascontiguousarray(value, dtype=np.int32)
        _check(lib().tsp_dev_tabu_set(self._h, _i(idx), _i(value), len(idx)))

    def get(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        out = np.zeros(len(idx), dtype=np.int32)
        _check(lib().tsp_dev_tabu_get(self._h, _i(idx), _i(out), len(idx)))
        return out

    def upload(self, stamps):
        stamps = np.ascontiguousarray(stamps, dtype=np.int32)
        n = self.inst.n
        assert len(stamps) == n * (n - 1) // 2
        _check(lib().tsp_dev_tabu_upload(self._h, _i(stamps)))

    def download(self):
        n = self.inst.n
        out = np.zeros(n * (n - 1) // 2, dtype=np.int32)
        _check(lib().tsp_dev_tabu_download(self._h, _i(out)))
        return out

    def list_info(self):
        """-> (entries of the compact list of non-zero stamps or -1 while out of date, last run worked from the list)"""
        e, u = C.c_int(0), C.c_int(0)
        _check(lib().tsp_dev_tabu_list_info(self._h, C.byref(e), C.byref(u)))
        return e.value, bool(u.value)

    def two_opt(self, succ, iter_, tenure, want_prev=False, time_limit=-1.0):
        """alg_2opt_tabu(inst, skip_edge, stored_prev, iter, tenure) -> (status, succ', obj', stats, prev)"""
        succ = np.array(succ, dtype=np.int32, copy=True, order="C")
        o = C.c_double(0.0)
        st = Stats()
        prev = np.zeros(self.inst.n, dtype=np.int32) if want_prev else None
        rc = lib().tsp_dev_two_opt_tabu(self.inst._h, self._h, iter_, tenure, _i(succ), 1, C.byref(o),
                                        _i(prev) if want_prev else None, time_limit, C.byref(st))
        _check(rc, allow=(OK, TIME_LIMIT_EXCEEDED))
        return rc, succ, o.value, st.as_dict(), prev


class Tours:
    """B tours resident in HBM (what bench.py times)."""

    def __init__(self, inst, B=1):
        self.inst, self.B = inst, B
        self._h = C.c_void_p()
        _check(lib().tsp_dev_tours_create(inst._h, B, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().tsp_dev_tours_destroy(self._h)
            self._h = C.c_void_p()

    def upload(self, succ, obj):
        succ = np.ascontiguousarray(succ, dtype=np.int32).reshape(self.B, self.inst.n)
        o = np.array(np.broadcast_to(np.asarray(obj, dtype=np.float64), (self.B,)), copy=True)
        _check(lib().tsp_dev_tours_upload(self._h, _i(succ), 1, self.inst.n, _d(o)))

    def reset(self):
        _check(lib().tsp_dev_tours_reset(self._h))

    def run(self, mode, max_steps=-1, time_limit=-1.0, sync=True):
        """-> (status, all_done).  max_steps < 0 (until done) needs sync=True."""
        if not sync and max_steps < 0:
            raise ValueError("an unbounded run needs sync=True (it is driven by polls of the done flags)")
        done = C.c_int(0)
        rc = lib().tsp_dev_tours_run(self._h, mode, max_steps, time_limit, 1 if sync else 0, C.byref(done))
        _check(rc, allow=(OK, TIME_LIMIT_EXCEEDED))
        return rc, bool(done.value)

    def device_ms(self):
        """Device time of the last run_engine / two_opt on this handle (HIP events on the engine's stream)."""
        ms = C.c_double(0)
        _check(lib().tsp_dev_tours_device_ms(self._h, C.byref(ms)))
        return ms.value

    def describe(self, mode):
        """The kernels one GRID-engine step of `mode` launches for this handle."""
        buf = C.create_string_buffer(256)
        _check(lib().tsp_dev_tours_describe(self._h, mode, buf, 256))
        return buf.value.decode()

    def run_engine(self, mode, engine=ENGINE_AUTO, max_steps=-1, time_limit=-1.0):
        """Resident tours on a chosen engine, waits for completion.  -> (status, all_done)"""
        done = C.c_int(0)
        rc = lib().tsp_dev_tours_run_engine(self._h, mode, engine, max_steps, time_limit, C.byref(done))
        _check(rc, allow=(OK, TIME_LIMIT_EXCEEDED))
        return rc, bool(done.value)

    # -- drivers on resident tours -------------------------------------------------------------
    def two_opt(self, mode, engine=ENGINE_AUTO, time_limit=-1.0):
        """alg_2opt / alg_2opt_tabu(NULL) on the tours as they are -> (status, obj [B])"""
        obj = np.zeros(self.B, dtype=np.float64)
        rc = lib().tsp_dev_tours_two_opt(self._h, mode, engine, time_limit, _d(obj))
        _check(rc, allow=(OK, TIME_LIMIT_EXCEEDED))
        return rc, obj

    def two_opt_tabu(self, tabu, iter_, tenure, time_limit=-1.0):
        obj = C.c_double(0)
        rc = lib().tsp_dev_tours_two_opt_tabu(self._h, tabu._h if tabu is not None else None, iter_, tenure, time_limit, C.byref(obj))
        _check(rc, allow=(OK, TIME_LIMIT_EXCEEDED))
        return rc, obj.value

    def tabu_kick(self, tabu, a, b, iter_, tenure):
        acc = C.c_int(0)
        _check(lib().tsp_dev_tours_tabu_kick(self._h, tabu._h, a, b, iter_, tenure, C.byref(acc)))
        return bool(acc.value)

    def tabu_iterations(self, tabu, iter0, tenures, ab, best_obj, time_limit=-1.0):
        """K = len(tenures) iterations of tabu() in one wait for the device (tsp_dev_tours_tabu_iterations)
        -> (status, completed, last_accepted, best_obj', obj [completed], improved [completed])"""
        K = len(tenures)
        ten = np.ascontiguousarray(tenures, dtype=np.int32)
        abv = np.ascontiguousarray(ab, dtype=np.int32).reshape(2 * K)
        best, obj, imp = C.c_double(best_obj), np.zeros(K), np.zeros(K, dtype=np.int32)
        done, acc = C.c_int(0), C.c_int(0)
        rc = lib().tsp_dev_tours_tabu_iterations(self._h, tabu._h, iter0, K, _i(ten), _i(abv), time_limit, C.byref(best), _d(obj), _i(imp),
                                                 C.byref(done), C.byref(acc))
        _check(rc, allow=(OK, TIME_LIMIT_EXCEEDED))
        return rc, done.value, bool(acc.value), best.value, obj[:done.value].copy(), imp[:done.value].copy()

    def tabu_iterations_ex(self, tabu, iter0, tenures, ab, best_obj, time_limit=-1.0):
        """K = len(tenures) iterations of tabu() in one launch with the kick's trials taken in order from the len(ab) >= K node pairs
        (tsp_dev_tours_tabu_iterations_ex) -> (status, completed, last_accepted, best_obj', obj [completed], improved [completed],
        trials [completed])"""
        K = len(tenures)
        ten = np.ascontiguousarray(tenures, dtype=np.int32)
        abv = np.ascontiguousarray(ab, dtype=np.int32)
        P = abv.size // 2
        abv = abv.reshape(2 * P)
        best, obj, imp, tri = C.c_double(best_obj), np.zeros(K), np.zeros(K, dtype=np.int32), np.zeros(K, dtype=np.int32)
        done, acc = C.c_int(0), C.c_int(0)
        rc = lib().tsp_dev_tours_tabu_iterations_ex(self._h, tabu._h, iter0, K, _i(ten), P, _i(abv), time_limit, C.byref(best), _d(obj), _i(imp),
                                                    _i(tri), C.byref(done), C.byref(acc))
        _check(rc, allow=(OK, TIME_LIMIT_EXCEEDED))
        d = done.value
        return rc, d, bool(acc.value), best.value, obj[:d].copy(), imp[:d].copy(), tri[:d].copy()

    def tabu_iteration(self, tabu, iter_, tenure, a, b, best_obj, time_limit=-1.0):
        """-> (status, obj, best_obj', improved, accepted): alg_2opt_tabu, incumbent, first kick trial (tabusearch.c:238-309)"""
        best, obj, imp, acc = C.c_double(best_obj), C.c_double(0), C.c_int(0), C.c_int(0)
        rc = lib().tsp_dev_tours_tabu_iteration(self._h, tabu._h, iter_, tenure, time_limit, a, b, C.byref(best), C.byref(obj),
                                                C.byref(imp), C.byref(acc))
        _check(rc, allow=(OK, TIME_LIMIT_EXCEEDED))
        return rc, obj.value, best.value, bool(imp.value), bool(acc.value)

    def vns_kick(self, p1, p2, p3):
        obj = C.c_double(0)
        _check(lib().tsp_dev_tours_vns_kick(self._h, p1, p2, p3, C.byref(obj)))
        return obj.value

    def snapshot(self):
        _check(lib().tsp_dev_tours_snapshot(self._h))

    def restore(self):
        _check(lib().tsp_dev_tours_restore(self._h))

    def download(self):
        """-> (succ [B,n], obj [B], [stats])"""
        n = self.inst.n
        succ = np.zeros((self.B, n), dtype=np.int32)
        obj = np.zeros(self.B, dtype=np.float64)
        st = (Stats * self.B)()
        _check(lib().tsp_dev_tours_download(self._h, _i(succ), 1, n, _d(obj), st))
        return succ, obj, [s.as_dict() for s in st]

    def time_scan(self, reps=20):
        """-> (mean kernel ms, evals per launch) for the BEST-mode sweep kernel"""
        ms = C.c_float(0)
        ev = C.c_int64(0)
        _check(lib().tsp_dev_tours_time_scan(self._h, reps, C.byref(ms), C.byref(ev)))
        return ms.value, ev.value

    def best(self, true_cost=True):
        """-> (cost, tour index) minimum over the handle's tours"""
        p = C.c_int64(0)
        _check(lib().tsp_dev_tours_best(self._h, 1 if true_cost else 0, C.byref(p)))
        return p.value >> 24, p.value & 0xFFFFFF, p.value


def multistart_pack(cost, start_id):
    """(cost, start id) -> cost << 24 | start id through the C ABI; raises ValueError for costs the all-reduce cannot carry
    (not a non-negative integer below 2^39: --fcost, GEO)."""
    p = C.c_int64(0)
    if lib().tsp_dev_multistart_pack(float(cost), int(start_id), C.byref(p)) != OK:
        raise ValueError("cost %r / start %r cannot be packed for the all-reduce(min)" % (cost, start_id))
    return p.value


def comm_available():
    """True if librccl can be opened by the C ABI (no communicator is formed)."""
    return bool(lib().tsp_dev_comm_available())


def comm_unique_id():
    """ncclGetUniqueId through the C ABI (rank 0): 128 bytes to hand to every rank."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().tsp_dev_comm_unique_id(buf))
    return buf.raw


class Comm:
    """One rank of the RCCL communicator the C ABI's multi-start epilogue runs on (tsp_dev_comm_init_rank)."""

    def __init__(self, ctx, world, rank, unique_id):
        assert len(unique_id) == COMM_ID_BYTES
        self.ctx, self.world, self.rank = ctx, world, rank
        self._h = C.c_void_p()
        _check(lib().tsp_dev_comm_init_rank(ctx._h, world, rank, unique_id, C.byref(self._h)))

    def rccl_version(self):
        v = C.c_int(0)
        _check(lib().tsp_dev_comm_info(self._h, None, None, C.byref(v)))
        return v.value

    def allreduce_min(self, packed):
        out = C.c_int64(0)
        _check(lib().tsp_dev_multistart_allreduce(self._h, int(packed), C.byref(out)))
        return out.value

    def allreduce_min_f64(self, cost):
        """all-reduce(min) of one double per rank (costs the packed word cannot carry: --fcost)."""
        out = C.c_double(0)
        _check(lib().tsp_dev_multistart_allreduce_f64(self._h, float(cost), C.byref(out)))
        return out.value

    def bcast_tour(self, root, succ):
        """succ: int32 [n], the winner's tour on `root`, overwritten with it on the other ranks."""
        assert succ.dtype == np.int32 and succ.flags["C_CONTIGUOUS"]
        _check(lib().tsp_dev_multistart_bcast_tour(self._h, root, _i(succ), 1, len(succ)))
        return succ

    def close(self):
        if self._h:
            lib().tsp_dev_comm_destroy(self._h)
            self._h = C.c_void_p()
