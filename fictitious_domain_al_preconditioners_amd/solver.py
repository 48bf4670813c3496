"""Host-side mirror of the reference's solver interface over the C ABI.

Everything here goes through ``lib/libalfd.so`` (include/alfd/alfd.h); there is
no Python or CPU fallback: if the HIP library is missing or no GPU is present
the calls raise.  The class names and ``vmult(dst, src)`` / ``solve(A, x, b, P)``
signatures follow the reference (augmented_lagrangian_preconditioner.h:14-110,
stokes_immersed_boundary.cc:1067-1074) so that tests read like the call sites.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libalfd.so")
_lib = None

# every symbol include/alfd/alfd.h declares
ABI_SYMBOLS = [
    "alfd_abi_version", "alfd_strerror", "alfd_last_error", "alfd_create", "alfd_destroy",
    "alfd_comm_unique_id", "alfd_comm_init", "alfd_set_partition", "alfd_set_matrix", "alfd_set_diag",
    "alfd_configure", "alfd_default_config", "alfd_setup", "alfd_precond_apply", "alfd_system_apply",
    "alfd_augment_rhs", "alfd_solve", "alfd_upload_rhs", "alfd_solve_resident", "alfd_download_solution",
    "alfd_get_history", "alfd_spmv", "alfd_dot", "alfd_matrix_lanes", "alfd_bench_spmv",
    "alfd_enable_timing", "alfd_get_timing", "alfd_host_halo_plan", "alfd_local_group_create",
    "alfd_local_group_destroy", "alfd_comm_init_local", "alfd_set_aggregates",
    "alfd_set_aggregate_partition", "alfd_get_matrix_info", "alfd_bench_spmv_format",
    "alfd_host_window_plan", "alfd_set_tunable", "alfd_build_aggregates", "alfd_get_aggregates",
    "alfd_host_aggregate_level", "alfd_comm_init_host",
    "alfd_get_device_memory", "alfd_set_row_blocks", "alfd_host_stream_plan",
    "alfd_host_row_blocks_from_points", "alfd_host_stream_plan_short", "alfd_set_prolongator", "alfd_set_controls", "alfd_get_timing_streamed", "alfd_get_setup_seconds",
    "alfd_host_numbering_from_points", "alfd_host_brick_blocks_from_points", "alfd_host_permute_csr",
    "alfd_build_smoothed_aggregation", "alfd_get_prolongator", "alfd_host_smoothed_prolongator",
    "alfd_build_smoothed_aggregation_truncated", "alfd_host_truncate_prolongator",
    "alfd_inner_prec_apply", "alfd_spmv_scaled", "alfd_spmv_pair", "alfd_get_last_spmv_launch",
    "alfd_estimate_spectrum", "alfd_get_cg_coefficients", "alfd_host_tridiagonal_extremes",
    "alfd_constraint_residual",
    "alfd_set_prolongator_block", "alfd_build_smoothed_aggregation_block", "alfd_get_prolongator_block",
    "alfd_clear_hierarchy", "alfd_get_inner_iterations", "alfd_get_aggregates_block",
    "alfd_host_strength_graph", "alfd_host_aggregate_graph", "alfd_build_strength_graph", "alfd_get_strength_graph",
    "alfd_upload_rhs_device", "alfd_download_solution_device", "alfd_solve_device", "alfd_precond_apply_device",
    "alfd_system_apply_device", "alfd_augment_rhs_device",
    "alfd_get_matrix_shape", "alfd_get_operator_shape", "alfd_bench_operator", "alfd_host_small_shape",
    "alfd_host_stream_plan_side", "alfd_get_side_rows",
    "alfd_host_sparse_product", "alfd_sparse_product", "alfd_smoothed_prolongator",
    "alfd_setup_coupling", "alfd_get_setup_counts",
    "alfd_set_preconditioner_values", "alfd_get_preconditioner_values", "alfd_spmv_preconditioner",
    "alfd_bench_spmv_preconditioner",
    "alfd_spmv_tail_step", "alfd_get_fused_tail_launches",
    "alfd_host_check_numbering", "alfd_set_numbering", "alfd_set_numbering_from_points", "alfd_get_numbering",
    "alfd_host_point_lattice", "alfd_host_point_prolongator", "alfd_host_grid_prolongator",
    "alfd_build_geometric_from_points", "alfd_host_point_hierarchy_cells",
]


class AlfdError(RuntimeError):
    """Non-zero status from the C ABI.  NoConvergence mirrors
    dealii::SolverControl::NoConvergence (stokes_immersed_boundary.cc:1233-1254)."""

    def __init__(self, status, message):
        super().__init__(f"alfd status {status}: {message}")
        self.status = status


class NoConvergence(AlfdError):
    pass


def load_library():
    """dlopen libalfd.so; raises ImportError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: the HIP extension is required (no CPU fallback). "
                          "Build it with `python -c 'import __graft_entry__ as g; g.build()'`.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    PP = C.POINTER(C.c_void_p)
    sig = {
        "alfd_abi_version": (C.c_int, []),
        "alfd_strerror": (C.c_char_p, [C.c_int]),
        "alfd_last_error": (C.c_char_p, [vp]),
        "alfd_create": (C.c_int, [C.POINTER(vp), C.c_int]),
        "alfd_destroy": (C.c_int, [vp]),
        "alfd_comm_unique_id": (C.c_int, [vp, C.c_size_t]),
        "alfd_comm_init": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_size_t]),
        "alfd_set_partition": (C.c_int, [vp, C.c_int, PP]),
        "alfd_set_matrix": (C.c_int, [vp, C.c_int, i64, i64, vp, vp, vp]),
        "alfd_set_diag": (C.c_int, [vp, C.c_int, i64, vp]),
        "alfd_configure": (C.c_int, [vp, C.POINTER(_abi.Config)]),
        "alfd_default_config": (None, [C.POINTER(_abi.Config), C.c_int]),
        "alfd_setup": (C.c_int, [vp]),
        "alfd_setup_coupling": (C.c_int, [vp]),
        "alfd_get_setup_counts": (C.c_int, [vp, vp]),
        "alfd_precond_apply": (C.c_int, [vp, PP, PP, C.POINTER(_abi.Result)]),
        "alfd_system_apply": (C.c_int, [vp, PP, PP]),
        "alfd_augment_rhs": (C.c_int, [vp, PP]),
        "alfd_solve": (C.c_int, [vp, PP, PP, C.POINTER(_abi.Result)]),
        "alfd_upload_rhs": (C.c_int, [vp, PP, PP]),
        "alfd_solve_resident": (C.c_int, [vp, C.POINTER(_abi.Result)]),
        "alfd_download_solution": (C.c_int, [vp, PP]),
        "alfd_get_history": (C.c_int, [vp, vp, i32, C.POINTER(i32)]),
        "alfd_spmv": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, dbl]),
        "alfd_spmv_scaled": (C.c_int, [vp, C.c_int, vp, vp, vp, vp]),
        "alfd_spmv_pair": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp]),
        "alfd_get_last_spmv_launch": (C.c_int, [vp, C.POINTER(_abi.SpmvLaunch)]),
        "alfd_spmv_tail_step": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(_abi.TailStep)]),
        "alfd_get_fused_tail_launches": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "alfd_dot": (C.c_int, [vp, i64, vp, vp, C.POINTER(dbl)]),
        "alfd_inner_prec_apply": (C.c_int, [vp, C.c_int, vp, vp]),
        "alfd_matrix_lanes": (C.c_int, [vp, C.c_int, C.POINTER(i32)]),
        "alfd_bench_spmv": (C.c_int, [vp, C.c_int, i32, C.POINTER(dbl), C.POINTER(dbl)]),
        "alfd_enable_timing": (C.c_int, [vp, C.c_int]),
        "alfd_get_timing": (C.c_int, [vp, vp, vp, vp]),
        "alfd_host_halo_plan": (C.c_int, [i64, vp, vp, C.c_int, C.c_int, vp, vp, i64, C.POINTER(i64), vp]),
        "alfd_local_group_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "alfd_local_group_destroy": (C.c_int, [vp]),
        "alfd_comm_init_local": (C.c_int, [vp, vp, C.c_int]),
        "alfd_set_aggregates": (C.c_int, [vp, C.c_int, i64, vp, vp, i64]),
        "alfd_set_aggregate_partition": (C.c_int, [vp, C.c_int, vp]),
        "alfd_set_prolongator": (C.c_int, [vp, C.c_int, i64, i64, vp, vp, vp]),
        "alfd_set_controls": (C.c_int, [vp, vp, vp, vp]),
        "alfd_get_timing_streamed": (C.c_int, [vp, vp]),
        "alfd_get_setup_seconds": (C.c_int, [vp, vp]),
        "alfd_get_matrix_info": (C.c_int, [vp, C.c_int, C.POINTER(_abi.MatrixInfo)]),
        "alfd_bench_spmv_format": (C.c_int, [vp, C.c_int, i32, C.c_int, C.POINTER(dbl), C.POINTER(dbl)]),
        "alfd_get_matrix_shape": (C.c_int, [vp, C.c_int, C.POINTER(_abi.BatchMajorShape)]),
        "alfd_get_operator_shape": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(_abi.BatchMajorShape)]),
        "alfd_bench_operator": (C.c_int, [vp, C.c_int, C.c_int, i32, i32, i32, C.POINTER(dbl), C.POINTER(_abi.BatchMajorShape)]),
        "alfd_host_small_shape": (C.c_int, [i64, i64, i64, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
        "alfd_host_window_plan": (C.c_int, [i64, vp, vp, vp, i32, i32, C.POINTER(_abi.WindowPlanInfo)]),
        "alfd_set_tunable": (C.c_int, [vp, C.c_char_p, C.c_int]),
        "alfd_build_aggregates": (C.c_int, [vp, i32, dbl, i32, i64, i32, C.POINTER(i32)]),
        "alfd_get_aggregates": (C.c_int, [vp, C.c_int, vp, i64, C.POINTER(i64), C.POINTER(i64)]),
        "alfd_host_aggregate_level": (C.c_int, [i64, vp, vp, vp, i32, dbl, i32, vp, C.POINTER(i64)]),
        "alfd_build_smoothed_aggregation": (C.c_int, [vp, i32, dbl, i32, dbl, i64, i32, C.POINTER(i32), vp]),
        "alfd_build_smoothed_aggregation_truncated": (C.c_int, [vp, i32, dbl, i32, dbl, dbl, i32, i64, i32,
                                                                C.POINTER(i32), vp]),
        "alfd_host_truncate_prolongator": (C.c_int, [i64, i64, vp, vp, vp, vp, i32, dbl, i32, vp, vp, vp, i64,
                                                     C.POINTER(i64)]),
        "alfd_get_prolongator": (C.c_int, [vp, C.c_int, vp, vp, vp, i64, C.POINTER(i64), C.POINTER(i64),
                                           C.POINTER(i64)]),
        "alfd_host_smoothed_prolongator": (C.c_int, [i64, vp, vp, vp, i64, vp, vp, vp, vp, dbl, vp, i64, dbl,
                                                     vp, vp, vp, i64, C.POINTER(i64)]),
        "alfd_host_sparse_product": (C.c_int, [i64, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, C.POINTER(i64)]),
        "alfd_sparse_product": (C.c_int, [vp, i64, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, C.POINTER(i64),
                                          C.POINTER(i32)]),
        "alfd_smoothed_prolongator": (C.c_int, [vp, i64, vp, vp, vp, i64, vp, vp, vp, vp, dbl, vp, i64, dbl, i32, dbl, i32,
                                                vp, vp, vp, i64, C.POINTER(i64), C.POINTER(i32)]),
        "alfd_comm_init_host": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp]),
        "alfd_get_device_memory": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64)]),
        "alfd_set_row_blocks": (C.c_int, [vp, C.c_int, i64, vp, vp]),
        "alfd_host_stream_plan": (C.c_int, [i64, vp, vp, vp, C.c_int32, i64, vp, vp, vp]),
        "alfd_host_row_blocks_from_points": (C.c_int, [i64, C.c_int32, vp, C.c_int32, vp, vp, vp]),
        "alfd_host_stream_plan_short": (C.c_int, [i64, vp, vp, vp, C.c_int32, vp]),
        "alfd_host_stream_plan_side": (C.c_int, [i64, vp, vp, vp, C.c_int32, i64, vp, vp, C.POINTER(i64), vp,
                                                 C.POINTER(i64), vp]),
        "alfd_get_side_rows": (C.c_int, [vp, C.c_int, C.POINTER(_abi.SideRowsInfo)]),
        "alfd_host_numbering_from_points": (C.c_int, [i64, C.c_int32, vp, vp]),
        "alfd_host_brick_blocks_from_points": (C.c_int, [i64, C.c_int32, vp, vp, C.c_int32, vp, vp, vp]),
        "alfd_host_permute_csr": (C.c_int, [i64, vp, vp, vp, vp, vp, vp, vp, vp]),
        "alfd_estimate_spectrum": (C.c_int, [vp, C.c_int, C.POINTER(_abi.Control), C.POINTER(_abi.Spectrum)]),
        "alfd_get_cg_coefficients": (C.c_int, [vp, vp, vp, i32, C.POINTER(i32)]),
        "alfd_host_tridiagonal_extremes": (C.c_int, [i32, vp, vp, C.POINTER(dbl), C.POINTER(dbl)]),
        "alfd_constraint_residual": (C.c_int, [vp, PP, vp, C.POINTER(dbl)]),
        "alfd_set_prolongator_block": (C.c_int, [vp, C.c_int, C.c_int, i64, i64, vp, vp, vp]),
        "alfd_build_smoothed_aggregation_block": (C.c_int, [vp, C.c_int, i32, dbl, i32, dbl, dbl, i32, i64, i32,
                                                            C.POINTER(i32), vp]),
        "alfd_get_prolongator_block": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, i64, C.POINTER(i64), C.POINTER(i64),
                                                 C.POINTER(i64)]),
        "alfd_clear_hierarchy": (C.c_int, [vp, C.c_int]),
        "alfd_get_aggregates_block": (C.c_int, [vp, C.c_int, C.c_int, vp, i64, C.POINTER(i64), C.POINTER(i64)]),
        "alfd_get_inner_iterations": (C.c_int, [vp, vp]),
        "alfd_host_strength_graph": (C.c_int, [i64, vp, vp, vp, i32, dbl, vp, vp, vp, vp, vp, i64, C.POINTER(i64)]),
        "alfd_host_aggregate_graph": (C.c_int, [i64, vp, vp, vp, vp, i32, i32, vp, C.POINTER(i64)]),
        "alfd_build_strength_graph": (C.c_int, [vp, i32, dbl, C.POINTER(i64), C.POINTER(i64)]),
        "alfd_get_strength_graph": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, C.POINTER(i32)]),
        # device-resident vectors: block tables of DEVICE pointers, the caller's hipStream_t last
        "alfd_upload_rhs_device": (C.c_int, [vp, PP, PP, vp]),
        "alfd_download_solution_device": (C.c_int, [vp, PP, vp]),
        "alfd_solve_device": (C.c_int, [vp, PP, PP, C.POINTER(_abi.Result), vp]),
        "alfd_precond_apply_device": (C.c_int, [vp, PP, PP, C.POINTER(_abi.Result), vp]),
        "alfd_system_apply_device": (C.c_int, [vp, PP, PP, vp]),
        "alfd_augment_rhs_device": (C.c_int, [vp, PP, vp]),
        "alfd_set_preconditioner_values": (C.c_int, [vp, C.c_int]),
        "alfd_get_preconditioner_values": (C.c_int, [vp, C.POINTER(_abi.PrecValuesInfo)]),
        "alfd_spmv_preconditioner": (C.c_int, [vp, vp, vp, C.c_int, dbl]),
        "alfd_bench_spmv_preconditioner": (C.c_int, [vp, i32, C.POINTER(dbl), C.POINTER(dbl)]),
        # numbering of block 0: declared once, the caller keeps its own numbering
        "alfd_host_check_numbering": (C.c_int, [i64, vp, vp]),
        "alfd_set_numbering": (C.c_int, [vp, i64, vp]),
        "alfd_set_numbering_from_points": (C.c_int, [vp, i64, i32, vp, vp]),
        "alfd_get_numbering": (C.c_int, [vp, vp, i64, C.POINTER(i64)]),
        # geometric hierarchies from support points
        "alfd_host_point_lattice": (C.c_int, [i64, i32, vp, vp, vp, vp, vp, C.POINTER(i32)]),
        "alfd_host_point_prolongator": (C.c_int, [i64, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, i64, C.POINTER(i64),
                                                  C.POINTER(i64)]),
        "alfd_host_grid_prolongator": (C.c_int, [i32, i32, vp, vp, i32, vp, vp, vp, i64, C.POINTER(i64), C.POINTER(i64),
                                                 C.POINTER(i64)]),
        "alfd_host_point_hierarchy_cells": (C.c_int, [i32, i32, vp, vp, i32, i64, i32, C.POINTER(i32), vp]),
        "alfd_build_geometric_from_points": (C.c_int, [vp, C.c_int, i64, i32, vp, vp, vp, vp, i64, i32, C.POINTER(i32), vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _hip_runtimes():
    """Paths of the HIP runtime libraries mapped into this process (more than one: see Context._ck_dev)."""
    try:
        with open("/proc/self/maps") as f:
            return sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    except OSError:
        return []


def _blocks(arrs):
    a = (C.c_void_p * len(arrs))()
    for i, x in enumerate(arrs):
        a[i] = x.ctypes.data
    return a


class Context:
    """One alfd_ctx_t: one GPU, HBM-resident operators."""

    def __init__(self, device_id=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        rc = self._lib.alfd_create(C.byref(self._h), device_id)
        if rc != _abi.OK:
            self._h = None
            raise AlfdError(rc, "alfd_create failed: " + self._lib.alfd_strerror(rc).decode() +
                            " (a HIP device is required; there is no CPU path)")
        self.block_sizes = None
        self.cfg = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.alfd_destroy(self._h)
            self._h = None

    __del__ = close

    def _ck(self, rc):
        if rc != _abi.OK:
            msg = self._lib.alfd_last_error(self._h).decode() or self._lib.alfd_strerror(rc).decode()
            cls = NoConvergence if rc in (_abi.E_NO_CONVERGENCE_OUTER, _abi.E_NO_CONVERGENCE_INNER) else AlfdError
            raise cls(rc, msg)

    # -- multi-GPU
    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(_abi.UNIQUE_ID_BYTES)
        rc = load_library().alfd_comm_unique_id(buf, _abi.UNIQUE_ID_BYTES)
        if rc != _abi.OK:
            raise AlfdError(rc, "alfd_comm_unique_id failed")
        return buf.raw

    def comm_init(self, rank, nranks, unique_id: bytes):
        self._ck(self._lib.alfd_comm_init(self._h, rank, nranks, unique_id, len(unique_id)))

    def comm_init_local(self, group, rank):
        self._ck(self._lib.alfd_comm_init_local(self._h, group, rank))

    def comm_init_torch(self, group=None):
        """Multi-rank through torch.distributed HOST collectives (gloo or any CPU backend): the
        library hands its all-gathers and neighbour exchanges to hostcomm's callbacks as host
        buffers (alfd_comm_init_host).  One process per rank; library calls are collective."""
        from . import hostcomm
        rank, world, ag, a2a = hostcomm.torch_callbacks(group)
        self._host_cbs = (ag, a2a)                               # keep the trampolines alive
        self._ck(self._lib.alfd_comm_init_host(self._h, rank, world, C.cast(ag, C.c_void_p), C.cast(a2a, C.c_void_p),
                                               None))

    def set_partition(self, offsets):
        arrs = [np.ascontiguousarray(o, np.int64) for o in offsets]
        self._ck(self._lib.alfd_set_partition(self._h, len(arrs), _blocks(arrs)))

    # -- numbering of block 0 (alfd_set_numbering): before the uploads; operators, level-0 transfers, row blocks and
    # every block vector are then taken and returned in the caller's numbering
    def set_numbering(self, new_to_old):
        """Internal index k of block 0 is the caller's index new_to_old[k] (alfd_set_numbering); None or an empty
        array clears it."""
        p = np.ascontiguousarray([] if new_to_old is None else new_to_old, np.int64)
        if p.ndim != 1:
            raise ValueError("set_numbering: a 1-D permutation is required")
        self._ck(self._lib.alfd_set_numbering(self._h, p.size, p.ctypes.data if p.size else None))

    def set_numbering_from_points(self, points, brick=(16, 4, 1)):
        """Numbering and brick row blocks of A from one support point per block-0 unknown
        (alfd_set_numbering_from_points)."""
        pts = np.ascontiguousarray(points, np.float64)
        if pts.ndim != 2:
            raise ValueError("set_numbering_from_points: points must be [n][dim]")
        b = np.ones(3, np.int32)
        b[:len(brick)] = brick
        self._ck(self._lib.alfd_set_numbering_from_points(self._h, pts.shape[0], pts.shape[1], pts.ctypes.data,
                                                          b.ctypes.data))

    def numbering(self):
        """new_to_old of the numbering in force (alfd_get_numbering), or None."""
        n = C.c_int64(0)
        self._ck(self._lib.alfd_get_numbering(self._h, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        out = np.empty(n.value, np.int64)
        self._ck(self._lib.alfd_get_numbering(self._h, out.ctypes.data, out.size, C.byref(n)))
        return out

    # -- upload
    def set_matrix(self, slot, m):
        rp = np.ascontiguousarray(m.row_ptr, np.int64)
        col = np.ascontiguousarray(m.col, np.int32)
        val = np.ascontiguousarray(m.val, np.float64)
        self._ck(self._lib.alfd_set_matrix(self._h, slot, m.nrows, m.ncols, rp.ctypes.data, col.ctypes.data,
                                           val.ctypes.data))

    def set_diag(self, slot, d):
        d = np.ascontiguousarray(d, np.float64)
        self._ck(self._lib.alfd_set_diag(self._h, slot, d.size, d.ctypes.data))

    def set_aggregates(self, level, agg, n_coarse, weight=None):
        agg = np.ascontiguousarray(agg, np.int32)
        w = None if weight is None else np.ascontiguousarray(weight, np.float64)
        self._ck(self._lib.alfd_set_aggregates(self._h, level, agg.size, agg.ctypes.data,
                                               None if w is None else w.ctypes.data, int(n_coarse)))

    def set_prolongator(self, level, P, block=0):
        """CSR prolongator (problems.Csr, n_fine x n_coarse) of a multigrid level: alfd_set_prolongator_block.
        block 0: the hierarchy of the augmented (1,1) block; block 1: the one of the immersed block A22 of the
        elliptic-interface variants (level 0 has the rows of A2)."""
        self._ck(self._lib.alfd_set_prolongator_block(self._h, int(block), level, P.nrows, P.ncols,
                                                      P.row_ptr.ctypes.data, P.col.ctypes.data, P.val.ctypes.data))

    def aggregates(self, level, block=0):
        """(agg, n_coarse) of a level that build_aggregates / build_smoothed_aggregation formed or set_aggregates set
        (alfd_get_aggregates_block)."""
        nf, nc = C.c_int64(0), C.c_int64(0)
        self._ck(self._lib.alfd_get_aggregates_block(self._h, int(block), level, None, 0, C.byref(nf), C.byref(nc)))
        agg = np.empty(nf.value, np.int32)
        self._ck(self._lib.alfd_get_aggregates_block(self._h, int(block), level, agg.ctypes.data, agg.size, C.byref(nf),
                                                     C.byref(nc)))
        return agg, int(nc.value)

    def clear_hierarchy(self, block=0):
        """Forget the aggregates / prolongators of a block (alfd_clear_hierarchy); the next setup runs without."""
        self._ck(self._lib.alfd_clear_hierarchy(self._h, int(block)))

    def inner_iterations(self):
        """Inner CG iterations of the last solve by inner operator: {"aug", "a22", "aug2"} (alfd_get_inner_iterations)."""
        counts = np.zeros(3, np.int64)
        self._ck(self._lib.alfd_get_inner_iterations(self._h, counts.ctypes.data))
        return dict(aug=int(counts[0]), a22=int(counts[1]), aug2=int(counts[2]))

    def build_aggregates(self, block_size=1, threshold=0.02, max_aggregate_nodes=8, min_coarse=600, max_levels=7):
        """Algebraic aggregation from the uploaded A alone (alfd_build_aggregates); returns
        [(agg, n_coarse), ...] -- the list Context.set_aggregates / the oracle take."""
        nlev = C.c_int32(0)
        self._ck(self._lib.alfd_build_aggregates(self._h, block_size, threshold, max_aggregate_nodes, min_coarse,
                                                 max_levels, C.byref(nlev)))
        out = []
        for level in range(nlev.value):
            nf, nc = C.c_int64(0), C.c_int64(0)
            self._ck(self._lib.alfd_get_aggregates(self._h, level, None, 0, C.byref(nf), C.byref(nc)))
            agg = np.empty(nf.value, np.int32)
            self._ck(self._lib.alfd_get_aggregates(self._h, level, agg.ctypes.data, agg.size, C.byref(nf), C.byref(nc)))
            out.append((agg, int(nc.value)))
        return out

    def build_smoothed_aggregation(self, block_size=1, threshold=0.02, max_aggregate_nodes=8, damping=4.0 / 3.0,
                                   min_coarse=600, max_levels=7, return_omega=False, drop_tolerance=0.0,
                                   max_row_entries=0, block=0):
        """Smoothed aggregation from the uploaded operators (alfd_build_smoothed_aggregation): every level's
        prolongator P = P_tent - omega D^-1 Aug P_tent, built on the device.  Upload A (and C / Ct / W^-1 and
        configure an AL variant for the penalty term) first.  drop_tolerance / max_row_entries other than 0 truncate
        every row on the device (alfd_build_smoothed_aggregation_truncated: entries below drop_tolerance * the row
        maximum go, at most max_row_entries stay, the dropped mass is lumped per component).  Returns
        [(Csr P, n_coarse), ...] -- the list upload_problem and the oracle take; with return_omega also the damping
        omega of every level.  block = 1: the hierarchy of the immersed block, built from (A2, M, W^-1, gamma2)
        (alfd_build_smoothed_aggregation_block); it stays in the context for the next setup.
        On a row-partitioned context (block 0) the call is collective and builds the single-rank hierarchy bit for bit:
        the level-0 entry holds this rank's rows of P_0 (global coarse ids), the levels below are whole on every rank,
        omega is the same on all ranks; setup() then uses the hierarchy as it stands (do not hand it back through
        set_prolongator: caller-supplied level-0 prolongators must keep their support inside the rank's rows + halo)."""
        nlev = C.c_int32(0)
        omega = np.zeros(max(max_levels, 8), np.float64)   # ALFD_MAX_LEVELS - 1 entries when max_levels is out of range
        if block != 0:
            self._ck(self._lib.alfd_build_smoothed_aggregation_block(
                self._h, int(block), block_size, threshold, max_aggregate_nodes, damping, drop_tolerance,
                max_row_entries, min_coarse, max_levels, C.byref(nlev), omega.ctypes.data))
        elif drop_tolerance == 0.0 and max_row_entries == 0:
            self._ck(self._lib.alfd_build_smoothed_aggregation(self._h, block_size, threshold, max_aggregate_nodes,
                                                               damping, min_coarse, max_levels, C.byref(nlev),
                                                               omega.ctypes.data))
        else:
            self._ck(self._lib.alfd_build_smoothed_aggregation_truncated(
                self._h, block_size, threshold, max_aggregate_nodes, damping, drop_tolerance, max_row_entries,
                min_coarse, max_levels, C.byref(nlev), omega.ctypes.data))
        out = []
        for level in range(nlev.value):
            P = self.prolongator(level, block)
            out.append((P, int(P.ncols)))
        return (out, omega[:nlev.value].copy()) if return_omega else out

    def build_geometric_from_points(self, points, block=0, component=None, constrained=None, base=None, min_coarse=None,
                                    max_levels=7, return_cells=False, return_levels=True):
        """The geometric hierarchy of a block from one support point per unknown (alfd_build_geometric_from_points; the
        rule: include/alfd/alfd.h).  block 0: points [rows of A][dim]; constrained (flags per unknown) defaults to the
        rows of the uploaded A that hold nothing but their diagonal.  block 1: the points of the immersed unknowns (rows
        of A2), all nodes are unknowns.  component: per unknown, default the rank among the unknowns of its lattice node.
        base: cells per axis of the uniform base grid, needed on a locally refined mesh.  min_coarse defaults to 400
        (block 0) / 100 (block 1), those of problems.tensor_prolongators / immersed_tensor_prolongators.  The levels stay
        in the context for the next setup.  Returns [(Csr P, n_coarse), ...] (with return_cells also the cells per axis
        of the lattice and of every level's coarse grid, [levels + 1][dim]); return_levels=False returns the number of
        levels instead and copies nothing out."""
        pts, comp, con, b = _point_args(points, component, constrained, base)
        if min_coarse is None:
            min_coarse = 400 if block == 0 else 100
        nlev = C.c_int32(0)
        cells = np.zeros(8 * pts.shape[1], np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._ck(self._lib.alfd_build_geometric_from_points(self._h, int(block), pts.shape[0], pts.shape[1], pts.ctypes.data,
                                                            ptr(comp), ptr(con), ptr(b), int(min_coarse), int(max_levels),
                                                            C.byref(nlev), cells.ctypes.data))
        out = nlev.value
        if return_levels:
            out = [(P, int(P.ncols)) for P in (self.prolongator(level, block) for level in range(nlev.value))]
        if return_cells:
            return out, cells[:(nlev.value + 1) * pts.shape[1]].reshape(-1, pts.shape[1]).copy()
        return out

    def build_strength_graph(self, block_size=1, threshold=0.02):
        """The node graph of the algebraic aggregation from the resident rows of slot A, on the device
        (alfd_build_strength_graph; collective on a partitioned context, where it holds the rows of this rank's nodes
        with global neighbour ids).  Returns the dict of solver.host_strength_graph plus on_device (False: a node
        had too many neighbours for the kernel and every rank used the host routine)."""
        nn, nnz, dev = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._ck(self._lib.alfd_build_strength_graph(self._h, int(block_size), float(threshold), C.byref(nn),
                                                     C.byref(nnz)))
        d = np.empty(nn.value, np.float64)
        fixed = np.empty(nn.value, np.int32)
        ptr = np.empty(nn.value + 1, np.int64)
        nbr = np.empty(nnz.value, np.int32)
        w = np.empty(nnz.value, np.float64)
        self._ck(self._lib.alfd_get_strength_graph(self._h, d.ctypes.data, fixed.ctypes.data, ptr.ctypes.data,
                                                   nbr.ctypes.data, w.ctypes.data, nbr.size, C.byref(dev)))
        return dict(d=d, fixed=fixed, node_ptr=ptr, nbr=nbr, weight=w, on_device=bool(dev.value))

    def prolongator(self, level, block=0):
        """The CSR prolongator of a level as a problems.Csr (alfd_get_prolongator_block): built by
        build_smoothed_aggregation or set by set_prolongator."""
        from .problems import Csr
        nf, nc, nnz = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._ck(self._lib.alfd_get_prolongator_block(self._h, int(block), level, None, None, None, 0, C.byref(nf),
                                                      C.byref(nc), C.byref(nnz)))
        rp = np.empty(nf.value + 1, np.int64)
        col = np.empty(nnz.value, np.int32)
        val = np.empty(nnz.value, np.float64)
        self._ck(self._lib.alfd_get_prolongator_block(self._h, int(block), level, rp.ctypes.data, col.ctypes.data,
                                                      val.ctypes.data, col.size, C.byref(nf), C.byref(nc), C.byref(nnz)))
        return Csr(int(nf.value), int(nc.value), rp, col, val)

    def set_aggregate_partition(self, level, coarse_offsets):
        o = np.ascontiguousarray(coarse_offsets, np.int64)
        self._ck(self._lib.alfd_set_aggregate_partition(self._h, level, o.ctypes.data))

    def configure(self, cfg: _abi.Config):
        self.cfg = cfg
        self._ck(self._lib.alfd_configure(self._h, C.byref(cfg)))

    def set_controls(self, outer=None, inner=None, mp_inner=None):
        """New stop rules for the next solves, keeping the setup (alfd_set_controls)."""
        ref = lambda c: None if c is None else C.byref(c)
        self._ck(self._lib.alfd_set_controls(self._h, ref(outer), ref(inner), ref(mp_inner)))
        for name, c in (("outer", outer), ("inner", inner), ("mp_inner", mp_inner)):
            if c is not None:
                setattr(self.cfg, name, c)

    def setup(self, block_sizes):
        self._ck(self._lib.alfd_setup(self._h))
        self.block_sizes = [int(b) for b in block_sizes]

    def setup_coupling(self):
        """Re-setup after a change of the coupling alone (alfd_setup_coupling): CT / C / M / INVW uploaded again, or a
        config that differs in gamma / gamma2 only.  Keeps A, the level operators A_l and the transfers; same bits as a
        fresh setup.  Raises AlfdError (E_INVALID "needs alfd_setup", E_UNSUPPORTED, E_NOT_SETUP) where only setup()
        will do; the context is then unchanged."""
        self._ck(self._lib.alfd_setup_coupling(self._h))

    def setup_counts(self):
        """What the last setup() or setup_coupling() ran (alfd_get_setup_counts), by _abi.SETUP_COUNT_NAMES."""
        k = np.zeros(_abi.SC_NCOUNTS, np.int64)
        self._ck(self._lib.alfd_get_setup_counts(self._h, k.ctypes.data))
        return {name: int(k[i]) for i, name in enumerate(_abi.SETUP_COUNT_NAMES)}

    # -- hot path
    def _in(self, blocks):
        out = [np.ascontiguousarray(b, np.float64) for b in blocks]
        if [b.size for b in out] != self.block_sizes:
            raise ValueError(f"block sizes {[b.size for b in out]} != {self.block_sizes}")
        return out

    def precond_apply(self, src):
        src = self._in(src)
        dst = [np.zeros(n) for n in self.block_sizes]
        res = _abi.Result()
        self._ck(self._lib.alfd_precond_apply(self._h, _blocks(src), _blocks(dst), C.byref(res)))
        return dst, res

    def system_apply(self, src):
        src = self._in(src)
        dst = [np.zeros(n) for n in self.block_sizes]
        self._ck(self._lib.alfd_system_apply(self._h, _blocks(src), _blocks(dst)))
        return dst

    def augment_rhs(self, rhs):
        rhs = [b.copy() for b in self._in(rhs)]
        self._ck(self._lib.alfd_augment_rhs(self._h, _blocks(rhs)))
        return rhs

    def solve(self, rhs, x0=None, raise_on_failure=True):
        rhs = self._in(rhs)
        x = [np.zeros(n) for n in self.block_sizes] if x0 is None else [b.copy() for b in self._in(x0)]
        res = _abi.Result()
        rc = self._lib.alfd_solve(self._h, _blocks(rhs), _blocks(x), C.byref(res))
        if rc != _abi.OK and raise_on_failure:
            self._ck(rc)
        return x, res

    def upload_rhs(self, rhs, x0=None):
        rhs = self._in(rhs)
        x0_arrs = self._in(x0) if x0 is not None else None   # kept alive across the call (may be copies)
        x0b = _blocks(x0_arrs) if x0_arrs is not None else None
        self._ck(self._lib.alfd_upload_rhs(self._h, _blocks(rhs), x0b))
        del x0_arrs

    def solve_resident(self, raise_on_failure=True):
        res = _abi.Result()
        rc = self._lib.alfd_solve_resident(self._h, C.byref(res))
        if rc != _abi.OK and raise_on_failure:
            self._ck(rc)
        return res

    def download_solution(self):
        x = [np.zeros(n) for n in self.block_sizes]
        self._ck(self._lib.alfd_download_solution(self._h, _blocks(x)))
        return x

    # -- hot path on caller DEVICE buffers (alfd_*_device): no copy through the host
    def _dev(self, blocks, what, writable=False):
        """ctypes pointer table of one device array per block: any object with __cuda_array_interface__ (torch ROCm
        tensors, cupy arrays), float64, 1-D, contiguous, as long as its block.  The optional "stream" entry of the
        interface (version 3) is not read: the stream to wait for is the `stream` argument of the call alone, so for
        arrays that are not torch tensors pass it explicitly (None is the null stream for them)."""
        blocks = list(blocks)
        if self.block_sizes is None or len(blocks) != len(self.block_sizes):
            raise ValueError(f"{what}: {len(blocks)} blocks, the context has {self.block_sizes}")
        table = (C.c_void_p * len(blocks))()
        for b, (arr, n) in enumerate(zip(blocks, self.block_sizes)):
            try:
                cai = getattr(arr, "__cuda_array_interface__", None)
            except Exception as e:   # noqa: BLE001  (torch raises RuntimeError for a tensor that requires grad)
                raise ValueError(f"{what}[{b}] does not export __cuda_array_interface__: {e}") from None
            if cai is None:
                raise ValueError(f"{what}[{b}] has no __cuda_array_interface__ (a device array is required; "
                                 "host arrays go through the calls without _device)")
            shape, strides = tuple(cai["shape"]), cai.get("strides")
            if np.dtype(cai["typestr"]) != np.dtype(np.float64):
                raise ValueError(f"{what}[{b}]: dtype {cai['typestr']}, float64 is required")
            if len(shape) != 1:
                raise ValueError(f"{what}[{b}]: shape {shape}, a 1-D array is required")
            if shape[0] != n:
                raise ValueError(f"{what}[{b}]: length {shape[0]}, the block has {n}")
            if strides is not None and shape[0] > 1 and tuple(strides) != (8,):
                raise ValueError(f"{what}[{b}]: strides {tuple(strides)}, a contiguous array is required")
            ptr, readonly = cai["data"]
            if writable and readonly:
                raise ValueError(f"{what}[{b}] is read-only")
            table[b] = int(ptr) if n > 0 else None
        return table

    def _ck_dev(self, rc):
        """_ck for the *_device calls.  A refused block may be a tensor of ANOTHER HIP runtime: a torch wheel ships its
        own libamdhip64 and, imported after libalfd.so was loaded, runs on that second copy -- whose allocations the
        library's runtime does not know.  Say so instead of "not device memory" alone."""
        if rc == _abi.E_INVALID and len(_hip_runtimes()) > 1:
            msg = self._lib.alfd_last_error(self._h).decode() or self._lib.alfd_strerror(rc).decode()
            raise AlfdError(rc, msg + "; this process has loaded more than one HIP runtime (" +
                            ", ".join(_hip_runtimes()) + "): import torch before the first use of this package, "
                            "so that the tensors and the library share one")
        self._ck(rc)

    @staticmethod
    def _stream(stream, *block_lists):
        """Raw hipStream_t handle: an integer as given (0: the null stream), an object with .cuda_stream (a
        torch.cuda.Stream), None: torch's current stream on the tensors' device when torch is already imported and all
        arguments are torch tensors, else the null stream."""
        if stream is not None:
            return C.c_void_p(int(getattr(stream, "cuda_stream", stream)) or None)
        import sys
        torch = sys.modules.get("torch")
        arrs = [a for blocks in block_lists if blocks is not None for a in blocks]
        if torch is None or not arrs or not all(isinstance(a, torch.Tensor) for a in arrs):
            return C.c_void_p(None)
        return C.c_void_p(int(torch.cuda.current_stream(arrs[0].device).cuda_stream) or None)

    def precond_apply_device(self, src, dst, stream=None):
        """dst = P^-1 src on device arrays (alfd_precond_apply_device); dst may be src.  Returns the result record."""
        res = _abi.Result()
        self._ck_dev(self._lib.alfd_precond_apply_device(self._h, self._dev(src, "src"), self._dev(dst, "dst", True),
                                                     C.byref(res), self._stream(stream, src, dst)))
        return res

    def system_apply_device(self, src, dst, stream=None):
        """dst = AA src on device arrays (alfd_system_apply_device); dst may be src."""
        self._ck_dev(self._lib.alfd_system_apply_device(self._h, self._dev(src, "src"), self._dev(dst, "dst", True),
                                                    self._stream(stream, src, dst)))

    def augment_rhs_device(self, rhs, stream=None):
        """rhs[0] += gamma Ct invW rhs[last], in place on device arrays (alfd_augment_rhs_device)."""
        self._ck_dev(self._lib.alfd_augment_rhs_device(self._h, self._dev(rhs, "rhs", True), self._stream(stream, rhs)))

    def solve_device(self, rhs, x, stream=None, raise_on_failure=True):
        """Solve on device arrays (alfd_solve_device): x holds the initial guess on entry and the solution on return
        (also when the solve did not converge); x blocks may alias rhs blocks.  Returns the result record."""
        res = _abi.Result()
        rc = self._lib.alfd_solve_device(self._h, self._dev(rhs, "rhs"), self._dev(x, "x", True), C.byref(res),
                                         self._stream(stream, rhs, x))
        if rc != _abi.OK and raise_on_failure:
            self._ck_dev(rc)
        return res

    def upload_rhs_device(self, rhs, x0=None, stream=None):
        """alfd_upload_rhs_device: right-hand side and initial guess (None: zero) of solve_resident from device arrays."""
        x0t = self._dev(x0, "x0") if x0 is not None else None
        self._ck_dev(self._lib.alfd_upload_rhs_device(self._h, self._dev(rhs, "rhs"), x0t, self._stream(stream, rhs, x0)))

    def download_solution_device(self, x, stream=None):
        """alfd_download_solution_device: the solution of the last solve_resident into device arrays."""
        self._ck_dev(self._lib.alfd_download_solution_device(self._h, self._dev(x, "x", True), self._stream(stream, x)))

    def history(self):
        cnt = C.c_int32(0)
        self._lib.alfd_get_history(self._h, None, 0, C.byref(cnt))
        out = np.zeros(max(cnt.value, 1))
        self._lib.alfd_get_history(self._h, out.ctypes.data, cnt.value, C.byref(cnt))
        return out[:cnt.value]

    # -- primitives
    def spmv(self, slot, x, y=None, mode=0, alpha=1.0):
        x = np.ascontiguousarray(x, np.float64)
        lanes = C.c_int32()
        self._ck(self._lib.alfd_matrix_lanes(self._h, slot, C.byref(lanes)))
        if y is None:
            raise ValueError("pass y (its length is the row count)")
        y = np.ascontiguousarray(y, np.float64).copy()
        self._ck(self._lib.alfd_spmv(self._h, slot, x.ctypes.data, y.ctypes.data, mode, alpha))
        return y, lanes.value

    def spmv_scaled(self, slot, x, d, y, y2=None):
        """The diagonal-scaled epilogues (alfd_spmv_scaled): y = d .* (A x), or with y2 given y = A x and
        y2 = d .* (A x).  y (and y2) are uploaded as given before the launch; returns y or (y, y2), as copies."""
        x = np.ascontiguousarray(x, np.float64)
        d = np.ascontiguousarray(d, np.float64)
        y = np.ascontiguousarray(y, np.float64).copy()
        if d.size != y.size or (y2 is not None and np.size(y2) != y.size):
            raise ValueError("d, y and y2 have the row count of the slot")
        if y2 is None:
            self._ck(self._lib.alfd_spmv_scaled(self._h, slot, x.ctypes.data, d.ctypes.data, y.ctypes.data, None))
            return y
        y2 = np.ascontiguousarray(y2, np.float64).copy()
        self._ck(self._lib.alfd_spmv_scaled(self._h, slot, x.ctypes.data, d.ctypes.data, y.ctypes.data, y2.ctypes.data))
        return y, y2

    def spmv_pair(self, slot_a, slot_c, x, d, y, t):
        """The pair launch (alfd_spmv_pair): y = A x for slot_a and t = d .* (C x) for slot_c out of one launch.
        y and t are uploaded as given before the launch; returns (y, t) as copies.  AlfdError with status
        E_UNSUPPORTED when the two slots do not qualify."""
        x = np.ascontiguousarray(x, np.float64)
        d = np.ascontiguousarray(d, np.float64)
        y = np.ascontiguousarray(y, np.float64).copy()
        t = np.ascontiguousarray(t, np.float64).copy()
        if d.size != t.size:
            raise ValueError("d and t have the row count of slot_c")
        self._ck(self._lib.alfd_spmv_pair(self._h, slot_a, slot_c, x.ctypes.data, d.ctypes.data, y.ctypes.data,
                                          t.ctypes.data))
        return y, t

    def fused_tail_launches(self):
        """A launches with the block-end epilogue ("ml_tail_in_spmv") since the context was created."""
        out = C.c_int64()
        self._ck(self._lib.alfd_get_fused_tail_launches(self._h, C.byref(out)))
        return out.value

    def spmv_tail_step(self, slot_a, form, mode, ct, x, t, *, gamma=0.0, c1=0.0, c2=0.0, store_res=0, slot_c=-1,
                       w=None, **vecs):
        """One smoother step of A + gamma Ct invW C (alfd_spmv_tail_step).  form 0: the A launch with the block-end
        epilogue, then the rows party of the tail; form 1: y = A x, then the whole tail launch.  ct = (rp, col, val,
        ncols), the caller's Ct over the rows of slot_a.  vecs: the arrays dinv, rin, din, zin, y, res, d, z, zout the
        mode uses; an argument given as the string "x", or as the name of a vector earlier in that list, is passed at that
        vector's address.  Returns a dict with the vectors the
        call may have written (y, res, d, z, zout as given, and t when slot_c >= 0), as copies."""
        rp, col, val, ncols = ct
        rp = np.ascontiguousarray(rp, np.int64)
        col = np.ascontiguousarray(col, np.int32)
        val = np.ascontiguousarray(val, np.float64)
        x = np.ascontiguousarray(x, np.float64).copy()
        t = np.ascontiguousarray(t, np.float64).copy()
        s = _abi.TailStep()
        s.mode, s.store_res, s.slot_c = int(mode), int(store_res), int(slot_c)
        s.gamma, s.c1, s.c2 = float(gamma), float(c1), float(c2)
        s.ct_nrows, s.ct_ncols = rp.size - 1, int(ncols)
        s.ct_rp, s.ct_col, s.ct_val = rp.ctypes.data, col.ctypes.data, val.ctypes.data
        s.x, s.t = x.ctypes.data, t.ctypes.data
        keep = [rp, col, val, x, t]
        if w is not None:
            w = np.ascontiguousarray(w, np.float64)
            keep.append(w)
            s.w = w.ctypes.data
        out, named = {}, {}
        for name in ("dinv", "rin", "din", "zin", "y", "res", "d", "z", "zout"):
            v = vecs.pop(name, None)
            if v is None:
                continue
            if isinstance(v, str):   # "x", or a vector named earlier in the list above: one address, one device vector
                a = x if v == "x" else named[v]
            else:
                a = np.ascontiguousarray(v, np.float64).copy()
            keep.append(a)
            named[name] = a
            setattr(s, name, a.ctypes.data)
            if name in ("y", "res", "d", "z", "zout"):
                out[name] = a
        if vecs:
            raise TypeError(f"unknown vectors {sorted(vecs)}")
        self._ck(self._lib.alfd_spmv_tail_step(self._h, int(slot_a), int(form), C.byref(s)))
        if slot_c >= 0:
            out["t"] = t
        return out

    def last_spmv_launch(self):
        """What the last SpMV launch of this context instantiated (alfd_get_last_spmv_launch), as a dict with the
        family's name beside its number; AlfdError with status E_NOT_SETUP before the first launch."""
        rec = _abi.SpmvLaunch()
        self._ck(self._lib.alfd_get_last_spmv_launch(self._h, C.byref(rec)))
        out = rec.as_dict()
        out["family_name"] = _abi.SPMV_FAMILY_NAMES[rec.family]
        return out

    def dot(self, x, y):
        x = np.ascontiguousarray(x, np.float64)
        y = np.ascontiguousarray(y, np.float64)
        out = C.c_double()
        self._ck(self._lib.alfd_dot(self._h, x.size, x.ctypes.data, y.ctypes.data, C.byref(out)))
        return out.value

    def inner_prec_apply(self, r, op=_abi.INNER_OP_AUG):
        """z = M^-1 r: one application of the inner CG's preconditioner alone (alfd_inner_prec_apply).  op: the
        augmented (1,1) block (r as long as block 0), A22 of the modified elliptic variant (block 1), or the
        2-block operator of the ideal elliptic variant (blocks 0 and 1, one after the other)."""
        r = np.ascontiguousarray(r, np.float64)
        bs = self.block_sizes
        if bs is None:                      # not set up: the library answers ALFD_E_NOT_SETUP
            n = r.size
        else:
            n = {_abi.INNER_OP_AUG: bs[0], _abi.INNER_OP_A22: bs[1]}.get(op, bs[0] + bs[1])
            if r.size != n:
                raise ValueError(f"r has {r.size} entries, the inner operator {n}")
        z = np.zeros(n)
        self._ck(self._lib.alfd_inner_prec_apply(self._h, int(op), r.ctypes.data, z.ctypes.data))
        return z

    # -- sanity checks of the drivers (elliptic_interface.cc:973-1009)
    def estimate_spectrum(self, op=_abi.SPECTRUM_CCT, control=None):
        """cond(C Ct) by unpreconditioned CG from the all-ones right-hand side (alfd_estimate_spectrum): the
        _abi.Spectrum with the extreme Ritz values, their ratio and `converged`, the full-rank verdict.  control
        None: SolverControl(n_lambda, 1e-12)."""
        out = _abi.Spectrum()
        self._ck(self._lib.alfd_estimate_spectrum(self._h, int(op), None if control is None else C.byref(control),
                                                  C.byref(out)))
        return out

    def cg_coefficients(self):
        """(alpha_1..alpha_k, beta_1..beta_{k-1}) of the last estimate_spectrum."""
        cnt = C.c_int32(0)
        self._ck(self._lib.alfd_get_cg_coefficients(self._h, None, None, 0, C.byref(cnt)))
        alpha, beta = np.zeros(cnt.value), np.zeros(max(cnt.value, 1))
        self._ck(self._lib.alfd_get_cg_coefficients(self._h, alpha.ctypes.data, beta.ctypes.data, cnt.value,
                                                    C.byref(cnt)))
        return alpha, beta[:max(cnt.value - 1, 0)].copy()

    def constraint_residual(self, x, g=None):
        """|| (last block row of the system) x - g ||_inf (alfd_constraint_residual); g None: zero."""
        x = self._in(x)
        gv = None if g is None else np.ascontiguousarray(g, np.float64)
        if gv is not None and gv.size != self.block_sizes[-1]:
            raise ValueError(f"g has {gv.size} entries, the multiplier block {self.block_sizes[-1]}")
        out = C.c_double()
        self._ck(self._lib.alfd_constraint_residual(self._h, _blocks(x), None if gv is None else gv.ctypes.data,
                                                    C.byref(out)))
        return out.value

    def bench_spmv(self, slot, reps=20):
        ms, nbytes = C.c_double(), C.c_double()
        self._ck(self._lib.alfd_bench_spmv(self._h, slot, reps, C.byref(ms), C.byref(nbytes)))
        return ms.value, nbytes.value

    def bench_spmv_format(self, slot, reps=20, value_index=True):
        """(ms per launch, bytes streamed by format) with the value-indexed kernel on or off."""
        ms, nbytes = C.c_double(), C.c_double()
        self._ck(self._lib.alfd_bench_spmv_format(self._h, slot, reps, int(value_index), C.byref(ms),
                                                  C.byref(nbytes)))
        return ms.value, nbytes.value

    # -- single-precision operator values inside the inner preconditioner
    def set_preconditioner_values(self, kind):
        """"fp32": the inner preconditioner applies slot A through a binary32 copy of its values where the storage
        form allows it (preconditioner_values() says whether, and why not); "fp64" (the default): as always.  A call
        that changes the request un-sets the context up, like configure."""
        if kind not in _abi.PREC_VALUES_BY_NAME:
            raise ValueError(f"preconditioner values {kind!r}: 'fp32' or 'fp64'")
        self._ck(self._lib.alfd_set_preconditioner_values(self._h, _abi.PREC_VALUES_BY_NAME[kind]))

    def preconditioner_values(self):
        """alfd_get_preconditioner_values as a dict; reason_name / family_name spell the two enums out."""
        info = _abi.PrecValuesInfo()
        self._ck(self._lib.alfd_get_preconditioner_values(self._h, C.byref(info)))
        out = {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"}
        out["reason_name"] = _abi.PREC_VALUES_REASON_NAMES[info.reason]
        out["family_name"] = _abi.PREC_VALUES_FAMILY_NAMES[info.family] if info.stored else None
        return out

    def spmv_preconditioner(self, x, y, mode=0, alpha=1.0):
        """y = A~ x (mode 0) or fma(alpha, A~ x, y) (mode 1) on the binary32 copy of slot A, through the dispatch the
        multigrid cycle uses (alfd_spmv_preconditioner).  y is uploaded as given; returns a copy.  AlfdError with
        status E_UNSUPPORTED when no copy is stored."""
        x = np.ascontiguousarray(x, np.float64)
        y = np.ascontiguousarray(y, np.float64).copy()
        self._ck(self._lib.alfd_spmv_preconditioner(self._h, x.ctypes.data, y.ctypes.data, int(mode), float(alpha)))
        return y

    def bench_spmv_preconditioner(self, reps=20):
        """(ms per launch, bytes streamed by format) of y = A~ x, as bench_spmv."""
        ms, nbytes = C.c_double(), C.c_double()
        self._ck(self._lib.alfd_bench_spmv_preconditioner(self._h, reps, C.byref(ms), C.byref(nbytes)))
        return ms.value, nbytes.value

    def matrix_info(self, slot):
        """alfd_get_matrix_info, and the batch-major shape (alfd_get_matrix_shape) under batch_major_rows / _waves /
        _small / _batches / _lds_bytes and nrows."""
        info, shape = _abi.MatrixInfo(), _abi.BatchMajorShape()
        self._ck(self._lib.alfd_get_matrix_info(self._h, slot, C.byref(info)))
        self._ck(self._lib.alfd_get_matrix_shape(self._h, slot, C.byref(shape)))
        out = {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"}
        out.update({k: v for k, v in shape.as_dict().items() if k not in out})
        return out

    def side_rows(self, slot):
        """alfd_get_side_rows: rows, nnz, longest, interior_rows and grid of the side list of a long-row batch-major
        matrix (tunable "batch_major_side_rows"); all zero for a matrix without one."""
        info = _abi.SideRowsInfo()
        self._ck(self._lib.alfd_get_side_rows(self._h, slot, C.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def operator_info(self, op, level=0):
        """The batch-major shape of an operator the library built at setup (alfd_get_operator_shape), keys as in
        matrix_info: _abi.OPERATOR_LEVEL with level >= 1, _abi.OPERATOR_PATCH_SS, _abi.OPERATOR_PATCH_S."""
        shape = _abi.BatchMajorShape()
        self._ck(self._lib.alfd_get_operator_shape(self._h, op, level, C.byref(shape)))
        return shape.as_dict()

    def bench_operator(self, op, level=0, rows=0, waves=0, reps=200):
        """(microseconds per launch, shape) of such an operator as it is (rows = 0) or re-planned at rows x waves."""
        us, shape = C.c_double(), _abi.BatchMajorShape()
        self._ck(self._lib.alfd_bench_operator(self._h, op, level, rows, waves, reps, C.byref(us), C.byref(shape)))
        return us.value, shape.as_dict()

    def set_tunable(self, name, value):
        """Run-time switch (alfd_set_tunable), e.g. ("value_index", 0): general-matrix SpMV kernel."""
        self._ck(self._lib.alfd_set_tunable(self._h, name.encode(), int(value)))

    def sparse_product(self, A, P):
        """out = A P on the device whatever the size (alfd_sparse_product), with the bits of host_sparse_product; A, P
        problems.Csr.  Returns (problems.Csr, on_device): on_device is False when a product row has more than 1024
        distinct columns and the host routine formed the product."""
        on = C.c_int32(-1)
        out = _two_call_product(lambda *a: self._lib.alfd_sparse_product(self._h, *a, C.byref(on)), A, P, self._ck)
        return out, bool(on.value)

    def smoothed_prolongator(self, A, agg, n_coarse, omega, Ct=None, w_inv=None, gamma=0.0, block_size=1,
                             drop_tolerance=0.0, max_row_entries=0):
        """ONE level's smoothed prolongator from the caller's aggregates on the device (alfd_smoothed_prolongator), by
        the routines of build_smoothed_aggregation: host_smoothed_prolongator's arguments and the truncation rule's.
        Returns (problems.Csr, on_device): on_device is False when a row has more than 512 candidates and the host
        routines formed the rows."""
        on = C.c_int32(-1)
        tail = (int(block_size), float(drop_tolerance), int(max_row_entries))
        out = _two_call_prolongator(
            lambda head, *res: self._lib.alfd_smoothed_prolongator(self._h, *head, *tail, *res, C.byref(on)),
            A, agg, n_coarse, omega, Ct, w_inv, gamma, self._ck)
        return out, bool(on.value)

    def set_row_blocks(self, slot, block_ptr, rows):
        """Row-block hint of the batch-major SpMV format (alfd_set_row_blocks); None removes it."""
        if block_ptr is None:
            self._ck(self._lib.alfd_set_row_blocks(self._h, slot, 0, None, None))
            return
        bp = np.ascontiguousarray(block_ptr, np.int64)
        rw = np.ascontiguousarray(rows, np.int32)
        self._ck(self._lib.alfd_set_row_blocks(self._h, slot, bp.size - 1, bp.ctypes.data, rw.ctypes.data))

    def device_memory(self):
        """(free, total) bytes of the context's GPU."""
        f, t = C.c_int64(0), C.c_int64(0)
        self._ck(self._lib.alfd_get_device_memory(self._h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def enable_timing(self, on=True):
        self._ck(self._lib.alfd_enable_timing(self._h, int(on)))

    def timing(self):
        ms = np.zeros(_abi.T_NCLASSES)
        n = np.zeros(_abi.T_NCLASSES, np.int64)
        b = np.zeros(_abi.T_NCLASSES)
        self._ck(self._lib.alfd_get_timing(self._h, ms.ctypes.data, n.ctypes.data, b.ctypes.data))
        fb = np.zeros(_abi.T_NCLASSES)
        self._ck(self._lib.alfd_get_timing_streamed(self._h, fb.ctypes.data))
        names = ["spmv_A", "spmv_other", "dot", "vec"]
        return {k: dict(ms=float(ms[i]), launches=int(n[i]), bytes=float(b[i]), format_bytes=float(fb[i]))
                for i, k in enumerate(names)}

    def setup_seconds(self):
        """Wall seconds of the last uploads + setup by phase (alfd_get_setup_seconds)."""
        s = np.zeros(8)
        self._ck(self._lib.alfd_get_setup_seconds(self._h, s.ctypes.data))
        names = ["upload", "diag_lambda", "ml_fetch", "ml_galerkin", "ml_upload", "ml_lambda", "ml_patch", "ml_coarse"]
        return {k: float(s[i]) for i, k in enumerate(names)}


class LocalGroup:
    """In-process rank group (alfd_local_group): N contexts driven by N threads."""

    def __init__(self, nranks):
        self._lib = load_library()
        self.handle = C.c_void_p()
        rc = self._lib.alfd_local_group_create(nranks, C.byref(self.handle))
        if rc != _abi.OK:
            raise AlfdError(rc, "alfd_local_group_create failed")
        self.nranks = nranks

    def close(self):
        if self.handle:
            self._lib.alfd_local_group_destroy(self.handle)
            self.handle = None


def host_halo_plan(col, col_offsets, rank):
    """Host-only halo plan (no GPU): returns (col_local, halo_globals, recv_off)."""
    lib = load_library()
    col = np.ascontiguousarray(col, np.int32)
    offs = np.ascontiguousarray(col_offsets, np.int64)
    nranks = offs.size - 1
    col_local = np.empty_like(col)
    halo = np.empty(max(col.size, 1), np.int32)
    n_halo = C.c_int64()
    recv_off = np.zeros(nranks + 1, np.int64)
    rc = lib.alfd_host_halo_plan(col.size, col.ctypes.data, offs.ctypes.data, nranks, rank,
                                 col_local.ctypes.data, halo.ctypes.data, halo.size, C.byref(n_halo),
                                 recv_off.ctypes.data)
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_halo_plan failed")
    return col_local, halo[:n_halo.value].copy(), recv_off


def host_tridiagonal_extremes(alpha, beta):
    """Host-only: (lambda_min, lambda_max) of the Lanczos matrix T_k of the CG coefficients alpha_1..alpha_k,
    beta_1..beta_{k-1} (alfd_host_tridiagonal_extremes: Sturm-count bisection, no LAPACK)."""
    a = np.ascontiguousarray(alpha, np.float64)
    b = np.ascontiguousarray(beta, np.float64)
    if a.size > 1 and b.size < a.size - 1:
        raise ValueError("beta needs k - 1 entries")
    lo, hi = C.c_double(), C.c_double()
    rc = load_library().alfd_host_tridiagonal_extremes(a.size, a.ctypes.data, b.ctypes.data if b.size else None,
                                                       C.byref(lo), C.byref(hi))
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_tridiagonal_extremes: bad coefficients")
    return lo.value, hi.value


def host_aggregate_level(m, block_size=1, threshold=0.02, max_aggregate_nodes=8):
    """Host-only: one level of the library's algebraic aggregation on a problems.Csr; (agg, n_coarse)."""
    lib = load_library()
    rp = np.ascontiguousarray(m.row_ptr, np.int64)
    col = np.ascontiguousarray(m.col, np.int32)
    val = np.ascontiguousarray(m.val, np.float64)
    agg = np.empty(m.nrows, np.int32)
    nc = C.c_int64(0)
    rc = lib.alfd_host_aggregate_level(m.nrows, rp.ctypes.data, col.ctypes.data, val.ctypes.data, block_size,
                                       threshold, max_aggregate_nodes, agg.ctypes.data, C.byref(nc))
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_aggregate_level failed")
    return agg, int(nc.value)


def host_strength_graph(m, block_size=1, threshold=0.02):
    """Host-only: the node graph of one level of the algebraic aggregation on a problems.Csr
    (alfd_host_strength_graph): dict with d, fixed (per node), node_ptr, nbr, weight (strong neighbours ascending)."""
    lib = load_library()
    rp = np.ascontiguousarray(m.row_ptr, np.int64)
    col = np.ascontiguousarray(m.col, np.int32)
    val = np.ascontiguousarray(m.val, np.float64)
    if block_size < 1 or m.nrows % block_size:
        raise ValueError("rows must be a multiple of block_size")
    nn = m.nrows // block_size
    d = np.empty(nn, np.float64)
    fixed = np.empty(nn, np.int32)
    ptr = np.empty(nn + 1, np.int64)
    nnz = C.c_int64(0)

    def call(nb, w, cap):
        return lib.alfd_host_strength_graph(m.nrows, rp.ctypes.data, col.ctypes.data, val.ctypes.data, int(block_size),
                                            float(threshold), d.ctypes.data, fixed.ctypes.data, ptr.ctypes.data, nb, w,
                                            cap, C.byref(nnz))
    rc = call(None, None, 0)
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_strength_graph failed")
    nbr = np.empty(nnz.value, np.int32)
    w = np.empty(nnz.value, np.float64)
    rc = call(nbr.ctypes.data, w.ctypes.data, nbr.size)
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_strength_graph failed")
    return dict(d=d, fixed=fixed, node_ptr=ptr, nbr=nbr, weight=w)


def host_aggregate_graph(graph, block_size=1, max_aggregate_nodes=8):
    """Host-only: the greedy passes of the algebraic aggregation on a node graph (host_strength_graph, or the rows of
    Context.build_strength_graph gathered in rank order); (agg, n_coarse) as host_aggregate_level."""
    lib = load_library()
    fixed = np.ascontiguousarray(graph["fixed"], np.int32)
    ptr = np.ascontiguousarray(graph["node_ptr"], np.int64)
    nbr = np.ascontiguousarray(graph["nbr"], np.int32)
    w = np.ascontiguousarray(graph["weight"], np.float64)
    if ptr.size != fixed.size + 1 or nbr.size != w.size or nbr.size < ptr[-1]:
        raise ValueError("inconsistent node graph")
    agg = np.empty(fixed.size * block_size, np.int32)
    nc = C.c_int64(0)
    rc = lib.alfd_host_aggregate_graph(fixed.size, fixed.ctypes.data, ptr.ctypes.data, nbr.ctypes.data, w.ctypes.data,
                                       int(block_size), int(max_aggregate_nodes), agg.ctypes.data, C.byref(nc))
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_aggregate_graph failed")
    return agg, int(nc.value)


def _two_call_prolongator(fn, A, agg, n_coarse, omega, Ct, w_inv, gamma, check):
    """The two calls of alfd_host_smoothed_prolongator / alfd_smoothed_prolongator: fn(head, p_row_ptr, p_col, p_val,
    capacity, nnz) with head = the arguments the two share; check(rc) raises."""
    from .problems import Csr
    rp = np.ascontiguousarray(A.row_ptr, np.int64)
    col = np.ascontiguousarray(A.col, np.int32)
    val = np.ascontiguousarray(A.val, np.float64)
    agg = np.ascontiguousarray(agg, np.int32)
    if agg.size != A.nrows:
        raise ValueError("agg must have one entry per row of A")
    if Ct is not None:
        crp = np.ascontiguousarray(Ct.row_ptr, np.int64)
        ccol = np.ascontiguousarray(Ct.col, np.int32)
        cval = np.ascontiguousarray(Ct.val, np.float64)
        w = np.ascontiguousarray(w_inv, np.float64)
        if w.size != Ct.ncols:
            raise ValueError("w_inv must have one entry per column of Ct")
        pen = (int(Ct.ncols), crp.ctypes.data, ccol.ctypes.data, cval.ctypes.data, w.ctypes.data, float(gamma))
    else:
        pen = (0, None, None, None, None, 0.0)
    head = (A.nrows, rp.ctypes.data, col.ctypes.data, val.ctypes.data, *pen, agg.ctypes.data, int(n_coarse), float(omega))
    prp = np.empty(A.nrows + 1, np.int64)
    nnz = C.c_int64(0)
    check(fn(head, prp.ctypes.data, None, None, 0, C.byref(nnz)))
    pcol = np.empty(nnz.value, np.int32)
    pval = np.empty(nnz.value, np.float64)
    check(fn(head, prp.ctypes.data, pcol.ctypes.data, pval.ctypes.data, pcol.size, C.byref(nnz)))
    return Csr(int(A.nrows), int(n_coarse), prp, pcol, pval)


def host_smoothed_prolongator(A, agg, n_coarse, omega, Ct=None, w_inv=None, gamma=0.0):
    """Host-only: ONE level's smoothed-aggregation prolongator P = P_tent - omega D^-1 (A + gamma Ct diag(w_inv) Ct^T)
    P_tent with the library's arithmetic (alfd_host_smoothed_prolongator); A, Ct problems.Csr, agg from
    host_aggregate_level / Context.build_smoothed_aggregation.  Ct None: A alone.  Returns a problems.Csr."""
    lib = load_library()

    def check(rc):
        if rc != _abi.OK:
            raise AlfdError(rc, "alfd_host_smoothed_prolongator failed")
    return _two_call_prolongator(lambda head, *res: lib.alfd_host_smoothed_prolongator(*head, *res), A, agg, n_coarse,
                                 omega, Ct, w_inv, gamma, check)


def _two_call_product(fn, A, P, check):
    """The two calls of alfd_host_sparse_product / alfd_sparse_product: fn(operands..., out_row_ptr, out_col, out_val,
    capacity, nnz); check(rc) raises."""
    from .problems import Csr
    if A.ncols != P.nrows:
        raise ValueError("A has as many columns as P has rows")
    arp = np.ascontiguousarray(A.row_ptr, np.int64)
    acol = np.ascontiguousarray(A.col, np.int32)
    aval = np.ascontiguousarray(A.val, np.float64)
    prp = np.ascontiguousarray(P.row_ptr, np.int64)
    pcol = np.ascontiguousarray(P.col, np.int32)
    pval = np.ascontiguousarray(P.val, np.float64)
    if arp.size != A.nrows + 1 or prp.size != P.nrows + 1 or acol.size != aval.size or pcol.size != pval.size:
        raise ValueError("inconsistent CSR arrays")
    ops = (int(A.nrows), int(A.ncols), arp.ctypes.data, acol.ctypes.data, aval.ctypes.data, int(P.ncols),
           prp.ctypes.data, pcol.ctypes.data, pval.ctypes.data)
    orp = np.empty(A.nrows + 1, np.int64)
    nnz = C.c_int64(0)
    check(fn(*ops, orp.ctypes.data, None, None, 0, C.byref(nnz)))
    ocol = np.empty(nnz.value, np.int32)
    oval = np.empty(nnz.value, np.float64)
    check(fn(*ops, orp.ctypes.data, ocol.ctypes.data, oval.ctypes.data, ocol.size, C.byref(nnz)))
    return Csr(int(A.nrows), int(P.ncols), orp, ocol, oval)


def host_sparse_product(A, P):
    """Host-only: out = A P with the library's arithmetic (alfd_host_sparse_product: one fma chain per entry, the rows
    sorted by column, the pattern structural); A, P problems.Csr.  Returns a problems.Csr."""
    lib = load_library()

    def check(rc):
        if rc != _abi.OK:
            raise AlfdError(rc, "alfd_host_sparse_product failed")
    return _two_call_product(lib.alfd_host_sparse_product, A, P, check)


def host_truncate_prolongator(P, agg, block_size=1, drop_tolerance=0.0, max_row_entries=0):
    """Host-only: the truncation rule of Context.build_smoothed_aggregation(drop_tolerance, max_row_entries) applied to
    a problems.Csr prolongator (alfd_host_truncate_prolongator, the device's bits); agg as for
    host_smoothed_prolongator.  Returns a problems.Csr."""
    from .problems import Csr
    lib = load_library()
    rp = np.ascontiguousarray(P.row_ptr, np.int64)
    col = np.ascontiguousarray(P.col, np.int32)
    val = np.ascontiguousarray(P.val, np.float64)
    agg = np.ascontiguousarray(agg, np.int32)
    if agg.size != P.nrows:
        raise ValueError("agg must have one entry per row of P")
    orp = np.empty(P.nrows + 1, np.int64)
    nnz = C.c_int64(0)

    def call(oc, ov, cap):
        return lib.alfd_host_truncate_prolongator(P.nrows, P.ncols, rp.ctypes.data, col.ctypes.data, val.ctypes.data,
                                                  agg.ctypes.data, int(block_size), float(drop_tolerance),
                                                  int(max_row_entries), orp.ctypes.data, oc, ov, cap, C.byref(nnz))
    rc = call(None, None, 0)
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_truncate_prolongator failed")
    ocol = np.empty(nnz.value, np.int32)
    oval = np.empty(nnz.value, np.float64)
    rc = call(ocol.ctypes.data, oval.ctypes.data, ocol.size)
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_truncate_prolongator failed")
    return Csr(int(P.nrows), int(P.ncols), orp, ocol, oval)


def host_window_plan(m, lanes=64, value_index=True):
    """Host-only plan of the LDS-window / value-indexed storage of a problems.Csr (no GPU);
    returns the alfd_window_plan_info fields, incl. decode_mismatches (0 for a correct plan)."""
    lib = load_library()
    rp = np.ascontiguousarray(m.row_ptr, np.int64)
    col = np.ascontiguousarray(m.col, np.int32)
    val = np.ascontiguousarray(m.val, np.float64)
    info = _abi.WindowPlanInfo()
    rc = lib.alfd_host_window_plan(m.nrows, rp.ctypes.data, col.ctypes.data, val.ctypes.data, lanes,
                                   int(value_index), C.byref(info))
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_window_plan failed")
    return {k: getattr(info, k) for k, _ in info._fields_}


def host_stream_plan_short(m, lanes):
    """Host-only plan + decode of the short-row batch-major form (alfd_host_stream_plan_short; lanes = 8, 16, 32)."""
    lib = load_library()
    rp = np.ascontiguousarray(m.row_ptr, np.int64)
    col = np.ascontiguousarray(m.col, np.int32)
    val = np.ascontiguousarray(m.val, np.float64)
    info = _abi.StreamPlanInfo()
    rc = lib.alfd_host_stream_plan_short(m.nrows, rp.ctypes.data, col.ctypes.data, val.ctypes.data, lanes, C.byref(info))
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_stream_plan_short failed")
    return {k: getattr(info, k) for k, _ in info._fields_}


def _point_args(points, component, constrained, base):
    """The arrays of the point-hierarchy calls: points [n][dim] float64, component int32 / constrained uint8 per unknown
    or None, base int32 [dim] or None (a scalar stands for every axis)."""
    pts = np.ascontiguousarray(points, np.float64)
    if pts.ndim != 2 or pts.shape[0] < 1 or not 1 <= pts.shape[1] <= 3:
        raise ValueError("points must be [n][dim], dim 1..3")
    comp = None if component is None else np.ascontiguousarray(component, np.int32)
    con = None if constrained is None else np.ascontiguousarray(np.asarray(constrained) != 0, np.uint8)
    for a, what in ((comp, "component"), (con, "constrained")):
        if a is not None and a.shape != (pts.shape[0],):
            raise ValueError(what + " must have one entry per point")
    b = None
    if base is not None:
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(base, np.int32), (pts.shape[1],)))
    return pts, comp, con, b


def point_lattice(points):
    """Host-only: the lattice of a set of support points (alfd_host_point_lattice; the rule: include/alfd/alfd.h).
    Returns a dict: cells [dim] (m_d), lo [dim], delta [dim], index [n][dim], complete.  AlfdError (E_INVALID) for
    points that are not finite or no lattice."""
    pts = _point_args(points, None, None, None)[0]
    n, dim = pts.shape
    cells = np.zeros(dim, np.int32)
    lo, delta = np.zeros(dim), np.zeros(dim)
    index = np.empty((n, dim), np.int32)
    complete = C.c_int32(0)
    rc = load_library().alfd_host_point_lattice(n, dim, pts.ctypes.data, cells.ctypes.data, lo.ctypes.data,
                                                delta.ctypes.data, index.ctypes.data, C.byref(complete))
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_point_lattice: the points are not finite or no lattice")
    return dict(cells=cells, lo=lo, delta=delta, index=index, complete=bool(complete.value))


def point_prolongator(points, ncomp=1, component=None, constrained=None, base=None, boundary_unknowns=False):
    """Host-only: level 0 of the geometric hierarchy from support points (alfd_host_point_prolongator): the unknowns at
    the points from the Q1 space of the base grid (base=None: (cells + 1) // 2 per axis on a complete lattice).  Returns a
    problems.Csr (n x n_coarse)."""
    from .problems import Csr
    pts, comp, con, b = _point_args(points, component, constrained, base)
    n, dim = pts.shape
    ptr = lambda a: None if a is None else a.ctypes.data
    rp = np.empty(n + 1, np.int64)
    nnz, nc = C.c_int64(0), C.c_int64(0)

    def call(oc, ov, cap):
        rc = load_library().alfd_host_point_prolongator(n, dim, pts.ctypes.data, int(ncomp), ptr(comp), ptr(con), ptr(b),
                                                        int(bool(boundary_unknowns)), rp.ctypes.data, oc, ov, cap,
                                                        C.byref(nnz), C.byref(nc))
        if rc != _abi.OK:
            raise AlfdError(rc, "alfd_host_point_prolongator refused the points, the components or the base grid")
    call(None, None, 0)
    col = np.empty(nnz.value, np.int32)
    val = np.empty(nnz.value, np.float64)
    call(col.ctypes.data, val.ctypes.data, col.size)
    return Csr(n, int(nc.value), rp, col, val)


def grid_prolongator(dim, ncomp, fine_cells, coarse_cells, boundary_unknowns=False):
    """Host-only: one lower level of the geometric hierarchy (alfd_host_grid_prolongator): the unknowns of a grid of
    fine_cells per axis from those of a grid of coarse_cells.  Returns a problems.Csr."""
    from .problems import Csr
    fine = np.ascontiguousarray(np.broadcast_to(np.asarray(fine_cells, np.int32), (dim,)))
    coarse = np.ascontiguousarray(np.broadcast_to(np.asarray(coarse_cells, np.int32), (dim,)))
    nf, nc, nnz = C.c_int64(0), C.c_int64(0), C.c_int64(0)

    def call(orp, oc, ov, cap):
        rc = load_library().alfd_host_grid_prolongator(int(dim), int(ncomp), fine.ctypes.data, coarse.ctypes.data,
                                                       int(bool(boundary_unknowns)), orp, oc, ov, cap, C.byref(nf),
                                                       C.byref(nc), C.byref(nnz))
        if rc != _abi.OK:
            raise AlfdError(rc, "alfd_host_grid_prolongator refused the grids")
    call(None, None, None, 0)
    rp = np.empty(nf.value + 1, np.int64)
    col = np.empty(nnz.value, np.int32)
    val = np.empty(nnz.value, np.float64)
    call(rp.ctypes.data, col.ctypes.data, val.ctypes.data, col.size)
    return Csr(int(nf.value), int(nc.value), rp, col, val)


def point_hierarchy_cells(lattice_cells, ncomp=1, base=None, boundary_unknowns=False, min_coarse=400, max_levels=7):
    """Host-only: the level rule of the geometric hierarchy (alfd_host_point_hierarchy_cells): the cells per axis of every
    level's coarse grid, [levels][dim], for a lattice of lattice_cells."""
    m = np.ascontiguousarray(lattice_cells, np.int32)
    dim = m.size
    b = None if base is None else np.ascontiguousarray(np.broadcast_to(np.asarray(base, np.int32), (dim,)))
    nlev = C.c_int32(0)
    cells = np.zeros(8 * dim, np.int32)
    rc = load_library().alfd_host_point_hierarchy_cells(dim, int(ncomp), m.ctypes.data, None if b is None else b.ctypes.data,
                                                        int(bool(boundary_unknowns)), int(min_coarse), int(max_levels),
                                                        C.byref(nlev), cells.ctypes.data)
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_point_hierarchy_cells refused the base grid")
    return cells[:nlev.value * dim].reshape(nlev.value, dim).copy()


def point_hierarchy(points, ncomp=1, component=None, constrained=None, base=None, boundary_unknowns=False,
                    min_coarse=400, max_levels=7):
    """Host-only: the levels Context.build_geometric_from_points stores, e.g. for the oracle or for another solver
    instance: the grids of point_hierarchy_cells, level 0 from point_prolongator, the levels below from grid_prolongator
    between consecutive grids.  Returns [(Csr P, n_coarse), ...]; with boundary unknowns a lattice direction of one cell
    gives []."""
    lat = point_lattice(points)
    cells = point_hierarchy_cells(lat["cells"], ncomp, base, boundary_unknowns, min_coarse, max_levels)
    levels = []
    for level in range(cells.shape[0]):
        if level == 0:
            P = point_prolongator(points, ncomp, component, constrained, base, boundary_unknowns)
        else:
            P = grid_prolongator(cells.shape[1], ncomp, cells[level - 1], cells[level], boundary_unknowns)
        levels.append((P, int(P.ncols)))
    return levels


def numbering_from_points(points):
    """new_to_old permutation that puts unknowns into the lexicographic order of their support points
    (alfd_host_numbering_from_points); the components of a node stay together."""
    pts = np.ascontiguousarray(points, np.float64)
    out = np.empty(pts.shape[0], np.int64)
    rc = load_library().alfd_host_numbering_from_points(pts.shape[0], pts.shape[1], pts.ctypes.data, out.ctypes.data)
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_numbering_from_points")
    return out


def check_numbering(new_to_old):
    """old_to_new of a permutation new_to_old of [0, n) (alfd_host_check_numbering); AlfdError (E_INVALID) when an entry
    is out of range or repeated."""
    p = np.ascontiguousarray(new_to_old, np.int64)
    if p.ndim != 1:
        raise ValueError("check_numbering: a 1-D permutation is required")
    inv = np.empty(p.size, np.int64)
    rc = load_library().alfd_host_check_numbering(p.size, p.ctypes.data if p.size else None,
                                                  inv.ctypes.data if p.size else None)
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_check_numbering: not a permutation of [0, n)")
    return inv


def brick_blocks_from_points(points, brick=(16, 4, 1), max_rows=250):
    """(block_ptr, rows) for Context.set_row_blocks: mesh bricks found from support points alone
    (alfd_host_brick_blocks_from_points)."""
    pts = np.ascontiguousarray(points, np.float64)
    n, dim = pts.shape
    b = np.ascontiguousarray(list(brick)[:dim], np.int32)
    bp = np.empty(n + 1, np.int64)
    rows = np.empty(n, np.int32)
    nb = C.c_int64(0)
    rc = load_library().alfd_host_brick_blocks_from_points(n, dim, pts.ctypes.data, b.ctypes.data, max_rows, C.byref(nb),
                                                           bp.ctypes.data, rows.ctypes.data)
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_brick_blocks_from_points")
    return bp[:nb.value + 1].copy(), rows


def permute_csr(m, row_new_to_old=None, col_old_to_new=None):
    """problems.Csr permuted on the host (alfd_host_permute_csr): rows taken in the order row_new_to_old, column j
    renamed col_old_to_new[j], rows re-sorted."""
    from .problems import Csr
    rp = np.empty(m.nrows + 1, np.int64)
    col = np.empty(m.nnz, np.int32)
    val = np.empty(m.nnz, np.float64)
    r = None if row_new_to_old is None else np.ascontiguousarray(row_new_to_old, np.int64)
    c = None if col_old_to_new is None else np.ascontiguousarray(col_old_to_new, np.int64)
    rc = load_library().alfd_host_permute_csr(m.nrows, m.row_ptr.ctypes.data, m.col.ctypes.data, m.val.ctypes.data,
                                              None if r is None else r.ctypes.data, None if c is None else c.ctypes.data,
                                              rp.ctypes.data, col.ctypes.data, val.ctypes.data)
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_permute_csr")
    return Csr(m.nrows, m.ncols, rp, col, val)


def row_blocks_from_points(points, max_rows=192):
    """(block_ptr, rows) for Context.set_row_blocks from one support point per matrix row
    (alfd_host_row_blocks_from_points: recursive coordinate bisection, no grid metadata needed)."""
    lib = load_library()
    pts = np.ascontiguousarray(points, np.float64)
    n, dim = pts.shape
    ptr = np.zeros(n + 1, np.int64)
    rows = np.zeros(n, np.int32)
    nb = C.c_int64(0)
    rc = lib.alfd_host_row_blocks_from_points(n, dim, pts.ctypes.data, max_rows, C.byref(nb), ptr.ctypes.data,
                                              rows.ctypes.data)
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_row_blocks_from_points failed")
    return ptr[:nb.value + 1].copy(), rows


def host_stream_plan(m, row_block=96, blocks=None, side_rows=False):
    """Host-only plan + decode of the batch-major format (alfd_host_stream_plan);
    blocks = (block_ptr, rows) as for Context.set_row_blocks, or None for runs of row_block rows.
    side_rows=True: as planned under the tunable "batch_major_side_rows" (alfd_host_stream_plan_side); the result then
    also has "side_rows" (the rows of the side list, in its order) and "side_nnz"."""
    lib = load_library()
    rp = np.ascontiguousarray(m.row_ptr, np.int64)
    col = np.ascontiguousarray(m.col, np.int32)
    val = np.ascontiguousarray(m.val, np.float64)
    info = _abi.StreamPlanInfo()
    if side_rows:
        bp = None if blocks is None else np.ascontiguousarray(blocks[0], np.int64)
        rw = None if blocks is None else np.ascontiguousarray(blocks[1], np.int32)
        n_side, side_nnz, side = C.c_int64(), C.c_int64(), np.zeros(max(m.nrows, 1), np.int32)
        rc = lib.alfd_host_stream_plan_side(m.nrows, rp.ctypes.data, col.ctypes.data, val.ctypes.data, row_block,
                                            0 if bp is None else bp.size - 1, None if bp is None else bp.ctypes.data,
                                            None if rw is None else rw.ctypes.data, C.byref(n_side), side.ctypes.data,
                                            C.byref(side_nnz), C.byref(info))
        if rc != _abi.OK:
            raise AlfdError(rc, "alfd_host_stream_plan_side failed")
        out = {k: getattr(info, k) for k, _ in info._fields_}
        out["side_rows"], out["side_nnz"] = side[:n_side.value].copy(), side_nnz.value
        return out
    if blocks is None:
        rc = lib.alfd_host_stream_plan(m.nrows, rp.ctypes.data, col.ctypes.data, val.ctypes.data, row_block,
                                       0, None, None, C.byref(info))
    else:
        bp = np.ascontiguousarray(blocks[0], np.int64)
        rw = np.ascontiguousarray(blocks[1], np.int32)
        rc = lib.alfd_host_stream_plan(m.nrows, rp.ctypes.data, col.ctypes.data, val.ctypes.data, row_block,
                                       bp.size - 1, bp.ctypes.data, rw.ctypes.data, C.byref(info))
    if rc != _abi.OK:
        raise AlfdError(rc, "alfd_host_stream_plan failed")
    return {k: getattr(info, k) for k, _ in info._fields_}


def upload_problem(ctx: Context, pb, cfg: _abi.Config, aggregates=None, row_blocks=None, immersed_levels=None,
                   numbering=None, hierarchy_from_points=None) -> Context:
    """Upload a problems.SyntheticProblem (whole, or this rank's rows) with the
    reference's diagonal choices: W^-1 = 1/M_ii^2 (stokes...:976-978), lumped
    pressure mass (stokes...:946-954).  aggregates: [(agg, n_coarse), ...] for
    ALFD_PREC_MULTILEVEL (problems.geometric_aggregates), or [(Csr P, n_coarse), ...]
    (problems.tensor_prolongators), or a zero-argument callable returning either (evaluated on a helper
    thread while the operators are uploaded).  row_blocks: (block_ptr, rows)
    for the SpMV on A (Context.set_row_blocks, e.g. problems.brick_row_blocks).  immersed_levels:
    [(Csr P, n_coarse), ...] of the immersed block of an elliptic-interface problem (block 1:
    problems.immersed_tensor_prolongators); None leaves whatever the context holds for that block.  numbering: a
    new_to_old permutation of block 0 (Context.set_numbering) or an [n][dim] array of support points
    (Context.set_numbering_from_points), declared before the uploads: pb, aggregates and row_blocks stay in the problem's
    own numbering.  hierarchy_from_points: a dict that asks the library for the geometric hierarchy once the operators are
    uploaded (Context.build_geometric_from_points) -- "points" (block 0) and / or "immersed_points" (block 1), with
    "base", "min_coarse", "max_levels", "component", "constrained" for block 0 and "immersed_min_coarse" for block 1;
    it replaces what aggregates / immersed_levels set for that block."""
    if numbering is not None:
        if np.ndim(numbering) == 2:
            ctx.set_numbering_from_points(numbering)
        else:
            ctx.set_numbering(numbering)
    if row_blocks is not None:
        ctx.set_row_blocks(_abi.A, *row_blocks)
    for level, entry in enumerate(immersed_levels or []):
        ctx.set_prolongator(level, entry[0], block=1)

    def set_hierarchy(levels):
        for level, entry in enumerate(levels or []):
            agg, nc = entry[0], entry[1]
            if hasattr(agg, "row_ptr"):                       # a CSR prolongator (problems.tensor_prolongators)
                ctx.set_prolongator(level, agg)
                if len(entry) > 2 and entry[2] is not None:   # partitioned context: coarse offsets by rank (partition.local_prolongators)
                    ctx.set_aggregate_partition(level, entry[2])
                continue
            ctx.set_aggregates(level, agg, nc, entry[3] if len(entry) > 3 else None)   # 4th entry: prolongation weights
            if len(entry) > 2 and entry[2] is not None:      # (agg_local, n_coarse_global, coarse_offsets)
                ctx.set_aggregate_partition(level, entry[2])

    # aggregates may be a zero-argument callable: the transfer operators are then built on a helper thread while this one
    # uploads the operators (the library's format planning runs outside the interpreter lock), and handed over before setup
    pending = None
    if callable(aggregates):
        import threading
        box = {}

        def work():
            try:
                box["levels"] = aggregates()
            except BaseException as e:   # noqa: BLE001  (re-raised on the caller's thread)
                box["error"] = e
        pending = threading.Thread(target=work)
        pending.start()
    else:
        set_hierarchy(aggregates)

    def finish_hierarchy():
        if pending is not None:
            pending.join()
            if "error" in box:
                raise box["error"]
            set_hierarchy(box["levels"])
        if hierarchy_from_points is not None:
            ph = dict(hierarchy_from_points)
            pts0, pts1, mc1 = ph.pop("points", None), ph.pop("immersed_points", None), ph.pop("immersed_min_coarse", None)
            if pts0 is not None:
                ctx.build_geometric_from_points(pts0, block=0, return_levels=False, **ph)
            if pts1 is not None:
                ctx.build_geometric_from_points(pts1, block=1, min_coarse=mc1, max_levels=ph.get("max_levels", 7),
                                                return_levels=False)

    ctx.set_matrix(_abi.A, pb.mats["A"])
    # C before CT (and B before BT): an explicitly uploaded transpose is left alone, otherwise alfd_set_matrix(CT) would
    # first derive C on the host (a single-threaded transpose + upload) only to see it replaced by the next call
    ctx.set_matrix(_abi.C_, pb.mats["C"])
    ctx.set_matrix(_abi.CT, pb.mats["Ct"])
    if cfg.variant == _abi.RATIONAL:
        # rational branch (immersed_laplace.cc:585-631): K, Ct, immersed stiffness and mass
        ctx.set_matrix(_abi.M, pb.mats["M"])
        ctx.set_matrix(_abi.KIMM, pb.mats["K"])
        finish_hierarchy()
        ctx.configure(cfg)
        ctx.setup(pb.block_sizes)
        return ctx
    if "A2" in pb.mats:
        # elliptic interface: W^-1 = 1/(M^2)_ii (utilities.h:348-374, elliptic_interface.cc:726)
        ctx.set_matrix(_abi.A2, pb.mats["A2"])
        ctx.set_matrix(_abi.M, pb.mats["M"])
        ctx.set_diag(_abi.INVW, pb.inv_w_diag_of_mass_squared())
        finish_hierarchy()
        ctx.configure(cfg)
        ctx.setup(pb.block_sizes)
        return ctx
    if cfg.w_inverse != _abi.W_DIAGONAL:
        ctx.set_matrix(_abi.M, pb.mats["M"])     # exact W^-1: CG on the immersed mass matrix
    ctx.set_diag(_abi.INVW, pb.inv_w_diag_squared())
    if "B" in pb.mats:
        ctx.set_matrix(_abi.B, pb.mats["B"])
        ctx.set_matrix(_abi.BT, pb.mats["Bt"])
        ctx.set_matrix(_abi.MP, pb.mats["Mp"])
        ctx.set_diag(_abi.MP_LUMPED_INV, pb.mp_lumped_inv())
    finish_hierarchy()
    ctx.configure(cfg)
    ctx.setup(pb.block_sizes)
    return ctx


def update_coupling(ctx: Context, Ct, inv_w=None, M=None, C=None, gamma=None) -> Context:
    """The immersed body moved over a fixed background mesh: upload the new coupling and redo only what depends on it
    (Context.setup_coupling).  Ct: the new coupling matrix (problems.Csr, n_u x n_l), or None when the body stayed (a
    gamma sweep: nothing is uploaded and no product C_l P_l is formed); C: its transpose, formed here when None so that an
    explicitly uploaded C never meets the Ct of another position; inv_w: the new W^-1 diagonal; M: the new immersed mass
    matrix (exact W^-1, elliptic variants); gamma: a new penalty weight, configured on a copy of the context's config
    (the caller's Config object is left alone).  Block sizes must be those of the last setup."""
    if Ct is None and C is not None:
        raise ValueError("update_coupling: C without Ct")
    if Ct is not None:
        ctx.set_matrix(_abi.C_, Ct.transpose() if C is None else C)
        ctx.set_matrix(_abi.CT, Ct)
    if M is not None:
        ctx.set_matrix(_abi.M, M)
    if inv_w is not None:
        ctx.set_diag(_abi.INVW, inv_w)
    if gamma is not None:
        cfg = _abi.Config.from_buffer_copy(ctx.cfg)
        cfg.gamma = float(gamma)
        ctx.configure(cfg)
    ctx.setup_coupling()
    return ctx


def context_from_problem(pb, cfg: _abi.Config, device_id=0, aggregates=None, row_blocks=None,
                         immersed_levels=None, numbering=None, hierarchy_from_points=None) -> Context:
    return upload_problem(Context(device_id), pb, cfg, aggregates, row_blocks, immersed_levels, numbering, hierarchy_from_points)


# ---------------------------------------------------------------------------
# Reference-shaped front-ends.  A BlockVector is a list of numpy arrays.
class _ALPreconditionerBase:
    variant = None

    def __init__(self, ctx: Context):
        if ctx.cfg is None or ctx.cfg.variant != self.variant:
            raise ValueError("context is configured for a different preconditioner variant")
        self.ctx = ctx
        self.last_result = None

    def vmult(self, dst, src):
        """void vmult(BlockVector<double>& v, const BlockVector<double>& u) const"""
        out, self.last_result = self.ctx.precond_apply(src)
        for d, o in zip(dst, out):
            d[...] = o


class BlockPreconditionerAugmentedLagrangian(_ALPreconditionerBase):
    """augmented_lagrangian_preconditioner.h:14-42."""
    variant = _abi.AL2


class BlockPreconditionerAugmentedLagrangianStokes(_ALPreconditionerBase):
    """augmented_lagrangian_preconditioner.h:44-79."""
    variant = _abi.AL_STOKES


class BlockPreconditionerAugmentedLagrangianDiagonal(_ALPreconditionerBase):
    """augmented_lagrangian_preconditioner.h:81-110."""
    variant = _abi.AL_STOKES_DIAG


class BlockTriangularALPreconditioner(_ALPreconditionerBase):
    """EllipticInterfacePreconditioners::BlockTriangularALPreconditioner,
    augmented_lagrangian_preconditioner.h:115-164."""
    variant = _abi.AL_ELL_IDEAL


class BlockTriangularALPreconditionerModified(_ALPreconditionerBase):
    """EllipticInterfacePreconditioners::BlockTriangularALPreconditionerModified,
    augmented_lagrangian_preconditioner.h:168-238."""
    variant = _abi.AL_ELL_MODIFIED


class RationalPreconditioner(_ALPreconditionerBase):
    """rational_preconditioner.h:12-99."""
    variant = _abi.RATIONAL


class SystemOperator:
    """The block_operator AA (stokes_immersed_boundary.cc:1000-1003)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def vmult(self, dst, src):
        out = self.ctx.system_apply(src)
        for d, o in zip(dst, out):
            d[...] = o


class SolverMinRes:
    """SolverMinRes<BlockVector<double>> (immersed_laplace.cc:629-631, stokes...:1057-1064):
    the context must be configured with outer_solver = OUTER_MINRES."""

    def __init__(self, ctx: Context):
        if ctx.cfg is None or ctx.cfg.outer_solver != _abi.OUTER_MINRES:
            raise ValueError("context is not configured for MinRes")
        self.ctx = ctx
        self.last_result = None

    def solve(self, A, x, b, P):
        if A.ctx is not self.ctx or P.ctx is not self.ctx:
            raise ValueError("operator, preconditioner and solver must share one context")
        sol, self.last_result = self.ctx.solve(b, x0=x)
        for d, o in zip(x, sol):
            d[...] = o

    def last_step(self):
        return self.last_result.outer_iterations


class SolverFGMRES:
    """SolverFGMRES<BlockVector<double>> (stokes_immersed_boundary.cc:1067): the
    control lives in the context's alfd_config.outer; solve() runs wholly on the GPU."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.last_result = None

    def solve(self, A: SystemOperator, x, b, P: _ALPreconditionerBase):
        if A.ctx is not self.ctx or P.ctx is not self.ctx:
            raise ValueError("operator, preconditioner and solver must share one context")
        sol, self.last_result = self.ctx.solve(b, x0=x)
        for d, o in zip(x, sol):
            d[...] = o

    def last_step(self):
        return self.last_result.outer_iterations
