"""ctypes binding of libhdbmi (include/hdbmi.h).

The product path: every call goes to the HIP library.  There is no CPU fallback -- if the
library is missing or no HIP device is visible, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HDBMI_LIB") or os.path.join(HERE, "lib", "libhdbmi.so")  # override: A/B builds

HDB_OK = 0
ERRORS = {
    -1: "HDB_EINVAL", -2: "HDB_EDEVICE", -3: "HDB_ENOMEM", -10: "HDB_EREF_NPE", -11: "HDB_EREF_OOB",
    -12: "HDB_EREF_NEGATIVE_CLUSTER", -13: "HDB_EREF_DIVZERO", -14: "HDB_EREF_NUMBER_FORMAT",
    -20: "HDB_EUNSUPPORTED",
}

METRIC = {"euclidean": 0, "cosine": 1, "pearson": 2, "manhattan": 3, "supremum": 4}
CORE_INCL_SELF_CUMULATIVE, CORE_INCL_SELF, CORE_EXCL_SELF = 0, 1, 2
EDGES_SELF, EDGES_MERGED = 1, 2  # hdb_exact_mst edge flags (include/hdbmi.h)
BUBBLE_COMBINESTEP, BUBBLE_CF = 0, 1
JMAX = float(np.finfo(np.float64).max)

# Java exceptions the reference raises on the same inputs.
class HdbError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class NullPointerException(HdbError):
    pass


class ArrayIndexOutOfBoundsException(HdbError):
    pass


class IllegalStateException(HdbError):
    """Clusters.java:45-46 "Cluster cannot have less than 0 points."."""


class ArithmeticException(HdbError):
    pass


class NumberFormatException(HdbError):
    """Double.parseDouble / Integer.parseInt on a malformed field."""


_EXC = {-10: NullPointerException, -11: ArrayIndexOutOfBoundsException, -12: IllegalStateException,
        -13: ArithmeticException, -14: NumberFormatException}

_vp = C.c_void_p  # every array, handle and opaque pointer
_i64, _i32, _int, _str = C.c_int64, C.c_int32, C.c_int, C.c_char_p
# One row per function of include/hdbmi.h: name -> (restype, argtypes); _int as restype is a status.
# lib() applies it, EXPORTED is its keys, and tests/test_capi.py compares every row with the header's
# prototype.
SIGNATURES = {
    "hdb_ctx_create": (_int, [_int, C.POINTER(_vp)]),
    "hdb_ctx_set_stream": (_int, [_vp, _vp]),
    "hdb_ctx_set_timing": (_int, [_vp, _int]),
    "hdb_ctx_kernel_time": (_int, [_vp, _str, C.POINTER(C.c_double), C.POINTER(_i64), _int]),
    "hdb_ctx_synchronize": (_int, [_vp]),
    "hdb_ctx_set_option": (_int, [_vp, _str, _i64]),
    "hdb_ctx_get_stat": (_int, [_vp, _str, C.POINTER(_i64)]),
    "hdb_distance_rows": (_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "hdb_core_distances": (_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "hdb_knn": (_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp]),
    "hdb_prim_mst": (_int, [_vp, _vp, _i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "hdb_prim_mst_batched": (_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "hdb_leaf_msts": (_int, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "hdb_mst_boruvka": (_int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp, _vp, _vp]),
    "hdb_exact_mst": (_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "hdb_nearest_sample": (_int, [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "hdb_attach_points": (_int, [_vp, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "hdb_attach_points_splits": (_int, [_vp, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "hdb_validity_index": (_int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, C.POINTER(C.c_double), _vp, _vp, _vp, _vp, _vp,
                                  _vp, _vp]),
    "hdb_validity_index_splits": (_int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, C.POINTER(C.c_double), _vp, _vp,
                                         _vp, _vp, _vp, _vp, _vp]),
    "hdb_validity_index_route": (_int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _i32, C.POINTER(C.c_double), _vp,
                                        _vp, _vp, _vp, _vp, _vp, _vp]),
    "hdb_bubble_stats": (_int, [_vp, _vp, _i64, _i32, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "hdb_bubble_partials": (_int, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _i32, _vp, _vp, _vp]),
    "hdb_bubble_combine": (_int, [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp]),
    "hdb_bubble_core_distances": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "hdb_bubble_prim_mst": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "hdb_local_model": (_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hdb_local_model_cores": (_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp]),
    "hdb_quicksort_edges": (_int, [_vp, _vp, _vp, _i64]),
    "hdb_sort_edges_desc": (_int, [_vp, _vp, _vp, _vp, _i64]),
    "hdb_merge_sorted_runs": (_int, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "hdb_flat_labels": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp]),
    "hdb_flat_outlier_scores": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "hdb_flat_cluster_tree": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp]),
    "hdb_labels_at_levels": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i32, _vp]),
    "hdb_predict_labels": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp]),
    "hdb_exemplars": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp]),
    "hdb_exemplar_distances": (_int, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp]),
    "hdb_exemplar_distances_splits": (_int, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp]),
    "hdb_membership_vectors": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "hdb_constrained_flat_labels": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp,
                                           _vp, _vp, _vp]),
    "hdb_local_mst_ids": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "hdb_comm_unique_id": (_int, [_vp, _i32]),
    "hdb_comm_init": (_int, [_vp, _i32, _i32, _vp, C.POINTER(_vp)]),
    "hdb_free": (_int, [_vp]),
    "hdb_copy": (_int, [_vp, _vp, _vp, _i64]),
    "hdb_merge_edges": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                               C.POINTER(_i64)]),
    "hdb_format_double": (_int, [C.c_double, _str, _i32]),
    "hdb_parse_points": (_int, [_str, _i64, _i32, _i32, _vp, _i64, _vp, _vp]),
    "hdb_format_mst_records": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    "hdb_parse_mst_records": (_int, [_str, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "hdb_last_error": (_str, []),
    "hdb_version": (_int, []),
    "hdb_ctx_destroy": (None, [_vp]),
    "hdb_comm_destroy": (None, [_vp]),
    "hdb_cluster_tree_bound": (_i64, [_i64, _i32]),
}
EXPORTED = list(SIGNATURES)

_lib = None
_lock = threading.Lock()


def lib():
    """Load libhdbmi.so; raise loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (SONAME
        # libamdhip64.so.7).  Loading torch first lets this library's NEEDED entry bind to
        # that runtime, so device pointers of torch tensors are valid here.  Loading us
        # first would map /opt/rocm's runtime and torch would then map a second one.
        try:
            import torch  # noqa: F401
        except ImportError:  # pragma: no cover - standalone use: /opt/rocm runtime
            pass
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libhdbmi.so not built ({LIB_PATH}); run build_lib.py / __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != HDB_OK:
        msg = lib().hdb_last_error().decode(errors="replace")
        raise _EXC.get(rc, HdbError)(rc, f"{what}: {msg}")


def call(name: str, *args, what: str | None = None):
    """One library call that returns a status: raises what check() raises."""
    check(getattr(lib(), name)(*args), what or name)


class Context:
    """One hdb_ctx per (thread, device); owns a stream (or borrows torch's)."""

    _tls = threading.local()
    _all: list = []  # every context created (diagnostic stat totals across threads)

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        call("hdb_ctx_create", device, C.byref(h))
        self.h = h
        self.device = device
        self._stream = None
        Context._all.append(self)

    @classmethod
    def stat_total(cls, name: str) -> int:
        return sum(c.get_stat(name) for c in cls._all)

    @classmethod
    def get(cls, device: int = 0) -> "Context":
        d = getattr(cls._tls, "ctxs", None)
        if d is None:
            d = cls._tls.ctxs = {}
        if device not in d:
            d[device] = Context(device)
        return d[device]

    def set_stream(self, stream_ptr: int | None):
        if stream_ptr != self._stream:
            call("hdb_ctx_set_stream", self.h, C.c_void_p(stream_ptr) if stream_ptr else None)
            self._stream = stream_ptr

    def use_torch_stream(self):
        import torch
        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def set_timing(self, on: bool):
        call("hdb_ctx_set_timing", self.h, int(on))

    def kernel_time(self, name: str, reset: bool = True):
        ms = C.c_double()
        n = C.c_int64()
        call("hdb_ctx_kernel_time", self.h, name.encode(), C.byref(ms), C.byref(n), int(reset))
        return ms.value, n.value

    def set_option(self, name: str, value: int):
        call("hdb_ctx_set_option", self.h, name.encode(), int(value))

    def get_stat(self, name: str) -> int:
        v = C.c_int64()
        call("hdb_ctx_get_stat", self.h, name.encode(), C.byref(v))
        return v.value

    def synchronize(self):
        call("hdb_ctx_synchronize", self.h)

    def __del__(self):
        try:
            if self.h and _lib is not None:
                _lib.hdb_ctx_destroy(self.h)
        except Exception:
            pass


# ------------------------------------------------------------- array plumbing
def is_torch(x) -> bool:
    try:
        import torch
        return isinstance(x, torch.Tensor)
    except ImportError:  # pragma: no cover
        return False


class Arr:
    """A caller array as (pointer, keep-alive), numpy (host) or torch (host/HIP)."""

    def __init__(self, x, dtype):
        if is_torch(x):
            import torch
            tdt = {np.float64: torch.float64, np.int32: torch.int32, np.int64: torch.int64}[dtype]
            t = x.contiguous()
            if t.dtype != tdt:
                t = t.to(tdt)
            self.obj = t
            self.ptr = t.data_ptr()
            self.device = t.device
        else:
            a = np.ascontiguousarray(x, dtype=dtype)
            self.obj = a
            self.ptr = a.ctypes.data
            self.device = None

    @property
    def p(self):
        return C.c_void_p(self.ptr)


def _on_device(a: Arr) -> bool:
    return a.device is not None and a.device.type == "cuda"


def context_for(ctx, *arrs: Arr, host_ok: bool = False):
    """The context a call runs on: an explicit ctx as it is; else this thread's context of the
    first array on a HIP device, on torch's current stream (ordered with the work that made the
    arrays); with host arrays only, None when the call has a host path (host_ok), else device 0."""
    if ctx is not None:
        return ctx
    for a in arrs:
        if _on_device(a):
            c = Context.get(a.device.index or 0)
            c.use_torch_stream()
            return c
    return None if host_ok else Context.get(0)


def new_like(ref: Arr, shape, dtype):
    if _on_device(ref):
        import torch
        tdt = {np.float64: torch.float64, np.int32: torch.int32, np.int64: torch.int64}[dtype]
        return torch.empty(shape, dtype=tdt, device=ref.device)
    return np.empty(shape, dtype=dtype)


def ptr(x):
    if x is None:
        return None
    if is_torch(x):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(x.ctypes.data)


def new_edges(ref: Arr, ne: int):
    """Empty (va, vb, w) for ne edges where ref lives."""
    return new_like(ref, (ne,), np.int32), new_like(ref, (ne,), np.int32), new_like(ref, (ne,), np.float64)
