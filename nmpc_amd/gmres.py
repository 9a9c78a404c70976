"""Python mirror of the reference's nmpc_cgmres::Gmres interface for a BATCH of independent dense systems A x = b.

Same member names and meaning as nmpc_cgmres/include/nmpc_cgmres/Gmres.h:21-204 (`make_triangular_`, `apply_reorth_`, `solve()`,
`H_`, `g_`, `err_list_`, `basis_`), with a leading batch axis.  Everything numeric happens in libnmpc_hip_ddp.so through the C-ABI
(include/nmpc_hip_gmres.h); this file marshals arrays and re-raises status codes.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _capi

(FIELD_X, FIELD_ITERS, FIELD_REORTH, FIELD_ERR_LIST, FIELD_H, FIELD_G, FIELD_BASIS, FIELD_STATUS) = range(8)
MAX_DIM = 512
HOUSEHOLDER_MAX_K = 128
STATUS_CONVERGED, STATUS_K_MAX, STATUS_NON_FINITE = 1, 2, 3


class CConfig(C.Structure):
    """nmpc_hip_gmres_config (include/nmpc_hip_gmres.h): the arguments k_max, eps (Gmres.h:45-46) and the members of :195-196."""

    _fields_ = [
        ("k_max", C.c_int),
        ("eps", C.c_double),
        ("make_triangular", C.c_int),
        ("apply_reorth", C.c_int),
        ("keep_basis", C.c_int),
    ]


# every symbol include/nmpc_hip_gmres.h declares
EXPORTS = (
    "nmpc_hip_gmres_default_config", "nmpc_hip_gmres_create", "nmpc_hip_gmres_destroy", "nmpc_hip_gmres_set_config",
    "nmpc_hip_gmres_get_config", "nmpc_hip_gmres_set_system", "nmpc_hip_gmres_solve", "nmpc_hip_gmres_solve_device",
    "nmpc_hip_gmres_synchronize", "nmpc_hip_gmres_get", "nmpc_hip_gmres_field_bytes", "nmpc_hip_gmres_kernel_name",
    "nmpc_hip_gmres_last_ms", "nmpc_hip_gmres_last_error",
)

_declared = False


def load():
    """The library of nmpc_amd._capi with the GMRES prototypes declared."""
    global _declared
    L = _capi.load()
    if _declared:
        return L
    vp, sz = C.c_void_p, C.c_size_t
    L.nmpc_hip_gmres_default_config.argtypes = [C.POINTER(CConfig)]
    L.nmpc_hip_gmres_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.nmpc_hip_gmres_destroy.argtypes = [vp]
    L.nmpc_hip_gmres_set_config.argtypes = [vp, C.POINTER(CConfig)]
    L.nmpc_hip_gmres_get_config.argtypes = [vp, C.POINTER(CConfig)]
    L.nmpc_hip_gmres_set_system.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int]
    L.nmpc_hip_gmres_solve.argtypes = [vp]
    L.nmpc_hip_gmres_solve_device.argtypes = [vp, vp]
    L.nmpc_hip_gmres_synchronize.argtypes = [vp]
    L.nmpc_hip_gmres_get.argtypes = [vp, C.c_int, vp, sz, C.c_int]
    L.nmpc_hip_gmres_field_bytes.argtypes = [vp, C.c_int, C.POINTER(sz)]
    L.nmpc_hip_gmres_kernel_name.argtypes = [vp, C.POINTER(C.c_char_p)]
    L.nmpc_hip_gmres_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.nmpc_hip_gmres_last_error.argtypes = []
    L.nmpc_hip_gmres_last_error.restype = C.c_char_p
    for name in EXPORTS:
        if name != "nmpc_hip_gmres_last_error":
            getattr(L, name).restype = C.c_int
    _declared = True
    return L


def check(rc: int) -> None:
    """Status code -> ValueError (invalid argument) or RuntimeError."""
    if rc == _capi.OK:
        return
    msg = load().nmpc_hip_gmres_last_error().decode(errors="replace")
    if rc == _capi.ERR_INVALID_ARGUMENT:
        raise ValueError(msg)
    raise RuntimeError(f"[nmpc_hip_gmres {rc}] {msg}")


def default_config() -> CConfig:
    cfg = CConfig()
    check(load().nmpc_hip_gmres_default_config(C.byref(cfg)))
    return cfg


class GmresBatch:
    """`batch` independent Gmres solvers for systems of size n on one GPU: A [B][n][n], b / x [B][n].

    `k_max_capacity` sizes the device buffers (clamped to n); solve()'s k_max may not exceed it."""

    def __init__(self, n: int, batch: int, k_max_capacity: int = 100, device: int = 0):
        self.n = int(n)
        self.B = int(batch)
        self.make_triangular_ = True  # Gmres.h:195
        self.apply_reorth_ = True  # Gmres.h:196
        self.keep_basis = False
        self._L = load()
        h = C.c_void_p()
        check(self._L.nmpc_hip_gmres_create(self.n, self.B, int(k_max_capacity), device, C.byref(h)))
        self._h = h
        self._cfg = CConfig()
        check(self._L.nmpc_hip_gmres_get_config(self._h, C.byref(self._cfg)))
        self._keep = ()  # device tensors the handle reads in place

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._L.nmpc_hip_gmres_destroy(h)
            self._h = None

    def config(self) -> CConfig:
        """The configuration of the last push (k_max and eps are solve()'s arguments, the flags this object's members)."""
        return self._cfg

    def _push(self, k_max: Optional[int], eps: Optional[float]):
        if k_max is not None:
            self._cfg.k_max = int(k_max)
        if eps is not None:
            self._cfg.eps = float(eps)
        self._cfg.make_triangular = int(bool(self.make_triangular_))
        self._cfg.apply_reorth = int(bool(self.apply_reorth_))
        self._cfg.keep_basis = int(bool(self.keep_basis))
        check(self._L.nmpc_hip_gmres_set_config(self._h, C.byref(self._cfg)))

    def _arr(self, a, shape, name):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"{name}: shape {a.shape}, expected {shape}")
        return a

    def set_system(self, A, b, x0=None, a_col_major: bool = False) -> None:
        """Host arrays: A [B][n][n] (row-major (i, j), or with a_col_major its transposed image), b and x0 [B][n] (x0 None = zeros)."""
        B, n = self.B, self.n
        A = self._arr(A, (B, n, n), "A")
        b = self._arr(b, (B, n), "b")
        x0 = None if x0 is None else self._arr(x0, (B, n), "x0")
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(self._L.nmpc_hip_gmres_set_system(self._h, vp(A), vp(b), vp(x0), 0, int(a_col_major)))
        self._keep = ()

    def set_system_device(self, A, b, x0=None, a_col_major: bool = False) -> None:
        """Same with device tensors (torch, float64, contiguous, on this solver's device).  With a_col_major the handle reads A in
        place: this object keeps a reference to it until the next set_system."""
        B, n = self.B, self.n
        for name, t, shape in (("A", A, (B, n, n)), ("b", b, (B, n)), ("x0", x0, (B, n))):
            if t is None and name == "x0":
                continue
            if tuple(t.shape) != shape or str(t.dtype) != "torch.float64" or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"{name}: a contiguous float64 device tensor of shape {shape} is expected")
        x0p = None if x0 is None else C.c_void_p(x0.data_ptr())
        check(self._L.nmpc_hip_gmres_set_system(self._h, C.c_void_p(A.data_ptr()), C.c_void_p(b.data_ptr()), x0p, 1, int(a_col_major)))
        self._keep = (A,) if a_col_major else ()

    def solve(self, A=None, b=None, x=None, k_max: Optional[int] = None, eps: Optional[float] = None) -> np.ndarray:
        """Gmres::solve(A, b, x, k_max, eps) (Gmres.h:42-51) for every system; returns x [B][n].  Without A and b the systems of
        the last set_system are solved again from the previous x (restarted GMRES)."""
        if (A is None) != (b is None):
            raise ValueError("A and b come together")
        if A is not None:
            self.set_system(A, b, x)
        self._push(k_max, eps)
        check(self._L.nmpc_hip_gmres_solve(self._h))
        return self.x()

    def solve_device(self, k_max: Optional[int] = None, eps: Optional[float] = None, stream=None) -> None:
        """The systems of the last set_system / set_system_device, asynchronous on `stream` (torch stream or None for the solver's
        own); read the results after synchronize()."""
        self._push(k_max, eps)
        s = None if stream is None else C.c_void_p(stream.cuda_stream)
        check(self._L.nmpc_hip_gmres_solve_device(self._h, s))

    def synchronize(self) -> None:
        check(self._L.nmpc_hip_gmres_synchronize(self._h))

    def _get(self, field, dtype):
        n = C.c_size_t()
        check(self._L.nmpc_hip_gmres_field_bytes(self._h, field, C.byref(n)))
        out = np.zeros(n.value // np.dtype(dtype).itemsize, dtype=dtype)
        check(self._L.nmpc_hip_gmres_get(self._h, field, out.ctypes.data_as(C.c_void_p), n.value, 0))
        return out.reshape(self.B, -1)

    def get_device(self, field: int, out) -> None:
        """One field into a device tensor of exactly its size (nmpc_hip_gmres_get with on_device = 1)."""
        check(self._L.nmpc_hip_gmres_get(self._h, field, C.c_void_p(out.data_ptr()), out.numel() * out.element_size(), 1))

    def x(self) -> np.ndarray:
        return self._get(FIELD_X, np.float64)

    def iters(self) -> np.ndarray:
        return self._get(FIELD_ITERS, np.int32)[:, 0]

    def reorth(self) -> np.ndarray:
        return self._get(FIELD_REORTH, np.int32)[:, 0]

    def status(self) -> np.ndarray:
        return self._get(FIELD_STATUS, np.int32)[:, 0]

    @property
    def err_list_(self) -> np.ndarray:
        """[B][k_max + 1]; NaN beyond iters()."""
        return self._get(FIELD_ERR_LIST, np.float64)

    def errList(self, b: int) -> list:
        """err_list_ (Gmres.h:201) of system b: its ITERS + 1 entries."""
        return self.err_list_[b][: int(self.iters()[b]) + 1].tolist()

    @property
    def g_(self) -> np.ndarray:
        return self._get(FIELD_G, np.float64)

    @property
    def H_(self) -> np.ndarray:
        """[B][k_max + 1][k_max]"""
        g = self._get(FIELD_G, np.float64)
        K = g.shape[1] - 1
        return self._get(FIELD_H, np.float64).reshape(self.B, K + 1, K)

    @property
    def basis_(self) -> np.ndarray:
        """[B][k_max + 1][n]; rows 0 .. iters() are basis_ (Gmres.h:203).  Needs keep_basis = True at the solve."""
        return self._get(FIELD_BASIS, np.float64).reshape(self.B, -1, self.n)

    def kernelName(self) -> str:
        p = C.c_char_p()
        check(self._L.nmpc_hip_gmres_kernel_name(self._h, C.byref(p)))
        return p.value.decode()

    def lastMs(self) -> float:
        ms = C.c_float()
        check(self._L.nmpc_hip_gmres_last_ms(self._h, C.byref(ms)))
        return float(ms.value)
