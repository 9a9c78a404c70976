"""Python mirror of the reference's nmpc_ddp::BoxQP<VarDim> interface for a BATCH of independent box-constrained QPs.

Same member names and meaning as nmpc_ddp/include/nmpc_ddp/BoxQP.h:18-397 (`config()`, `solve()`, `retval_`, `retstr_`,
`free_idxs_`, `traceDataList()`), with a leading batch axis.  Everything numeric happens in libnmpc_hip_ddp.so through the C-ABI
(include/nmpc_hip_boxqp.h); this file marshals arrays and re-raises status codes.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _capi

(FIELD_X, FIELD_RETVAL, FIELD_ITER, FIELD_FACTORIZATION_NUM, FIELD_FREE_MASK, FIELD_OBJ, FIELD_FACTOR, FIELD_TRACE) = range(8)
MAX_DIM = 64
LANE_MAX_DIM = 16
AUTO_LANE_MAX_DIM, AUTO_LANE_MIN_BATCH = 3, 65536  # the automatic choice: lane iff var_dim <= 3 and batch >= 65536, else wave
TRACE_COLUMNS = ("iter", "obj", "factorization_num", "step_num", "clamped_mask", "grad_norm")
# one row of TRACE: doubles, except the clamped mask, which is the bit pattern of a uint64
TRACE_DTYPE = np.dtype([(name, np.uint64 if name == "clamped_mask" else np.float64) for name in TRACE_COLUMNS])

# retstr_ (BoxQP.h:375-383)
RETSTR = {
    -2: "Gradient of search direction is positive",
    -1: "Hessian is not positive definite",
    0: "Computation is not finished",
    1: "Maximum main iterations exceeded",
    2: "Maximum line-search iterations exceeded",
    3: "No bounds, returning Newton point",
    4: "Improvement smaller than tolerance",
    5: "Gradient norm smaller than tolerance",
    6: "All dimensions are clamped",
}


class CConfig(C.Structure):
    """nmpc_hip_boxqp_config (include/nmpc_hip_boxqp.h) = BoxQP::Configuration (BoxQP.h:33-55) without print_level."""

    _fields_ = [
        ("max_iter", C.c_int),
        ("grad_thre", C.c_double),
        ("rel_improve_thre", C.c_double),
        ("step_factor", C.c_double),
        ("min_step", C.c_double),
        ("armijo_param", C.c_double),
        ("trace_capacity", C.c_int),
    ]


# every symbol include/nmpc_hip_boxqp.h declares
EXPORTS = (
    "nmpc_hip_boxqp_default_config", "nmpc_hip_boxqp_create", "nmpc_hip_boxqp_destroy", "nmpc_hip_boxqp_set_config",
    "nmpc_hip_boxqp_get_config", "nmpc_hip_boxqp_solve", "nmpc_hip_boxqp_solve_device", "nmpc_hip_boxqp_synchronize",
    "nmpc_hip_boxqp_get", "nmpc_hip_boxqp_field_bytes", "nmpc_hip_boxqp_kernel_name", "nmpc_hip_boxqp_set_kernel",
    "nmpc_hip_boxqp_last_solve_ms", "nmpc_hip_boxqp_last_error",
)

_declared = False


def load():
    """The library of nmpc_amd._capi with the BoxQP prototypes declared."""
    global _declared
    L = _capi.load()
    if _declared:
        return L
    vp, dp, sz = C.c_void_p, C.POINTER(C.c_double), C.c_size_t
    L.nmpc_hip_boxqp_default_config.argtypes = [C.POINTER(CConfig)]
    L.nmpc_hip_boxqp_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.nmpc_hip_boxqp_destroy.argtypes = [vp]
    L.nmpc_hip_boxqp_set_config.argtypes = [vp, C.POINTER(CConfig)]
    L.nmpc_hip_boxqp_get_config.argtypes = [vp, C.POINTER(CConfig)]
    L.nmpc_hip_boxqp_solve.argtypes = [vp, dp, dp, dp, dp, dp]
    L.nmpc_hip_boxqp_solve_device.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.nmpc_hip_boxqp_synchronize.argtypes = [vp]
    L.nmpc_hip_boxqp_get.argtypes = [vp, C.c_int, vp, sz, C.c_int]
    L.nmpc_hip_boxqp_field_bytes.argtypes = [vp, C.c_int, C.POINTER(sz)]
    L.nmpc_hip_boxqp_kernel_name.argtypes = [vp, C.POINTER(C.c_char_p)]
    L.nmpc_hip_boxqp_set_kernel.argtypes = [vp, C.c_char_p]
    L.nmpc_hip_boxqp_last_solve_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.nmpc_hip_boxqp_last_error.argtypes = []
    L.nmpc_hip_boxqp_last_error.restype = C.c_char_p
    for name in EXPORTS:
        if name != "nmpc_hip_boxqp_last_error":
            getattr(L, name).restype = C.c_int
    _declared = True
    return L


def check(rc: int) -> None:
    """Status code -> ValueError (invalid argument) or RuntimeError."""
    if rc == _capi.OK:
        return
    msg = load().nmpc_hip_boxqp_last_error().decode(errors="replace")
    if rc == _capi.ERR_INVALID_ARGUMENT:
        raise ValueError(msg)
    raise RuntimeError(f"[nmpc_hip_boxqp {rc}] {msg}")


def _dp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def default_config() -> CConfig:
    cfg = CConfig()
    check(load().nmpc_hip_boxqp_default_config(C.byref(cfg)))
    return cfg


class BoxQPBatch:
    """`batch` independent BoxQP<var_dim> solvers on one GPU: H [B][n][n] (symmetric), g / lower / upper / initial_x [B][n]."""

    def __init__(self, var_dim: int, batch: int, device: int = 0):
        self.var_dim_ = int(var_dim)
        self.B = int(batch)
        self.print_level = 1  # BoxQP.h:36; stays on this side of the boundary
        self._L = load()
        h = C.c_void_p()
        check(self._L.nmpc_hip_boxqp_create(self.var_dim_, self.B, device, C.byref(h)))
        self._h = h
        self._cfg = CConfig()
        check(self._L.nmpc_hip_boxqp_get_config(self._h, C.byref(self._cfg)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._L.nmpc_hip_boxqp_destroy(h)
            self._h = None

    def config(self) -> CConfig:
        """BoxQP::config() (BoxQP.h:350-359); pushed to the library by the next solve."""
        return self._cfg

    def _push(self):
        check(self._L.nmpc_hip_boxqp_set_config(self._h, C.byref(self._cfg)))

    def _arr(self, a, shape, name):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"{name}: shape {a.shape}, expected {shape}")
        return a

    def solve(self, H, g, lower, upper, initial_x=None) -> np.ndarray:
        """BoxQP::solve (BoxQP.h:126-347) for every QP; returns x [B][n]."""
        self._push()
        B, n = self.B, self.var_dim_
        H = self._arr(H, (B, n, n), "H")
        g = self._arr(g, (B, n), "g")
        lower = self._arr(lower, (B, n), "lower")
        upper = self._arr(upper, (B, n), "upper")
        x0 = None if initial_x is None else self._arr(initial_x, (B, n), "initial_x")
        check(self._L.nmpc_hip_boxqp_solve(self._h, _dp(H), _dp(g), _dp(lower), _dp(upper), _dp(x0)))
        if self.print_level >= 2:
            for b, (r, it, o, f) in enumerate(zip(self.retval_, self.iter(), self.obj(), self.factorization_num())):
                print(f"[BoxQP] {b}: result: {r} ({RETSTR[int(r)]}), iter: {it}, obj: {o}, factorization_num: {f}")
        return self.x()

    def solve_device(self, H, g, lower, upper, initial_x=None, stream=None) -> None:
        """Same on device tensors (torch, float64, contiguous, on this solver's device), asynchronous on `stream` (torch stream or
        None for the solver's own); read the results with x() ... after synchronize()."""
        self._push()
        B, n = self.B, self.var_dim_
        for name, t, shape in (("H", H, (B, n, n)), ("g", g, (B, n)), ("lower", lower, (B, n)), ("upper", upper, (B, n)),
                               ("initial_x", initial_x, (B, n))):
            if t is None and name == "initial_x":
                continue
            if tuple(t.shape) != shape or str(t.dtype) != "torch.float64" or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"{name}: a contiguous float64 device tensor of shape {shape} is expected")
        s = None if stream is None else C.c_void_p(stream.cuda_stream)
        x0 = None if initial_x is None else C.c_void_p(initial_x.data_ptr())
        check(self._L.nmpc_hip_boxqp_solve_device(self._h, C.c_void_p(H.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(lower.data_ptr()),
                                                  C.c_void_p(upper.data_ptr()), x0, s))

    def synchronize(self) -> None:
        check(self._L.nmpc_hip_boxqp_synchronize(self._h))

    def _get(self, field, dtype, shape):
        n = C.c_size_t()
        check(self._L.nmpc_hip_boxqp_field_bytes(self._h, field, C.byref(n)))
        out = np.zeros(n.value // np.dtype(dtype).itemsize, dtype=dtype)
        check(self._L.nmpc_hip_boxqp_get(self._h, field, out.ctypes.data_as(C.c_void_p), n.value, 0))
        return out.reshape(shape)

    def get_device(self, field: int, out) -> None:
        """One field into a device tensor of exactly its size (nmpc_hip_boxqp_get with on_device = 1)."""
        check(self._L.nmpc_hip_boxqp_get(self._h, field, C.c_void_p(out.data_ptr()), out.numel() * out.element_size(), 1))

    def x(self, b: Optional[int] = None) -> np.ndarray:
        x = self._get(FIELD_X, np.float64, (self.B, self.var_dim_))
        return x if b is None else x[b]

    @property
    def retval_(self) -> np.ndarray:
        return self._get(FIELD_RETVAL, np.int32, (self.B,))

    def retval(self, b: int) -> int:
        return int(self.retval_[b])

    def retstr(self, b: int) -> str:
        return RETSTR[self.retval(b)]

    def iter(self) -> np.ndarray:
        return self._get(FIELD_ITER, np.int32, (self.B,))

    def factorization_num(self) -> np.ndarray:
        return self._get(FIELD_FACTORIZATION_NUM, np.int32, (self.B,))

    def free_mask(self) -> np.ndarray:
        return self._get(FIELD_FREE_MASK, np.uint64, (self.B,))

    def freeIdxs(self, b: int) -> list:
        """free_idxs_ (BoxQP.h:389) of QP b."""
        m = int(self.free_mask()[b])
        return [j for j in range(self.var_dim_) if m >> j & 1]

    def obj(self) -> np.ndarray:
        return self._get(FIELD_OBJ, np.float64, (self.B,))

    def factor(self) -> np.ndarray:
        """[B][n][n]: the lower Cholesky factor of H[free, free] in the leading nf x nf corner (llt_free_, BoxQP.h:386)."""
        return self._get(FIELD_FACTOR, np.float64, (self.B, self.var_dim_, self.var_dim_))

    def trace(self) -> np.ndarray:
        """[B][trace_capacity] records with the fields TRACE_COLUMNS; rows beyond iter()[b] were not written by the last solve."""
        raw = self._get(FIELD_TRACE, np.float64, (-1,))
        return raw.view(TRACE_DTYPE).reshape(self.B, -1)

    def traceDataList(self, b: int) -> list:
        """traceDataList() (BoxQP.h:362) of QP b: its scalar members, one dict per entry (the initial one first), as far as
        trace_capacity reaches."""
        rows = self.trace()[b][: int(self.iter()[b]) + 1]
        return [dict(iter=int(r["iter"]), obj=float(r["obj"]), factorization_num=int(r["factorization_num"]), step_num=int(r["step_num"]),
                     clamped_flag=[bool(int(r["clamped_mask"]) >> j & 1) for j in range(self.var_dim_)], grad_norm=float(r["grad_norm"]))
                for r in rows]

    def kernelName(self) -> str:
        p = C.c_char_p()
        check(self._L.nmpc_hip_boxqp_kernel_name(self._h, C.byref(p)))
        return p.value.decode()

    def setKernel(self, kernel: Optional[str]) -> None:
        """"lane", "wave" or None (the automatic choice)."""
        check(self._L.nmpc_hip_boxqp_set_kernel(self._h, None if kernel is None else kernel.encode()))

    def lastSolveMs(self) -> float:
        ms = C.c_float()
        check(self._L.nmpc_hip_boxqp_last_solve_ms(self._h, C.byref(ms)))
        return float(ms.value)
