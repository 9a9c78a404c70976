"""Batched Riccati backward pass on caller-supplied derivatives: the model-free part of the reference's DDP solver.

`RiccatiBatch` runs DDPSolver::backwardPass (nmpc_ddp/include/nmpc_ddp/DDPSolver.hpp:342-534) with the lambda retry loop (:188-214)
and the BoxQP feed-forward (:450-497) for a batch of instances whose Derivative blocks (Fx, Fu, Lx, Lu, Lxx, Luu, Lxu) and terminal
Vx, Vxx come from anywhere: a network differentiated with autograd, a simulator, a table.  Everything numeric happens in
libnmpc_hip_ddp.so through the C-ABI (include/nmpc_hip_riccati.h); this file marshals arrays and re-raises status codes.  There is
no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _capi

(FIELD_K_FF, FIELD_K_FB, FIELD_DV, FIELD_VX0, FIELD_VXX0, FIELD_STATUS, FIELD_N_BACKWARD, FIELD_LAMBDA, FIELD_DLAMBDA, FIELD_FAIL_STEP,
 FIELD_QP_RETVAL, FIELD_FREE_MASK) = range(12)
MAX_DIM = 16
STATUS_OK, STATUS_LAMBDA_MAX, STATUS_PASS_FAILED = 1, -1, -2


class CConfig(C.Structure):
    """nmpc_hip_riccati_config (include/nmpc_hip_riccati.h)."""

    _fields_ = [
        ("reg_type", C.c_int),
        ("lambda_", C.c_double),  # `lambda` in C
        ("dlambda", C.c_double),
        ("lambda_factor", C.c_double),
        ("lambda_min", C.c_double),
        ("lambda_max", C.c_double),
        ("with_input_constraint", C.c_int),
        ("retry", C.c_int),
        ("row_major", C.c_int),
    ]


# every symbol include/nmpc_hip_riccati.h declares
EXPORTS = (
    "nmpc_hip_riccati_default_config", "nmpc_hip_riccati_create", "nmpc_hip_riccati_destroy", "nmpc_hip_riccati_set_config",
    "nmpc_hip_riccati_get_config", "nmpc_hip_riccati_set_input_dims", "nmpc_hip_riccati_set_derivatives", "nmpc_hip_riccati_set_inputs",
    "nmpc_hip_riccati_set_lambda", "nmpc_hip_riccati_solve", "nmpc_hip_riccati_solve_device", "nmpc_hip_riccati_synchronize",
    "nmpc_hip_riccati_get", "nmpc_hip_riccati_field_bytes", "nmpc_hip_riccati_kernel_name", "nmpc_hip_riccati_last_ms",
    "nmpc_hip_riccati_last_error",
)

_declared = False


def load():
    """The library of nmpc_amd._capi with the Riccati prototypes declared."""
    global _declared
    L = _capi.load()
    if _declared:
        return L
    vp, sz = C.c_void_p, C.c_size_t
    L.nmpc_hip_riccati_default_config.argtypes = [C.POINTER(CConfig)]
    L.nmpc_hip_riccati_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.nmpc_hip_riccati_destroy.argtypes = [vp]
    L.nmpc_hip_riccati_set_config.argtypes = [vp, C.POINTER(CConfig)]
    L.nmpc_hip_riccati_get_config.argtypes = [vp, C.POINTER(CConfig)]
    L.nmpc_hip_riccati_set_input_dims.argtypes = [vp, vp]
    L.nmpc_hip_riccati_set_derivatives.argtypes = [vp] + [vp] * 9 + [C.c_int]
    L.nmpc_hip_riccati_set_inputs.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int]
    L.nmpc_hip_riccati_set_lambda.argtypes = [vp, vp, vp, C.c_int]
    L.nmpc_hip_riccati_solve.argtypes = [vp]
    L.nmpc_hip_riccati_solve_device.argtypes = [vp, vp]
    L.nmpc_hip_riccati_synchronize.argtypes = [vp]
    L.nmpc_hip_riccati_get.argtypes = [vp, C.c_int, vp, sz, C.c_int]
    L.nmpc_hip_riccati_field_bytes.argtypes = [vp, C.c_int, C.POINTER(sz)]
    L.nmpc_hip_riccati_kernel_name.argtypes = [vp, C.POINTER(C.c_char_p)]
    L.nmpc_hip_riccati_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.nmpc_hip_riccati_last_error.argtypes = []
    L.nmpc_hip_riccati_last_error.restype = C.c_char_p
    for name in EXPORTS:
        if name != "nmpc_hip_riccati_last_error":
            getattr(L, name).restype = C.c_int
    _declared = True
    return L


def check(rc: int) -> None:
    """Status code -> ValueError (invalid argument) or RuntimeError."""
    if rc == _capi.OK:
        return
    msg = load().nmpc_hip_riccati_last_error().decode(errors="replace")
    if rc == _capi.ERR_INVALID_ARGUMENT:
        raise ValueError(msg)
    raise RuntimeError(f"[nmpc_hip_riccati {rc}] {msg}")


def default_config() -> CConfig:
    cfg = CConfig()
    check(load().nmpc_hip_riccati_default_config(C.byref(cfg)))
    return cfg


class Result:
    """One backward pass per instance: k [B, T, m], K [B, T, m, n], dV [B, 2], Vx0 [B, n], Vxx0 [B, n, n], status / n_backward /
    fail_step [B], lam / dlam [B] (to be carried into the caller's next iteration), qp_retval / free_mask [B, T].  numpy arrays from
    backward(), torch tensors from backwardDevice()."""

    __slots__ = ("k", "K", "dV", "Vx0", "Vxx0", "status", "n_backward", "lam", "dlam", "fail_step", "qp_retval", "free_mask")


_DERIVATIVES = ("Fx", "Fu", "Lx", "Lu", "Lxx", "Luu", "Lxu", "Vx_T", "Vxx_T")


class RiccatiBatch:
    """`batch` instances of state dimension n, input capacity m and T steps on one GPU."""

    def __init__(self, n: int, m: int, T: int, batch: int, device: int = 0):
        self.n, self.m, self.T, self.B = int(n), int(m), int(T), int(batch)
        self.device = int(device)
        self._L = load()
        h = C.c_void_p()
        check(self._L.nmpc_hip_riccati_create(self.n, self.m, self.T, self.B, self.device, C.byref(h)))
        self._h = h
        self._cfg = CConfig()
        check(self._L.nmpc_hip_riccati_get_config(self._h, C.byref(self._cfg)))
        self._keep = ()  # device tensors the handle reads in place
        self._lam = self._dlam = None  # setLambda's host arrays
        self._device_lambda = False
        self._side_stream = None  # see backwardDevice

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._L.nmpc_hip_riccati_destroy(h)
            self._h = None

    def config(self) -> CConfig:
        """The configuration; pushed to the library by the next backward (which sets row_major itself)."""
        return self._cfg

    def setInputDims(self, dims) -> None:
        """Fu.cols() per step ([T], each 0 .. m), shared by the batch; None = m everywhere."""
        if dims is None:
            check(self._L.nmpc_hip_riccati_set_input_dims(self._h, None))
            return
        d = np.ascontiguousarray(dims, dtype=np.int32)
        if d.shape != (self.T,):
            raise ValueError(f"dims: shape {d.shape}, expected {(self.T,)}")
        check(self._L.nmpc_hip_riccati_set_input_dims(self._h, d.ctypes.data_as(C.c_void_p)))

    def setLambda(self, lam=None, dlam=None) -> None:
        """lambda_ and dlambda_ per instance ([B] each, host arrays); None = the config's scalar.  backwardDevice's own lam / dlam
        take their place for that call."""
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        lam = None if lam is None else self._arr(lam, (self.B,), "lam")
        dlam = None if dlam is None else self._arr(dlam, (self.B,), "dlam")
        check(self._L.nmpc_hip_riccati_set_lambda(self._h, vp(lam), vp(dlam), 0))
        self._lam, self._dlam, self._device_lambda = lam, dlam, False

    def _arr(self, a, shape, name):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"{name}: shape {a.shape}, expected {shape}")
        return a

    def _shapes(self, limits_per_step: bool):
        B, T, n, m = self.B, self.T, self.n, self.m
        lim = (B, T, m) if limits_per_step else (m,)
        return dict(Fx=(B, T, n, n), Fu=(B, T, n, m), Lx=(B, T, n), Lu=(B, T, m), Lxx=(B, T, n, n), Luu=(B, T, m, m), Lxu=(B, T, n, m),
                    Vx_T=(B, n), Vxx_T=(B, n, n), U=(B, T, m), lower=lim, upper=lim)

    def _push(self, row_major: bool, constrained: bool):
        self._cfg.row_major = int(row_major)
        self._cfg.with_input_constraint = int(constrained)
        check(self._L.nmpc_hip_riccati_set_config(self._h, C.byref(self._cfg)))

    def backward(self, Fx, Fu, Lx, Lu, Lxx, Luu, Lxu, Vx_T, Vxx_T, U=None, lower=None, upper=None, col_major: bool = False) -> Result:
        """One backward pass (with retries) on host arrays [B, T, rows, cols] (Vx_T [B, n], Vxx_T [B, n, n]).  With U, lower and upper
        (lower / upper [m], or [B, T, m] per step) the feed-forward is the BoxQP's.  col_major: the matrix blocks are handed over and
        returned column-major instead (arrays [B, T, cols, rows])."""
        constrained = U is not None
        if constrained and (lower is None or upper is None):
            raise ValueError("U, lower and upper come together")
        per_step = constrained and np.ndim(lower) == 3
        shapes = self._shapes(per_step)
        if col_major:
            shapes = {k: (s[:-2] + (s[-1], s[-2]) if k in ("Fx", "Fu", "Lxx", "Luu", "Lxu", "Vxx_T") else s) for k, s in shapes.items()}
        given = dict(Fx=Fx, Fu=Fu, Lx=Lx, Lu=Lu, Lxx=Lxx, Luu=Luu, Lxu=Lxu, Vx_T=Vx_T, Vxx_T=Vxx_T, U=U, lower=lower, upper=upper)
        a = {k: self._arr(v, shapes[k], k) for k, v in given.items() if v is not None}
        self._push(not col_major, constrained)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        check(self._L.nmpc_hip_riccati_set_derivatives(self._h, *[vp(a[k]) for k in _DERIVATIVES], 0))
        if constrained:
            check(self._L.nmpc_hip_riccati_set_inputs(self._h, vp(a["U"]), vp(a["lower"]), vp(a["upper"]), int(per_step), 0))
        if self._device_lambda:  # the tensors of the last backwardDevice are let go: back to setLambda's arrays or the scalars
            self.setLambda(self._lam, self._dlam)
        self._keep = ()
        check(self._L.nmpc_hip_riccati_solve(self._h))
        return self._result(col_major)

    def backwardDevice(self, Fx, Fu, Lx, Lu, Lxx, Luu, Lxu, Vx_T, Vxx_T, U=None, lower=None, upper=None, lam=None, dlam=None,
                       stream=None) -> Result:
        """The same on torch tensors (float64, contiguous, on this solver's device, [B, T, rows, cols]), read in place.  lam / dlam:
        per-instance tensors [B], e.g. the `lam` / `dlam` of the previous result.  Asynchronous on `stream` (a torch stream; None =
        the current one); the returned tensors are filled in stream order: work queued on that stream afterwards sees them."""
        import torch
        constrained = U is not None
        if constrained and (lower is None or upper is None):
            raise ValueError("U, lower and upper come together")
        per_step = constrained and lower.dim() == 3
        shapes = self._shapes(per_step)
        shapes.update(lam=(self.B,), dlam=(self.B,))
        given = dict(Fx=Fx, Fu=Fu, Lx=Lx, Lu=Lu, Lxx=Lxx, Luu=Luu, Lxu=Lxu, Vx_T=Vx_T, Vxx_T=Vxx_T, U=U, lower=lower, upper=upper, lam=lam,
                     dlam=dlam)
        for name, t in given.items():
            if t is None:
                continue
            if (tuple(t.shape) != shapes[name] or str(t.dtype) != "torch.float64" or not t.is_contiguous() or not t.is_cuda
                    or t.device.index != self.device):
                raise ValueError(f"{name}: a contiguous float64 tensor of shape {shapes[name]} on device {self.device} is expected")
        self._push(True, constrained)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        check(self._L.nmpc_hip_riccati_set_derivatives(self._h, *[ptr(given[k]) for k in _DERIVATIVES], 1))
        if constrained:
            check(self._L.nmpc_hip_riccati_set_inputs(self._h, ptr(U), ptr(lower), ptr(upper), int(per_step), 1))
        if lam is not None or dlam is not None or self._device_lambda:
            check(self._L.nmpc_hip_riccati_set_lambda(self._h, ptr(lam), ptr(dlam), 1))
            self._device_lambda = lam is not None or dlam is not None
            if not self._device_lambda:
                self.setLambda(self._lam, self._dlam)
        self._keep = tuple(t for t in given.values() if t is not None)
        cur = torch.cuda.current_stream(self.device) if stream is None else stream
        s = cur
        if not cur.cuda_stream:
            # the null stream has no handle to pass (NULL is "the solver's own stream" at the C-ABI): a side stream ordered behind it,
            # and the null stream behind the side stream again once the results are written
            if self._side_stream is None:
                self._side_stream = torch.cuda.Stream(self.device)
            s = self._side_stream
            s.wait_stream(cur)
        check(self._L.nmpc_hip_riccati_solve_device(self._h, C.c_void_p(s.cuda_stream)))
        B, T, n, m = self.B, self.T, self.n, self.m
        dev = torch.device("cuda", self.device)
        r = Result()
        with torch.cuda.stream(s):
            for name, field, shape, dtype in (
                    ("k", FIELD_K_FF, (B, T, m), torch.float64), ("K", FIELD_K_FB, (B, T, m, n), torch.float64),
                    ("dV", FIELD_DV, (B, 2), torch.float64), ("Vx0", FIELD_VX0, (B, n), torch.float64),
                    ("Vxx0", FIELD_VXX0, (B, n, n), torch.float64), ("status", FIELD_STATUS, (B,), torch.int32),
                    ("n_backward", FIELD_N_BACKWARD, (B,), torch.int32), ("lam", FIELD_LAMBDA, (B,), torch.float64),
                    ("dlam", FIELD_DLAMBDA, (B,), torch.float64), ("fail_step", FIELD_FAIL_STEP, (B,), torch.int32),
                    ("qp_retval", FIELD_QP_RETVAL, (B, T), torch.int32), ("free_mask", FIELD_FREE_MASK, (B, T), torch.int32)):
                t = torch.empty(shape, dtype=dtype, device=dev)
                check(self._L.nmpc_hip_riccati_get(self._h, field, C.c_void_p(t.data_ptr()), t.numel() * t.element_size(), 1))
                setattr(r, name, t)
        if s is not cur:
            cur.wait_stream(s)
        return r

    def solveDevice(self, stream=None) -> None:
        """The pass on the inputs of the last backwardDevice again (resident inputs), asynchronous; for timing loops."""
        s = None if stream is None else C.c_void_p(stream.cuda_stream)
        check(self._L.nmpc_hip_riccati_solve_device(self._h, s))

    def synchronize(self) -> None:
        check(self._L.nmpc_hip_riccati_synchronize(self._h))

    def _get(self, field, dtype, shape):
        nb = C.c_size_t()
        check(self._L.nmpc_hip_riccati_field_bytes(self._h, field, C.byref(nb)))
        out = np.zeros(nb.value // np.dtype(dtype).itemsize, dtype=dtype)
        check(self._L.nmpc_hip_riccati_get(self._h, field, out.ctypes.data_as(C.c_void_p), nb.value, 0))
        return out.reshape(shape)

    def _result(self, col_major: bool = False) -> Result:
        B, T, n, m = self.B, self.T, self.n, self.m
        r = Result()
        r.k = self._get(FIELD_K_FF, np.float64, (B, T, m))
        r.K = self._get(FIELD_K_FB, np.float64, (B, T, n, m) if col_major else (B, T, m, n))
        r.dV = self._get(FIELD_DV, np.float64, (B, 2))
        r.Vx0 = self._get(FIELD_VX0, np.float64, (B, n))
        r.Vxx0 = self._get(FIELD_VXX0, np.float64, (B, n, n))
        r.status = self._get(FIELD_STATUS, np.int32, (B,))
        r.n_backward = self._get(FIELD_N_BACKWARD, np.int32, (B,))
        r.lam = self._get(FIELD_LAMBDA, np.float64, (B,))
        r.dlam = self._get(FIELD_DLAMBDA, np.float64, (B,))
        r.fail_step = self._get(FIELD_FAIL_STEP, np.int32, (B,))
        r.qp_retval = self._get(FIELD_QP_RETVAL, np.int32, (B, T))
        r.free_mask = self._get(FIELD_FREE_MASK, np.uint32, (B, T))
        return r

    def kernelName(self) -> str:
        p = C.c_char_p()
        check(self._L.nmpc_hip_riccati_kernel_name(self._h, C.byref(p)))
        return p.value.decode()

    def lastMs(self) -> float:
        ms = C.c_float()
        check(self._L.nmpc_hip_riccati_last_ms(self._h, C.byref(ms)))
        return float(ms.value)
