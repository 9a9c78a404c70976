"""Batched FMPC iteration on caller-supplied linearisations: the model-free part of the reference's interior-point solver.

`FmpcStepBatch` runs one FmpcSolver::procOnce (nmpc_fmpc/include/nmpc_fmpc/FmpcSolver.hpp:365-493, enable_line_search = false) per
`step()` for a batch of instances whose Jacobians A, B, C, D, cost derivatives and function values stateEq / ineqConst come from
anywhere: a torch function linearised with torch.func, a simulator, a table.  The handle owns the variable (x, u, lambda, s, nu,
barrier_eps): linearise at `variable()`, call `step()`, repeat until `kkt_error <= kkt_error_thre` (status 1).  Everything numeric
happens in libnmpc_hip_ddp.so through the C-ABI (include/nmpc_hip_fmpc_step.h); this file marshals arrays and re-raises status codes.
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import _capi

(FIELD_STATUS, FIELD_KKT_ERROR, FIELD_BARRIER_EPS, FIELD_ALPHA_S_MAX, FIELD_ALPHA_NU_MAX, FIELD_K_FF, FIELD_K_FB, FIELD_S, FIELD_P,
 FIELD_DELTA_X, FIELD_DELTA_U, FIELD_DELTA_LAMBDA, FIELD_DELTA_S, FIELD_DELTA_NU, FIELD_VAR_X, FIELD_VAR_U, FIELD_VAR_LAMBDA,
 FIELD_VAR_S, FIELD_VAR_NU) = range(19)
MAX_DIM = 16
MAX_INEQ = 32
# FmpcSolver::Status (FmpcSolver.h:92-114)
(STATUS_UNINITIALIZED, STATUS_SUCCEEDED, STATUS_ERROR_IN_FORWARD, STATUS_ERROR_IN_BACKWARD, STATUS_ERROR_IN_UPDATE,
 STATUS_MAX_ITERATION_REACHED, STATUS_ITERATION_CONTINUED) = range(7)


class CConfig(ct.Structure):
    """nmpc_hip_fmpc_step_config (include/nmpc_hip_fmpc_step.h)."""

    _fields_ = [
        ("dt", ct.c_double),
        ("kkt_error_thre", ct.c_double),
        ("check_nan", ct.c_int),
        ("init_complementary_variable", ct.c_int),
        ("update_barrier_eps", ct.c_int),
        ("break_if_llt_fails", ct.c_int),
        ("apply_update", ct.c_int),
        ("row_major", ct.c_int),
    ]


# every symbol include/nmpc_hip_fmpc_step.h declares
EXPORTS = (
    "nmpc_hip_fmpc_step_default_config", "nmpc_hip_fmpc_step_create", "nmpc_hip_fmpc_step_destroy", "nmpc_hip_fmpc_step_set_config",
    "nmpc_hip_fmpc_step_get_config", "nmpc_hip_fmpc_step_set_step_dims", "nmpc_hip_fmpc_step_set_linearisation",
    "nmpc_hip_fmpc_step_set_variable", "nmpc_hip_fmpc_step_step", "nmpc_hip_fmpc_step_step_device", "nmpc_hip_fmpc_step_synchronize",
    "nmpc_hip_fmpc_step_get", "nmpc_hip_fmpc_step_field_bytes", "nmpc_hip_fmpc_step_kernel_name", "nmpc_hip_fmpc_step_last_ms",
    "nmpc_hip_fmpc_step_last_error",
)

_declared = False


def load():
    """The library of nmpc_amd._capi with the FMPC step prototypes declared."""
    global _declared
    L = _capi.load()
    if _declared:
        return L
    vp, sz = ct.c_void_p, ct.c_size_t
    L.nmpc_hip_fmpc_step_default_config.argtypes = [ct.POINTER(CConfig)]
    L.nmpc_hip_fmpc_step_create.argtypes = [ct.c_int] * 6 + [ct.POINTER(vp)]
    L.nmpc_hip_fmpc_step_destroy.argtypes = [vp]
    L.nmpc_hip_fmpc_step_set_config.argtypes = [vp, ct.POINTER(CConfig)]
    L.nmpc_hip_fmpc_step_get_config.argtypes = [vp, ct.POINTER(CConfig)]
    L.nmpc_hip_fmpc_step_set_step_dims.argtypes = [vp, vp, vp]
    L.nmpc_hip_fmpc_step_set_linearisation.argtypes = [vp] + [vp] * 14 + [ct.c_int]
    L.nmpc_hip_fmpc_step_set_variable.argtypes = [vp] + [vp] * 6 + [ct.c_int]
    L.nmpc_hip_fmpc_step_step.argtypes = [vp]
    L.nmpc_hip_fmpc_step_step_device.argtypes = [vp, vp]
    L.nmpc_hip_fmpc_step_synchronize.argtypes = [vp]
    L.nmpc_hip_fmpc_step_get.argtypes = [vp, ct.c_int, vp, sz, ct.c_int]
    L.nmpc_hip_fmpc_step_field_bytes.argtypes = [vp, ct.c_int, ct.POINTER(sz)]
    L.nmpc_hip_fmpc_step_kernel_name.argtypes = [vp, ct.POINTER(ct.c_char_p)]
    L.nmpc_hip_fmpc_step_last_ms.argtypes = [vp, ct.POINTER(ct.c_float)]
    L.nmpc_hip_fmpc_step_last_error.argtypes = []
    L.nmpc_hip_fmpc_step_last_error.restype = ct.c_char_p
    for name in EXPORTS:
        if name != "nmpc_hip_fmpc_step_last_error":
            getattr(L, name).restype = ct.c_int
    _declared = True
    return L


def check(rc: int) -> None:
    """Status code -> ValueError (invalid argument) or RuntimeError."""
    if rc == _capi.OK:
        return
    msg = load().nmpc_hip_fmpc_step_last_error().decode(errors="replace")
    if rc == _capi.ERR_INVALID_ARGUMENT:
        raise ValueError(msg)
    raise RuntimeError(f"[nmpc_hip_fmpc_step {rc}] {msg}")


def default_config() -> CConfig:
    cfg = CConfig()
    check(load().nmpc_hip_fmpc_step_default_config(ct.byref(cfg)))
    return cfg


class Result:
    """One iteration per instance: status [B] (FmpcSolver::Status; 6 = IterationContinued), kkt_error / barrier_eps / alpha_s_max /
    alpha_nu_max [B], the gains k [B, T, m], K [B, T, m, n], s [B, T+1, n], P [B, T+1, n, n], the delta dx / dlam [B, T+1, n],
    du [B, T, m], ds / dnu [B, T, g], and the variable after the call x / lam [B, T+1, n], u [B, T, m], vs / vnu [B, T, g]."""

    __slots__ = ("status", "kkt_error", "barrier_eps", "alpha_s_max", "alpha_nu_max", "k", "K", "s", "P", "dx", "du", "dlam", "ds", "dnu",
                 "x", "u", "lam", "vs", "vnu")


_LINEARISATION = ("A", "B", "C", "D", "Lx", "Lu", "Lxx", "Luu", "Lxu", "f", "g", "Lx_T", "Lxx_T", "current_x")
_MATRICES = ("A", "B", "C", "D", "Lxx", "Luu", "Lxu", "Lxx_T")
_VARIABLE = ("x", "u", "lam", "s", "nu")


class FmpcStepBatch:
    """`batch` instances of state dimension n, input capacity m, inequality capacity g and T steps on one GPU."""

    def __init__(self, n: int, m: int, g: int, T: int, batch: int, device: int = 0):
        self.n, self.m, self.g, self.T, self.B = int(n), int(m), int(g), int(T), int(batch)
        self.device = int(device)
        self._L = load()
        h = ct.c_void_p()
        check(self._L.nmpc_hip_fmpc_step_create(self.n, self.m, self.g, self.T, self.B, self.device, ct.byref(h)))
        self._h = h
        self._cfg = CConfig()
        check(self._L.nmpc_hip_fmpc_step_get_config(self._h, ct.byref(self._cfg)))
        self._keep = ()  # device tensors the handle reads in place

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._L.nmpc_hip_fmpc_step_destroy(h)
            self._h = None

    def config(self) -> CConfig:
        """The configuration; pushed to the library by the next step (which sets row_major itself)."""
        return self._cfg

    def setStepDims(self, input_dims=None, ineq_dims=None) -> None:
        """inputDim(t) and ineqDim(t) per step ([T] each), shared by the batch; None = the capacity everywhere."""
        arrs = []
        for name, d in (("input_dims", input_dims), ("ineq_dims", ineq_dims)):
            if d is not None:
                d = np.ascontiguousarray(d, dtype=np.int32)
                if d.shape != (self.T,):
                    raise ValueError(f"{name}: shape {d.shape}, expected {(self.T,)}")
            arrs.append(d)
        vp = lambda a: None if a is None else a.ctypes.data_as(ct.c_void_p)
        check(self._L.nmpc_hip_fmpc_step_set_step_dims(self._h, vp(arrs[0]), vp(arrs[1])))

    def _shapes(self, col_major: bool = False):
        B, T, n, m, g = self.B, self.T, self.n, self.m, self.g
        sh = dict(A=(B, T, n, n), B=(B, T, n, m), C=(B, T, g, n), D=(B, T, g, m), Lx=(B, T, n), Lu=(B, T, m), Lxx=(B, T, n, n),
                  Luu=(B, T, m, m), Lxu=(B, T, n, m), f=(B, T, n), g=(B, T, g), Lx_T=(B, n), Lxx_T=(B, n, n), current_x=(B, n),
                  x=(B, T + 1, n), u=(B, T, m), lam=(B, T + 1, n), s=(B, T, g), nu=(B, T, g), barrier_eps=(B,))
        if col_major:
            sh = {k: (s[:-2] + (s[-1], s[-2]) if k in _MATRICES else s) for k, s in sh.items()}
        return sh

    def _arr(self, a, shape, name):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"{name}: shape {a.shape}, expected {shape}")
        return a

    def _is_tensor(self, a) -> bool:
        return hasattr(a, "data_ptr") and hasattr(a, "is_cuda")

    def _marshal(self, given: dict, shapes: dict):
        """(pointers in order, arrays to keep alive, on_device) of one group of arrays: all numpy (or array-likes), or all torch
        tensors on this solver's device (float64, contiguous; read in place)."""
        present = {k: v for k, v in given.items() if v is not None}
        on_device = any(self._is_tensor(v) and v.is_cuda for v in present.values())
        keep, ptrs = [], []
        for name, v in given.items():
            if v is None or int(np.prod(shapes[name])) == 0:
                ptrs.append(None)
                continue
            if on_device:
                if (not self._is_tensor(v) or not v.is_cuda or tuple(v.shape) != shapes[name] or str(v.dtype) != "torch.float64"
                        or not v.is_contiguous() or v.device.index != self.device):
                    raise ValueError(f"{name}: a contiguous float64 tensor of shape {shapes[name]} on device {self.device} is expected")
                keep.append(v)
                ptrs.append(ct.c_void_p(v.data_ptr()))
            else:
                if self._is_tensor(v):
                    v = v.detach().cpu().numpy()
                a = self._arr(v, shapes[name], name)
                keep.append(a)
                ptrs.append(a.ctypes.data_as(ct.c_void_p))
        return ptrs, keep, int(on_device)

    def _wait_for_producers(self) -> None:
        """Device tensors are read by the handle's own stream, which is non-blocking: it waits for no torch stream.  The kernels that
        write the tensors are queued on torch's current stream (torch's convention for a tensor handed to a library), so that stream
        is drained before the handle's stream touches them.  step() and setVariable() are synchronous calls anyway."""
        import torch
        torch.cuda.current_stream(self.device).synchronize()

    def _push(self, row_major: bool) -> None:
        self._cfg.row_major = int(row_major)
        check(self._L.nmpc_hip_fmpc_step_set_config(self._h, ct.byref(self._cfg)))

    def setVariable(self, x, u, lam, s, nu, barrier_eps=None) -> None:
        """variable_ of every instance (numpy arrays or device tensors; copied into the handle, device tensors once the work queued
        on torch's current stream has finished); barrier_eps [B] or None to keep
        the handle's (1e-4 after construction)."""
        given = dict(x=x, u=u, lam=lam, s=s, nu=nu, barrier_eps=barrier_eps)
        ptrs, keep, on_device = self._marshal(given, self._shapes())
        if on_device:
            self._wait_for_producers()
        check(self._L.nmpc_hip_fmpc_step_set_variable(self._h, *ptrs, on_device))

    def step(self, A, B, C, D, Lx, Lu, Lxx, Luu, Lxu, f, g, Lx_T, Lxx_T, current_x, col_major: bool = False,
             fields=None) -> Result:
        """One iteration on the linearisation at the handle's variable: numpy arrays or torch tensors [B, T, rows, cols] (Lx_T [B, n],
        Lxx_T [B, n, n], current_x [B, n]); device tensors are read in place, once the work queued on torch's current stream of that
        device (the kernels that write them) has finished.  col_major: the matrix blocks are handed over and
        returned column-major instead (arrays [B, T, cols, rows]).  fields: names of the Result members to fetch (None = all)."""
        given = dict(zip(_LINEARISATION, (A, B, C, D, Lx, Lu, Lxx, Luu, Lxu, f, g, Lx_T, Lxx_T, current_x)))
        ptrs, keep, on_device = self._marshal(given, self._shapes(col_major))
        self._push(not col_major)
        check(self._L.nmpc_hip_fmpc_step_set_linearisation(self._h, *ptrs, on_device))
        self._keep = tuple(keep) if on_device else ()
        if on_device:
            self._wait_for_producers()
        check(self._L.nmpc_hip_fmpc_step_step(self._h))
        return self.result(col_major, fields)

    def stepDevice(self, stream=None) -> None:
        """The iteration on the inputs of the last step() again (resident inputs), asynchronous; for timing loops."""
        s = None if stream is None else ct.c_void_p(stream.cuda_stream)
        check(self._L.nmpc_hip_fmpc_step_step_device(self._h, s))

    def synchronize(self) -> None:
        check(self._L.nmpc_hip_fmpc_step_synchronize(self._h))

    def _get(self, field, dtype, shape):
        nb = ct.c_size_t()
        check(self._L.nmpc_hip_fmpc_step_field_bytes(self._h, field, ct.byref(nb)))
        out = np.zeros(nb.value // np.dtype(dtype).itemsize, dtype=dtype)
        check(self._L.nmpc_hip_fmpc_step_get(self._h, field, out.ctypes.data_as(ct.c_void_p), nb.value, 0))
        return out.reshape(shape)

    def _fields(self, col_major: bool):
        B, T, n, m, g = self.B, self.T, self.n, self.m, self.g
        f64, i32 = np.float64, np.int32
        return dict(status=(FIELD_STATUS, i32, (B,)), kkt_error=(FIELD_KKT_ERROR, f64, (B,)), barrier_eps=(FIELD_BARRIER_EPS, f64, (B,)),
                    alpha_s_max=(FIELD_ALPHA_S_MAX, f64, (B,)), alpha_nu_max=(FIELD_ALPHA_NU_MAX, f64, (B,)),
                    k=(FIELD_K_FF, f64, (B, T, m)), K=(FIELD_K_FB, f64, (B, T, n, m) if col_major else (B, T, m, n)),
                    s=(FIELD_S, f64, (B, T + 1, n)), P=(FIELD_P, f64, (B, T + 1, n, n)), dx=(FIELD_DELTA_X, f64, (B, T + 1, n)),
                    du=(FIELD_DELTA_U, f64, (B, T, m)), dlam=(FIELD_DELTA_LAMBDA, f64, (B, T + 1, n)),
                    ds=(FIELD_DELTA_S, f64, (B, T, g)), dnu=(FIELD_DELTA_NU, f64, (B, T, g)), x=(FIELD_VAR_X, f64, (B, T + 1, n)),
                    u=(FIELD_VAR_U, f64, (B, T, m)), lam=(FIELD_VAR_LAMBDA, f64, (B, T + 1, n)), vs=(FIELD_VAR_S, f64, (B, T, g)),
                    vnu=(FIELD_VAR_NU, f64, (B, T, g)))

    def result(self, col_major: bool = False, fields=None) -> Result:
        r = Result()
        for name, (field, dtype, shape) in self._fields(col_major).items():
            setattr(r, name, self._get(field, dtype, shape) if fields is None or name in fields else None)
        return r

    def variable(self):
        """(x, u, lam, s, nu) the handle holds, as numpy arrays."""
        f = self._fields(False)
        return tuple(self._get(*f[k]) for k in ("x", "u", "lam", "vs", "vnu"))

    def barrierEps(self):
        return self._get(FIELD_BARRIER_EPS, np.float64, (self.B,))

    def kernelName(self) -> str:
        p = ct.c_char_p()
        check(self._L.nmpc_hip_fmpc_step_kernel_name(self._h, ct.byref(p)))
        return p.value.decode()

    def lastMs(self) -> float:
        ms = ct.c_float()
        check(self._L.nmpc_hip_fmpc_step_last_ms(self._h, ct.byref(ms)))
        return float(ms.value)
