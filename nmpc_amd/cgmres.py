"""Python mirror of the reference's nmpc_cgmres::CgmresSolver interface for a BATCH of independent solvers.

Same member names and meaning as nmpc_cgmres/include/nmpc_cgmres/CgmresSolver.h:25-132 (`setup()`, `run()`,
`calcControlInput()`, the C/GMRES parameters `sim_duration_` ... `dump_step_`, the variables `x_`, `u_`, `u_list_`,
`delta_u_vec_`), with a leading batch axis.  Everything numeric happens in libnmpc_hip_ddp.so through the C-ABI
(include/nmpc_hip_cgmres.h); this file marshals arrays and re-raises status codes.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _capi

(FIELD_X, FIELD_U, FIELD_U_LIST, FIELD_DELTA_U, FIELD_STATUS, FIELD_ERR, FIELD_LOG_T, FIELD_LOG_X, FIELD_LOG_U, FIELD_LOG_ERR,
 FIELD_LOG_ITERS, FIELD_LOG_REORTH) = range(12)
ODE_EULER, ODE_RUNGE_KUTTA = 0, 1


class Status:
    """nmpc_hip_cgmres_instance_status."""
    Uninitialized = 0
    Succeeded = 1
    SetupNotConverged = 2
    NonFinite = 3


class CConfig(C.Structure):
    """nmpc_hip_cgmres_config (include/nmpc_hip_cgmres.h)."""

    _fields_ = [
        ("sim_duration", C.c_double),
        ("steady_horizon_duration", C.c_double),
        ("horizon_divide_num", C.c_int),
        ("horizon_increase_ratio", C.c_double),
        ("dt", C.c_double),
        ("eq_zeta", C.c_double),
        ("k_max", C.c_int),
        ("finite_diff_delta", C.c_double),
        ("dump_step", C.c_int),
        ("ode_solver", C.c_int),
        ("sim_ode_solver", C.c_int),
        ("ticks_per_launch", C.c_int),
    ]


# every symbol include/nmpc_hip_cgmres.h declares
EXPORTS = (
    "nmpc_hip_cgmres_default_config", "nmpc_hip_cgmres_model_count", "nmpc_hip_cgmres_model_name", "nmpc_hip_cgmres_model_info",
    "nmpc_hip_cgmres_model_default_params", "nmpc_hip_cgmres_create", "nmpc_hip_cgmres_destroy", "nmpc_hip_cgmres_set_config",
    "nmpc_hip_cgmres_get_config", "nmpc_hip_cgmres_set_problem", "nmpc_hip_cgmres_set_initial", "nmpc_hip_cgmres_setup",
    "nmpc_hip_cgmres_run", "nmpc_hip_cgmres_control_input", "nmpc_hip_cgmres_control_input_device", "nmpc_hip_cgmres_synchronize",
    "nmpc_hip_cgmres_get", "nmpc_hip_cgmres_field_bytes", "nmpc_hip_cgmres_dense_gmres", "nmpc_hip_cgmres_model_eval",
    "nmpc_hip_cgmres_last_ms", "nmpc_hip_cgmres_last_error", "nmpc_hip_cgmres_set_kernel", "nmpc_hip_cgmres_kernel_name",
    "nmpc_hip_cgmres_wave_lds_bytes",
)

_declared = False


def load():
    """The library of nmpc_amd._capi with the C/GMRES prototypes declared."""
    global _declared
    L = _capi.load()
    if _declared:
        return L
    vp, dp, ip, sz = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_size_t
    L.nmpc_hip_cgmres_default_config.argtypes = [C.POINTER(CConfig)]
    L.nmpc_hip_cgmres_model_count.argtypes = []
    L.nmpc_hip_cgmres_model_name.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.nmpc_hip_cgmres_model_info.argtypes = [C.c_char_p, ip, ip, ip, C.POINTER(sz), dp, dp]
    L.nmpc_hip_cgmres_model_default_params.argtypes = [C.c_char_p, vp, sz]
    L.nmpc_hip_cgmres_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.nmpc_hip_cgmres_destroy.argtypes = [vp]
    L.nmpc_hip_cgmres_set_config.argtypes = [vp, C.POINTER(CConfig)]
    L.nmpc_hip_cgmres_get_config.argtypes = [vp, C.POINTER(CConfig)]
    L.nmpc_hip_cgmres_set_problem.argtypes = [vp, vp, sz, C.c_int]
    L.nmpc_hip_cgmres_set_initial.argtypes = [vp, dp, dp]
    L.nmpc_hip_cgmres_setup.argtypes = [vp]
    L.nmpc_hip_cgmres_run.argtypes = [vp]
    L.nmpc_hip_cgmres_control_input.argtypes = [vp, dp, dp, dp, dp]
    L.nmpc_hip_cgmres_control_input_device.argtypes = [vp, vp, vp, vp, vp, vp]
    L.nmpc_hip_cgmres_synchronize.argtypes = [vp]
    L.nmpc_hip_cgmres_get.argtypes = [vp, C.c_int, vp, sz]
    L.nmpc_hip_cgmres_field_bytes.argtypes = [vp, C.c_int, C.POINTER(sz)]
    L.nmpc_hip_cgmres_dense_gmres.argtypes = [C.c_int, C.c_int, C.c_int, dp, dp, dp, C.c_int, C.c_int, C.c_double, ip, ip]
    L.nmpc_hip_cgmres_model_eval.argtypes = [vp, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp]
    L.nmpc_hip_cgmres_last_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.nmpc_hip_cgmres_set_kernel.argtypes = [vp, C.c_char_p]
    L.nmpc_hip_cgmres_kernel_name.argtypes = [vp, C.POINTER(C.c_char_p)]
    L.nmpc_hip_cgmres_wave_lds_bytes.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(sz)]
    L.nmpc_hip_cgmres_last_error.argtypes = []
    L.nmpc_hip_cgmres_last_error.restype = C.c_char_p
    for name in EXPORTS:
        if name != "nmpc_hip_cgmres_last_error":
            getattr(L, name).restype = C.c_int
    _declared = True
    return L


def check(rc: int) -> None:
    """Status code -> ValueError (invalid argument / unknown problem type) or RuntimeError."""
    if rc == _capi.OK:
        return
    msg = load().nmpc_hip_cgmres_last_error().decode(errors="replace")
    if rc in (_capi.ERR_INVALID_ARGUMENT, _capi.ERR_UNKNOWN_MODEL):
        raise ValueError(msg)
    raise RuntimeError(f"[nmpc_hip_cgmres {rc}] {msg}")


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def default_config() -> CConfig:
    cfg = CConfig()
    check(load().nmpc_hip_cgmres_default_config(C.byref(cfg)))
    return cfg


def model_names():
    L = load()
    out = []
    for i in range(L.nmpc_hip_cgmres_model_count()):
        p = C.c_char_p()
        check(L.nmpc_hip_cgmres_model_name(i, C.byref(p)))
        out.append(p.value.decode())
    return out


def model_info(model: str):
    """(dim_x, dim_u, dim_c, param_bytes, x_initial, u_initial)."""
    nx, nu, nc, pb = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    L = load()
    check(L.nmpc_hip_cgmres_model_info(model.encode(), C.byref(nx), C.byref(nu), C.byref(nc), C.byref(pb), None, None))
    x0, u0 = np.zeros(nx.value), np.zeros(nu.value + nc.value)
    check(L.nmpc_hip_cgmres_model_info(model.encode(), None, None, None, None, _dp(x0), _dp(u0)))
    return nx.value, nu.value, nc.value, pb.value, x0, u0


def wave_lds_bytes(model: str, horizon_divide_num: int, k_max: int) -> int:
    """LDS bytes one workgroup of the wave kernels needs for a registered problem type (no device needed); a handle accepts
    setKernel("wave") up to 65536."""
    n = C.c_size_t()
    check(load().nmpc_hip_cgmres_wave_lds_bytes(model.encode(), horizon_divide_num, k_max, C.byref(n)))
    return n.value


class CgmresProblem:
    """A problem object as the library sees it: the name of a registered problem type and the memory image of the C++ object
    (include/nmpc_amd/models/Cgmres*.hpp, all doubles) as the float64 array `p`, with CgmresProblem.h's members."""

    # leading entries of the image that the reference's dumpData writes as state_eq_param (CgmresProblem.h:58-61)
    n_state_eq_param = 0

    def __init__(self, model: str):
        self.model = model
        nx, nu, nc, pb, x0, u0 = model_info(model)
        self.dim_x_, self.dim_u_, self.dim_c_, self.dim_uc_ = nx, nu, nc, nu + nc
        self.x_initial_, self.u_initial_ = x0, u0
        blob = (C.c_ubyte * pb)()
        check(load().nmpc_hip_cgmres_model_default_params(model.encode(), blob, pb))
        self.p = np.frombuffer(bytes(blob), dtype=np.float64).copy()

    @property
    def state_eq_param_(self) -> np.ndarray:
        return self.p[:self.n_state_eq_param].copy()

    def blob(self) -> bytes:
        return np.ascontiguousarray(self.p, dtype=np.float64).tobytes()

    def dumpData(self, f) -> None:
        f.write('"state_eq_param": [' + ", ".join("%g" % v for v in self.state_eq_param_) + "],\n")


class CgmresProblemSemiactiveDamper(CgmresProblem):
    """nmpc_amd::CgmresProblemSemiactiveDamper.  Image: a, b, u_max, q1, q2, r1, r2, sf1, sf2."""
    n_state_eq_param = 3

    def __init__(self):
        super().__init__("cgmres_semiactive_damper")


class CgmresProblemCartPole(CgmresProblem):
    """nmpc_amd::CgmresProblemCartPoleT<with_input_bound>.  Image: m1, m2, l, f_max, q[4], r1, r2, sf[4], ref[4], g.
    `ref` is the constant reference state (the reference's default RefFunc gives zero)."""
    n_state_eq_param = 4

    def __init__(self, with_input_bound: bool = False, ref=None):
        super().__init__("cgmres_cartpole_with_input_bound" if with_input_bound else "cgmres_cartpole")
        self.with_input_bound_ = with_input_bound
        if ref is not None:
            self.p[14:18] = np.asarray(ref, dtype=np.float64)

    @property
    def ref(self) -> np.ndarray:
        return self.p[14:18].copy()


def dense_gmres(A, b, x0=None, k_max: int = 100, apply_reorth: bool = True, eps: float = 1e-10, device: int = 0):
    """Diagnostic: Gmres::solve on a batch of dense systems on the GPU.  A [batch][n][n], b [batch][n]; returns (x, iters, reorth)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    batch, n = b.shape
    x = np.zeros((batch, n)) if x0 is None else np.array(x0, dtype=np.float64, order="C")
    it, ro = np.zeros(batch, np.int32), np.zeros(batch, np.int32)
    check(load().nmpc_hip_cgmres_dense_gmres(device, batch, n, _dp(A), _dp(b), _dp(x), k_max, int(apply_reorth), eps, _ip(it), _ip(ro)))
    return x, it, ro


class CgmresSolverBatch:
    """B independent CgmresSolver instances of one problem type on one GPU.

    `problem`: a CgmresProblem shared by every instance, or a list of B of the same type (per-instance parameters).
    `ode_solver` / `sim_ode_solver`: "euler" or "rk4"; the simulation solver defaults to the horizon one (CgmresSolver.h:30-40)."""

    _CFG = ("sim_duration", "steady_horizon_duration", "horizon_increase_ratio", "dt", "eq_zeta", "k_max", "finite_diff_delta",
            "dump_step")

    def __init__(self, problem, batch: int, horizon_divide_num: int = 25, device: int = 0, ode_solver: str = "euler",
                 sim_ode_solver: Optional[str] = None):
        problems = list(problem) if isinstance(problem, (list, tuple)) else None
        self.problem_ = problems[0] if problems else problem
        self.B = int(batch)
        self._L = load()
        h = C.c_void_p()
        check(self._L.nmpc_hip_cgmres_create(self.problem_.model.encode(), horizon_divide_num, self.B, device, C.byref(h)))
        self._h = h
        self._cfg = CConfig()
        check(self._L.nmpc_hip_cgmres_get_config(self._h, C.byref(self._cfg)))
        solvers = {"euler": ODE_EULER, "rk4": ODE_RUNGE_KUTTA}
        self._cfg.ode_solver = solvers[ode_solver]
        self._cfg.sim_ode_solver = -1 if sim_ode_solver is None else solvers[sim_ode_solver]
        if problems:
            if len(problems) != self.B or any(p.model != self.problem_.model for p in problems):
                raise ValueError("per-instance problems: one object of the same problem type per instance")
            self.setProblem(problems)
        else:
            self.setProblem(self.problem_)
        self.x_initial_ = np.tile(self.problem_.x_initial_, (self.B, 1))
        self.u_initial_ = np.tile(self.problem_.u_initial_, (self.B, 1))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._L.nmpc_hip_cgmres_destroy(h)
            self._h = None

    # ---- the C/GMRES parameters as the reference's members (CgmresSolver.h:72-86)
    def __getattr__(self, name):
        if name.endswith("_") and name[:-1] in CgmresSolverBatch._CFG:
            return getattr(self.__dict__["_cfg"], name[:-1])
        if name == "horizon_divide_num_":
            return self.__dict__["_cfg"].horizon_divide_num
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name.endswith("_") and name[:-1] in CgmresSolverBatch._CFG:
            setattr(self._cfg, name[:-1], value)
        else:
            object.__setattr__(self, name, value)

    def config(self) -> CConfig:
        return self._cfg

    def _push(self):
        check(self._L.nmpc_hip_cgmres_set_config(self._h, C.byref(self._cfg)))

    def setKernel(self, kernel: str) -> None:
        """"lane" (default: one lane per instance) or "wave" (one wavefront per instance, the tick in LDS): the kernel family of run()
        and calcControlInput*().  Same results bit for bit; may be changed between calls.  ValueError when the problem type has no
        wave kernels or the shape (horizon_divide_num_, k_max_) exceeds their LDS budget."""
        if kernel == "wave":  # the handle has to know k_max_ to judge the shape; "lane" takes every config, so it is set first
            self._push()
        check(self._L.nmpc_hip_cgmres_set_kernel(self._h, kernel.encode()))
        self._push()

    def kernelName(self) -> str:
        """The kernel symbol run() launches next: "cgmres_run_kernel" or "cgmres_wave_run_kernel"."""
        p = C.c_char_p()
        check(self._L.nmpc_hip_cgmres_kernel_name(self._h, C.byref(p)))
        return p.value.decode()

    def setProblem(self, problem) -> None:
        if isinstance(problem, (list, tuple)):
            blob = b"".join(p.blob() for p in problem)
            check(self._L.nmpc_hip_cgmres_set_problem(self._h, blob, len(blob), 1))
        else:
            blob = problem.blob()
            check(self._L.nmpc_hip_cgmres_set_problem(self._h, blob, len(blob), 0))

    def setInitial(self, x=None, u=None) -> None:
        """x_initial_ [B][dim_x] / u_initial_ [B][dim_uc] of every instance (a single row is broadcast)."""
        if x is not None:
            self.x_initial_ = np.ascontiguousarray(np.broadcast_to(np.asarray(x, float), (self.B, self.problem_.dim_x_)))
        if u is not None:
            self.u_initial_ = np.ascontiguousarray(np.broadcast_to(np.asarray(u, float), (self.B, self.problem_.dim_uc_)))
        check(self._L.nmpc_hip_cgmres_set_initial(self._h, _dp(self.x_initial_), _dp(self.u_initial_)))

    def setup(self) -> None:
        """CgmresSolver::setup (CgmresSolver.cpp:8-64) for every instance."""
        self._push()
        self.setInitial()
        check(self._L.nmpc_hip_cgmres_setup(self._h))

    def run(self) -> None:
        """CgmresSolver::run (CgmresSolver.cpp:66-107) for every instance; the logs stay on the handle (log_* / dump)."""
        self._push()
        self.setInitial()
        check(self._L.nmpc_hip_cgmres_run(self._h))

    def calcControlInput(self, t, x, next_x) -> np.ndarray:
        """CgmresSolver::calcControlInput for every instance: t scalar or [B], x / next_x [B][dim_x]; returns u [B][dim_uc]."""
        self._push()
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, float), (self.B,)))
        x = np.ascontiguousarray(x, dtype=np.float64)
        nx = np.ascontiguousarray(next_x, dtype=np.float64)
        u = np.zeros((self.B, self.problem_.dim_uc_))
        check(self._L.nmpc_hip_cgmres_control_input(self._h, _dp(t), _dp(x), _dp(nx), _dp(u)))
        return u

    def calcControlInputDevice(self, t, x, next_x, u, stream=None) -> None:
        """Same on device tensors (torch, float64, contiguous, on this solver's device), asynchronous on `stream` (torch stream or
        None for the solver's own)."""
        s = None if stream is None else C.c_void_p(stream.cuda_stream)
        check(self._L.nmpc_hip_cgmres_control_input_device(self._h, C.c_void_p(t.data_ptr()), C.c_void_p(x.data_ptr()),
                                                            C.c_void_p(next_x.data_ptr()), C.c_void_p(u.data_ptr()), s))

    def synchronize(self) -> None:
        check(self._L.nmpc_hip_cgmres_synchronize(self._h))

    def _get(self, field, dtype, shape):
        n = C.c_size_t()
        check(self._L.nmpc_hip_cgmres_field_bytes(self._h, field, C.byref(n)))
        out = np.zeros(n.value // np.dtype(dtype).itemsize, dtype=dtype)
        check(self._L.nmpc_hip_cgmres_get(self._h, field, out.ctypes.data_as(C.c_void_p), n.value))
        return out.reshape(shape)

    @property
    def x_(self) -> np.ndarray:
        return self._get(FIELD_X, np.float64, (self.B, self.problem_.dim_x_))

    @property
    def u_(self) -> np.ndarray:
        return self._get(FIELD_U, np.float64, (self.B, self.problem_.dim_uc_))

    @property
    def u_list_(self) -> np.ndarray:
        """[B][horizon_divide_num][dim_uc]: column i of the reference's matrix as row i."""
        return self._get(FIELD_U_LIST, np.float64, (self.B, -1, self.problem_.dim_uc_))

    @property
    def delta_u_vec_(self) -> np.ndarray:
        return self._get(FIELD_DELTA_U, np.float64, (self.B, -1))

    def status(self) -> np.ndarray:
        return self._get(FIELD_STATUS, np.int32, (self.B,))

    def err(self) -> np.ndarray:
        """|DhDu_vec_| of the last tick per instance (after setup: |DhDu| at the end of its Newton loop)."""
        return self._get(FIELD_ERR, np.float64, (self.B,))

    def log_t(self) -> np.ndarray:
        return self._get(FIELD_LOG_T, np.float64, (-1,))

    def log_x(self) -> np.ndarray:
        return self._get(FIELD_LOG_X, np.float64, (self.B, -1, self.problem_.dim_x_))

    def log_u(self) -> np.ndarray:
        return self._get(FIELD_LOG_U, np.float64, (self.B, -1, self.problem_.dim_uc_))

    def log_err(self) -> np.ndarray:
        return self._get(FIELD_LOG_ERR, np.float64, (self.B, -1))

    def log_iters(self) -> np.ndarray:
        return self._get(FIELD_LOG_ITERS, np.int32, (self.B, -1))

    def log_reorth(self) -> np.ndarray:
        return self._get(FIELD_LOG_REORTH, np.int32, (self.B, -1))

    def lastDurationMs(self) -> float:
        ms = C.c_float()
        check(self._L.nmpc_hip_cgmres_last_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def modelEval(self, t, x, u, lmd):
        """The four problem functions at P points (point p with instance p % B's problem object): (dotx, dotlmd, DphiDx, DhDu)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        P = x.shape[0]
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, float), (P,)))
        u = np.ascontiguousarray(u, dtype=np.float64)
        lmd = np.ascontiguousarray(lmd, dtype=np.float64)
        nx, nuc = self.problem_.dim_x_, self.problem_.dim_uc_
        dotx, dotlmd, dphidx, dhdu = np.zeros((P, nx)), np.zeros((P, nx)), np.zeros((P, nx)), np.zeros((P, nuc))
        check(self._L.nmpc_hip_cgmres_model_eval(self._h, P, _dp(t), _dp(x), _dp(u), _dp(lmd), _dp(dotx), _dp(dotlmd), _dp(dphidx),
                                                 _dp(dhdu)))
        return dotx, dotlmd, dphidx, dhdu

    def dump(self, instance: int, directory: str) -> None:
        """The files CgmresSolver::run writes (CgmresSolver.cpp:68-106) for one instance of the last run, in its format:
        cgmres_x.dat, cgmres_u.dat, cgmres_err.dat ("t, v0, v1, ..." per logged tick) and cgmres_param.dat."""
        os.makedirs(directory, exist_ok=True)
        t = self.log_t()
        fmt = lambda row: ", ".join("%g" % v for v in row)  # noqa: E731  (std::ostream's default: 6 significant digits)
        for name, data in (("x", self.log_x()[instance]), ("u", self.log_u()[instance]), ("err", self.log_err()[instance][:, None])):
            with open(os.path.join(directory, "cgmres_%s.dat" % name), "w") as f:
                for ti, row in zip(t, data):
                    f.write("%g, %s\n" % (ti, fmt(row)))
        with open(os.path.join(directory, "cgmres_param.dat"), "w") as f:
            f.write("{\n")
            f.write('"log_dt": %g,\n' % (self._cfg.dt * self._cfg.dump_step))
            self.problem_.dumpData(f)
            f.write("}\n")
