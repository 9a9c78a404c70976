"""TEST INFRASTRUCTURE — NOT PRODUCT CODE.

ctypes front end of the CPU FMPC oracle (oracle/fmpc_oracle.hpp: a restatement of the reference's nmpc_fmpc::FmpcSolver on
plain arrays).  Only tests/ and bench.py's cpu_baseline leg may import it, and only as the checker /
reported baseline.  Nothing under nmpc_amd/ imports it.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from dataclasses import dataclass
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_BUILD = os.path.join(_HERE, "_build")
NTRACE = 6
TRACE_FIELDS = ("iter", "kkt_error", "barrier_eps", "alpha_s_max", "alpha_nu_max", "alpha_s")
# FmpcSolver::Status (FmpcSolver.h:92-114); negative: the exceptions of checkVariable (FmpcSolver.hpp:285-354)
STATUS = {0: "Uninitialized", 1: "Succeeded", 2: "ErrorInForward", 3: "ErrorInBackward", 4: "ErrorInUpdate",
          5: "MaxIterationReached", -1: "invalid_argument", -2: "runtime_error"}


class FmpcConfig(C.Structure):
    """Mirror of `oracle_fmpc_config` (fmpc_capi.cpp) = FmpcSolver::Configuration (FmpcSolver.h:57-89) without print_level."""

    _fields_ = [
        ("horizon_steps", C.c_int),
        ("max_iter", C.c_int),
        ("kkt_error_thre", C.c_double),
        ("check_nan", C.c_int),
        ("init_complementary_variable", C.c_int),
        ("update_barrier_eps", C.c_int),
        ("break_if_llt_fails", C.c_int),
        ("enable_line_search", C.c_int),
        ("merit_const_scale_from_lagrange_multipliers", C.c_int),
    ]


_libs: dict = {}


def lib(native: bool = False, out_dir: Optional[str] = None):
    key = (native, out_dir)
    if key in _libs:
        return _libs[key]
    name = "liboracle_fmpc_native.so" if native else "liboracle_fmpc.so"
    path = os.path.join(out_dir or _BUILD, name)
    srcs = [os.path.join(_HERE, f) for f in ("fmpc_capi.cpp", "fmpc_oracle.hpp", "fmpc_models.hpp")]
    if (not os.path.exists(path)) or any(os.path.getmtime(s) > os.path.getmtime(path) for s in srcs):
        subprocess.run(["make", "-C", _HERE, os.path.join(out_dir or "_build", name), f"OUT={out_dir or '_build'}"],
                       check=True, stdout=subprocess.DEVNULL)
    L = C.CDLL(path)
    L.oracle_fmpc_default_config.restype = None
    L.oracle_fmpc_l1_dir_deriv.restype = C.c_double
    _libs[key] = L
    return L


def default_config(**kw) -> FmpcConfig:
    c = FmpcConfig()
    lib().oracle_fmpc_default_config(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, int(v) if isinstance(v, bool) else v)
    return c


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


def model_info(model: str):
    """(state_dim, input_dim, ineq_dim, number of parameter doubles); the two dimensions are capacities where dims_at varies."""
    n, m, g, p = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = lib().oracle_fmpc_model_info(model.encode(), C.byref(n), C.byref(m), C.byref(g), C.byref(p))
    if rc != 0:
        raise ValueError(f"unknown FMPC oracle model {model!r}")
    return n.value, m.value, g.value, p.value


def default_params(model: str) -> np.ndarray:
    out = np.zeros(model_info(model)[3])
    assert lib().oracle_fmpc_default_params(model.encode(), _dp(out)) == 0
    return out


def dims_at(model: str, t: float, params=None):
    """(input_dim, ineq_dim) of a step at time t."""
    m, g = C.c_int(), C.c_int()
    p = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
    if lib().oracle_fmpc_dims_at(model.encode(), _dp(p), C.c_double(t), C.byref(m), C.byref(g)) != 0:
        raise ValueError(f"unknown FMPC oracle model {model!r}")
    return m.value, g.value


@dataclass
class Variable:
    """FmpcSolver::Variable (FmpcSolver.h:117-158): x [T+1][N], u [T][M], lambda [T+1][N], s [T][G], nu [T][G]; a leading
    batch axis in the batched calls."""
    x: np.ndarray
    u: np.ndarray
    lam: np.ndarray
    s: np.ndarray
    nu: np.ndarray

    @staticmethod
    def reset(model: str, T: int, x=0.0, u=0.0, lam=0.0, s=1.0, nu=1.0, batch: Optional[int] = None) -> "Variable":
        """Variable(horizon_steps) + reset (FmpcSolver.hpp:42-69)."""
        n, m, g, _ = model_info(model)
        lead = () if batch is None else (batch,)
        return Variable(np.full(lead + (T + 1, n), float(x)), np.full(lead + (T, m), float(u)),
                        np.full(lead + (T + 1, n), float(lam)), np.full(lead + (T, g), float(s)),
                        np.full(lead + (T, g), float(nu)))

    def copy(self) -> "Variable":
        return Variable(*(a.copy() for a in (self.x, self.u, self.lam, self.s, self.nu)))

    def arrays(self):
        return self.x, self.u, self.lam, self.s, self.nu


@dataclass
class SolveResult:
    status: int
    iters: int
    variable: Variable
    barrier_eps: float
    trace: np.ndarray  # [max_iter][NTRACE], rows beyond iters are zero
    k: np.ndarray  # [T][M]
    K: np.ndarray  # [T][M][N] (row-major view of the column-major m x n gain: K[i][:, j] is column j)
    s: np.ndarray  # [T+1][N]
    P: np.ndarray  # [T+1][N][N] (symmetric)
    delta: Variable


def solve(model: str, cfg: FmpcConfig, params, current_t: float, current_x, var: Variable,
          barrier_eps: float = 1e-4) -> SolveResult:
    n, m, g, _ = model_info(model)
    T = cfg.horizon_steps
    v = Variable(*(np.ascontiguousarray(a, dtype=np.float64).copy() for a in var.arrays()))
    assert v.x.shape == (T + 1, n) and v.u.shape == (T, m) and v.lam.shape == (T + 1, n)
    assert v.s.shape == (T, g) and v.nu.shape == (T, g)
    p = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
    x0 = np.ascontiguousarray(current_x, dtype=np.float64)
    be = C.c_double(barrier_eps)
    iters = C.c_int(0)
    trace = np.zeros((cfg.max_iter, NTRACE))
    gk = np.zeros((T, m))
    gK = np.zeros((T, n, m))  # column-major m x n per step
    gs = np.zeros((T + 1, n))
    gP = np.zeros((T + 1, n, n))
    delta = np.zeros(2 * (T + 1) * n + T * m + 2 * T * g)
    status = lib().oracle_fmpc_solve(model.encode(), C.byref(cfg), _dp(p), C.c_double(current_t), _dp(x0), _dp(v.x), _dp(v.u),
                                     _dp(v.lam), _dp(v.s), _dp(v.nu), C.byref(be), C.byref(iters), _dp(trace), _dp(gk),
                                     _dp(gK), _dp(gs), _dp(gP), _dp(delta))
    o = 0
    parts = []
    for shape in ((T + 1, n), (T, m), (T + 1, n), (T, g), (T, g)):
        size = int(np.prod(shape))
        parts.append(delta[o:o + size].reshape(shape).copy())
        o += size
    return SolveResult(status, iters.value, v, be.value, trace, gk, np.transpose(gK, (0, 2, 1)).copy(), gs,
                       np.transpose(gP, (0, 2, 1)).copy(), Variable(*parts))


@dataclass
class BatchResult:
    status: np.ndarray
    iters: np.ndarray
    variable: Variable
    barrier_eps: np.ndarray
    trace: np.ndarray  # [B][max_iter][NTRACE]
    K0: np.ndarray  # [B][M][N]


def solve_batch(model: str, cfg: FmpcConfig, params, current_t, current_x, var: Variable, barrier_eps=None,
                n_threads: int = 1, native: bool = False, out_dir: Optional[str] = None) -> BatchResult:
    n, m, g, pd = model_info(model)
    T = cfg.horizon_steps
    x0 = np.ascontiguousarray(current_x, dtype=np.float64)
    B = x0.shape[0]
    v = Variable(*(np.ascontiguousarray(a, dtype=np.float64).copy() for a in var.arrays()))
    assert v.x.shape == (B, T + 1, n) and v.u.shape == (B, T, m) and v.s.shape == (B, T, g)
    p = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
    per_instance = int(p is not None and p.ndim == 2)
    if per_instance:
        assert p.shape == (B, pd)
    t0 = np.zeros(B) if current_t is None else np.ascontiguousarray(np.broadcast_to(current_t, (B,)), dtype=np.float64)
    be = np.full(B, 1e-4) if barrier_eps is None else np.ascontiguousarray(np.broadcast_to(barrier_eps, (B,)),
                                                                          dtype=np.float64).copy()
    status = np.zeros(B, dtype=np.int32)
    iters = np.zeros(B, dtype=np.int32)
    trace = np.zeros((B, cfg.max_iter, NTRACE))
    K0 = np.zeros((B, n, m))
    rc = lib(native, out_dir).oracle_fmpc_solve_batch(model.encode(), C.byref(cfg), _dp(p), per_instance, B, _dp(t0), _dp(x0),
                                                      _dp(v.x), _dp(v.u), _dp(v.lam), _dp(v.s), _dp(v.nu), _dp(be),
                                                      _ip(status), _ip(iters), _dp(trace), _dp(K0), int(n_threads))
    assert rc == 0, rc
    return BatchResult(status, iters, v, be, trace, np.transpose(K0, (0, 2, 1)).copy())


def _batch_args(model, cfg, params, current_t, current_x, var, barrier_eps):
    """The leading arguments the batched entry points share, the arrays they point into (to be kept alive over the call), and the
    copies of the variable and barrier_eps that the call updates in place."""
    n, m, g, pd = model_info(model)
    T = cfg.horizon_steps
    x0 = np.ascontiguousarray(current_x, dtype=np.float64)
    B = x0.shape[0]
    v = Variable(*(np.ascontiguousarray(a, dtype=np.float64).copy() for a in var.arrays()))
    assert v.x.shape == (B, T + 1, n) and v.u.shape == (B, T, m) and v.s.shape == (B, T, g)
    p = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
    per_instance = int(p is not None and p.ndim == 2)
    if per_instance:
        assert p.shape == (B, pd)
    t0 = np.ascontiguousarray(np.broadcast_to(0.0 if current_t is None else current_t, (B,)), dtype=np.float64)
    be = np.array(np.broadcast_to(1e-4 if barrier_eps is None else barrier_eps, (B,)), dtype=np.float64)
    args = (model.encode(), C.byref(cfg), _dp(p), per_instance, B, _dp(t0), _dp(x0), _dp(v.x), _dp(v.u), _dp(v.lam), _dp(v.s),
            _dp(v.nu), _dp(be))
    return args, (t0, x0, p), v, be


@dataclass
class FullBatchResult:
    status: np.ndarray
    iters: np.ndarray
    variable: Variable
    barrier_eps: np.ndarray
    trace: np.ndarray  # [B][max_iter][NTRACE]
    k: np.ndarray  # [B][T][M], 0 beyond a step's input dimension
    K: np.ndarray  # [B][T][M][N], rows beyond a step's input dimension 0
    s: np.ndarray  # [B][T+1][N]
    P: np.ndarray  # [B][T+1][N][N]
    delta: Variable  # of the last iteration that reached the forward pass, 0 beyond a step's dimensions
    merit: np.ndarray  # [B][3]: merit_func_, merit_deriv_, merit_const_scale_ of the last line search


def solve_batch_full(model: str, cfg: FmpcConfig, params, current_t, current_x, var: Variable, barrier_eps=None,
                     n_threads: int = 16) -> FullBatchResult:
    """solve_batch with every intermediate solve() returns, for each instance."""
    n, m, g, _ = model_info(model)
    T = cfg.horizon_steps
    args, keep, v, be = _batch_args(model, cfg, params, current_t, current_x, var, barrier_eps)
    B = len(be)
    status, iters = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    trace = np.zeros((B, cfg.max_iter, NTRACE))
    gk, gK, gs, gP = np.zeros((B, T, m)), np.zeros((B, T, n, m)), np.zeros((B, T + 1, n)), np.zeros((B, T + 1, n, n))
    shapes = ((T + 1, n), (T, m), (T + 1, n), (T, g), (T, g))
    delta = np.zeros((B, sum(int(np.prod(sh)) for sh in shapes)))
    merit = np.zeros((B, 3))
    rc = lib().oracle_fmpc_solve_batch_full(*args, _ip(status), _ip(iters), _dp(trace), _dp(gk), _dp(gK), _dp(gs), _dp(gP),
                                            _dp(delta), _dp(merit), int(n_threads))
    assert rc == 0, rc
    parts, o = [], 0
    for sh in shapes:
        size = int(np.prod(sh))
        parts.append(delta[:, o:o + size].reshape((B,) + sh).copy())
        o += size
    return FullBatchResult(status, iters, v, be, trace, gk, np.transpose(gK, (0, 1, 3, 2)).copy(), gs,
                           np.transpose(gP, (0, 1, 3, 2)).copy(), Variable(*parts), merit)


@dataclass
class ClosedLoopResult:
    variable: Variable  # after the last tick
    barrier_eps: np.ndarray
    x_log: np.ndarray  # [B][n_ticks][N]: the state each tick's solve started from
    u0_log: np.ndarray  # [B][n_ticks][M]: u_list[0] of each tick, 0 beyond the step's input dimension
    status_log: np.ndarray
    iter_log: np.ndarray


def closed_loop(model: str, cfg: FmpcConfig, params, current_t, current_x, var: Variable, n_ticks: int, sim_dt: float,
                substeps: int = 1, barrier_eps=None, n_threads: int = 16) -> ClosedLoopResult:
    """n_ticks times { solve from the variable of the tick before; `substeps` plant steps stateEq(t, x, u_list[0], sim_dt) }."""
    n, m, _, _ = model_info(model)
    args, keep, v, be = _batch_args(model, cfg, params, current_t, current_x, var, barrier_eps)
    B = len(be)
    x_log, u0_log = np.zeros((B, n_ticks, n)), np.zeros((B, n_ticks, m))
    status_log, iter_log = np.zeros((B, n_ticks), dtype=np.int32), np.zeros((B, n_ticks), dtype=np.int32)
    rc = lib().oracle_fmpc_closed_loop(*args, int(n_ticks), C.c_double(sim_dt), int(substeps), _dp(x_log), _dp(u0_log),
                                       _ip(status_log), _ip(iter_log), int(n_threads))
    assert rc == 0, rc
    return ClosedLoopResult(v, be, x_log, u0_log, status_log, iter_log)


def evaluate(model: str, params, t: float, x, u, step_dt: float = 0.0) -> dict:
    """Values and derivatives of the problem at (t, x, u); matrices returned row-major (A[i, j] = d f_i / d x_j)."""
    n, m, g, _ = model_info(model)
    x = np.ascontiguousarray(x, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    p = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
    o = dict(f=np.zeros(n), g=np.zeros(g), costs=np.zeros(2), A=np.zeros((n, n)), B=np.zeros((m, n)), C=np.zeros((n, g)),
             D=np.zeros((m, g)), Lx=np.zeros(n), Lu=np.zeros(m), Lxx=np.zeros((n, n)), Luu=np.zeros((m, m)),
             Lxu=np.zeros((m, n)), Vx=np.zeros(n), Vxx=np.zeros((n, n)))
    rc = lib().oracle_fmpc_eval(model.encode(), _dp(p), C.c_double(t), _dp(x), _dp(u), C.c_double(step_dt),
                                *[_dp(o[k]) for k in ("f", "g", "costs", "A", "B", "C", "D", "Lx", "Lu", "Lxx", "Luu", "Lxu",
                                                      "Vx", "Vxx")])
    assert rc == 0
    for k in ("A", "B", "C", "D", "Lxx", "Luu", "Lxu", "Vxx"):
        o[k] = o[k].T.copy()  # stored column-major
    return o


def l1_norm_directional_deriv(func, jac, direction) -> float:
    """l1NormDirectionalDeriv (MathUtils.h:17-38); jac [out_dim][in_dim]."""
    func = np.ascontiguousarray(func, dtype=np.float64)
    jac = np.asarray(jac, dtype=np.float64)
    direction = np.ascontiguousarray(direction, dtype=np.float64)
    jc = np.ascontiguousarray(jac.T)  # column-major image
    return float(lib().oracle_fmpc_l1_dir_deriv(_dp(func), _dp(jc), _dp(direction), jac.shape[0], jac.shape[1]))


def ldlt_solve(G, b, use_lu: bool = False):
    """(x, ok): x = G^-1 b through the Eigen::LDLT restatement (or the full-pivot LU fallback)."""
    G = np.asarray(G, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    n = G.shape[0]
    bb = b.reshape(n, -1)
    bc = np.ascontiguousarray(bb.T).copy()
    ok = lib().oracle_fmpc_ldlt_solve(_dp(np.ascontiguousarray(G.T)), n, _dp(bc), bb.shape[1], int(use_lu))
    return bc.T.reshape(b.shape).copy(), bool(ok)
