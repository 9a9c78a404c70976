"""ctypes wrapper of the CPU checker of FMPC problems with time-varying dimensions (tests/cpp/fmpc_dynamic_checker.cpp): built with
g++ -O2 -ffp-contract=off into a directory the caller owns (a pytest tmp_path), never into the tree.

Arrays follow the library's boundary layouts (include/nmpc_hip_fmpc.h), padded to the capacities: x [B][T+1][N], u [B][T][M],
lambda [B][T+1][N], s / nu [B][T][G]; gains k [B][T][M], K [B][T][N][M] (entry (a, c) at [c][a]), s [B][T+1][N], P [B][T+1][N][N]."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"fmpc_oscillator": 0, "fmpc_cartpole": 1, "fmpc_pointmass": 2, "fmpc_vertical": 3}
CFG_FIELDS = ("horizon_steps", "max_iter", "check_nan", "init_complementary_variable", "update_barrier_eps", "break_if_llt_fails",
              "enable_line_search", "merit_const_scale_from_lagrange_multipliers")


def build(out_dir) -> "Checker":
    lib = os.path.join(str(out_dir), "libfmpc_dynamic_checker.so")
    src = os.path.join(ROOT, "tests", "cpp", "fmpc_dynamic_checker.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", src, "-o", lib],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return Checker(lib)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Checker:
    def __init__(self, path: str):
        self.L = C.CDLL(path)

    def model_info(self, model):
        n, m, g, p = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        assert self.L.chk_model_info(MODELS[model], C.byref(n), C.byref(m), C.byref(g), C.byref(p)) == 0
        return n.value, m.value, g.value, p.value

    def default_params(self, model):
        out = np.zeros(self.model_info(model)[3])
        assert self.L.chk_default_params(MODELS[model], _p(out)) == 0
        return out

    def dims_at(self, model, t, params=None):
        m, g = C.c_int(), C.c_int()
        p = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
        assert self.L.chk_dims_at(MODELS[model], _p(p), C.c_double(t), C.byref(m), C.byref(g)) == 0
        return m.value, g.value

    @staticmethod
    def _cfg(cfg):
        """cfg: an object with the attributes of nmpc_amd.fmpc.Configuration (or a dict)."""
        get = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
        return np.array([int(get(k)) for k in CFG_FIELDS], dtype=np.int32), float(get("kkt_error_thre"))

    @staticmethod
    def _params(params, B):
        p = np.ascontiguousarray(params, dtype=np.float64)
        return p, int(p.ndim == 2)

    def solve(self, model, cfg, params, t0, x0, var, barrier_eps=None, n_threads=16):
        """var: (x, u, lambda, s, nu) [B][...] — copied, the result holds the updated variable."""
        n, m, g, _ = self.model_info(model)
        ci, kkt = self._cfg(cfg)
        T, max_iter = int(ci[0]), int(ci[1])
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        B = x0.shape[0]
        t0 = np.ascontiguousarray(np.broadcast_to(t0, (B,)), dtype=np.float64)
        p, per = self._params(params, B)
        r = SimpleNamespace()
        r.x, r.u, r.lam, r.s, r.nu = (np.array(a, dtype=np.float64, copy=True) for a in var)
        r.barrier_eps = np.full(B, 1e-4) if barrier_eps is None else np.array(np.broadcast_to(barrier_eps, (B,)), dtype=np.float64)
        r.status, r.iters = np.zeros(B, np.int32), np.zeros(B, np.int32)
        r.trace = np.zeros((B, max_iter, 6))
        r.dx, r.du, r.dlam = np.zeros((B, T + 1, n)), np.zeros((B, T, m)), np.zeros((B, T + 1, n))
        r.ds, r.dnu = np.zeros((B, T, g)), np.zeros((B, T, g))
        r.k, r.K, r.gs, r.P = np.zeros((B, T, m)), np.zeros((B, T, n, m)), np.zeros((B, T + 1, n)), np.zeros((B, T + 1, n, n))
        r.merit = np.zeros((B, 3))
        assert self.L.chk_solve(MODELS[model], _p(p), per, _p(ci), C.c_double(kkt), B, _p(t0), _p(x0), _p(r.x), _p(r.u), _p(r.lam),
                                _p(r.s), _p(r.nu), _p(r.barrier_eps), _p(r.status), _p(r.iters), _p(r.trace), _p(r.dx), _p(r.du),
                                _p(r.dlam), _p(r.ds), _p(r.dnu), _p(r.k), _p(r.K), _p(r.gs), _p(r.P), _p(r.merit), int(n_threads)) == 0
        return r

    def closed_loop(self, model, cfg, params, t0, x0, var, n_ticks, sim_dt, substeps=1, barrier_eps=None, n_threads=16):
        n, m, g, _ = self.model_info(model)
        ci, kkt = self._cfg(cfg)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        B = x0.shape[0]
        t0 = np.ascontiguousarray(np.broadcast_to(t0, (B,)), dtype=np.float64)
        p, per = self._params(params, B)
        r = SimpleNamespace()
        r.x, r.u, r.lam, r.s, r.nu = (np.array(a, dtype=np.float64, copy=True) for a in var)
        r.barrier_eps = np.full(B, 1e-4) if barrier_eps is None else np.array(np.broadcast_to(barrier_eps, (B,)), dtype=np.float64)
        r.x_log, r.u0_log = np.zeros((B, n_ticks, n)), np.zeros((B, n_ticks, m))
        r.status_log, r.iter_log = np.zeros((B, n_ticks), np.int32), np.zeros((B, n_ticks), np.int32)
        assert self.L.chk_closed_loop(MODELS[model], _p(p), per, _p(ci), C.c_double(kkt), B, _p(t0), _p(x0), _p(r.x), _p(r.u),
                                      _p(r.lam), _p(r.s), _p(r.nu), _p(r.barrier_eps), int(n_ticks), C.c_double(sim_dt), int(substeps),
                                      _p(r.x_log), _p(r.u0_log), _p(r.status_log), _p(r.iter_log), int(n_threads)) == 0
        return r
