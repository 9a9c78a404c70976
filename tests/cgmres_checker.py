"""ctypes wrapper of the C/GMRES CPU checker (tests/cpp/cgmres_checker.cpp): built with g++ -O2 -ffp-contract=off into a
directory the caller owns (a pytest tmp_path), never into the tree."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"cgmres_semiactive_damper": 0, "cgmres_cartpole": 1, "cgmres_cartpole_with_input_bound": 2}
N_PARAMS = {0: 9, 1: 19, 2: 19}


def build(out_dir: str) -> "Checker":
    lib = os.path.join(str(out_dir), "libcgmres_checker.so")
    src = os.path.join(ROOT, "tests", "cpp", "cgmres_checker.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", src, "-o", lib],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return Checker(lib)


def default_params(model: str) -> np.ndarray:
    """The default problem objects (the models' member initialisers), as the checker reads them."""
    if MODELS[model] == 0:
        return np.array([-1.0, -1.0, 1.0, 1.0, 10.0, 1.0, 0.1, 1.0, 10.0])
    return np.array([1.0, 1.0, 1.0, 100.0, 10, 100, 1, 10, 10, 0.01, 100, 300, 1, 10, 0, 0, 0, 0, 9.80665])


def initial(model: str):
    return {0: ([2.0, 0.0], [0.01, 0.9, 0.03]), 1: ([0.0, math.pi, 0.0, 0.0], [0.0]),
            2: ([0.0, math.pi, 0.0, 0.0], [0.0, 1.0, 0.01])}[MODELS[model]]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Result:
    pass


class Checker:
    def __init__(self, path: str):
        self.L = C.CDLL(path)

    def dims(self, model: str):
        nx, nuc = C.c_int(), C.c_int()
        assert self.L.chk_model_dims(MODELS[model], C.byref(nx), C.byref(nuc)) == 0
        return nx.value, nuc.value

    def model_eval(self, model, params, t, x, u, lmd):
        nx, nuc = self.dims(model)
        P = x.shape[0]
        t, x, u, lmd = (np.ascontiguousarray(a, dtype=np.float64) for a in (t, x, u, lmd))
        params = np.ascontiguousarray(params, dtype=np.float64)
        out = [np.zeros((P, nx)), np.zeros((P, nx)), np.zeros((P, nx)), np.zeros((P, nuc))]
        assert self.L.chk_model_eval(MODELS[model], _p(params), P, _p(t), _p(x), _p(u), _p(lmd), *[_p(o) for o in out]) == 0
        return out

    def dense_gmres(self, A, b, x0=None, k_max=1000, apply_reorth=True, eps=1e-10):
        A = np.ascontiguousarray(A, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        n = b.shape[0]
        x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
        it, ro = C.c_int(), C.c_int()
        self.L.chk_dense_gmres(n, _p(A), _p(b), _p(x), k_max, int(apply_reorth), C.c_double(eps), C.byref(it), C.byref(ro))
        return x, it.value, ro.value

    def solve(self, model, cfg, x0, u0, params=None, per_instance=False, run=True, n_threads=16):
        """cfg: the C-ABI's config as a dict (nmpc_amd.cgmres.CConfig field names).  Returns the final state / input / input list,
        status, |DhDu| and the logs [B][rows][...] (rows = 0 when dump_step = 0)."""
        nx, nuc = self.dims(model)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        u0 = np.ascontiguousarray(u0, dtype=np.float64)
        B = x0.shape[0]
        params = default_params(model) if params is None else np.ascontiguousarray(params, dtype=np.float64)
        c = np.array([cfg["sim_duration"], cfg["steady_horizon_duration"], cfg["horizon_divide_num"], cfg["horizon_increase_ratio"],
                      cfg["dt"], cfg["eq_zeta"], cfg["k_max"], cfg["finite_diff_delta"], cfg["dump_step"], cfg["ode_solver"],
                      cfg["sim_ode_solver"]], dtype=np.float64)
        n_ticks = 0
        if run:
            t = 0.0
            while t <= cfg["sim_duration"]:
                n_ticks += 1
                t += cfg["dt"]
        rows = (n_ticks - 1) // cfg["dump_step"] + 1 if (run and cfg["dump_step"] > 0 and n_ticks > 0) else 0
        r = Result()
        N = cfg["horizon_divide_num"]
        r.x, r.u, r.U = np.zeros((B, nx)), np.zeros((B, nuc)), np.zeros((B, N, nuc))
        r.status, r.err = np.zeros(B, np.int32), np.zeros(B)
        r.log_x, r.log_u = np.full((B, rows, nx), np.nan), np.full((B, rows, nuc), np.nan)
        r.log_err, r.log_iters, r.log_reorth = np.full((B, rows), np.nan), np.full((B, rows), -1, np.int32), np.full((B, rows), -1, np.int32)
        logs = [_p(a) for a in (r.log_x, r.log_u, r.log_err, r.log_iters, r.log_reorth)] if rows else [None] * 5
        r.n_ticks = self.L.chk_solve(MODELS[model], _p(params), int(per_instance), _p(c), B, _p(x0), _p(u0), int(run), n_threads,
                                     _p(r.x), _p(r.u), _p(r.U), _p(r.status), _p(r.err), *logs, rows)
        return r
