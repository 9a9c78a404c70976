"""ctypes wrapper of the FMPC step CPU checker (tests/cpp/fmpc_step_checker.cpp, g++ -O2 -ffp-contract=off, built into a directory
the caller owns, never into the tree), and the cases both FMPC step test files run: linearisations of the pinned oracle's models,
seeded synthetic linearisations (the shapes at which a run-time offset or mask of the kernel can slip, time-varying dimensions with
NaN beyond them), the zero-pivot case and the exactly converged case; and the linearised KKT system as equations (kkt_residuals).

Arrays are numpy [B, T, rows, cols] with the capacities (n, m, g) as block sizes, as nmpc_amd.fmpc_step.FmpcStepBatch.step takes them.
The bar of every comparison of device outputs with the checker is TOL * (1 + |ref|) with TOL = 1e-9; the bars against
the oracle are those of tests/test_gpu_fmpc.py."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
LIN = ("A", "B", "C", "D", "Lx", "Lu", "Lxx", "Luu", "Lxu", "f", "g", "Lx_T", "Lxx_T", "current_x")
VAR = ("x", "u", "lam", "s", "nu")
REAL_FIELDS = ("kkt_error", "barrier_eps", "alpha_s_max", "alpha_nu_max", "k", "K", "s", "P", "dx", "du", "dlam", "ds", "dnu", "x", "u",
               "lam", "vs", "vnu")
# the reference's defaults (FmpcSolver.h:57-89) and this boundary's switches
CONFIG_DEFAULTS = dict(kkt_error_thre=1e-4, check_nan=1, init_complementary_variable=0, update_barrier_eps=1, break_if_llt_fails=0,
                       apply_update=1)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Result:
    """The fields of nmpc_amd.fmpc_step.Result."""


class Case:
    """Inputs of one batch: name, n, m, g, T, dt, the fourteen linearisation arrays in `lin`, the variable in `var`, barrier_eps [B],
    the per-step dimensions (or None)."""

    def __init__(self, name, n, m, g, T, dt, lin, var, eps=None, mdims=None, gdims=None):
        self.name, self.n, self.m, self.g, self.T, self.dt = name, n, m, g, T, dt
        self.lin = {k: np.ascontiguousarray(lin[k], dtype=np.float64) for k in LIN}
        self.var = {k: np.ascontiguousarray(var[k], dtype=np.float64) for k in VAR}
        self.B = self.lin["A"].shape[0]
        self.eps = np.full(self.B, 1e-4) if eps is None else np.ascontiguousarray(eps, dtype=np.float64)
        self.mdims = None if mdims is None else np.ascontiguousarray(mdims, dtype=np.int32)
        self.gdims = None if gdims is None else np.ascontiguousarray(gdims, dtype=np.int32)
        for a in list(self.lin.values()) + list(self.var.values()) + [self.eps]:
            a.setflags(write=False)

    def take(self, idx):
        """The case restricted to (or re-ordered into) the instances `idx`."""
        idx = np.asarray(idx)
        return Case(self.name, self.n, self.m, self.g, self.T, self.dt, {k: v[idx].copy() for k, v in self.lin.items()},
                    {k: v[idx].copy() for k, v in self.var.items()}, self.eps[idx].copy(), self.mdims, self.gdims)

    def replace(self, lin=None, var=None):
        """A copy with some arrays replaced."""
        l2 = {k: v.copy() for k, v in self.lin.items()}
        v2 = {k: v.copy() for k, v in self.var.items()}
        l2.update(lin or {})
        v2.update(var or {})
        return Case(self.name, self.n, self.m, self.g, self.T, self.dt, l2, v2, self.eps.copy(), self.mdims, self.gdims)


def concat(cases) -> Case:
    c0 = cases[0]
    assert all((c.n, c.m, c.g, c.T, c.dt) == (c0.n, c0.m, c0.g, c0.T, c0.dt) for c in cases)
    return Case("+".join(c.name for c in cases), c0.n, c0.m, c0.g, c0.T, c0.dt, {k: np.concatenate([c.lin[k] for c in cases]) for k in LIN},
                {k: np.concatenate([c.var[k] for c in cases]) for k in VAR}, np.concatenate([c.eps for c in cases]), c0.mdims, c0.gdims)


class Checker:
    def __init__(self, path: str):
        self.L = C.CDLL(path)
        f = self.L.fmpc_step_chk_step
        f.argtypes = [C.c_int] * 5 + [C.c_void_p] * 22 + [C.c_double] * 2 + [C.c_int] * 6 + [C.c_void_p] * 13
        f.restype = C.c_int
        g = self.L.fmpc_step_chk_ldlt_solve
        g.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        g.restype = C.c_int

    def step(self, case: Case, n_threads=16, **config) -> Result:
        """One iteration of every instance of `case` from its variable; the Result carries the variable after the call."""
        cfg = dict(CONFIG_DEFAULTS)
        cfg.update(config)
        B, T, n, m, g = case.B, case.T, case.n, case.m, case.g
        r = Result()
        r.x, r.u, r.lam, r.vs, r.vnu = (case.var[k].copy() for k in VAR)
        r.barrier_eps = case.eps.copy()
        r.status = np.zeros(B, np.int32)
        r.kkt_error, r.alpha_s_max, r.alpha_nu_max = np.zeros(B), np.zeros(B), np.zeros(B)
        r.k, r.K = np.zeros((B, T, m)), np.zeros((B, T, m, n))
        r.s, r.P = np.zeros((B, T + 1, n)), np.zeros((B, T + 1, n, n))
        r.dx, r.du, r.dlam = np.zeros((B, T + 1, n)), np.zeros((B, T, m)), np.zeros((B, T + 1, n))
        r.ds, r.dnu = np.zeros((B, T, g)), np.zeros((B, T, g))
        rc = self.L.fmpc_step_chk_step(
            B, n, m, g, T, _p(case.mdims), _p(case.gdims), *[_p(case.lin[k]) for k in LIN], _p(r.x), _p(r.u), _p(r.lam), _p(r.vs),
            _p(r.vnu), _p(r.barrier_eps), case.dt, cfg["kkt_error_thre"], int(cfg["check_nan"]), int(cfg["init_complementary_variable"]),
            int(cfg["update_barrier_eps"]), int(cfg["break_if_llt_fails"]), int(cfg["apply_update"]), n_threads, _p(r.status),
            _p(r.kkt_error), _p(r.alpha_s_max), _p(r.alpha_nu_max), _p(r.k), _p(r.K), _p(r.s), _p(r.P), _p(r.dx), _p(r.du), _p(r.dlam),
            _p(r.ds), _p(r.dnu))
        assert rc == 0
        return r

    def ldlt_solve(self, G, b, use_lu=False):
        """(x, ok): x = G^-1 b through the checker's LDLT (or LU); ok = the LDLT's info() == Success."""
        G = np.ascontiguousarray(G, dtype=np.float64)
        m = G.shape[0]
        bb = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(m, -1).T).copy()  # [c][m]
        ok = self.L.fmpc_step_chk_ldlt_solve(_p(G), m, _p(bb), bb.shape[0], int(use_lu))
        assert ok >= 0
        return bb.T.reshape(np.shape(b)).copy(), bool(ok)


def build(out_dir: str) -> Checker:
    lib = os.path.join(str(out_dir), "libfmpc_step_checker.so")
    src = os.path.join(ROOT, "tests", "cpp", "fmpc_step_checker.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", src, "-o", lib], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return Checker(lib)


_checker = None


def shared_checker(tmp_dir) -> Checker:
    global _checker
    if _checker is None:
        _checker = build(tmp_dir)
    return _checker


def rel_err(a, ref) -> float:
    """max |a - ref| / (1 + |ref|); inf where the NaN patterns differ."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if not np.array_equal(np.isnan(a), np.isnan(ref)):
        return float("inf")
    ok = ~np.isnan(ref)
    with np.errstate(invalid="ignore"):
        e = np.abs(a[ok] - ref[ok]) / (1 + np.abs(ref[ok]))
    e = np.where(a[ok] == ref[ok], 0.0, e)  # equal infinities
    return float(np.nan_to_num(e, nan=np.inf).max()) if ok.any() else 0.0


def compare(got, ref, label, reals=REAL_FIELDS, instances=None):
    """Every status equal and every real field within TOL (1 + |ref|); the figures are printed first."""
    sel = slice(None) if instances is None else instances
    errs = {f: rel_err(np.asarray(getattr(got, f))[sel], np.asarray(getattr(ref, f))[sel]) for f in reals}
    print("fmpc_step %s: %s" % (label, ", ".join("%s %.2e" % kv for kv in errs.items())))
    g, r = np.asarray(got.status)[sel], np.asarray(ref.status)[sel]
    assert np.array_equal(g, r), (label, "status", g, r)
    for f, e in errs.items():
        assert e <= TOL, (label, f, e)


def assert_close(a, b, rtol, atol, what):
    """The comparison of tests/test_gpu_fmpc.py; the worst excess over the bound is printed."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(a)
    err = np.abs(a[ok] - b[ok])
    bound = atol + rtol * np.maximum(np.abs(a[ok]), np.abs(b[ok]))
    if err.size:
        print("  %s: max err %.3e, worst err / bound %.3e" % (what, float(err.max()), float((err / bound).max())))
    assert np.all(err <= bound), (what, float(np.max(err - bound)))


# ---- synthetic cases -------------------------------------------------------------------------------------------------------
# (n, m, g): the smallest shape, one with no input, one that fills no tile with g not a multiple of the MFMA's 4, the largest
BASE_SHAPES = ((1, 1, 1), (2, 0, 1), (3, 2, 5), (16, 16, 32))
# where a run-time offset or mask can slip: n, m at 4 / 5, 8 / 9, 12 / 13 and 15 / 16 (a contraction group of four just full or just
# started), g at 16 / 17 (the second inequality tile empty, or holding one row), 20, 24 and 31 (partly filled), strongly non-square
BOUNDARY_SHAPES = ((4, 4, 4), (5, 3, 16), (5, 3, 17), (8, 9, 20), (13, 12, 31), (16, 1, 24), (1, 16, 9), (15, 15, 15), (9, 16, 32),
                   (16, 16, 17))
SYNTHETIC_SHAPES = BASE_SHAPES + BOUNDARY_SHAPES
NO_INEQ_SHAPES = ((5, 3, 0), (16, 16, 0))  # g = 0: no inequality tile in the layout; needs update_barrier_eps = 0
ONE_STEP_SHAPES = ((1, 1, 1), (5, 3, 17), (13, 12, 31))  # run with T = 1: no next record to request
SYNTHETIC_T = 4
SYNTHETIC_B = 5
VARYING_DIMS = ((2, 0, 1, 2), (5, 0, 3, 5))  # m_i and g_i of the (3, 2, 5) case with time-varying dimensions
# a two-tile handle (gt() = 2) with T = 5: (m_i, g_i) with the second tile full, dead, absent, holding one row and dead again; with
# the second tile holding one row, full and dead in turn; and with the second tile dead at every step
VARYING_SHAPE = (7, 6, 29)
VARYING_T = 5
VARYING_CASES = (((6, 0, 3, 6, 1), (29, 16, 0, 17, 5)), ((1, 2, 3, 4, 5), (17, 29, 1, 15, 28)), ((6,) * 5, (16,) * 5))


def varying_id(dims) -> str:
    return "m%s-g%s" % ("".join("%x" % d for d in dims[0]), ".".join(str(d) for d in dims[1]))


@functools.lru_cache(maxsize=None)
def synthetic_case(n: int, m: int, g: int, B: int = SYNTHETIC_B, T: int = SYNTHETIC_T, varying=False, seed: int = 0) -> Case:
    """Seeded strictly feasible linearisations with Lxx = Luu = I (U uniform in +-1): A = I + 0.1 U, B = 0.3 U, C, D = 0.5 U,
    Lxu = 0.1 U, Lx, Lu = U, g in [-1.5, -0.5], s, nu in [0.5, 2], x, u, lambda = 0.3 N(0, 1), f = x_{i+1} + 0.1 U, dt = 0.1.
    varying: False (the capacities at every step), True (VARYING_DIMS, for the (3, 2, 5) case) or a pair of tuples (m_i, g_i) of
    length T.  The arrays do not depend on it: the entries beyond a step's dimensions are ordinary numbers."""
    rng = np.random.default_rng(10000 * n + 100 * m + g + 7 * seed)
    U = lambda *shape: rng.uniform(-1, 1, shape)
    eye = lambda k, *lead: np.broadcast_to(np.eye(k), lead + (k, k)).copy()
    var = dict(x=0.3 * rng.standard_normal((B, T + 1, n)), u=0.3 * rng.standard_normal((B, T, m)),
               lam=0.3 * rng.standard_normal((B, T + 1, n)), s=rng.uniform(0.5, 2.0, (B, T, g)), nu=rng.uniform(0.5, 2.0, (B, T, g)))
    lin = dict(A=eye(n, B, T) + 0.1 * U(B, T, n, n), B=0.3 * U(B, T, n, m), C=0.5 * U(B, T, g, n), D=0.5 * U(B, T, g, m), Lx=U(B, T, n),
               Lu=U(B, T, m), Lxx=eye(n, B, T), Luu=eye(m, B, T), Lxu=0.1 * U(B, T, n, m), f=var["x"][:, 1:] + 0.1 * U(B, T, n),
               g=rng.uniform(-1.5, -0.5, (B, T, g)), Lx_T=U(B, n), Lxx_T=eye(n, B), current_x=var["x"][:, 0] + 0.1 * U(B, n))
    md, gd = (None, None) if varying is False else (VARYING_DIMS if varying is True else varying)
    if md is not None:
        assert len(md) == T == len(gd) and 0 <= min(md) and max(md) <= m and 0 <= min(gd) and max(gd) <= g, (md, gd)
    name = "synthetic-%dx%dx%d%s%s" % (n, m, g, "" if T == SYNTHETIC_T else "-T%d" % T,
                                       "" if varying is False else "-varying" if varying is True else "-" + varying_id(varying))
    return Case(name, n, m, g, T, 0.1, lin, var, None, md, gd)


def step_dims(case: Case):
    """(m_i, g_i) of every step, the capacities written out where the case has none."""
    md = [case.m] * case.T if case.mdims is None else [int(d) for d in case.mdims]
    gd = [case.g] * case.T if case.gdims is None else [int(d) for d in case.gdims]
    return md, gd


def poisoned(case: Case, variable: bool = False) -> Case:
    """A copy of `case` with NaN in every entry beyond a step's dimensions, which the boundary promises not to read: the columns
    >= m_i of B, D and Lxu, the rows and columns >= m_i of Luu, Lu[m_i:], the rows >= g_i of C and D, g[g_i:]; with `variable` also
    u[m_i:], s[g_i:] and nu[g_i:], which the boundary promises to leave alone."""
    lin = {k: case.lin[k].copy() for k in ("B", "C", "D", "Lu", "Luu", "Lxu", "g")}
    var = {k: case.var[k].copy() for k in ("u", "s", "nu")}
    for i, (mi, gi) in enumerate(zip(*step_dims(case))):
        for k in ("B", "D", "Lxu", "Luu"):
            lin[k][:, i, :, mi:] = np.nan
        lin["Luu"][:, i, mi:, :] = np.nan
        lin["Lu"][:, i, mi:] = np.nan
        lin["C"][:, i, gi:, :] = np.nan
        lin["D"][:, i, gi:, :] = np.nan
        lin["g"][:, i, gi:] = np.nan
        var["u"][:, i, mi:] = np.nan
        var["s"][:, i, gi:] = np.nan
        var["nu"][:, i, gi:] = np.nan
    c = case.replace(lin=lin, var=var if variable else None)
    c.name = case.name + (" poisoned with its variable" if variable else " poisoned")
    return c


def beyond_dims(case: Case):
    """Boolean masks [T, m] and [T, g]: the entries of u (du, k) and of s, nu (ds, dnu) beyond a step's dimensions."""
    md, gd = step_dims(case)
    return (np.arange(case.m)[None, :] >= np.array(md)[:, None], np.arange(case.g)[None, :] >= np.array(gd)[:, None])


def assert_poison_left_no_trace(clean, dirty, case: Case, variable: bool, fields=REAL_FIELDS + ("status",)):
    """`dirty` (the Result on poisoned(case, variable)) has the bits of `clean` (the Result on `case`); where the variable was
    poisoned too, those entries come back as NaN and every other entry of the variable has the bits of `clean`."""
    mu, mg = beyond_dims(case)
    for f in fields:
        a, b = np.asarray(getattr(clean, f)), np.asarray(getattr(dirty, f))
        if variable and f in ("u", "vs", "vnu"):
            mask = np.broadcast_to(mu if f == "u" else mg, b.shape)
            assert np.isnan(b[mask]).all(), f
            a, b = np.where(mask, 0.0, a), np.where(mask, 0.0, b)
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (case.name, f)
        if not (variable and f in ("u", "vs", "vnu")):
            assert not np.isnan(b).any(), (case.name, f)


def assert_zero_beyond_dims(r, case: Case):
    """k, K, du, ds, dnu beyond a step's dimensions are exactly 0."""
    mu, mg = beyond_dims(case)
    for f, mask in (("k", mu), ("du", mu), ("ds", mg), ("dnu", mg)):
        a = np.asarray(getattr(r, f))
        assert (a[np.broadcast_to(mask, a.shape)] == 0).all(), (case.name, f)
    K = np.asarray(r.K)  # [B, T, m, n]
    assert (K[np.broadcast_to(mu[None, :, :, None], K.shape)] == 0).all(), (case.name, "K")


# ---- the linearised KKT system, stated as equations ------------------------------------------------------------------------
def kkt_residuals(case: Case, r) -> dict:
    """Scaled residuals, per block, of the linear system FmpcSolver::procOnce solves for the delta (FmpcSolver.hpp, the equations
    behind the Riccati recursion (2.33)-(2.36) and behind (2.27)), evaluated in numpy longdouble from the arrays of `case` (its
    variable is the one the delta was computed at: r comes from step(case, apply_update=0)), r.barrier_eps and r's delta:

      dynamics        dx_0 = current_x - x_0;   dx_{i+1} = A_i dx_i + B_i du_i + (f_i - x_{i+1})
      stationarity x  (-lam_i + dt Lx_i + A_i' lam_{i+1} + C_i' nu_i) + dt Lxx_i dx_i + dt Lxu_i du_i + A_i' dlam_{i+1} - dlam_i
                      + C_i' dnu_i = 0;   (Lx_T - lam_T) + Lxx_T dx_T - dlam_T = 0
      stationarity u  (dt Lu_i + B_i' lam_{i+1} + D_i' nu_i) + dt Lxu_i' dx_i + dt Luu_i du_i + B_i' dlam_{i+1} + D_i' dnu_i = 0
      inequality      C_i dx_i + D_i du_i + ds_i + (g_i + s_i) = 0
      complementarity s_i dnu_i + nu_i ds_i + s_i nu_i - barrier_eps = 0     (elementwise)

    Each block's figure is max over instances of max|residual| / (1 + max|term|), with the terms being the summands written above
    (matrix-vector products as one term each) of that instance."""
    L = np.longdouble
    T, dt = case.T, L(case.dt)
    md, gd = step_dims(case)
    lin = {k: v.astype(L) for k, v in case.lin.items()}
    x, u, lam, s, nu = (case.var[k].astype(L) for k in VAR)
    dx, du, dlam, ds, dnu = (np.asarray(getattr(r, k)).astype(L) for k in ("dx", "du", "dlam", "ds", "dnu"))
    eps = np.asarray(r.barrier_eps).astype(L)
    worst = dict(dynamics=0.0, stationarity_x=0.0, stationarity_u=0.0, inequality=0.0, complementarity=0.0)

    def note(block, terms):
        res = sum(terms)
        scale = 1 + max([float(np.abs(t).max()) for t in terms if t.size] + [0.0])
        if res.size:
            worst[block] = max(worst[block], float(np.abs(res).max()) / scale)

    for b in range(case.B):
        note("dynamics", [lin["current_x"][b], -x[b, 0], -dx[b, 0]])
        for i in range(T):
            m, g = md[i], gd[i]
            A, Bm, Cm, Dm = lin["A"][b, i], lin["B"][b, i][:, :m], lin["C"][b, i][:g], lin["D"][b, i][:g, :m]
            Lxx, Luu, Lxu = lin["Lxx"][b, i], lin["Luu"][b, i][:m, :m], lin["Lxu"][b, i][:, :m]
            dui, si, nui, dsi, dnui = du[b, i, :m], s[b, i, :g], nu[b, i, :g], ds[b, i, :g], dnu[b, i, :g]
            note("dynamics", [A @ dx[b, i], Bm @ dui, lin["f"][b, i], -x[b, i + 1], -dx[b, i + 1]])
            note("stationarity_x", [-lam[b, i], dt * lin["Lx"][b, i], A.T @ lam[b, i + 1], Cm.T @ nui, dt * (Lxx @ dx[b, i]),
                                    dt * (Lxu @ dui), A.T @ dlam[b, i + 1], -dlam[b, i], Cm.T @ dnui])
            note("stationarity_u", [dt * lin["Lu"][b, i][:m], Bm.T @ lam[b, i + 1], Dm.T @ nui, dt * (Lxu.T @ dx[b, i]), dt * (Luu @ dui),
                                    Bm.T @ dlam[b, i + 1], Dm.T @ dnui])
            note("inequality", [Cm @ dx[b, i], Dm @ dui, dsi, lin["g"][b, i][:g], si])
            note("complementarity", [si * dnui, nui * dsi, si * nui, np.full(g, -eps[b])])
        note("stationarity_x", [lin["Lx_T"][b], -lam[b, T], lin["Lxx_T"][b] @ dx[b, T], -dlam[b, T]])
    return worst


def zero_pivot_case(B: int = 3, at: int = 1) -> Case:
    """n 3, m 2 (g 5) among synthetic neighbours: at the last step of instance `at` Luu = [[0, 1], [1, 0]], D = 0 and Lxx_T = 0, so
    G is exactly dt Luu: the whole diagonal is zero and the lower part is not, and the LDLT reports failure at pivot 0."""
    base = synthetic_case(3, 2, 5, B=B)
    lin = {k: base.lin[k].copy() for k in ("Luu", "D", "Lxx_T")}
    lin["Luu"][at, -1] = [[0.0, 1.0], [1.0, 0.0]]
    lin["D"][at, -1] = 0.0
    lin["Lxx_T"][at] = 0.0
    c = base.replace(lin=lin)
    c.name = "zero-pivot"
    return c


def converged_case(n=3, m=2, g=5, B=2) -> Case:
    """Every residual exactly 0: f = x_{i+1}, g = -s, lambda = nu = 0, all cost gradients 0, current_x = x_0."""
    base = synthetic_case(n, m, g, B=B)
    var = dict(lam=np.zeros_like(base.var["lam"]), nu=np.zeros_like(base.var["nu"]))
    lin = dict(f=base.var["x"][:, 1:].copy(), g=-base.var["s"], Lx=np.zeros_like(base.lin["Lx"]), Lu=np.zeros_like(base.lin["Lu"]),
               Lx_T=np.zeros_like(base.lin["Lx_T"]), current_x=base.var["x"][:, 0].copy())
    c = base.replace(lin=lin, var=var)
    c.name = "converged"
    return c


# ---- model cases: the pinned oracle's FMPC models --------------------------------------------------------------------------
MODELS = ("fmpc_oscillator", "fmpc_cartpole", "fmpc_pointmass", "fmpc_vertical")
MODEL_B, MODEL_T = 6, 8
VERTICAL_T0 = 1.96  # dt 0.01: the contact schedule switches from one contact to two at t = 2.0, the horizon's fifth step


def model_start(model: str, B: int = MODEL_B, T: int = MODEL_T):
    """(variable, current_x, t0, params) as make_case of tests/test_gpu_fmpc.py generates them (spread 0.3, seed 1000 + T)."""
    from oracle import fmpc as O
    n, m, g, _ = O.model_info(model)
    spread = 0.3
    rng = np.random.default_rng(1000 + T)
    var = dict(x=spread * rng.standard_normal((B, T + 1, n)), u=spread * rng.standard_normal((B, T, m)),
               lam=spread * rng.standard_normal((B, T + 1, n)), s=rng.uniform(0.5, 2.0, (B, T, g)), nu=rng.uniform(0.5, 2.0, (B, T, g)))
    x0 = spread * rng.standard_normal((B, n))
    t0 = rng.uniform(0, 1, B)
    if model == "fmpc_vertical":
        t0 = np.full(B, VERTICAL_T0)
    return var, x0, t0, O.default_params(model)


def model_dims(model: str, t0: float, T: int = MODEL_T):
    """(m_i, g_i) of every step; None, None where they are the capacities everywhere."""
    from oracle import fmpc as O
    n, m, g, _ = O.model_info(model)
    dt = float(O.default_params(model)[0])
    d = np.array([O.dims_at(model, t0 + i * dt, O.default_params(model)) for i in range(T)], dtype=np.int32)
    if (d[:, 0] == m).all() and (d[:, 1] == g).all():
        return None, None
    return d[:, 0].copy(), d[:, 1].copy()


def linearise(model: str, var: dict, x0, t0, params) -> Case:
    """The linearisation of `model` at the variable, by oracle.fmpc.evaluate on the host."""
    from oracle import fmpc as O
    n, m, g, _ = O.model_info(model)
    B, T = var["u"].shape[:2]
    dt = float(params[0])
    lin = dict(A=np.zeros((B, T, n, n)), B=np.zeros((B, T, n, m)), C=np.zeros((B, T, g, n)), D=np.zeros((B, T, g, m)), Lx=np.zeros((B, T, n)),
               Lu=np.zeros((B, T, m)), Lxx=np.zeros((B, T, n, n)), Luu=np.zeros((B, T, m, m)), Lxu=np.zeros((B, T, n, m)),
               f=np.zeros((B, T, n)), g=np.zeros((B, T, g)), Lx_T=np.zeros((B, n)), Lxx_T=np.zeros((B, n, n)),
               current_x=np.array(x0, dtype=np.float64))
    for b in range(B):
        for i in range(T):
            ev = O.evaluate(model, params, t0[b] + i * dt, var["x"][b, i], var["u"][b, i])
            for k in ("A", "B", "C", "D", "Lx", "Lu", "Lxx", "Luu", "Lxu", "f", "g"):
                lin[k][b, i] = ev[k]
        ev = O.evaluate(model, params, t0[b] + T * dt, var["x"][b, T], np.zeros(m))
        lin["Lx_T"][b], lin["Lxx_T"][b] = ev["Vx"], ev["Vxx"]
    md, gd = model_dims(model, float(t0[0]), T)
    return Case(model, n, m, g, T, dt, lin, var, None, md, gd)


def oracle_solve(model: str, var: dict, x0, t0, params, max_iter: int, T: int = MODEL_T, **config):
    """oracle.fmpc.solve_batch_full from the variable with `max_iter` iterations and kkt_error_thre 0 (never Succeeded early)."""
    from oracle import fmpc as O
    cfg = O.default_config(horizon_steps=T, max_iter=max_iter, **config)
    return O.solve_batch_full(model, cfg, params, t0, x0, O.Variable(var["x"], var["u"], var["lam"], var["s"], var["nu"]), n_threads=4)


def masked(a, dims, axis=2):
    """`a` [B, T, cap, ...] with the entries beyond a step's dimension set to 0."""
    a = np.array(a, dtype=np.float64)
    if dims is None:
        return a
    for i, d in enumerate(dims):
        idx = [slice(None)] * a.ndim
        idx[1] = i
        idx[axis] = slice(int(d), None)
        a[tuple(idx)] = 0.0
    return a


# ---- iterating a model and comparing with the oracle ----------------------------------------------------------------------
def compare_with_oracle(got, ref, case, label, iters=1):
    """The bars of tests/test_gpu_fmpc.py: rtol 1e-8, atol 1e-10 on gains, trace columns and variables; 1e-7 / 1e-9 on the delta.
    `got`: the last iteration's Result (kkt / eps / alphas stacked over the iterations in got.trace)."""
    print("fmpc_step %s vs oracle:" % label)
    assert (ref.status == 5).all() and (np.asarray(got.status) == 6).all(), (ref.status, got.status)  # the oracle's 5 is this 6
    assert (ref.iters == iters).all()
    assert (ref.trace[:, :, 1] < 1e4).all()  # no instance is left out: none diverges
    for col, name in ((1, "kkt_error"), (2, "barrier_eps"), (3, "alpha_s_max"), (4, "alpha_nu_max")):
        assert_close(got.trace[:, :, col - 1], ref.trace[:, :, col], 1e-8, 1e-10, name)
    for name, a, b in (("k", got.k, ref.k), ("K", got.K, ref.K), ("s", got.s, ref.s), ("P", got.P, ref.P)):
        assert_close(a, b, 1e-8, 1e-10, name)
    md, gd = case.mdims, case.gdims
    v = ref.variable
    for name, a, b, dims in (("x", got.x, v.x, None), ("u", got.u, v.u, md), ("lambda", got.lam, v.lam, None), ("s_var", got.vs, v.s, gd),
                             ("nu_var", got.vnu, v.nu, gd)):
        assert_close(masked(a, dims), masked(b, dims), 1e-8, 1e-10, name)
    assert_close(got.barrier_eps, ref.barrier_eps, 1e-8, 1e-10, "barrier_eps after")
    d = ref.delta
    for name, a, b in (("dx", got.dx, d.x), ("du", got.du, d.u), ("dlam", got.dlam, d.lam), ("ds", got.ds, d.s), ("dnu", got.dnu, d.nu)):
        assert_close(a, b, 1e-7, 1e-9, name)


def iterate(step, model, iters, **config):
    """`iters` iterations of `model` from its start through `step(case, **config) -> Result`, relinearising with
    oracle.fmpc.evaluate in between; the last Result with the per-iteration trace, and the first case."""
    var, x0, t0, params = model_start(model)
    trace, first, eps = [], None, None
    for it in range(iters):
        case = linearise(model, var, x0, t0, params)
        if eps is not None:
            case = Case(case.name, case.n, case.m, case.g, case.T, case.dt, case.lin, case.var, eps, case.mdims, case.gdims)
        first = first or case
        r = step(case, **(config if it == 0 else {k: v for k, v in config.items() if k != "init_complementary_variable"}))
        trace.append(np.stack([r.kkt_error, r.barrier_eps, r.alpha_s_max, r.alpha_nu_max], axis=1))
        var = dict(x=r.x, u=r.u, lam=r.lam, s=r.vs, nu=r.vnu)
        eps = r.barrier_eps
    out = Result()
    for f in REAL_FIELDS + ("status",):
        setattr(out, f, getattr(r, f))
    out.trace = np.stack(trace, axis=1)
    return out, first
