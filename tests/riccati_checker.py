"""ctypes wrapper of the Riccati CPU checker (tests/cpp/riccati_checker.cpp, g++ -O2 -ffp-contract=off, built into a directory the
caller owns, never into the tree), and the cases both Riccati test files run: derivatives of the pinned oracle's models along a
rollout, seeded synthetic derivatives (the shapes at which a run-time offset or mask of the kernel can slip, time-varying input
dimensions with NaN beyond them), and the retry cases.

Arrays are numpy [B, T, rows, cols] with the capacities (n, m) as block sizes, as nmpc_amd.riccati.RiccatiBatch.backward takes them.
The bar of every comparison of real outputs is TOL * (1 + |ref|) with TOL = 1e-9."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
B_CASE = 5  # instances per case, different x0 / seeds
REAL_FIELDS = ("k", "K", "dV", "Vx0", "Vxx0", "lam", "dlam")
INT_FIELDS = ("status", "n_backward", "fail_step", "qp_retval", "free_mask")
LAMBDA_DEFAULTS = dict(lam=1e-4, dlam=1.0, lambda_factor=1.6, lambda_min=1e-6, lambda_max=1e10)  # DDPSolver.h:47-110


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Result:
    """The fields of nmpc_amd.riccati.Result."""


class Case:
    """Inputs of one batch: name, n, m, T, dims ([T] or None), the nine derivative arrays in `d`, U / lower / upper (or None),
    reg_type, and what a reference other than the checker says (`expect`: dict of field -> array, possibly empty)."""

    def __init__(self, name, n, m, T, d, dims=None, U=None, lower=None, upper=None, reg_type=1, expect=None):
        self.name, self.n, self.m, self.T, self.d, self.dims = name, n, m, T, d, dims
        self.U, self.lower, self.upper, self.reg_type = U, lower, upper, reg_type
        self.expect = expect or {}
        self.B = d["Fx"].shape[0]
        for a in list(d.values()) + [x for x in (U, lower, upper) if x is not None]:
            a.setflags(write=False)

    @property
    def constrained(self):
        return self.U is not None

    def take(self, idx):
        """The case restricted to (or re-ordered into) the instances `idx`."""
        idx = np.asarray(idx)
        per_step = self.constrained and self.lower.ndim == 3
        return Case(self.name, self.n, self.m, self.T, {k: v[idx].copy() for k, v in self.d.items()}, self.dims,
                    None if self.U is None else self.U[idx].copy(),
                    None if self.lower is None else (self.lower[idx].copy() if per_step else self.lower.copy()),
                    None if self.upper is None else (self.upper[idx].copy() if per_step else self.upper.copy()), self.reg_type)

    def with_limits_per_step(self):
        """The same case with the shared limits [m] written out as [B, T, m]."""
        shape = (self.B, self.T, self.m)
        return Case(self.name, self.n, self.m, self.T, {k: v.copy() for k, v in self.d.items()}, self.dims, self.U.copy(),
                    np.broadcast_to(self.lower, shape).copy(), np.broadcast_to(self.upper, shape).copy(), self.reg_type)


class Checker:
    def __init__(self, path: str):
        self.L = C.CDLL(path)

    def backward(self, case: Case, lam=None, dlam=None, retry=True, lambda_factor=LAMBDA_DEFAULTS["lambda_factor"],
                 lambda_min=LAMBDA_DEFAULTS["lambda_min"], lambda_max=LAMBDA_DEFAULTS["lambda_max"], n_threads=16) -> Result:
        B, T, n, m = case.B, case.T, case.n, case.m
        d = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in case.d.items()}
        dims = None if case.dims is None else np.ascontiguousarray(case.dims, dtype=np.int32)
        lam = np.full(B, LAMBDA_DEFAULTS["lam"] if lam is None else lam, dtype=np.float64)
        dlam = np.full(B, LAMBDA_DEFAULTS["dlam"] if dlam is None else dlam, dtype=np.float64)
        U, lo, up = (None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (case.U, case.lower, case.upper))
        r = Result()
        r.k, r.K, r.dV = np.zeros((B, T, m)), np.zeros((B, T, m, n)), np.zeros((B, 2))
        r.Vx0, r.Vxx0 = np.zeros((B, n)), np.zeros((B, n, n))
        r.status, r.n_backward, r.fail_step = (np.zeros(B, np.int32) for _ in range(3))
        r.lam, r.dlam = np.zeros(B), np.zeros(B)
        r.qp_retval, r.free_mask = np.zeros((B, T), np.int32), np.zeros((B, T), np.uint32)
        f = self.L.riccati_chk_backward
        f.argtypes = ([C.c_int] * 4 + [C.c_void_p] * 13 + [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_double] * 3 + [C.c_int] * 2
                      + [C.c_void_p] * 12)
        f.restype = C.c_int
        rc = f(B, n, m, T, _p(dims), *[_p(d[k]) for k in ("Fx", "Fu", "Lx", "Lu", "Lxx", "Luu", "Lxu", "Vx_T", "Vxx_T")],
               _p(U), _p(lo), _p(up), int(case.constrained and lo.ndim == 3), int(case.constrained), int(case.reg_type),
               _p(lam), _p(dlam), lambda_factor, lambda_min, lambda_max, int(retry), n_threads,
               _p(r.k), _p(r.K), _p(r.dV), _p(r.Vx0), _p(r.Vxx0), _p(r.status), _p(r.n_backward), _p(r.lam), _p(r.dlam),
               _p(r.fail_step), _p(r.qp_retval), _p(r.free_mask))
        assert rc == 0
        return r


def build(out_dir: str) -> Checker:
    lib = os.path.join(str(out_dir), "libriccati_checker.so")
    src = os.path.join(ROOT, "tests", "cpp", "riccati_checker.cpp")
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
    return float((np.abs(a[ok] - ref[ok]) / (1 + np.abs(ref[ok]))).max()) if ok.any() else 0.0


def compare(got, ref, label, reals=REAL_FIELDS, ints=INT_FIELDS, instances=None):
    """Every real field within TOL (1 + |ref|) and every integer field equal; the figures are printed first."""
    sel = slice(None) if instances is None else instances
    errs = {f: rel_err(np.asarray(getattr(got, f))[sel], np.asarray(getattr(ref, f))[sel]) for f in reals}
    print("riccati %s: %s" % (label, ", ".join("%s %.2e" % kv for kv in errs.items())))
    for f in ints:
        g, r = np.asarray(getattr(got, f))[sel], np.asarray(getattr(ref, f))[sel]
        assert np.array_equal(g.astype(np.int64), r.astype(np.int64)), (label, f, g, r)
    for f, e in errs.items():
        assert e <= TOL, (label, f, e)


# ---- model cases: the pinned oracle's models along a rollout ---------------------------------------------------------------
# (model, T, t0): DDPSolver test models; the last three have time-varying input dimensions (1 -> 2, 1 -> 0 -> 1, 16 -> 0 -> 16)
MODELS = (("cartpole", 7, 0.0), ("quadrotor", 5, 0.0), ("manipulator", 4, 0.0), ("vertical", 12, 1.95), ("vertical", 60, 4.45),
          ("centroidal", 12, 1.3))
BOXED = ("cartpole", "quadrotor", "manipulator")
LIMITS = (0.5, 2.0)
USCALE = 1.0
MODEL_CASES = tuple([(mdl, T, t0, None, reg) for mdl, T, t0 in MODELS for reg in (1, 2)]
                    + [(mdl, T, t0, lim, reg) for mdl, T, t0 in MODELS if mdl in BOXED for lim in LIMITS for reg in (1, 2)])


def model_case_id(c):
    mdl, T, t0, lim, reg = c
    return "%s-T%d-%s-reg%d" % (mdl, T, "free" if lim is None else "box%g" % lim, reg)


@functools.lru_cache(maxsize=None)
def model_case(mdl: str, T: int, t0: float, lim, reg: int, B: int = B_CASE) -> Case:
    """Derivatives of `mdl` along the rollout of u_init from x0 (x0 uniform in +-0.3, u_init uniform in +-USCALE, one seed per
    instance), and the oracle's own first backward pass (oracle.solve with max_iter = 1) as `expect`."""
    import oracle
    n, mmax, _ = oracle.model_dims(mdl)
    mm = max(mmax, 1)
    params = oracle.default_params(mdl)
    dt = float(params[0])
    dims = oracle.input_dims(mdl, params, t0, T).astype(np.int32)
    d = dict(Fx=np.zeros((B, T, n, n)), Fu=np.zeros((B, T, n, mm)), Lx=np.zeros((B, T, n)), Lu=np.zeros((B, T, mm)),
             Lxx=np.zeros((B, T, n, n)), Luu=np.zeros((B, T, mm, mm)), Lxu=np.zeros((B, T, n, mm)), Vx_T=np.zeros((B, n)),
             Vxx_T=np.zeros((B, n, n)))
    U = np.zeros((B, T, mm))
    exp = dict(k=np.zeros((B, T, mm)), K=np.zeros((B, T, mm, n)), dV=np.zeros((B, 2)), n_backward=np.zeros(B, np.int32),
               qp_retval=np.zeros((B, T), np.int32), free_mask=np.zeros((B, T), np.uint32))
    lower = None if lim is None else np.full(mm, -lim)
    upper = None if lim is None else np.full(mm, lim)
    for b in range(B):
        rng = np.random.default_rng(7919 * b + 13 * T + len(mdl))
        x = rng.uniform(-0.3, 0.3, n)
        u_init = rng.uniform(-USCALE, USCALE, (T, mm))
        x0 = x.copy()
        for i in range(T):
            ev = oracle.model_eval(mdl, params, t0 + i * dt, x, u_init[i])
            mi = ev.m
            assert mi == dims[i]
            d["Fx"][b, i], d["Lx"][b, i], d["Lxx"][b, i] = ev.Fx, ev.Lx, ev.Lxx
            d["Fu"][b, i, :, :mi], d["Lxu"][b, i, :, :mi] = ev.Fu, ev.Lxu
            d["Lu"][b, i, :mi], d["Luu"][b, i, :mi, :mi] = ev.Lu, ev.Luu
            x = ev.xn
        ev = oracle.model_eval(mdl, params, t0 + T * dt, x, np.zeros(mm))
        d["Vx_T"][b], d["Vxx_T"][b] = ev.Vx, ev.Vxx
        U[b] = u_init
        cfg = oracle.default_config(horizon_steps=T, max_iter=1, reg_type=reg, with_input_constraint=int(lim is not None))
        ref = oracle.solve(mdl, cfg, x0, u_init, t0=t0, params=params, lower=lower, upper=upper)
        exp["k"][b], exp["K"][b], exp["dV"][b] = ref.k, ref.K, ref.dV
        exp["n_backward"][b] = int(ref.trace[-1, 10])
        exp["qp_retval"][b], exp["free_mask"][b] = ref.qp_retval, ref.qp_free_mask
    return Case(model_case_id((mdl, T, t0, lim, reg)), n, mm, T, d, dims, U if lim is not None else None, lower, upper, reg, exp)


# ---- synthetic cases -------------------------------------------------------------------------------------------------------
BASE_SHAPES = ((1, 0), (1, 1), (16, 16), (3, 2))  # the smallest, the largest, and one that fills no tile
# where a run-time offset or mask can slip: n, m at 4 / 5, 8 / 9, 12 / 13 and 15 / 16 (a contraction group of four just full or just
# started), and strongly non-square blocks
BOUNDARY_SHAPES = ((4, 4), (5, 3), (8, 9), (13, 12), (16, 1), (1, 16), (15, 15), (9, 4), (12, 5), (4, 13))
SYNTHETIC_SHAPES = BASE_SHAPES + BOUNDARY_SHAPES
ONE_STEP_SHAPES = ((5, 3), (13, 12))  # run with T = 1: no next record to request
SYNTHETIC_T = 4
# (n, m, boxed, reg_type); without an input there is no QP
SYNTHETIC_CASES = tuple((n, m, boxed, reg) for n, m in SYNTHETIC_SHAPES for boxed in (False, True) for reg in (1, 2) if m > 0 or not boxed)
ONE_STEP_CASES = tuple((n, m, boxed, reg) for n, m in ONE_STEP_SHAPES for boxed in (False, True) for reg in (1, 2))
# time-varying input dimensions on a (7, 6) handle with T = 5
VARYING_SHAPE = (7, 6)
VARYING_T = 5
VARYING_DIMS = ((6, 0, 3, 6, 1), (1, 2, 3, 4, 5), (0, 6, 0, 6, 0))
VARYING_CASES = tuple((dims, boxed) for dims in VARYING_DIMS for boxed in (False, True))
# the model cases with time-varying input dimensions
VARYING_MODEL_CASES = tuple(c for c in MODEL_CASES if c[0] in ("vertical", "centroidal"))


@functools.lru_cache(maxsize=None)
def synthetic_case(n: int, m: int, boxed: bool = False, reg: int = 1, B: int = B_CASE, T: int = SYNTHETIC_T, dims=None) -> Case:
    """Seeded derivatives with Lxx = I and Luu = I: every Quu_F is positive definite at the first lambda.  dims: None (m at every
    step) or a tuple of T input dimensions.  The arrays do not depend on it: the entries beyond a step's dimension are ordinary
    numbers."""
    rng = np.random.default_rng(100 * n + m)
    u = lambda *shape: rng.uniform(-1, 1, shape)
    d = dict(Fx=np.eye(n) + 0.1 * u(B, T, n, n), Fu=0.3 * u(B, T, n, m), Lx=u(B, T, n), Lu=u(B, T, m),
             Lxx=np.broadcast_to(np.eye(n), (B, T, n, n)).copy(), Luu=np.broadcast_to(np.eye(m), (B, T, m, m)).copy(),
             Lxu=0.1 * u(B, T, n, m), Vx_T=u(B, n), Vxx_T=np.broadcast_to(np.eye(n), (B, n, n)).copy())
    U = 0.2 * u(B, T, m) if boxed else None
    lim = (np.full(m, -0.4), np.full(m, 0.4)) if boxed else (None, None)
    if dims is not None:
        assert len(dims) == T and 0 <= min(dims) and max(dims) <= m, dims
        dims = np.array(dims, dtype=np.int32)
    name = "synthetic-%dx%d%s%s-%s-reg%d" % (n, m, "" if T == SYNTHETIC_T else "-T%d" % T,
                                             "" if dims is None else "-m" + "".join("%x" % v for v in dims), "box" if boxed else "free", reg)
    return Case(name, n, m, T, d, dims, U, lim[0], lim[1], reg)


def step_dims(case: Case):
    """The input dimension of every step, the capacity written out where the case has none."""
    return [case.m] * case.T if case.dims is None else [int(v) for v in case.dims]


def poisoned(case: Case) -> Case:
    """A copy of `case` with NaN in every entry beyond a step's input dimension, which the boundary promises not to read: the
    columns >= m_i of Fu and Lxu, the rows and columns >= m_i of Luu, Lu[m_i:], and U[m_i:] of a boxed case."""
    d = {k: v.copy() for k, v in case.d.items()}
    U = None if case.U is None else case.U.copy()
    for i, mi in enumerate(step_dims(case)):
        for k in ("Fu", "Lxu", "Luu"):
            d[k][:, i, :, mi:] = np.nan
        d["Luu"][:, i, mi:, :] = np.nan
        d["Lu"][:, i, mi:] = np.nan
        if U is not None:
            U[:, i, mi:] = np.nan
    return Case(case.name + " poisoned", case.n, case.m, case.T, d, case.dims, U, None if case.lower is None else case.lower.copy(),
                None if case.upper is None else case.upper.copy(), case.reg_type, case.expect)


def same_bits(a, b, fields=REAL_FIELDS + INT_FIELDS) -> bool:
    """Every output field of two results has the same shape, type and bits (NaN equal to NaN)."""
    for f in fields:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y, equal_nan=x.dtype.kind == "f"):
            print("differs:", f)
            return False
    return True


def assert_zero_beyond_dims(r, case: Case):
    """k and K beyond a step's input dimension are exactly 0."""
    for i, mi in enumerate(step_dims(case)):
        assert not np.asarray(r.k)[:, i, mi:].any() and not np.asarray(r.K)[:, i, mi:, :].any(), (case.name, i)


def assert_box_is_active(ref, case: Case):
    """The premise of a boxed case with m >= 4: at some step the free set is mixed, and over the case the limits clamp some variable
    and leave some variable free, so that neither branch of the BoxQP goes unused."""
    dims = np.array(step_dims(case))
    fm = np.asarray(ref.free_mask).astype(np.int64)
    full = (1 << dims.astype(np.int64)) - 1  # [T]
    free = np.array([[bin(int(v)).count("1") for v in row] for row in fm])
    print("riccati %s: free variables per step %d .. %d of %d" % (case.name, free[:, dims > 0].min(), free[:, dims > 0].max(), dims.max()))
    assert (fm & ~full[None, :] == 0).all()  # no bit beyond a step's dimension
    assert ((free > 0) & (free < dims[None, :])).any(), (case.name, "no step has both clamped and free variables")


@functools.lru_cache(maxsize=None)
def retry_case(luu: float = -0.5, B: int = 1, seed: int = 0, n: int = 3, m: int = 2, T: int = 4, at: int = 1, row=None, reg: int = 1) -> Case:
    """Fx = I + 0.05 U, Fu = 0.1 U (U uniform in +-1), Lxx = I, Lxu = 0, Luu = I except at step `at`: there `luu` I (row = None), or
    I with `luu` at the diagonal entry (row, row).  The defaults: n 3, m 2, T 4, step 1, the whole diagonal."""
    rng = np.random.default_rng(4242 + seed)
    u = lambda *shape: rng.uniform(-1, 1, shape)
    Luu = np.broadcast_to(np.eye(m), (B, T, m, m)).copy()
    if row is None:
        Luu[:, at] = luu * np.eye(m)
    else:
        Luu[:, at, row, row] = luu
    d = dict(Fx=np.eye(n) + 0.05 * u(B, T, n, n), Fu=0.1 * u(B, T, n, m), Lx=u(B, T, n), Lu=u(B, T, m),
             Lxx=np.broadcast_to(np.eye(n), (B, T, n, n)).copy(), Luu=Luu, Lxu=np.zeros((B, T, n, m)), Vx_T=u(B, n),
             Vxx_T=np.broadcast_to(np.eye(n), (B, n, n)).copy())
    name = "retry%g" % luu if (n, m, T, at, row, reg) == (3, 2, 4, 1, None, 1) else "retry%g-%dx%d-T%d-at%d-row%s-reg%d" % (
        luu, n, m, T, at, row, reg)
    return Case(name, n, m, T, d, reg_type=reg)


# (n, m, T, at, row): Luu[row, row] = -0.5 at step `at`, B = 3.  With reg_type 1 each fails at lambda_5 = 0.115 and passes at
# lambda_6 = 1.934 (seven passes); the margin is wide, so rounding cannot move the decision.
RETRY_CASES = ((13, 12, 4, 3, 11), (13, 12, 4, 0, 11), (13, 12, 4, 1, 5), (5, 16, 4, 3, 15), (16, 1, 4, 0, 0))
# with reg_type 2 only these are decision-stable (eight passes, lambda_7 = 51.923 on every instance); tests/test_riccati_host_cpu.py
# guards that with a perturbation premise
RETRY_CASES_REG2 = ((13, 12, 4, 0, 11), (16, 1, 4, 0, 0))
RETRY_B = 3


def retry_id(c) -> str:
    return "%dx%d-T%d-at%d-row%d" % c


def retry_shape_case(c, reg: int = 1) -> Case:
    n, m, T, at, row = c
    return retry_case(-0.5, RETRY_B, 0, n, m, T, at, row, reg)


def concat(cases) -> Case:
    """Cases of one shape and configuration side by side in one batch."""
    c0 = cases[0]
    assert all((c.n, c.m, c.T, c.reg_type, c.constrained) == (c0.n, c0.m, c0.T, c0.reg_type, c0.constrained) for c in cases)
    return Case("+".join(c.name for c in cases), c0.n, c0.m, c0.T, {k: np.concatenate([c.d[k] for c in cases]) for k in c0.d}, c0.dims,
                None if c0.U is None else np.concatenate([c.U for c in cases]), c0.lower, c0.upper, c0.reg_type)
