"""ctypes wrapper of the GMRES CPU checker (tests/cpp/gmres_checker.cpp, g++ -O2 -ffp-contract=off, built into a directory the
caller owns, never into the tree), the systems and cases of tests/test_gpu_gmres.py, and the tolerance both GMRES test files use.

The checker sums in two orders: "sequential" (the reference's left to right) and "wave" (gmres_wave_kernel's: lane partials over
rows l, l + 64, ..., then the butterfly).  The difference between the two on a case IS the rounding freedom of a reordered sum on
that case; the GPU tests take 10 x the largest relative difference as their tolerance against the sequential checker (tolerance())."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = ("sequential", "wave")
# cond(A) of an accepted system.  After a full GMRES the true residual is about u * cond(A) * |b| (u = 1.1e-16): with |b| <= sqrt(500)
# that stays under 3e-11 for cond <= 1e4, inside the reference's bar of 1e-10 (TestGmres.cpp:98-142).  For entries uniform in [-1, 1]
# cond / n has a limiting distribution with about 90 % of its mass below 20, so at n = 500 roughly one draw in ten is redrawn.
COND_MAX = 1e4
TOL_FLOOR = 1e-13


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Result:
    """Fields of include/nmpc_hip_gmres.h with a leading batch axis, plus y ([B][K]) and fired_at ([B][K + 1])."""


class Checker:
    def __init__(self, path: str):
        self.L = C.CDLL(path)

    def solve(self, A, b, x0=None, k_max=100, eps=1e-10, make_triangular=True, apply_reorth=True, order="sequential", n_threads=16) -> Result:
        A = np.ascontiguousarray(A, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        B, n = b.shape
        assert A.shape == (B, n, n) and order in ORDERS
        K = min(k_max, n)
        r = Result()
        r.x = np.zeros((B, n)) if x0 is None else np.array(x0, dtype=np.float64).reshape(B, n).copy()
        r.iters, r.reorth, r.status = (np.zeros(B, np.int32) for _ in range(3))
        r.err, r.g = np.zeros((B, K + 1)), np.zeros((B, K + 1))
        r.H, r.basis, r.y = np.zeros((B, K + 1, K)), np.zeros((B, K + 1, n)), np.zeros((B, K))
        r.fired_at = np.zeros((B, K + 1), np.int32)
        rc = self.L.gmres_chk_solve(B, n, _p(A), _p(b), _p(r.x), int(k_max), C.c_double(eps), int(make_triangular), int(apply_reorth),
                                    ORDERS.index(order), n_threads, _p(r.iters), _p(r.reorth), _p(r.status), _p(r.err), _p(r.H), _p(r.g),
                                    _p(r.basis), _p(r.y), _p(r.fired_at))
        assert rc == 0
        return r


def build(out_dir: str) -> Checker:
    lib = os.path.join(str(out_dir), "libgmres_checker.so")
    src = os.path.join(ROOT, "tests", "cpp", "gmres_checker.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", src, "-o", lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return Checker(lib)


# Generator seeds per size.  At n = 500 the re-orthogonalisation test of the last iteration (Gmres.h:120: the new vector is rounding
# noise of about 1e-13 |A v|) sits on its threshold: with most seeds the two sum orders of the CHECKER disagree on it for two or
# three of ten systems.  Seed 5 is the first of 0 .. 8 whose ten systems decide alike in both orders (seeds 3 and 4 do too).
SEEDS = {500: 5}


@functools.lru_cache(maxsize=None)
def systems(n: int, B: int, seed: int = -1):
    """B systems of size n with entries uniform in [-1, 1] (TestGmres.cpp:100-110), each accepted only with cond(A) <= COND_MAX
    (redrawn from the same generator otherwise).  Read-only arrays: every test shares them."""
    rng = np.random.default_rng(1000 * n + (SEEDS.get(n, 0) if seed < 0 else seed))
    As, bs = [], []
    while len(As) < B:
        A = rng.uniform(-1, 1, (n, n))
        bb = rng.uniform(-1, 1, n)
        if np.linalg.cond(A) <= COND_MAX:
            As.append(A)
            bs.append(bb)
    A, b = np.array(As), np.array(bs)
    A.setflags(write=False)
    b.setflags(write=False)
    return A, b


@functools.lru_cache(maxsize=None)
def low_rank_systems(n: int, B: int = 3):
    """A = I + U V' with U, V of three columns, entries uniform in [-1, 1] / sqrt(n): the minimal polynomial of A has degree <= 4, so
    GMRES from x0 = 0 ends at k = 4."""
    rng = np.random.default_rng(77 + n)
    U, V = (rng.uniform(-1, 1, (B, n, 3)) / np.sqrt(n) for _ in range(2))
    A = np.eye(n) + U @ V.transpose(0, 2, 1)
    b = rng.uniform(-1, 1, (B, n))
    A.setflags(write=False)
    b.setflags(write=False)
    return A, b


# ---- the cases of tests/test_gpu_gmres.py ----------------------------------------------------------------------------------
# (n, B): either side of one row per lane (63, 64, 65), two rows per lane and a partial stripe (130), the last partial stripe (500),
# the degenerate sizes, and (16, 67) for more systems than one wavefront has lanes
SHAPES = ((1, 3), (2, 1), (10, 10), (63, 5), (64, 5), (65, 5), (100, 10), (130, 3), (500, 10), (16, 67))
SUBCASES = ("tri", "tri_noreorth", "tri_k20", "householder")


def subcase_config(n: int, sub: str):
    """dict(k_max, make_triangular, apply_reorth) of a sub-case, or None where it does not apply to size n."""
    if sub == "tri":
        return dict(k_max=1000, make_triangular=True, apply_reorth=True)
    if sub == "tri_noreorth":
        return dict(k_max=1000, make_triangular=True, apply_reorth=False)
    if sub == "tri_k20":
        return dict(k_max=20, make_triangular=True, apply_reorth=True) if n > 20 else None
    if sub == "householder":
        return dict(k_max=1000, make_triangular=False, apply_reorth=True) if n <= 100 else None
    raise KeyError(sub)


CASES = tuple((n, B, sub) for n, B in SHAPES for sub in SUBCASES if subcase_config(n, sub) is not None)


def residual_bar(sub: str) -> float:
    """The reference's bars on the mean of |A x - b| (TestGmres.cpp:98-142)."""
    return 1e2 if sub == "tri_k20" else 1e-10


_checker = None
_results = {}


def shared_checker(tmp_dir) -> Checker:
    global _checker
    if _checker is None:
        _checker = build(tmp_dir)
    return _checker


def case_results(checker: Checker, n: int, B: int, sub: str):
    """(sequential, wave) checker results of one case, computed once per process and shared; callers do not modify them."""
    key = (n, B, sub)
    if key not in _results:
        A, b = systems(n, B)
        _results[key] = tuple(checker.solve(A, b, order=o, **subcase_config(n, sub)) for o in ORDERS)
    return _results[key]


def rel_diff(a, ref) -> float:
    """max |a - ref| / (1 + |ref|) where NaN patterns agree; inf where they do not."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if not np.array_equal(np.isnan(a), np.isnan(ref)):
        return float("inf")
    m = ~np.isnan(ref)
    return float((np.abs(a[m] - ref[m]) / (1 + np.abs(ref[m]))).max()) if m.any() else 0.0


def leading_H(r: Result, s: int) -> np.ndarray:
    """The leading ITERS columns of H of system s."""
    return r.H[s][:, : int(r.iters[s])]


def tolerance(seq: Result, wave: Result, label="") -> dict:
    """Per quantity (X, ERR_LIST, G, H): 10 x the largest relative difference |wave - sequential| / (1 + |sequential|) over the case's
    systems, with a floor of 1e-13; a value v of the device is then accepted within tol * (1 + |sequential v|).  Printed per case."""
    spread = {"X": rel_diff(wave.x, seq.x), "ERR_LIST": rel_diff(wave.err, seq.err), "G": rel_diff(wave.g, seq.g),
              "H": max(rel_diff(leading_H(wave, s), leading_H(seq, s)) if wave.iters[s] == seq.iters[s] else float("inf")
                       for s in range(len(seq.iters)))}
    tol = {q: max(10 * v, TOL_FLOOR) for q, v in spread.items()}
    print("gmres tolerance %s: %s" % (label, ", ".join("%s %.3e" % kv for kv in tol.items())))
    return tol


def decision_stable(seq: Result, wave: Result) -> np.ndarray:
    """Systems whose REORTH count is the same in both sum orders."""
    return seq.reorth == wave.reorth
