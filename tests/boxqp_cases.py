"""The box QPs of tests/test_gpu_boxqp_batch.py and tests/test_boxqp_host_cpu.py, and what oracle.ddp_numpy.boxqp makes of them.

For size n: 70 cases drawn with rng = np.random.default_rng(100 + n) by the body of random_cases of
tests/test_gpu_boxqp_known_answers.py:233-256 at m = n without padding; case c has kind c % 5 (0 every entry clamped, 1 lower == upper
on some entries, 2 +-1e30 one-sided limits, 3 the optimum strictly inside the box, 4 generic).  After all 70 are drawn, one
initial_x = rng.normal(size=n) per case from the same generator (often outside the box).  The scaled twin of a case is
(H * 2**30, g * 2**30) with the same limits and start; the scaling is exact."""
import functools
from dataclasses import dataclass

import numpy as np

from oracle import ddp_numpy as dn

COUNT = 70
SIZES = (1, 2, 3, 8, 16, 17, 33, 63, 64)
SCALE = 2.0 ** 30

# TestBoxQP.cpp:35-98 (qpOASES example1b): H = diag(1, 0.5); (g, lower, upper, x_gt)
H_QP = np.array([[1.0, 0.0], [0.0, 0.5]])
QP_CASES = [
    ((1.5, 1.0), (-10.0, -10.0), (10.0, 10.0), (-1.5, -2.0)),
    ((1.5, 1.0), (0.5, -2.0), (5.0, 2.0), (0.5, -2.0)),
    ((1.0, 1.5), (0.0, -1.0), (5.0, -0.5), (0.0, -1.0)),
    ((1.5, 1.0), (-5.0, -1.0), (-2.0, 2.0), (-2.0, -1.0)),
    ((1.0, 1.5), (-5.0, -10.0), (-2.0, 10.0), (-2.0, -3.0)),
]


@dataclass(frozen=True)
class Cases:
    H: np.ndarray  # (70, n, n)
    g: np.ndarray  # (70, n)
    lower: np.ndarray
    upper: np.ndarray
    x0: np.ndarray
    kind: np.ndarray  # (70,)

    def scaled(self) -> "Cases":
        return Cases(self.H * SCALE, self.g * SCALE, self.lower, self.upper, self.x0, self.kind)


@functools.lru_cache(maxsize=None)
def cases(n: int) -> Cases:
    rng = np.random.default_rng(100 + n)
    m = n
    Hs, gs, los, ups, kinds = [], [], [], [], []
    for c in range(COUNT):
        A = rng.normal(size=(m, m))
        H = A @ A.T + 0.3 * np.eye(m)
        g = rng.normal(size=m) * 2
        lo, up = -rng.uniform(0.1, 1.5, m), rng.uniform(0.1, 1.5, m)
        kind = c % 5
        if kind == 0:  # every entry clamped: a steep gradient outward at the box's corner
            H = np.diag(rng.uniform(0.5, 2.0, m))
            g = np.where(rng.uniform(size=m) < 0.5, 50.0, -50.0)
        elif kind == 1:  # lower == upper on some entries
            fix = rng.uniform(size=m) < 0.5
            fix[0] = True
            v = rng.uniform(-0.5, 0.5, m)
            lo[fix], up[fix] = v[fix], v[fix]
        elif kind == 2:  # one-sided infinite-like limits
            side = rng.uniform(size=m) < 0.5
            lo[side], up[~side] = -1e30, 1e30
        elif kind == 3:  # the unconstrained optimum strictly inside the box
            xs = -np.linalg.solve(H, g)
            lo, up = xs - rng.uniform(0.5, 1.0, m), xs + rng.uniform(0.5, 1.0, m)
        Hs.append(H)
        gs.append(g)
        los.append(lo)
        ups.append(up)
        kinds.append(kind)
    x0 = np.array([rng.normal(size=n) for _ in range(COUNT)])
    out = Cases(np.array(Hs, dtype=np.float64), np.array(gs, dtype=np.float64), np.array(los), np.array(ups), x0, np.array(kinds))
    for a in (out.H, out.g, out.lower, out.upper, out.x0, out.kind):
        a.setflags(write=False)
    return out


@dataclass(frozen=True)
class OracleResults:
    x: np.ndarray  # (70, n)
    retval: np.ndarray
    iters: np.ndarray
    free_mask: np.ndarray  # uint64


def mask_of(idxs) -> int:
    return sum(1 << int(j) for j in idxs)


def solve_oracle(cs: Cases, **kw) -> OracleResults:
    with np.errstate(invalid="ignore", divide="ignore"):  # (0 / 0 in the Armijo quotient of the scaled twins: false, as in C++)
        res = [dn.boxqp(cs.H[b], cs.g[b], cs.lower[b], cs.upper[b], x0=cs.x0[b], **kw) for b in range(len(cs.g))]
    out = OracleResults(np.array([r.x for r in res]), np.array([r.retval for r in res]), np.array([r.iters for r in res]),
                        np.array([mask_of(r.free_idxs) for r in res], dtype=np.uint64))
    for a in (out.x, out.retval, out.iters, out.free_mask):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(n: int, scaled: bool = False) -> OracleResults:
    """oracle.ddp_numpy.boxqp on the 70 cases of size n (or their scaled twins), computed once per process."""
    cs = cases(n)
    return solve_oracle(cs.scaled() if scaled else cs)


def replay(H, g, lower, upper, x0, max_iter=500, grad_thre=1e-8, rel_improve_thre=1e-8, step_factor=0.6, min_step=1e-22, armijo=0.1):
    """BoxQP.h:141-347 once more in NumPy, recording per COMPLETED iteration (iter, factorization_num, clamped mask, step_num): the
    TraceData entries that BoxQP.h:320-325 fills.  Returns (rows, retval, iter)."""
    import scipy.linalg as sla
    m = g.size
    x = np.maximum(np.minimum(x0, upper), lower)
    objective = lambda v: v @ g + 0.5 * (v @ (H @ v))  # noqa: E731
    obj = old_obj = objective(x)
    clamped = np.zeros(m, bool)
    rows, chol, nfac, it = [], None, 0, 1
    while True:
        if it > 1 and (old_obj - obj) < rel_improve_thre * abs(old_obj):
            return rows, 4, it
        old_obj = obj
        grad = g + H @ x
        old_clamped = clamped
        clamped = ((x == lower) & (grad > 0)) | ((x == upper) & (grad < 0))
        free, cl = np.flatnonzero(~clamped), np.flatnonzero(clamped)
        if clamped.all():
            return rows, 6, it
        if it == 1 or (clamped != old_clamped).any():
            try:
                chol = sla.cho_factor(H[np.ix_(free, free)], lower=True)
            except sla.LinAlgError:
                return rows, -1, it
            nfac += 1
        if np.sum(grad[free] ** 2) < grad_thre ** 2:
            return rows, 5, it
        sd = np.zeros(m)
        sd[free] = -sla.cho_solve(chol, g[free] + H[np.ix_(free, cl)] @ x[cl]) - x[free]
        sdg = sd @ grad
        if sdg > 1e-10:
            return rows, -2, it
        step, step_num = 1.0, 0
        xc = np.maximum(np.minimum(x + step * sd, upper), lower)
        oc = objective(xc)
        with np.errstate(invalid="ignore", divide="ignore"):
            while (oc - old_obj) / (step * sdg) < armijo:
                step *= step_factor
                step_num += 1
                xc = np.maximum(np.minimum(x + step * sd, upper), lower)
                oc = objective(xc)
                if step < min_step:
                    break
        rows.append((it, nfac, mask_of(cl), step_num))
        x, obj = xc, oc
        if it == max_iter:
            return rows, 1, it
        it += 1
