"""The reference's BoxQP known answers (TestBoxQP.cpp:35-98) and KKT-checked random box QPs, through every device BoxQP.

The problems are the test-only BoxQP probes (tests/cpp/boxqp_probe.hpp, compiled into libnmpc_test_models.so by
nmpc_amd.build.build_test_models): the input never moves the state and the running cost is 1/2 u'Hu + g'u + u'Cx, so with x0 = 0,
u_init = 0 and reg_type = 2 the backward pass hands the BoxQP of every timestep exactly Quu_F = H, Qu = g and Qux = C
(tests/test_model_functors_cpu.py checks that the probe means this).  The last timestep solves from a zero start, the earlier ones
warm-start from k of the next timestep (DDPSolver.hpp:452-467); both must give the answer.  Families reached, each pinned and checked
by kernelName():

  probe                        families              device BoxQP
  <double, 4, 2>               1w                    boxQP (lane kernel, static m)
  <double, 4, 1>               quad, 1w, 2w          the quad kernel's constrained variant, boxQP
  <double, 9, 2>               1w, wpi, tile64       boxQPMasked (wave-per-instance), qpBatch (tile kernel)
  <double, 9, Dynamic, 16>     1w                    boxQP at run-time m <= 16 (the centroidal box path)
  <float, 4, 2>                tile32                the fp32 tile kernel's float boxQP

The two-wave kernel exists only where ModelOpsFor::kTwoWaveFits holds: of the probes, for <double, 4, 1> alone (the fixture checks
this against the probe library).

Families with per-instance problem objects carry all cases of a sweep in one batch (set_model_params_batch +
set_input_limits_batch); the lane kernel, which has none, runs one solve per case.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import ddp_numpy as dn

pytestmark = pytest.mark.gpu

T = 4  # >= 3: the last timestep starts from zero, the others warm-start
KSTEPS = 16  # BoxQPProbe::kSteps
# name -> (index in the probe library, ctypes scalar, n, MM, dynamic, families).  "2w" is listed where ModelOpsFor::kTwoWaveFits
# holds; the fixture checks that against the probe library rather than assuming it.
PROBES = {
    "boxqp_probe_d4m2": (0, C.c_double, 4, 2, False, ("1w",)),
    "boxqp_probe_d4m1": (1, C.c_double, 4, 1, False, ("quad", "1w", "2w")),
    "boxqp_probe_d9m2": (2, C.c_double, 9, 2, False, ("1w", "wpi", "tile64")),
    "boxqp_probe_d9dyn16": (3, C.c_double, 9, 16, True, ("1w",)),
    "boxqp_probe_f4m2": (4, C.c_float, 4, 2, False, ("tile32",)),
}
KERNEL = {"1w": "ddp_solve_tpi_kernel", "2w": "ddp_solve_tpi2w_kernel", "quad": "ddp_solve_quad_kernel",
          "wpi": "ddp_solve_wpi_kernel", "tile64": "ddp_solve_tile64_kernel", "tile32": "ddp_solve_tile32_kernel"}
OWN_PROBLEMS = {"2w", "quad", "wpi", "tile64", "tile32"}  # families with a per-instance-problem instantiation

# TestBoxQP.cpp:35-98 (qpOASES example1b): H = diag(1, 0.5); (g, lower, upper, x_gt)
H_QP = np.array([[1.0, 0.0], [0.0, 0.5]])
QP_CASES = [
    ((1.5, 1.0), (-10.0, -10.0), (10.0, 10.0), (-1.5, -2.0)),
    ((1.5, 1.0), (0.5, -2.0), (5.0, 2.0), (0.5, -2.0)),
    ((1.0, 1.5), (0.0, -1.0), (5.0, -0.5), (0.0, -1.0)),
    ((1.5, 1.0), (-5.0, -1.0), (-2.0, 2.0), (-2.0, -1.0)),
    ((1.0, 1.5), (-5.0, -10.0), (-2.0, 10.0), (-2.0, -3.0)),
]

_state = {}


@pytest.fixture(scope="module")
def probes():
    """Loads the probe library and registers its tables with the DDP library _capi.load() opened (under scripts/fuzz_suite.sh the
    fuzz build).  Registering a name twice is answered NMPC_HIP_OK by the library (the first table stays), and the probe library,
    once loaded, is never unloaded: the module-level cache keeps one registration per process."""
    if not _state:
        from nmpc_amd import _capi
        from nmpc_amd import build as hip_build
        from nmpc_amd.models import _Problem
        L = _capi.load()
        T_lib = C.CDLL(hip_build.build_test_models())
        T_lib.nmpc_test_model_ops.argtypes = [C.c_int]
        T_lib.nmpc_test_model_ops.restype = C.c_void_p
        T_lib.nmpc_test_model_two_wave_fits.argtypes = [C.c_int]
        L.nmpc_hip_ddp_register_model.argtypes = [C.c_void_p]
        L.nmpc_hip_ddp_register_model.restype = C.c_int
        assert T_lib.nmpc_test_model_count() == len(PROBES)
        classes = {}
        for name, (i, real, n, mm, dyn, fams) in PROBES.items():
            ops = T_lib.nmpc_test_model_ops(i)
            assert ops
            assert L.nmpc_hip_ddp_register_model(ops) == _capi.OK, _capi.last_error()

            class Blob(C.Structure):
                _fields_ = [("dt", real), ("H", real * (mm * mm)), ("g", real * mm), ("C", real * (mm * n)), ("m_steps", C.c_int * KSTEPS)]

            classes[name] = type("Probe_" + name, (_Problem,), {"name": name, "_Blob": Blob})
            got = classes[name].dims()
            assert got == (n, mm, dyn, C.sizeof(Blob)), (name, got)
            assert T_lib.nmpc_test_model_two_wave_fits(i) == int("2w" in fams), f"{name}: kTwoWaveFits is not what PROBES lists"
        _state.update(lib=T_lib, classes=classes)
    return _state


def family_params():
    return [(name, f) for name, (_, _, _, _, _, fams) in PROBES.items() for f in fams]


def make_problem(st, name, H, g, Cm, m_steps=None):
    _, real, n, mm, _, _ = PROBES[name]
    p = st["classes"][name]()
    Hb, gb, Cb = np.zeros((mm, mm)), np.zeros(mm), np.zeros((mm, n))
    Hb[: H.shape[0], : H.shape[1]] = H
    gb[: len(g)] = g
    Cb[: Cm.shape[0]] = Cm
    for i, v in enumerate(Hb.T.ravel()):
        p.blob.H[i] = v
    for i, v in enumerate(gb):
        p.blob.g[i] = v
    for i, v in enumerate(Cb.T.ravel()):
        p.blob.C[i] = v
    steps = [mm] * KSTEPS if m_steps is None else list(m_steps) + [m_steps[-1]] * (KSTEPS - len(m_steps))
    for i, v in enumerate(steps):
        p.blob.m_steps[i] = v
    return p


def solve_cases(st, name, family, cases, m_steps=None):
    """cases: list of (H, g, C, lower, upper) with lower / upper of length MM.  Returns per case (kff (T, MM), Kfb (T, MM, n),
    qp retval (T,), free mask (T,), U (T, MM), input dims (T,))."""
    import nmpc_amd
    _, real, n, mm, _, _ = PROBES[name]
    probs = [make_problem(st, name, H, g, Cm, m_steps) for H, g, Cm, _, _ in cases]
    lo = np.array([c[3] for c in cases], dtype=np.float64).reshape(len(cases), mm)
    up = np.array([c[4] for c in cases], dtype=np.float64).reshape(len(cases), mm)

    def run(problem, B):
        s = nmpc_amd.DDPSolverBatch(problem, B)
        c = s.config()
        c.print_level = 0
        c.horizon_steps = T
        c.max_iter = 1
        c.reg_type = 2
        c.with_input_constraint = True
        s.setKernel(family)
        return s

    out = []
    if family in OWN_PROBLEMS:
        B = len(cases)
        s = run(probs[0], B)
        s.setProblemBatch(probs)
        s.setInputLimitsBatch(lo, up)
        assert s.kernelName() == KERNEL[family]
        s.solve(0.0, np.zeros((B, n)), np.zeros((B, T, mm)))
        res = (s.kff(), s.Kfb(), s.qpRetval(), s.qpFreeMask(), s.U(), s.inputDimList())
        for b in range(B):
            out.append(tuple(r[b] for r in res))
    else:
        for b, p in enumerate(probs):
            s = run(p, 1)
            s.setInputLimits(lo[b], up[b])
            assert s.kernelName() == KERNEL[family]
            s.solve(0.0, np.zeros((1, n)), np.zeros((1, T, mm)))
            out.append(tuple(r[0] for r in (s.kff(), s.Kfb(), s.qpRetval(), s.qpFreeMask(), s.U(), s.inputDimList())))
    return out


def numpy_chain(H, g, lo, up, dims):
    """The reference's sequence of QPs of one backward pass (k of timestep i+1 as the start of timestep i when the sizes agree),
    restated in NumPy (oracle/ddp_numpy.py): per timestep (x, retval, free mask) or None where m = 0."""
    res = [None] * T
    nxt, m_next = None, -1
    for i in range(T - 1, -1, -1):
        m = int(dims[i])
        if m > 0:
            x0 = nxt if (i != T - 1 and m_next == m) else np.zeros(m)
            r = dn.boxqp(H[:m, :m], g[:m], lo[:m], up[:m], x0=x0)
            mask = sum(1 << j for j in r.free_idxs)
            res[i] = (r.x, r.retval, mask)
            nxt = r.x
        else:
            nxt = np.zeros(0)
        m_next = m
    return res


def check_gains(k, K, mask, H, Cm, m, tol):
    """Clamped rows of K exactly 0, free rows -H_ff^-1 C_f; entries beyond m of k and K exactly 0."""
    free = [j for j in range(m) if mask >> j & 1]
    clamped = [j for j in range(m) if not mask >> j & 1]
    assert not K[clamped].any(), "clamped rows of K must be exactly zero"
    assert not k[m:].any() and not K[m:].any(), "entries beyond inputDim(t) must be zero"
    if free:
        Kf = -np.linalg.solve(H[np.ix_(free, free)], Cm[free])
        err = np.abs(K[free] - Kf) / (1.0 + np.abs(Kf))
        assert err.max() <= tol, f"free rows of K: {err.max():.3e}"


def fp32_bar(H, x_gt):
    """fp32: the float BoxQP's answer carries the rounding of its Cholesky factor and triangular solves, a few float ulps times the
    condition number of H_ff; the bar is 32 eps_f kappa(H) (1 + max |x_gt|), 2.8e-5 for the known answers (kappa 2)."""
    return 32 * np.finfo(np.float32).eps * np.linalg.cond(H) * (1.0 + np.abs(x_gt).max())


@pytest.mark.parametrize("name,family", family_params())
def test_reference_boxqp_known_answers(probes, name, family):
    """TestBoxQP.cpp:35-98 on the family: every timestep ||k - x_gt|| < 1e-6 (TestBoxQP.cpp:29; fp32: fp32_bar), qpRetval > 0 and the
    reference's retval sequence, qpFreeMask the active set x_gt implies, K's clamped rows 0 and free rows -H_ff^-1 C_f."""
    _, real, n, mm, dyn, _ = PROBES[name]
    f32 = real is C.c_float
    rng = np.random.default_rng(3)
    cases = []
    for g, lo, up, x_gt in QP_CASES:
        m = min(mm, 2)
        H = np.eye(mm)
        H[:m, :m] = H_QP[:m, :m]
        Cm = np.round(rng.normal(size=(mm, n)) * 8) / 8  # (dyadic: exact in float)
        gg, ll, uu = np.zeros(mm), np.full(mm, -1.0), np.full(mm, 1.0)
        gg[:m], ll[:m], uu[:m] = g[:m], lo[:m], up[:m]
        cases.append((H, gg, Cm, ll, uu, np.array(x_gt[:m])))
    m_steps = [2] * KSTEPS if dyn else None
    got = solve_cases(probes, name, family, [c[:5] for c in cases], m_steps)
    for (H, g, Cm, lo, up, x_gt), (k, K, ret, mask, U, dims) in zip(cases, got):
        # (the one-input probe takes the first coordinate of each case: H is diagonal, so that is a QP of its own with answer x_gt[0])
        m = x_gt.size
        x = np.concatenate([x_gt, np.zeros(mm - m)])
        Hm = H[:m, :m]
        xa = ((lo[:m] == x[:m]) & (g[:m] + Hm @ x[:m] > 0)) | ((up[:m] == x[:m]) & (g[:m] + Hm @ x[:m] < 0))
        want_mask = sum(1 << j for j in range(m) if not xa[j])
        chain = numpy_chain(H, g, lo, up, np.full(T, mm if not dyn else 2))
        bar = fp32_bar(Hm, x[:m]) if f32 else 1e-6
        for i in range(T):
            mi = int(dims[i])
            assert mi == (2 if dyn else mm)
            assert np.linalg.norm(k[i, :mi] - x[:mi]) < bar, (i, k[i], x)
            assert ret[i] > 0
            assert int(mask[i]) == want_mask, (i, int(mask[i]), want_mask)
            if not f32:
                assert ret[i] == chain[i][1] and int(mask[i]) == chain[i][2]
            check_gains(k[i], K[i], int(mask[i]), H[:mi, :mi], Cm[:mi], mi, 1e-4 if f32 else 1e-10)


def random_cases(rng, n, mm, m, count):
    """SPD H, g, C and limits of size m (padded to MM), with the edges: every entry clamped, lower == upper on some entries, one-sided
    infinite-like limits (+-1e30), the unconstrained optimum strictly inside the box, and generic boxes."""
    cases = []
    for c in range(count):
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
        Hp = np.eye(mm)
        Hp[:m, :m] = H
        pad = lambda v, fill: np.concatenate([v, np.full(mm - m, fill)])  # noqa: E731
        cases.append((Hp, pad(g, 0.0), rng.normal(size=(mm, n)), pad(lo, -1.0), pad(up, 1.0), kind))
    return cases


def check_kkt(k, H, g, lo, up, mask, m, f32):
    """k inside the box; the gradient of 1/2 k'Hk + g'k vanishes on the free entries (<= 1e-9 scale; fp32 1e-4 scale) and points
    out of the box on the clamped ones."""
    k = k[:m]
    assert np.all(k >= lo[:m]) and np.all(k <= up[:m]), (k, lo[:m], up[:m])
    grad = H[:m, :m] @ k + g[:m]
    scale = 1.0 + np.abs(g[:m]).max() + np.abs(H[:m, :m]).max() * np.abs(k).max()
    tol = (1e-4 if f32 else 1e-9) * scale
    for j in range(m):
        if mask >> j & 1:
            assert abs(grad[j]) <= tol, (j, grad[j], tol)
        elif k[j] == lo[j] and k[j] != up[j]:
            assert grad[j] >= -tol, (j, grad[j])
        elif k[j] == up[j] and k[j] != lo[j]:
            assert grad[j] <= tol, (j, grad[j])
        else:
            assert lo[j] == up[j], (j, k[j], lo[j], up[j])


@pytest.mark.parametrize("name,family", family_params())
def test_random_box_qps_by_kkt(probes, name, family):
    """Random SPD box QPs (m = MM on the static probes; m in 1 .. 16 on the dynamic one), including every edge of random_cases: the
    answer satisfies the KKT conditions, and retval and the free set equal oracle.ddp_numpy.boxqp's along the same warm-start chain
    (fp32: the free set; its retval may differ where float rounding ends the iteration by another test)."""
    _, real, n, mm, dyn, _ = PROBES[name]
    f32 = real is C.c_float
    rng = np.random.default_rng(11 + PROBES[name][0])
    if dyn:
        sweeps = [(m, random_cases(rng, n, mm, m, 1 if m not in (1, 2, 16) else 5)) for m in range(1, 17)]
    else:
        sweeps = [(mm, random_cases(rng, n, mm, mm, 10))]
    n_kinds = set()
    for m, cases in sweeps:
        if f32:
            cases = [tuple(np.asarray(v, np.float32).astype(np.float64) if isinstance(v, np.ndarray) else v for v in c) for c in cases]
        got = solve_cases(probes, name, family, [c[:5] for c in cases], [m] * KSTEPS if dyn else None)
        for (H, g, Cm, lo, up, kind), (k, K, ret, mask, U, dims) in zip(cases, got):
            chain = numpy_chain(H, g, lo, up, np.full(T, m))
            for i in range(T):
                assert int(dims[i]) == m
                check_kkt(k[i], H, g, lo, up, int(mask[i]), m, f32)
                assert int(mask[i]) == chain[i][2], (kind, i, int(mask[i]), chain[i][2])
                if not f32:
                    assert ret[i] == chain[i][1], (kind, i, ret[i], chain[i][1])
                if kind == 0:
                    assert int(mask[i]) == 0 and not K[i].any()
                check_gains(k[i], K[i], int(mask[i]), H[:m, :m], Cm[:m], m, 1e-3 if f32 else 1e-9)
            n_kinds.add(kind)
    assert n_kinds == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("steps", [[16, 0, 16, 16], [4, 2, 2, 4], [0, 16, 4, 0]])
def test_dynamic_probe_with_switching_input_dimension(probes, steps):
    """The run-time m boxQP of the lane kernel with inputDim(t) switching along the horizon: per timestep the answer of that
    timestep's m (the reference warm-starts only when the next timestep has the same size), retval and free set as the NumPy chain,
    and every entry beyond m of k, K and U exactly 0."""
    name = "boxqp_probe_d9dyn16"
    rng = np.random.default_rng(sum(steps))
    cases = random_cases(rng, 9, 16, 16, 5)
    got = solve_cases(probes, name, "1w", [c[:5] for c in cases], steps)
    for (H, g, Cm, lo, up, kind), (k, K, ret, mask, U, dims) in zip(cases, got):
        np.testing.assert_array_equal(dims, steps)
        chain = numpy_chain(H, g, lo, up, dims)
        for i in range(T):
            m = int(dims[i])
            assert not U[i, m:].any() and not k[i, m:].any() and not K[i, m:].any()
            if m == 0:
                continue
            check_kkt(k[i], H, g, lo, up, int(mask[i]), m, False)
            assert np.abs(k[i, :m] - chain[i][0]).max() <= 1e-9 * (1 + np.abs(chain[i][0]).max())
            assert ret[i] == chain[i][1] and int(mask[i]) == chain[i][2], (kind, i)
            check_gains(k[i], K[i], int(mask[i]), H[:m, :m], Cm[:m], m, 1e-9)
