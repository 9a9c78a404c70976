"""FMPC with time-varying input / inequality dimensions on the MI355X (fmpc_vertical: 1, 2, 1, 0, 1 contacts), against the CPU
FMPC oracle (oracle/fmpc_oracle.hpp, which sizes every step by the model's dims(t); `checker` below is that oracle in the
library's layouts, tests/fmpc_dynamic_checker.py).  The oracle is pinned by the reference's assertions on the fixed-dimension models
(tests/test_fmpc_oracle_pins.py) and bit for bit by recorded vectors on fmpc_vertical (tests/test_fmpc_dynamic_host_cpu.py).

Bar: as tests/test_gpu_fmpc.py — equal statuses and iteration counts, floating-point results within 1e-8 relative / 1e-10
absolute (the device contracts a * b + c into FMAs, the checker is built with -ffp-contract=off), on the instances whose iteration
does not diverge.  Entries beyond a step's dimensions are compared exactly."""
import os
import subprocess

import numpy as np
import pytest

import fmpc_dynamic_checker as DC
from nmpc_amd import fmpc as F

pytestmark = pytest.mark.gpu

MODEL = "fmpc_vertical"
POISON = -1234.5  # a value no solve may read or write beyond a step's dimensions (negative: checkVariable would reject it)


@pytest.fixture(scope="module")
def checker():
    return DC


def make_case(B, T, seed, t_hi=6.0, poison=True):
    """Nominal hover starts with per-instance t0 in [0, t_hi], so that the switches fall on different steps per instance; the
    entries beyond each step's dimensions hold POISON."""
    rng = np.random.default_rng(seed)
    prob = F.FmpcProblemVerticalMotion()
    t0 = rng.uniform(0.0, t_hi, B)
    x = np.tile([1.0, 0.0], (B, T + 1, 1)) + 0.05 * rng.standard_normal((B, T + 1, 2))
    u = 9.80665 + rng.uniform(-2.0, 2.0, (B, T, 2))
    lam = 0.1 * rng.standard_normal((B, T + 1, 2))
    s = rng.uniform(0.5, 2.0, (B, T, 4))
    nu = rng.uniform(0.5, 2.0, (B, T, 4))
    x0 = np.stack([1.0 + 0.1 * rng.standard_normal(B), 0.1 * rng.standard_normal(B)], axis=1)
    if poison:
        for b in range(B):
            for i in range(T):
                m, g = prob.dimsAt(t0[b] + i * prob.dt())
                u[b, i, m:] = POISON
                s[b, i, g:] = POISON
                nu[b, i, g:] = POISON
    return prob, F.Variable(x, u, lam, s, nu), x0, t0


def active_masks(prob, t0, T):
    B = len(t0)
    mm = np.zeros((B, T, 2), bool)
    gm = np.zeros((B, T, 4), bool)
    for b in range(B):
        for i in range(T):
            m, g = prob.dimsAt(t0[b] + i * prob.dt())
            mm[b, i, :m] = True
            gm[b, i, :g] = True
    return mm, gm


def assert_close(a, b, rtol, atol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(a)
    err = np.abs(a[ok] - b[ok])
    bound = atol + rtol * np.maximum(np.abs(a[ok]), np.abs(b[ok]))
    assert np.all(err <= bound), (what, float(np.max(err - bound)))


def compare(solver, ref, rtol=1e-8, atol=1e-10, min_stable=0.9, gains=True):
    stable = ref.trace[:, :, 1].max(axis=1) < 1e4
    assert stable.mean() >= min_stable, stable.mean()
    st, it = solver.status(), solver.iters()
    assert np.array_equal(st[stable], ref.status[stable]), (st[:16], ref.status[:16])
    assert np.array_equal(it[stable], ref.iters[stable])
    tr = solver.traceDataList()
    assert np.array_equal(tr[stable, :, 0], ref.trace[stable, :, 0])
    for col, name in enumerate(F.TRACE_COLUMNS[1:], start=1):
        assert_close(tr[stable, :, col], ref.trace[stable, :, col], rtol, atol, name)
    v = solver.variable()
    for name, a, c in zip(("x", "u", "lambda", "s", "nu"), v.arrays(), (ref.x, ref.u, ref.lam, ref.s, ref.nu)):
        assert_close(a[stable], c[stable], rtol, atol, name)
    assert_close(solver.barrierEps()[stable], ref.barrier_eps[stable], rtol, atol, "barrier_eps")
    if gains:
        # gains and deltas of the last backward / forward pass, where the last iteration ran one (MaxIterationReached)
        ran = stable & (ref.status == 5)
        cl, dv = solver.coeffList(), solver.deltaVariable()
        for name, a, c in (("k", cl["k"], ref.k), ("K", np.transpose(cl["K"], (0, 1, 3, 2)), ref.K), ("s", cl["s"], ref.gs),
                           ("P", np.transpose(cl["P"], (0, 1, 3, 2)), ref.P)):
            assert_close(a[ran], c[ran], rtol, atol, name)
        for name, a, c in zip(("dx", "du", "dlambda", "ds", "dnu"), dv.arrays(), (ref.dx, ref.du, ref.dlam, ref.ds, ref.dnu)):
            assert_close(a[ran], c[ran], 1e-7, 1e-9, name)
    return stable


def run_both(checker, B, T, max_iter, seed, per_instance=None, **cfg_kw):
    prob, var, x0, t0 = make_case(B, T, seed)
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = max_iter
    for k, v in cfg_kw.items():
        setattr(s.config(), k, v)
    params = prob.p
    if per_instance is not None:
        s.setProblem(per_instance, per_instance=True)
        params = np.stack([p.p for p in per_instance])
    s.solve(t0, x0, var)
    ref = checker.solve(MODEL, s.config(), params, t0, x0, var.arrays())
    return prob, var, x0, t0, s, ref


@pytest.mark.parametrize("B,T,max_iter", [(1, 37, 10), (63, 1, 10), (63, 100, 6), (1000, 37, 4), (63, 300, 3), (1000, 100, 2)])
def test_solve_matches_checker(checker, B, T, max_iter):
    prob, var, x0, t0, s, ref = run_both(checker, B, T, max_iter, seed=B + T)
    compare(s, ref)
    names = s.kernelNames()
    assert "fmpc_riccati_kernel" in names and "fmpc_coeff_dims_kernel" in names
    assert not any(n in names for n in ("fmpc_riccati_quad_kernel", "fmpc_riccati_fused_kernel", "fmpc_tail_kernel"))


def test_entries_beyond_a_steps_dimensions(checker):
    B, T = 200, 100
    prob, var, x0, t0, s, ref = run_both(checker, B, T, 5, seed=3)
    mm, gm = active_masks(prob, t0, T)
    v = s.variable()
    # variable: bit for bit what was set before the solve
    assert np.array_equal(v.u_list[~mm], var.u_list[~mm])
    assert np.array_equal(v.s_list[~gm], var.s_list[~gm]) and np.array_equal(v.nu_list[~gm], var.nu_list[~gm])
    assert (v.u_list[~mm] == POISON).all()
    # gains and deltas: exactly 0
    cl, dv = s.coeffList(), s.deltaVariable()
    assert (cl["k"][~mm] == 0).all()
    assert (cl["K"][~mm] == 0).all()  # ([B][T][M][N]: rows a >= m(i))
    assert (dv.u_list[~mm] == 0).all() and (dv.s_list[~gm] == 0).all() and (dv.nu_list[~gm] == 0).all()
    assert np.isfinite(dv.u_list[mm]).all()


def test_step_dims_agree_with_the_host_schedule():
    prob = F.FmpcProblemVerticalMotion()
    T = 60
    # t0 on and within 1e-8 of the switch times, plus random ones
    t0 = np.concatenate([[2.0 - 0.3, 2.0 - 1e-8 - 0.2, 3.0 - 0.25 + 1e-8, 4.5 - 0.1, 5.0 - 0.35 - 1e-9, 0.0],
                         np.random.default_rng(5).uniform(0, 6, 58)])
    B = len(t0)
    solver = F.FmpcSolverBatch(prob, B, T)
    v = F.Variable.make(prob, T, B)
    v.reset(1.0, 9.8, 0.0, 1.0, 1.0)
    with pytest.raises(RuntimeError):
        solver.inputDimList()  # before the first solve
    solver.config().max_iter = 1
    solver.solve(t0, np.tile([1.0, 0.0], (B, 1)), v)
    md, gd = solver.inputDimList(), solver.ineqDimList()
    for b in range(B):
        for i in range(T):
            assert (md[b, i], gd[b, i]) == F.model_dims_at(MODEL, t0[b] + i * prob.dt()), (b, i)
    assert set(np.unique(md)) == {0, 1, 2}


@pytest.mark.parametrize("opts", [dict(enable_line_search=True), dict(init_complementary_variable=True),
                                  dict(update_barrier_eps=False),
                                  dict(enable_line_search=True, merit_const_scale_from_lagrange_multipliers=True)])
def test_configuration_switches_match_checker(checker, opts):
    prob, var, x0, t0, s, ref = run_both(checker, 96, 80, 5, seed=11, **opts)
    compare(s, ref)
    if opts.get("enable_line_search"):
        stable = ref.trace[:, :, 1].max(axis=1) < 1e4
        ran = stable & (ref.status == 5)
        # merit_func_ and merit_const_scale_; merit_deriv_ sums the l1 rule's sign(g + s) d per row (MathUtils.h:17-38), and once
        # a row is satisfied g + s is a rounding-level residual whose sign FMA contraction flips: that column is only required finite
        m = s.meritFunc()
        assert_close(m[ran][:, [0, 2]], ref.merit[ran][:, [0, 2]], 1e-8, 1e-10, "merit")
        assert np.isfinite(m[ran][:, 1]).all()


def test_invalid_variable_only_in_active_rows(checker):
    B, T = 64, 50
    prob, var, x0, t0 = make_case(B, T, seed=21)
    mm, gm = active_masks(prob, t0, T)
    bad_active = [b for b in range(B) if gm[b, 7].sum() > 0][:5]
    for b in bad_active:
        var.s_list[b, 7, 0] = -0.5  # an active row
    # an inactive row holding the same value is ignored (the poison is negative as well)
    assert (var.s_list[~gm] < 0).all()
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = 4
    with pytest.raises(RuntimeError):
        s.solve(t0, x0, var)
    st = s.status()
    ref = checker.solve(MODEL, s.config(), prob.p, t0, x0, var.arrays())
    assert (st[bad_active] == -2).all()  # NMPC_HIP_FMPC_STATUS_INVALID_VARIABLE
    assert (st != -2).sum() == B - len(bad_active)
    assert np.array_equal(st, ref.status)
    compare(s, ref)


def test_horizon_without_inequality_rows(checker):
    """T = 20 steps inside the flight phase (4.5, 5): no input, no inequality row anywhere; the barrier parameter is 0 / 0."""
    B, T = 8, 20
    prob = F.FmpcProblemVerticalMotion()
    t0 = np.linspace(4.55, 4.7, B)
    x = np.tile([1.0, 0.0], (B, T + 1, 1))
    var = F.Variable(x, np.full((B, T, 2), POISON), np.zeros((B, T + 1, 2)), np.full((B, T, 4), POISON), np.full((B, T, 4), POISON))
    x0 = np.tile([1.0, -0.5], (B, 1))
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = 3
    s.solve(t0, x0, var)
    assert (s.inputDimList() == 0).all() and (s.ineqDimList() == 0).all()
    ref = checker.solve(MODEL, s.config(), prob.p, t0, x0, var.arrays())
    assert np.array_equal(s.status(), ref.status) and np.array_equal(s.iters(), ref.iters)
    assert_close(s.barrierEps(), ref.barrier_eps, 1e-8, 1e-10, "barrier_eps")
    assert_close(s.traceDataList(), ref.trace, 1e-8, 1e-10, "trace")
    v = s.variable()
    assert_close(v.x_list, ref.x, 1e-8, 1e-10, "x")
    assert (v.u_list == POISON).all() and (v.s_list == POISON).all()


def test_per_instance_problem_objects(checker):
    B, T = 48, 60
    rng = np.random.default_rng(31)
    probs = []
    for b in range(B):
        a = rng.uniform(0.2, 0.8)
        probs.append(F.FmpcProblemVerticalMotion(double_support_begin=a, double_support_end=a + rng.uniform(0.05, 0.3),
                                                 flight_begin=a + 0.35, flight_end=a + 0.35 + rng.uniform(0.02, 0.2),
                                                 f_max=rng.uniform(15.0, 30.0)))
    prob, var, x0, _ = make_case(B, T, seed=32, poison=False)
    t0 = np.zeros(B)
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = 5
    s.setProblem(probs, per_instance=True)
    s.solve(t0, x0, var)
    ref = checker.solve(MODEL, s.config(), np.stack([p.p for p in probs]), t0, x0, var.arrays())
    compare(s, ref)
    md = s.inputDimList()
    for b in range(B):
        assert [probs[b].dimsAt(t0[b] + i * prob.dt())[0] for i in range(T)] == md[b].tolist()


def test_graph_replay_equals_stream_launches_and_is_deterministic():
    B, T = 300, 80
    prob, var, x0, t0 = make_case(B, T, seed=41)
    outs = []
    for use_graph in (True, True, False):
        s = F.FmpcSolverBatch(prob, B, T)
        s.config().max_iter = 5
        s.config().use_graph = use_graph
        s.solve(t0, x0, var)
        s.solve(t0, x0, var)  # (the graph is captured at the first solve, replayed at the second)
        v = s.variable()
        outs.append([s.status(), s.traceDataList()] + list(v.arrays()) + [s.coeffList()["K"]])
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b, equal_nan=True)
    for a, b in zip(outs[0], outs[2]):
        assert np.array_equal(a, b, equal_nan=True)


def test_closed_loop_tracks_within_force_bounds(checker):
    """6 s of the contact schedule (100 Hz ticks, T = 100): active forces inside [f_min, f_max] up to 1e-9, the height tracks the
    reference; instance 0 follows the checker's closed loop for 100 ticks."""
    B, T = 16, 100
    prob = F.FmpcProblemVerticalMotion()
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = 10
    s.config().kkt_error_thre = 1e-6
    v = F.Variable.make(prob, T, B)
    v.reset(1.0, 9.80665, 0.0, 1.0, 1.0)
    s.setVariable(v)
    t0 = np.zeros(B)
    x0 = np.tile([1.0, 0.0], (B, 1)) + np.linspace(0, 0.05, B)[:, None] * np.array([1.0, 0.0])
    n_ticks = 600
    out = s.mpcRun(t0, x0, n_ticks, prob.dt())
    assert np.isin(out["status"], (1, 5)).all()
    for k in range(n_ticks):
        m = prob.dimsAt(k * prob.dt())[0]
        f = out["u0"][:, k, :m]
        assert (f >= prob.p[7] - 1e-9).all() and (f <= prob.p[8] + 1e-9).all(), k
        assert (out["u0"][:, k, m:] == 0).all()
    z = out["x"][:, :, 0]
    assert np.abs(z[:, 100:440] - 1.0).max() < 0.2  # through the contact switches before the flight phase (checker: 0.11)
    assert np.abs(z[:, -50:] - 1.0).max() < 0.15  # recovered after the flight phase (checker: 0.07)
    vv = F.Variable.make(prob, T, 1)
    vv.reset(1.0, 9.80665, 0.0, 1.0, 1.0)
    ref = checker.closed_loop(MODEL, s.config(), prob.p, t0[:1], x0[:1], vv.arrays(), 100, prob.dt())
    assert_close(out["x"][0, :100], ref.x_log[0], 1e-7, 1e-9, "closed-loop state")
    assert np.array_equal(out["status"][0, :100], ref.status_log[0])


def test_cpp_mirror_solves_and_rejects_wrong_sizes(tmp_path):
    from nmpc_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(_capi.lib_path())
    F.load()
    exe = str(tmp_path / "fmpc_vertical_mirror")
    cmd = ["g++", "-std=c++17", "-O2", f"-I{root}/include", os.path.join(root, "tests", "cpp", "fmpc_vertical_mirror.cpp"),
           f"-L{libdir}", "-lnmpc_hip_ddp", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    T = 50
    r = subprocess.run([exe, str(T)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("runtime_error: [FMPC] u_list[i] dimension should be "), lines[-1]
    # the same solve through the Python mirror
    prob = F.FmpcProblemVerticalMotion()
    t0 = np.array([0.0, 1.95, 2.5, 4.45])
    B = len(t0)
    v = F.Variable.make(prob, T, B)
    v.reset(1.0, 9.80665, 0.0, 1.0, 1.0)
    mm, gm = active_masks(prob, t0, T)
    v.u_list[~mm] = 0.0  # (the C++ mirror packs 0 beyond a step's dimension)
    v.s_list[~gm] = 0.0
    v.nu_list[~gm] = 0.0
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = 8
    st = s.solve(t0, np.tile([1.0, 0.0], (B, 1)), v)
    out = s.variable()
    for line in lines:
        p = line.split()
        if p[0] == "status":
            assert int(p[2]) == st[int(p[1])]
        elif p[0] == "u":
            b, i, m = int(p[1]), int(p[2]), int(p[3])
            assert m == int(mm[b, i].sum())
            assert np.array_equal(np.array([float(q) for q in p[4:]]), out.u_list[b, i, :m])
        elif p[0] == "x":
            b, i = int(p[1]), int(p[2])
            assert np.array_equal(np.array([float(p[3]), float(p[4])]), out.x_list[b, i])
