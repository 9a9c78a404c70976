"""C/GMRES solver: what can be checked without a GPU — the C-ABI's exports, the shipped problem types' dimensions, the reference's
defaults, and the CPU checker itself against the bars of the reference's own tests (nmpc_cgmres/tests/src/TestGmres.cpp,
TestCgmresSolver.cpp)."""
import math
import os
import re

import numpy as np
import pytest

import cgmres_checker
from nmpc_amd import cgmres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return cgmres_checker.build(tmp_path_factory.mktemp("cgmres_checker"))


def test_every_declared_entry_point_is_exported():
    text = open(os.path.join(ROOT, "include", "nmpc_hip_cgmres.h")).read()
    declared = set(re.findall(r"\b(nmpc_hip_cgmres_\w+)\s*\(", text))
    assert declared == set(cgmres.EXPORTS)
    L = cgmres.load()
    for name in declared:
        getattr(L, name)


def test_model_dimensions():
    assert set(cgmres.model_names()) >= {"cgmres_semiactive_damper", "cgmres_cartpole", "cgmres_cartpole_with_input_bound"}
    dims = {m: cgmres.model_info(m)[:3] for m in ("cgmres_semiactive_damper", "cgmres_cartpole", "cgmres_cartpole_with_input_bound")}
    assert dims == {"cgmres_semiactive_damper": (2, 2, 1), "cgmres_cartpole": (4, 1, 0), "cgmres_cartpole_with_input_bound": (4, 2, 1)}
    nx, nu, nc, pb, x0, u0 = cgmres.model_info("cgmres_cartpole_with_input_bound")
    assert pb == 19 * 8 and list(x0) == [0.0, math.pi, 0.0, 0.0] and list(u0) == [0.0, 1.0, 0.01]
    nx, nu, nc, pb, x0, u0 = cgmres.model_info("cgmres_semiactive_damper")
    assert pb == 9 * 8 and list(x0) == [2.0, 0.0] and list(u0) == [0.01, 0.9, 0.03]
    with pytest.raises(ValueError):
        cgmres.model_info("no_such_problem")


def test_default_params_are_the_checkers():
    for m in cgmres_checker.MODELS:
        assert np.array_equal(cgmres.CgmresProblem(m).p, cgmres_checker.default_params(m)), m
    assert np.array_equal(cgmres.CgmresProblemCartPole(ref=[0.5, 0, 0, 0]).ref, [0.5, 0, 0, 0])


def test_default_config_is_the_references():
    c = cgmres.default_config()
    assert (c.sim_duration, c.steady_horizon_duration, c.horizon_divide_num, c.horizon_increase_ratio, c.dt, c.eq_zeta, c.k_max,
            c.finite_diff_delta, c.dump_step) == (10, 1.0, 25, 0.5, 1e-3, 1000, 5, 0.002, 5)
    assert c.ode_solver == cgmres.ODE_EULER and c.sim_ode_solver == -1 and c.ticks_per_launch == 0


def test_dense_gmres_needs_valid_arguments():
    with pytest.raises(ValueError):
        cgmres.dense_gmres(np.zeros((1, 600, 600)), np.zeros((1, 600)))


@pytest.mark.parametrize("n", [10, 50, 100, 500])
def test_checker_gmres_meets_the_reference_bars(checker, n):
    """TestGmres.cpp:102-160: ten random systems (entries uniform in [-1, 1]) per size; mean |Ax - b| < 1e-10 with full k_max, with
    and without re-orthogonalisation, and < 1e2 with k_max = 20."""
    rng = np.random.default_rng(n)
    As = rng.uniform(-1, 1, (10, n, n))
    bs = rng.uniform(-1, 1, (10, n))
    for k_max, reorth, bar in ((1000, True, 1e-10), (1000, False, 1e-10), (20, True, 1e2)):
        errs = []
        for A, b in zip(As, bs):
            x, it, _ = checker.dense_gmres(A, b, k_max=k_max, apply_reorth=reorth)
            errs.append(np.linalg.norm(A @ x - b))
            assert it <= min(k_max, n)
        assert np.mean(errs) < bar, (n, k_max, reorth, np.mean(errs))
        if k_max == 1000:
            x_ref = np.linalg.solve(As[0], bs[0])
            x, _, _ = checker.dense_gmres(As[0], bs[0], k_max=k_max, apply_reorth=reorth)
            assert np.abs(x - x_ref).max() < 1e-6 * (1 + np.abs(x_ref).max())


@pytest.mark.parametrize("model", ["cgmres_semiactive_damper", "cgmres_cartpole_with_input_bound"])
def test_checker_closed_loop_meets_the_reference_bar(checker, model):
    """TestCgmresSolver.cpp:10-30: 20 s closed loop, Euler inside the horizon, RK4 for the simulation, |x| < 0.1 at the end."""
    cfg = {n: getattr(cgmres.default_config(), n) for n, _ in cgmres.CConfig._fields_}
    cfg.update(sim_duration=20.0, dump_step=0, ode_solver=cgmres.ODE_EULER, sim_ode_solver=cgmres.ODE_RUNGE_KUTTA)
    x0, u0 = cgmres_checker.initial(model)
    r = checker.solve(model, cfg, np.array([x0]), np.array([u0]), n_threads=1)
    assert r.n_ticks == 20000
    assert r.status[0] == cgmres.Status.Succeeded
    assert np.linalg.norm(r.x[0]) < 0.1, r.x
