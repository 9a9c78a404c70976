"""FMPC problems with time-varying input / inequality dimensions, what can be checked without a GPU: the registration of
fmpc_vertical and its dimensions, its parameter image, the host-side inputDim(t) / ineqDim(t), and the CPU FMPC oracle on
fmpc_vertical (`checker` is oracle/fmpc.py in the library's layouts, tests/fmpc_dynamic_checker.py) — reproducing bit for bit the
vectors recorded in tests/golden/fmpc_vertical_golden.npz, and converging with its forces inside their bounds."""
import importlib.util
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import fmpc_dynamic_checker as DC
from nmpc_amd import fmpc as F
from oracle import fmpc as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXED = ("fmpc_oscillator", "fmpc_cartpole", "fmpc_pointmass")
SWITCHES = (2.0, 3.0, 4.5, 5.0)


@pytest.fixture(scope="module")
def checker():
    return DC


def test_vertical_is_registered_with_capacities_and_dynamic_flags():
    assert "fmpc_vertical" in F.model_names()
    assert F.model_info("fmpc_vertical") == (2, 2, 4, 14 * 8)
    assert F.model_dynamic("fmpc_vertical") == (1, 1)
    for model in FIXED:
        assert F.model_dynamic(model) == (0, 0)
    assert F.FmpcProblemVerticalMotion().dynamic and not F.FmpcProblemCartPole().dynamic


def test_new_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "nmpc_hip_fmpc.h")).read()
    declared = set(re.findall(r"\b(nmpc_hip_fmpc_\w+)\s*\(", text))
    for name in ("nmpc_hip_fmpc_model_dynamic", "nmpc_hip_fmpc_model_dims_at", "nmpc_hip_fmpc_get_step_dims"):
        assert name in declared and name in F.EXPORTS
        getattr(F.load(), name)


def test_python_image_equals_the_default_object_and_the_checker_image(checker):
    prob = F.FmpcProblemVerticalMotion()
    assert prob.p.tolist() == [0.01, 1.0, 1e-3, 1e-3, 1.0, 1e-3, 1.0, 0.0, 30.0, 8.0, 2.0, 3.0, 4.5, 5.0]
    assert np.array_equal(prob.p, checker.default_params("fmpc_vertical"))
    assert checker.model_info("fmpc_vertical") == (2, 2, 4, 14)
    for model in FIXED:
        assert np.array_equal(F.FmpcProblem(model).p, checker.default_params(model)), model


def test_dims_follow_the_schedule_on_both_sides_of_every_switch(checker):
    prob = F.FmpcProblemVerticalMotion()
    want = {0.0: 1, 1.999: 1, 2.001: 2, 2.999: 2, 3.001: 1, 4.499: 1, 4.501: 0, 4.999: 0, 5.001: 1, 7.0: 1}
    for t, m in want.items():
        assert F.model_dims_at("fmpc_vertical", t) == (m, 2 * m), t
        assert prob.dimsAt(t) == (m, 2 * m)
        assert checker.dims_at("fmpc_vertical", t) == (m, 2 * m)
    # the 1e-6 offset: a time a hair before a switch (t0 + i dt rounding) already counts as after it
    for ts in SWITCHES:
        for eps in (1e-8, 1e-12):
            assert F.model_dims_at("fmpc_vertical", ts - eps) == F.model_dims_at("fmpc_vertical", ts + 1e-3)
    # a per-instance object with its own schedule
    other = F.FmpcProblemVerticalMotion(double_support_begin=0.5, double_support_end=0.7)
    assert other.dimsAt(0.6) == (2, 4) and F.FmpcProblemVerticalMotion().dimsAt(0.6) == (1, 2)
    assert checker.dims_at("fmpc_vertical", 0.6, other.p) == (2, 4)
    for model in FIXED:
        n, m, g, _ = F.model_info(model)
        assert F.model_dims_at(model, 2.5) == (m, g)


def _cfg(**kw):
    c = SimpleNamespace(horizon_steps=0, max_iter=10, kkt_error_thre=1e-4, check_nan=1, init_complementary_variable=0,
                        update_barrier_eps=1, break_if_llt_fails=0, enable_line_search=0, merit_const_scale_from_lagrange_multipliers=0)
    c.__dict__.update(kw)
    return c


def _rel_close(a, b, rtol=1e-10, atol=1e-13):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    return bool(np.all(np.abs(a[ok] - b[ok]) <= atol + rtol * np.maximum(np.abs(a[ok]), np.abs(b[ok]))))


@pytest.mark.parametrize("model", FIXED)
@pytest.mark.parametrize("opts", [{}, {"enable_line_search": 1}, {"init_complementary_variable": 1}, {"update_barrier_eps": 0},
                                  {"enable_line_search": 1, "merit_const_scale_from_lagrange_multipliers": 1}])
def test_checker_equals_the_oracle_on_fixed_dimensions(checker, model, opts):
    """The threaded batch entry point with every output, in the library's layouts (`checker`), against the single solve O.solve:
    both are the one oracle now, so this pins the batch path's strides, the packing of its outputs and the adapter's layouts."""
    n, m, g, _ = O.model_info(model)
    B, T = 12, 25
    rng = np.random.default_rng(7 + len(opts))
    var = (0.3 * rng.standard_normal((B, T + 1, n)), 0.3 * rng.standard_normal((B, T, m)), 0.3 * rng.standard_normal((B, T + 1, n)),
           rng.uniform(0.5, 2.0, (B, T, g)), rng.uniform(0.5, 2.0, (B, T, g)))
    x0 = 0.3 * rng.standard_normal((B, n))
    t0 = rng.uniform(0, 1, B)
    cfg = _cfg(horizon_steps=T, max_iter=6, **opts)
    params = O.default_params(model)
    r = checker.solve(model, cfg, params, t0, x0, var)
    ocfg = O.default_config(**{k: getattr(cfg, k) for k in DC.CFG_FIELDS + ("kkt_error_thre",)})
    compared = 0
    for b in range(B):
        o = O.solve(model, ocfg, params, t0[b], x0[b], O.Variable(*(a[b] for a in var)))
        if o.trace[:, 1].max() >= 1e4:  # diverging starts amplify rounding without bound (tests/test_gpu_fmpc.py)
            continue
        assert r.status[b] == o.status and r.iters[b] == o.iters, (b, r.status[b], o.status)
        for name, a, c in (("x", r.x[b], o.variable.x), ("u", r.u[b], o.variable.u), ("lambda", r.lam[b], o.variable.lam),
                           ("s", r.s[b], o.variable.s), ("nu", r.nu[b], o.variable.nu), ("trace", r.trace[b], o.trace),
                           ("k", r.k[b], o.k), ("K", np.transpose(r.K[b], (0, 2, 1)), o.K), ("s_gain", r.gs[b], o.s),
                           ("P", np.transpose(r.P[b], (0, 2, 1)), o.P)):
            assert _rel_close(a, c), (model, b, name)
        assert _rel_close(r.barrier_eps[b], o.barrier_eps)
        compared += 1
    assert compared >= B // 2, compared


def _golden():
    here = os.path.join(ROOT, "tests", "golden")
    spec = importlib.util.spec_from_file_location("make_fmpc_vertical_golden", os.path.join(here, "make_fmpc_vertical_golden.py"))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    return make, np.load(os.path.join(here, "fmpc_vertical_golden.npz"))


MAKE, GOLDEN = _golden()


@pytest.mark.parametrize("name", MAKE.SOLVES + ("loop",))
def test_oracle_reproduces_the_vertical_golden_bit_for_bit(name):
    """Every stored array of every instance, diverging or not: the file holds what the per-step-dimension checker that preceded
    the oracle's dims(t) computed, from the inputs stored next to it."""
    got = MAKE.run_loop(GOLDEN) if name == "loop" else MAKE.run_solve(name, GOLDEN)
    stored = {k.split("/", 1)[1] for k in GOLDEN.files if k.startswith(name + "/")}
    assert stored == set(got) and stored
    for k, a in got.items():
        want = GOLDEN[f"{name}/{k}"]
        assert a.dtype == want.dtype and np.array_equal(a, want, equal_nan=True), (name, k)


def test_vertical_golden_covers_its_cases():
    """The recorded horizons hold every switch of the input dimension, a horizon without inequality rows that succeeds at its
    second iteration, poison beyond every step's dimensions, and its inputs are what the generator draws."""
    inputs = MAKE.make_inputs()
    for k, a in inputs.items():
        assert np.array_equal(a, GOLDEN[k]), k
    t0 = GOLDEN["t0"]
    md = np.array([[DC.dims_at("fmpc_vertical", t + i * 0.01)[0] for i in range(MAKE.T)] for t in t0])
    steps = {(a, b) for row in md for a, b in zip(row[:-1], row[1:]) if a != b}
    assert steps == {(1, 2), (2, 1), (1, 0), (0, 1)}
    assert (md == 2).all(axis=1).any() and (md == 0).all(axis=1).sum() == 1
    none = int(np.argmax((md == 0).all(axis=1)))
    assert GOLDEN["default/status"][none] == 1 and GOLDEN["default/iters"][none] == 2
    assert (GOLDEN["in_u"][md < 2][:, 1] == MAKE.POISON).all() and (GOLDEN["default/u"][md < 2][:, 1] == MAKE.POISON).all()
    assert (GOLDEN["default/du"][md < 2][:, 1] == 0).all()
    assert np.isin(GOLDEN["loop/status_log"], (1, 5)).all()


def test_checker_converges_on_vertical_with_forces_in_bounds(checker):
    prob = F.FmpcProblemVerticalMotion()
    B, T = 40, 100
    t0 = np.linspace(0.0, 6.0, B)
    x0 = np.tile([1.0, 0.0], (B, 1))
    var = (np.tile([1.0, 0.0], (B, T + 1, 1)), np.full((B, T, 2), 9.80665), np.zeros((B, T + 1, 2)), np.ones((B, T, 4)),
           np.ones((B, T, 4)))
    r = checker.solve("fmpc_vertical", _cfg(horizon_steps=T, max_iter=60, kkt_error_thre=1e-6), prob.p, t0, x0, var)
    assert (r.status == 1).all(), r.status
    for b in range(B):
        for i in range(T):
            m, g = prob.dimsAt(t0[b] + i * prob.dt())
            f = r.u[b, i, :m]
            assert (f >= prob.p[7] - 1e-9).all() and (f <= prob.p[8] + 1e-9).all()
            assert (r.u[b, i, m:] == 9.80665).all()  # beyond the step's dimension: untouched
            assert (r.s[b, i, g:] == 1.0).all() and (r.nu[b, i, g:] == 1.0).all()
            assert (r.k[b, i, m:] == 0).all() and (r.K[b, i, :, m:] == 0).all()
