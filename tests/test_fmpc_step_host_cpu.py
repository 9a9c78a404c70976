"""Batched FMPC iteration on caller-supplied linearisations: what can be checked without a GPU — the C-ABI's exports and the mirror's
constants against the header, the defaults, the create-time refusals, and the CPU checker (tests/cpp/fmpc_step_checker.cpp) against
the pinned C++ oracle: one iteration and four iterations on the oracle's models, and its LDLT on small matrices.

The cases live in tests/fmpc_step_checker.py and are shared with tests/test_gpu_fmpc_step.py, where the device runs them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fmpc_step_checker as fk
from nmpc_amd import _capi, fmpc_step
from oracle import fmpc as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nmpc_hip_fmpc_step.h")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return fk.shared_checker(tmp_path_factory.mktemp("fmpc_step_checker"))


# ---- library checks ----------------------------------------------------------------------------------------------------------
def test_every_declared_entry_point_is_exported():
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(nmpc_hip_fmpc_step_\w+)\s*\(", text))
    assert declared == set(fmpc_step.EXPORTS)
    L = fmpc_step.load()
    for name in declared:
        getattr(L, name)
    import nmpc_amd
    assert nmpc_amd.FmpcStepBatch is fmpc_step.FmpcStepBatch


def test_default_config_and_struct_are_the_headers_and_the_references():
    c = fmpc_step.default_config()
    o = O.default_config()  # FmpcSolver::Configuration's defaults (FmpcSolver.h:57-89) as the oracle quotes them
    assert (c.kkt_error_thre, c.check_nan, c.init_complementary_variable, c.update_barrier_eps, c.break_if_llt_fails) == (
        o.kkt_error_thre, o.check_nan, o.init_complementary_variable, o.update_barrier_eps, o.break_if_llt_fails) == (1e-4, 1, 0, 1, 0)
    assert o.enable_line_search == 0  # the default this boundary restates
    assert (c.dt, c.apply_update, c.row_major) == (0.01, 1, 0)
    body = re.search(r"typedef struct\s*\{(.*?)\}\s*nmpc_hip_fmpc_step_config;", open(HEADER).read(), re.S).group(1)
    fields = re.findall(r"^\s*(int|double)\s+(\w+);", body, re.M)
    assert [(n, {"int": C.c_int, "double": C.c_double}[t]) for t, n in fields] == fmpc_step.CConfig._fields_
    assert {k: getattr(c, k) for k in fk.CONFIG_DEFAULTS} == fk.CONFIG_DEFAULTS


def test_mirror_constants_are_the_headers():
    text = open(HEADER).read()
    fields = {k: int(v) for k, v in re.findall(r"NMPC_HIP_FMPC_STEP_FIELD_(\w+) = (\d+)", text)}
    assert fields == {k[len("FIELD_"):]: getattr(fmpc_step, k) for k in dir(fmpc_step) if k.startswith("FIELD_")} and len(fields) == 19
    status = {k: int(v) for k, v in re.findall(r"NMPC_HIP_FMPC_STEP_([A-Z_]+) = (\d+)", text) if not k.startswith("FIELD_")}
    assert status == {k[len("STATUS_"):]: getattr(fmpc_step, k) for k in dir(fmpc_step) if k.startswith("STATUS_")}
    assert status == {"UNINITIALIZED": 0, "SUCCEEDED": 1, "ERROR_IN_FORWARD": 2, "ERROR_IN_BACKWARD": 3, "ERROR_IN_UPDATE": 4,
                      "MAX_ITERATION_REACHED": 5, "ITERATION_CONTINUED": 6}  # FmpcSolver.h:92-114
    assert {v: k for k, v in O.STATUS.items() if v in ("Succeeded", "ErrorInForward", "ErrorInBackward", "ErrorInUpdate")} == {
        "Succeeded": 1, "ErrorInForward": 2, "ErrorInBackward": 3, "ErrorInUpdate": 4}
    assert int(re.search(r"#define NMPC_HIP_FMPC_STEP_MAX_DIM (\d+)", text).group(1)) == fmpc_step.MAX_DIM == 16
    assert int(re.search(r"#define NMPC_HIP_FMPC_STEP_MAX_INEQ (\d+)", text).group(1)) == fmpc_step.MAX_INEQ == 32
    kernels = open(os.path.join(ROOT, "include", "nmpc_amd", "hip", "fmpc_step_kernels.hpp")).read()
    assert int(re.search(r"kMaxDim = (\d+);", kernels).group(1)) == fmpc_step.MAX_DIM
    assert int(re.search(r"kMaxIneq = (\d+);", kernels).group(1)) == fmpc_step.MAX_INEQ
    assert "#include <nmpc_amd/" not in kernels and '#include "' not in kernels  # no existing kernel header
    mirror = open(os.path.join(ROOT, "include", "nmpc_amd", "FmpcStepBatch.hpp")).read()
    assert int(re.search(r"MaxDim = (\d+);", mirror).group(1)) == fmpc_step.MAX_DIM
    assert int(re.search(r"MaxIneq = (\d+);", mirror).group(1)) == fmpc_step.MAX_INEQ


@pytest.mark.parametrize("n,m,g,T,B", [(0, 1, 1, 4, 2), (17, 1, 1, 4, 2), (-1, 1, 1, 4, 2), (4, -1, 1, 4, 2), (4, 17, 1, 4, 2),
                                       (4, 1, -1, 4, 2), (4, 1, 33, 4, 2), (4, 1, 1, 0, 2), (4, 1, 1, -2, 2), (4, 1, 1, 4, 0),
                                       (4, 1, 1, 4, -1)])
def test_create_refuses_sizes_outside_its_range(n, m, g, T, B):
    """Arguments are validated before the device is probed: the code is INVALID_ARGUMENT with or without a GPU."""
    L = fmpc_step.load()
    h = C.c_void_p()
    assert L.nmpc_hip_fmpc_step_create(n, m, g, T, B, 0, C.byref(h)) == _capi.ERR_INVALID_ARGUMENT
    assert not h.value
    assert L.nmpc_hip_fmpc_step_last_error().decode()
    with pytest.raises(ValueError):
        fmpc_step.FmpcStepBatch(n, m, g, T, B)


def test_create_reports_no_device_or_succeeds_and_null_arguments_are_refused():
    L = fmpc_step.load()
    assert L.nmpc_hip_fmpc_step_create(4, 1, 4, 4, 2, 0, None) == _capi.ERR_INVALID_ARGUMENT
    assert L.nmpc_hip_fmpc_step_default_config(None) == _capi.ERR_INVALID_ARGUMENT
    assert L.nmpc_hip_fmpc_step_step(None) == _capi.ERR_INVALID_ARGUMENT
    assert L.nmpc_hip_fmpc_step_destroy(None) == _capi.OK
    h = C.c_void_p()
    rc = L.nmpc_hip_fmpc_step_create(4, 1, 4, 4, 2, 0, C.byref(h))
    assert rc in (_capi.OK, _capi.ERR_NO_DEVICE)  # never a quiet CPU fallback
    if rc == _capi.OK:
        assert L.nmpc_hip_fmpc_step_destroy(h) == _capi.OK
    else:
        assert not h.value and "no CPU fallback" in L.nmpc_hip_fmpc_step_last_error().decode()


def test_cpp_mirror_and_example_compile_with_a_host_compiler_alone(tmp_path):
    """examples/fmpc_step_batch.cpp against FmpcStepBatch.hpp: g++, no HIP headers.  Run, it either iterates a constrained double
    integrator to its KKT threshold (a device is there) or reports the library's no-device error."""
    fmpc_step.load()
    libdir = os.path.dirname(_capi.lib_path())
    exe = str(tmp_path / "fmpc_step_batch")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT}/include", os.path.join(ROOT, "examples", "fmpc_step_batch.cpp"),
           f"-L{libdir}", "-lnmpc_hip_ddp", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "3", "20"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    last = r.stdout.splitlines()[-1]
    assert last.startswith("ok fmpc_step_wave_kernel") or last.startswith("runtime_error: no HIP device available"), last
    r = subprocess.run([exe, "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


# ---- the checker against the pinned C++ oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", fk.MODELS)
def test_checker_matches_the_oracle_over_one_iteration(checker, model):
    got, case = fk.iterate(checker.step, model, 1, kkt_error_thre=0.0)
    var, x0, t0, params = fk.model_start(model)
    ref = fk.oracle_solve(model, var, x0, t0, params, 1, kkt_error_thre=0.0)
    fk.compare_with_oracle(got, ref, case, model + " 1 iteration")
    if model == "fmpc_vertical":
        assert sorted(set(case.mdims)) == [1, 2] and sorted(set(case.gdims)) == [2, 4]  # the horizon crosses a contact switch


@pytest.mark.parametrize("model", fk.MODELS)
def test_checker_matches_the_oracle_over_four_iterations(checker, model):
    got, case = fk.iterate(checker.step, model, 4, kkt_error_thre=0.0)
    var, x0, t0, params = fk.model_start(model)
    ref = fk.oracle_solve(model, var, x0, t0, params, 4, kkt_error_thre=0.0)
    print("max KKT error of the oracle over four iterations: %.3g" % ref.trace[:, :, 1].max())
    fk.compare_with_oracle(got, ref, case, model + " 4 iterations", iters=4)


def test_checker_matches_the_oracle_with_initial_complementarity(checker):
    model = "fmpc_cartpole"
    got, case = fk.iterate(checker.step, model, 1, kkt_error_thre=0.0, init_complementary_variable=1)
    var, x0, t0, params = fk.model_start(model)
    ref = fk.oracle_solve(model, var, x0, t0, params, 1, kkt_error_thre=0.0, init_complementary_variable=1)
    fk.compare_with_oracle(got, ref, case, model + " init_complementary_variable")


# ---- the checker's LDLT against the oracle's -----------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(1, 9))
def test_checker_ldlt_matches_the_oracles(checker, m):
    rng = np.random.default_rng(300 + m)
    worst = 0.0
    for trial in range(6):
        R = rng.uniform(-1, 1, (m, m))
        G = R @ R.T + 0.1 * np.eye(m) if trial < 3 else 0.5 * (R + R.T)  # positive definite, and indefinite (pivoting matters)
        b = rng.uniform(-1, 1, (m, 3))
        for use_lu in (False, True):
            x, ok = checker.ldlt_solve(G, b, use_lu)
            xr, okr = O.ldlt_solve(G, b, use_lu)
            assert ok == okr
            worst = max(worst, fk.rel_err(x, xr))
    print("fmpc_step ldlt m=%d checker vs oracle: %.2e" % (m, worst))
    assert worst <= fk.TOL


def test_checker_ldlt_reports_the_zero_diagonal_matrix_as_the_oracle_does(checker):
    G = np.array([[0.0, 0.1], [0.1, 0.0]])  # dt Luu of the zero-pivot case
    b = np.array([[1.0, 2.0], [3.0, -1.0]])
    x, ok = checker.ldlt_solve(G, b)
    xr, okr = O.ldlt_solve(G, b)
    assert ok is False and okr is False
    x, _ = checker.ldlt_solve(G, b, use_lu=True)
    xr, _ = O.ldlt_solve(G, b, use_lu=True)
    assert fk.rel_err(x, xr) <= fk.TOL and fk.rel_err(G @ x, b) <= fk.TOL
    assert checker.ldlt_solve(np.zeros((2, 2)), b)[1] is True  # an all-zero matrix is a success (Eigen's rule)


def test_checker_statuses_on_the_special_cases(checker):
    """The zero-pivot case (status 3 with break_if_llt_fails, the LU otherwise) and the exactly converged one."""
    case = fk.zero_pivot_case()
    r = checker.step(case, break_if_llt_fails=1)
    assert list(r.status) == [6, 3, 6]
    for k, a in zip(fk.VAR, (r.x, r.u, r.lam, r.vs, r.vnu)):
        assert np.array_equal(a[1], case.var[k][1])
    r = checker.step(case, break_if_llt_fails=0)
    assert list(r.status) == [6, 6, 6] and np.isfinite(r.K).all()
    c = fk.converged_case()
    r = checker.step(c)
    assert (r.status == 1).all() and (r.kkt_error == 0.0).all() and (r.barrier_eps == 1e-8).all()
    for k, a in zip(fk.VAR, (r.x, r.u, r.lam, r.vs, r.vnu)):
        assert np.array_equal(a, c.var[k])
    for shape in fk.SYNTHETIC_SHAPES:
        r = checker.step(fk.synthetic_case(*shape))
        assert (r.status == 6).all(), (shape, r.status)
    r = checker.step(fk.synthetic_case(3, 2, 5, varying=True))
    assert (r.status == 6).all()


# ---- the premises of the boundary shapes -------------------------------------------------------------------------------------
def boundary_cases():
    """(case, config) of every synthetic case the device tests run beyond the four base shapes."""
    out = [(fk.synthetic_case(*shape), {}) for shape in fk.BOUNDARY_SHAPES]
    out += [(fk.synthetic_case(*shape), dict(update_barrier_eps=0)) for shape in fk.NO_INEQ_SHAPES]
    out += [(fk.synthetic_case(*shape, T=1), {}) for shape in fk.ONE_STEP_SHAPES]
    out += [(fk.synthetic_case(*fk.VARYING_SHAPE, T=fk.VARYING_T, varying=dims), {}) for dims in fk.VARYING_CASES]
    return out


def test_every_boundary_case_takes_a_full_iteration_on_the_checker(checker):
    """The premise of the device tests: every G is positive definite and every step length is in (0, 1], so every instance ends as
    ITERATION_CONTINUED and no output is left unwritten."""
    lo = 1.0
    for case, config in boundary_cases():
        r = checker.step(case, **config)
        assert (r.status == 6).all(), (case.name, r.status)
        assert np.isfinite(r.K).all() and np.isfinite(r.P).all() and np.isfinite(r.dnu).all()
        lo = min(lo, float(r.alpha_s_max.min()), float(r.alpha_nu_max.min()))
        if config:
            assert (r.barrier_eps == case.eps).all()  # update_barrier_eps = 0 keeps the caller's
    print("fmpc_step boundary cases: smallest step length %.3f" % lo)
    assert 0 < lo <= 1


# ---- the checker honours "only the leading m_i, g_i rows and columns are read" --------------------------------------------------
@pytest.mark.parametrize("dims", fk.VARYING_CASES, ids=fk.varying_id)
def test_checker_does_not_read_or_write_beyond_a_steps_dimensions(checker, dims):
    """NaN in every entry beyond a step's dimensions (check_nan on) changes no bit of the checker's result, so the reference of the
    device's poison test honours the contract itself."""
    case = fk.synthetic_case(*fk.VARYING_SHAPE, T=fk.VARYING_T, varying=dims)
    clean = checker.step(case)
    assert (clean.status == 6).all()
    for variable in (False, True):
        dirty = checker.step(fk.poisoned(case, variable))
        fk.assert_poison_left_no_trace(clean, dirty, case, variable)
    fk.assert_zero_beyond_dims(clean, case)
    if min(dims[1]) < fk.VARYING_SHAPE[2]:  # the helper poisons something: the premise of the test itself
        assert np.isnan(fk.poisoned(case).lin["C"]).any() and np.isnan(fk.poisoned(case, True).var["nu"]).any()
        assert not np.isnan(fk.poisoned(case).var["nu"]).any()


# ---- the checker's delta solves the linearised KKT system ------------------------------------------------------------------------
KKT_CASES = ([(shape, fk.SYNTHETIC_T, False) for shape in fk.BOUNDARY_SHAPES if shape[2] > 5]
             + [(shape, 1, False) for shape in fk.ONE_STEP_SHAPES if shape[2] > 5] + [(fk.VARYING_SHAPE, fk.VARYING_T, fk.VARYING_CASES[0])])
KKT_BAR = 100 * 7.7e-16  # 100 times the measured worst figure: see the test's docstring


def test_checker_delta_solves_the_linearised_kkt_system(checker):
    """Where the pinned oracle cannot reach (g > 16, n, m > 4): the checker's (dx, du, dlambda, ds, dnu) put into the linear system
    it claims to solve, assembled in numpy longdouble from the case's arrays as the equations themselves (fk.kkt_residuals), not as
    a Riccati recursion.  The figure of a block is max |residual| / (1 + max |term of the block|).

    Measured on the CPU over these cases (x86-64, g++ -O2 -ffp-contract=off): worst block figure 7.69e-16 (stationarity u 7.69e-16,
    stationarity x 7.25e-16, inequality 2.32e-16, dynamics 2.06e-16, complementarity 1.98e-16), rounded up to 7.7e-16.  The bar is
    100 times that, 7.7e-14: the margin leaves room for another order of summation, and a wrong offset or mask in the checker moves
    a residual to the order of the terms themselves, 1e-2 and more."""
    assert len(KKT_CASES) == 12
    worst, instances = {}, 0
    for shape, T, varying in KKT_CASES:
        case = fk.synthetic_case(*shape, T=T, varying=varying)
        r = checker.step(case, apply_update=0)
        assert (r.status == 6).all(), case.name  # no instance is left out
        instances += case.B
        res = fk.kkt_residuals(case, r)
        print("fmpc_step %s KKT residuals: %s" % (case.name, ", ".join("%s %.2e" % kv for kv in res.items())))
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("fmpc_step KKT residuals, worst per block: %s; bar %.1e" % (", ".join("%s %.2e" % kv for kv in worst.items()), KKT_BAR))
    assert instances == 12 * fk.SYNTHETIC_B
    for k, v in worst.items():
        assert v <= KKT_BAR, (k, v)


def test_kkt_residuals_notice_a_wrong_delta(checker):
    """The residual check has teeth: one entry of the delta moved by 1e-9 relative, or the delta of a neighbouring inequality row
    swapped in, puts a block over the bar."""
    case = fk.synthetic_case(13, 12, 31)
    r = checker.step(case, apply_update=0)
    dnu = r.dnu.copy()
    dnu[0, 2, 30] *= 1 + 1e-9
    r.dnu = dnu
    assert max(fk.kkt_residuals(case, r).values()) > KKT_BAR
    r = checker.step(case, apply_update=0)
    du = r.du.copy()
    du[1, 3, [10, 11]] = du[1, 3, [11, 10]]
    r.du = du
    assert max(fk.kkt_residuals(case, r).values()) > 1e-6
