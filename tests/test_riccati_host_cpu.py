"""Batched Riccati backward pass: what can be checked without a GPU — the C-ABI's exports and the mirror's constants against the
header, the create-time refusals, and the CPU checker (tests/cpp/riccati_checker.cpp) against the pinned C++ oracle on model
derivatives, against the NumPy restatement (oracle/ddp_numpy.py) on synthetic derivatives, and on the retry case.

The cases live in tests/riccati_checker.py and are shared with tests/test_gpu_riccati.py, where the device runs them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import riccati_checker as rk
from nmpc_amd import _capi, riccati
from oracle import ddp_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nmpc_hip_riccati.h")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return rk.shared_checker(tmp_path_factory.mktemp("riccati_checker"))


# ---- library checks ----------------------------------------------------------------------------------------------------------
def test_every_declared_entry_point_is_exported():
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(nmpc_hip_riccati_\w+)\s*\(", text))
    assert declared == set(riccati.EXPORTS)
    L = riccati.load()
    for name in declared:
        getattr(L, name)


def test_default_config_and_struct_are_the_headers():
    c = riccati.default_config()
    assert (c.reg_type, c.lambda_, c.dlambda, c.lambda_factor, c.lambda_min, c.lambda_max) == (1, 1e-4, 1.0, 1.6, 1e-6, 1e10)
    assert (c.with_input_constraint, c.retry, c.row_major) == (0, 1, 0)
    d = ddp_numpy.Config()  # the reference's defaults as the NumPy restatement quotes them
    assert (c.reg_type, c.lambda_, c.dlambda, c.lambda_factor, c.lambda_min, c.lambda_max) == (
        d.reg_type, d.initial_lambda, d.initial_dlambda, d.lambda_factor, d.lambda_min, d.lambda_max)
    body = re.search(r"typedef struct\s*\{(.*?)\}\s*nmpc_hip_riccati_config;", open(HEADER).read(), re.S).group(1)
    fields = re.findall(r"^\s*(int|double)\s+(\w+);", body, re.M)
    assert [(n + "_" if n == "lambda" else n, {"int": C.c_int, "double": C.c_double}[t]) for t, n in fields] == riccati.CConfig._fields_


def test_mirror_constants_are_the_headers():
    text = open(HEADER).read()
    fields = {k: int(v) for k, v in re.findall(r"NMPC_HIP_RICCATI_FIELD_(\w+) = (\d+)", text)}
    assert fields == {"K_FF": riccati.FIELD_K_FF, "K_FB": riccati.FIELD_K_FB, "DV": riccati.FIELD_DV, "VX0": riccati.FIELD_VX0,
                      "VXX0": riccati.FIELD_VXX0, "STATUS": riccati.FIELD_STATUS, "N_BACKWARD": riccati.FIELD_N_BACKWARD,
                      "LAMBDA": riccati.FIELD_LAMBDA, "DLAMBDA": riccati.FIELD_DLAMBDA, "FAIL_STEP": riccati.FIELD_FAIL_STEP,
                      "QP_RETVAL": riccati.FIELD_QP_RETVAL, "FREE_MASK": riccati.FIELD_FREE_MASK}
    status = {k: int(v) for k, v in re.findall(r"NMPC_HIP_RICCATI_(OK|LAMBDA_MAX|PASS_FAILED) = (-?\d+)", text)}
    assert status == {"OK": riccati.STATUS_OK, "LAMBDA_MAX": riccati.STATUS_LAMBDA_MAX, "PASS_FAILED": riccati.STATUS_PASS_FAILED}
    assert int(re.search(r"#define NMPC_HIP_RICCATI_MAX_DIM (\d+)", text).group(1)) == riccati.MAX_DIM == 16
    kernels = open(os.path.join(ROOT, "include", "nmpc_amd", "hip", "riccati_kernels.hpp")).read()
    assert int(re.search(r"kMaxDim = (\d+);", kernels).group(1)) == riccati.MAX_DIM
    mirror = open(os.path.join(ROOT, "include", "nmpc_amd", "RiccatiBatch.hpp")).read()
    assert int(re.search(r"MaxDim = (\d+);", mirror).group(1)) == riccati.MAX_DIM


@pytest.mark.parametrize("n,m,T,B", [(0, 1, 4, 2), (17, 1, 4, 2), (-1, 1, 4, 2), (4, -1, 4, 2), (4, 17, 4, 2), (4, 1, 0, 2), (4, 1, 4, 0),
                                     (4, 1, -2, 2), (4, 1, 4, -1)])
def test_create_refuses_sizes_outside_its_range(n, m, T, B):
    """Arguments are validated before the device is probed: the code is INVALID_ARGUMENT with or without a GPU."""
    L = riccati.load()
    h = C.c_void_p()
    assert L.nmpc_hip_riccati_create(n, m, T, B, 0, C.byref(h)) == _capi.ERR_INVALID_ARGUMENT
    assert not h.value
    assert L.nmpc_hip_riccati_last_error().decode()
    with pytest.raises(ValueError):
        riccati.RiccatiBatch(n, m, T, B)


def test_create_reports_no_device_or_succeeds_and_null_arguments_are_refused():
    L = riccati.load()
    assert L.nmpc_hip_riccati_create(4, 1, 4, 2, 0, None) == _capi.ERR_INVALID_ARGUMENT
    assert L.nmpc_hip_riccati_default_config(None) == _capi.ERR_INVALID_ARGUMENT
    assert L.nmpc_hip_riccati_solve(None) == _capi.ERR_INVALID_ARGUMENT
    assert L.nmpc_hip_riccati_destroy(None) == _capi.OK
    h = C.c_void_p()
    rc = L.nmpc_hip_riccati_create(4, 1, 4, 2, 0, C.byref(h))
    assert rc in (_capi.OK, _capi.ERR_NO_DEVICE)  # never a quiet CPU fallback
    if rc == _capi.OK:
        assert L.nmpc_hip_riccati_destroy(h) == _capi.OK
    else:
        assert not h.value and "no CPU fallback" in L.nmpc_hip_riccati_last_error().decode()


def test_cpp_mirror_and_example_compile_with_a_host_compiler_alone(tmp_path):
    """examples/riccati_batch.cpp against RiccatiBatch.hpp: g++, no HIP headers.  Run, it either reproduces the LQR recursion (a device
    is there) or reports the library's no-device error; bad arguments end it with the usage line."""
    riccati.load()
    libdir = os.path.dirname(_capi.lib_path())
    exe = str(tmp_path / "riccati_batch")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT}/include", os.path.join(ROOT, "examples", "riccati_batch.cpp"),
           f"-L{libdir}", "-lnmpc_hip_ddp", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "3", "20"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    last = r.stdout.splitlines()[-1]
    assert last.startswith("ok riccati_wave_kernel") or last.startswith("runtime_error: no HIP device available"), last
    r = subprocess.run([exe, "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


# ---- the checker against the pinned C++ oracle on model derivatives ----------------------------------------------------------
@pytest.mark.parametrize("c", rk.MODEL_CASES, ids=rk.model_case_id)
def test_checker_matches_the_oracle_on_model_derivatives(checker, c):
    case = rk.model_case(*c)
    got = checker.backward(case)
    ref = rk.Result()
    for f, v in case.expect.items():
        setattr(ref, f, v)
    rk.compare(got, ref, case.name + " checker vs oracle", reals=("k", "K", "dV"), ints=("n_backward", "qp_retval", "free_mask"))
    assert (got.status == 1).all()
    mdl = c[0]
    if mdl == "vertical" and c[1] == 12:
        assert sorted(set(case.dims)) == [1, 2]
    if mdl == "vertical" and c[1] == 60:
        assert set(case.dims) == {0, 1} and case.dims[0] == 1 and case.dims[-1] == 1
    if mdl == "centroidal":
        assert set(case.dims) == {0, 16} and case.dims[0] == 16 and case.dims[-1] == 16
    if mdl == "manipulator" and c[3] is not None:
        masks = sorted(set(int(v) for v in case.expect["free_mask"].ravel()))
        print("manipulator free masks at +-%g:" % c[3], masks)
        if c[3] == 0.5:  # some step mixes free and clamped variables
            assert any(0 < v < (1 << case.m) - 1 for v in masks)


# ---- the checker against the NumPy restatement --------------------------------------------------------------------------------
class _Model:
    def __init__(self, n):
        self.n = n


def numpy_backward(case: rk.Case, b: int, lam0=1e-4, dlam0=1.0, retry=True, cfg=None):
    """ddp_numpy.DDP._backward with the retry loop of DDP._proc_once on instance b of `case`."""
    cfg = cfg or ddp_numpy.Config()
    cfg.horizon_steps, cfg.reg_type, cfg.with_input_constraint = case.T, case.reg_type, case.constrained
    s = ddp_numpy.DDP(_Model(case.n), cfg, None if not case.constrained else (case.lower, case.upper))
    dims = [case.m] * case.T if case.dims is None else list(case.dims)
    d = case.d
    s.D = [(d["Fx"][b, i], d["Fu"][b, i][:, :m], d["Lx"][b, i], d["Lu"][b, i][:m], d["Lxx"][b, i], d["Luu"][b, i][:m, :m],
            d["Lxu"][b, i][:, :m]) for i, m in enumerate(dims)]
    s.VxT, s.VxxT = d["Vx_T"][b], d["Vxx_T"][b]
    s.U = None if case.U is None else [case.U[b, i][:m] for i, m in enumerate(dims)]
    s.lam, s.dlam = lam0, dlam0
    r = dict(n_backward=1, status=1)
    while not s._backward():
        if not retry:
            r["status"] = -2
            break
        s.dlam = max(s.dlam * cfg.lambda_factor, cfg.lambda_factor)
        s.lam = max(s.lam * s.dlam, cfg.lambda_min)
        if s.lam > cfg.lambda_max:
            r["status"] = -1
            break
        r["n_backward"] += 1
    r.update(lam=s.lam, dlam=s.dlam, k=s.k, K=s.K, dV=s.dV, qp_retval=s.qp_ret, qp_free=s.qp_free)
    return r


def assert_checker_matches_numpy(checker, case):
    """The checker on `case` against the NumPy restatement, which is handed the leading m_i columns and rows alone."""
    got = checker.backward(case)
    assert (got.status == 1).all() and (got.n_backward == 1).all() and (got.fail_step == -1).all()
    worst = 0.0
    for b in range(case.B):
        ref = numpy_backward(case, b)
        assert ref["status"] == 1 and ref["n_backward"] == 1
        for i, mi in enumerate(rk.step_dims(case)):
            worst = max(worst, rk.rel_err(got.k[b, i, :mi], ref["k"][i]), rk.rel_err(got.K[b, i, :mi], ref["K"][i]))
            if case.constrained and mi > 0:
                assert got.qp_retval[b, i] == ref["qp_retval"][i]
                assert int(got.free_mask[b, i]) == sum(1 << j for j in ref["qp_free"][i])
        worst = max(worst, rk.rel_err(got.dV[b], ref["dV"]))
    print("riccati %s checker vs numpy: %.2e" % (case.name, worst))
    assert worst <= rk.TOL
    if case.constrained:
        assert (got.free_mask != (1 << case.m) - 1).any()  # the limits bind somewhere
        if case.m >= 4:
            rk.assert_box_is_active(got, case)
    return got


@pytest.mark.parametrize("n,m,boxed,reg", rk.SYNTHETIC_CASES, ids=lambda v: str(v))
def test_checker_matches_numpy_on_synthetic_derivatives(checker, n, m, boxed, reg):
    assert_checker_matches_numpy(checker, rk.synthetic_case(n, m, boxed, reg))


@pytest.mark.parametrize("n,m,boxed,reg", rk.ONE_STEP_CASES, ids=lambda v: str(v))
def test_checker_matches_numpy_on_a_horizon_of_one_step(checker, n, m, boxed, reg):
    assert_checker_matches_numpy(checker, rk.synthetic_case(n, m, boxed, reg, T=1))


# ---- the checker honours "only the leading m_i columns and rows of a block are read" ---------------------------------------------
@pytest.mark.parametrize("reg", (1, 2))
@pytest.mark.parametrize("dims,boxed", rk.VARYING_CASES, ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else ("box" if v else "free"))
def test_checker_does_not_read_beyond_a_steps_input_dimension(checker, dims, boxed, reg):
    """NaN in every entry beyond a step's input dimension changes no bit of the checker's result, and the result is the NumPy
    restatement's on the leading blocks."""
    case = rk.synthetic_case(*rk.VARYING_SHAPE, boxed, reg, T=rk.VARYING_T, dims=dims)
    clean = assert_checker_matches_numpy(checker, case)
    dirty_case = rk.poisoned(case)
    assert np.isnan(dirty_case.d["Luu"]).any() and (not boxed or np.isnan(dirty_case.U).any())  # the helper poisons something
    assert rk.same_bits(clean, checker.backward(dirty_case))
    rk.assert_zero_beyond_dims(clean, case)
    assert not any(np.isnan(np.asarray(getattr(clean, f), dtype=np.float64)).any() for f in rk.REAL_FIELDS)


@pytest.mark.parametrize("c", rk.VARYING_MODEL_CASES, ids=rk.model_case_id)
def test_checker_does_not_read_beyond_a_models_input_dimension(checker, c):
    case = rk.model_case(*c)
    assert len(set(rk.step_dims(case))) > 1
    clean = checker.backward(case)
    assert (clean.status == 1).all()
    dirty_case = rk.poisoned(case)
    assert np.isnan(dirty_case.d["Fu"]).any()
    assert rk.same_bits(clean, checker.backward(dirty_case))


# ---- the retry case ----------------------------------------------------------------------------------------------------------
def test_retry_case_succeeds_at_the_seventh_pass(checker):
    """lambda_k = 1e-4 * 1.6^(k (k + 1) / 2): lambda_5 = 0.115 < 0.5 < lambda_6 = 1.934."""
    case = rk.retry_case(-0.5)
    got = checker.backward(case)
    ref = numpy_backward(case, 0)
    assert got.status[0] == 1 and got.n_backward[0] == 7 == ref["n_backward"] and got.fail_step[0] == 1
    assert got.lam[0] == ref["lam"] and got.dlam[0] == ref["dlam"]
    assert abs(got.lam[0] - 1.9342813) < 1e-7 and abs(got.dlam[0] - 16.777216) < 1e-12
    for i in range(case.T):
        assert rk.rel_err(got.k[0, i], ref["k"][i]) <= rk.TOL and rk.rel_err(got.K[0, i], ref["K"][i]) <= rk.TOL
    once = checker.backward(case, retry=False)
    assert once.status[0] == -2 and once.n_backward[0] == 1 and once.fail_step[0] == 1 and once.lam[0] == 1e-4


@pytest.mark.parametrize("c", rk.RETRY_CASES, ids=rk.retry_id)
def test_retry_at_other_shapes_steps_and_rows_succeeds_at_the_seventh_pass(checker, c):
    """One negative diagonal entry of Luu, -0.5, at step `at`: as the (3, 2) case, lambda_5 = 0.115 fails and lambda_6 = 1.934 passes,
    and the failing step is reported whether it is the first the sweep meets (at = T - 1) or the last (at = 0)."""
    case = rk.retry_shape_case(c)
    assert case.B == 3 and case.d["Luu"][0, c[3], c[4], c[4]] == -0.5 and np.trace(case.d["Luu"][0, c[3]]) == c[1] - 1.5
    got = checker.backward(case)
    assert (got.status == 1).all() and (got.n_backward == 7).all() and (got.fail_step == c[3]).all()
    assert (np.abs(got.lam - 1.9342813) < 1e-7).all() and (np.abs(got.dlam - 16.777216) < 1e-12).all()
    for b in range(case.B):
        ref = numpy_backward(case, b)
        assert ref["n_backward"] == 7 and got.lam[b] == ref["lam"]
        for i in range(case.T):
            assert rk.rel_err(got.k[b, i], ref["k"][i]) <= rk.TOL and rk.rel_err(got.K[b, i], ref["K"][i]) <= rk.TOL


@pytest.mark.parametrize("c", rk.RETRY_CASES_REG2, ids=rk.retry_id)
def test_retry_with_reg_type_2_is_decision_stable_where_the_device_runs_it(checker, c):
    """reg_type 2 (lambda on Vxx): eight passes, lambda_7 = 51.923, on every instance; and the premise of the device test, that
    rounding cannot move a decision: the integers are the same with Fx perturbed by 1e-12 relative."""
    case = rk.retry_shape_case(c, reg=2)
    got = checker.backward(case)
    assert (got.status == 1).all() and (got.n_backward == 8).all() and (got.fail_step == c[3]).all()
    assert (np.abs(got.lam - 51.923) < 1e-3).all()
    rng = np.random.default_rng(77)
    for trial in range(4):
        d = {k: v.copy() for k, v in case.d.items()}
        d["Fx"] = d["Fx"] * (1 + 1e-12 * rng.uniform(-1, 1, d["Fx"].shape))
        assert not np.array_equal(d["Fx"], case.d["Fx"])
        moved = checker.backward(rk.Case(case.name + " perturbed", case.n, case.m, case.T, d, reg_type=2))
        for f in ("status", "n_backward", "fail_step"):
            assert np.array_equal(getattr(moved, f), getattr(got, f)), f
        assert np.array_equal(moved.lam, got.lam) and np.array_equal(moved.dlam, got.dlam)
        assert rk.rel_err(moved.K, got.K) <= rk.TOL  # and the answer moves with the perturbation, not with a decision


def test_retry_case_gives_up_after_twelve_passes(checker):
    """Luu = -1e11 I: lambda_11 = 3.0e9 < 1e10 < lambda_12."""
    case = rk.retry_case(-1e11)
    got = checker.backward(case)
    ref = numpy_backward(case, 0)
    assert got.status[0] == -1 == ref["status"] and got.n_backward[0] == 12 == ref["n_backward"] and got.fail_step[0] == 1
    assert got.lam[0] == ref["lam"] > 1e10 and got.dlam[0] == ref["dlam"]
