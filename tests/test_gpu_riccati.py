"""Batched Riccati backward pass on the device (riccati_wave_kernel through nmpc_amd.riccati.RiccatiBatch) against the CPU checker
(tests/cpp/riccati_checker.cpp) and, on model derivatives, the pinned C++ oracle: every real output within 1e-9 (1 + |ref|), every
integer output equal.  The cases and the references live in tests/riccati_checker.py and are shared with
tests/test_riccati_host_cpu.py, which checks the checker itself."""
import ctypes as C

import numpy as np
import pytest

import riccati_checker as rk
from nmpc_amd import _capi, riccati

pytestmark = pytest.mark.gpu

MATRICES = ("Fx", "Fu", "Lxx", "Luu", "Lxu", "Vxx_T")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return rk.shared_checker(tmp_path_factory.mktemp("riccati_checker"))


def device_backward(case: rk.Case, col_major=False, solver=None, retry=True, lam=None, dlam=None):
    s = solver or riccati.RiccatiBatch(case.n, case.m, case.T, case.B)
    s.config().reg_type = case.reg_type
    s.config().retry = int(retry)
    s.setInputDims(case.dims)
    s.setLambda(lam, dlam)
    d = {k: (np.swapaxes(v, -1, -2) if col_major and k in MATRICES else v) for k, v in case.d.items()}
    r = s.backward(U=case.U, lower=case.lower, upper=case.upper, col_major=col_major, **d)
    if col_major:
        r.K = np.swapaxes(r.K, -1, -2)
        r.Vxx0 = np.swapaxes(r.Vxx0, -1, -2)
    assert s.kernelName() == "riccati_wave_kernel" and s.lastMs() > 0
    return r


same_bits = rk.same_bits


def pick(r, idx):
    """The instances idx of a result."""
    out = rk.Result()
    for f in rk.REAL_FIELDS + rk.INT_FIELDS:
        setattr(out, f, np.asarray(getattr(r, f))[np.asarray(idx)])
    return out


# ---- parity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col_major", [False, True], ids=["row_major", "col_major"])
@pytest.mark.parametrize("c", rk.MODEL_CASES, ids=rk.model_case_id)
def test_model_case_matches_checker_and_oracle(checker, c, col_major):
    case = rk.model_case(*c)
    assert case.B == 5
    ref = checker.backward(case)
    got = device_backward(case, col_major)
    rk.compare(got, ref, case.name + " device vs checker")
    oracle_ref = rk.Result()
    for f, v in case.expect.items():
        setattr(oracle_ref, f, v)
    rk.compare(got, oracle_ref, case.name + " device vs oracle", reals=("k", "K", "dV"), ints=("n_backward", "qp_retval", "free_mask"))
    if case.dims is not None:  # outputs beyond the step's input dimension are exactly 0
        for i, m in enumerate(case.dims):
            assert not got.k[:, i, m:].any() and not got.K[:, i, m:, :].any()


@pytest.mark.parametrize("c", [c for c in rk.MODEL_CASES if c[3] is not None], ids=rk.model_case_id)
def test_box_case_with_limits_per_step(checker, c):
    case = rk.model_case(*c)
    ref = checker.backward(case)
    got = device_backward(case.with_limits_per_step())
    rk.compare(got, ref, case.name + " limits per step, device vs checker")
    assert same_bits(got, device_backward(case))


@pytest.mark.parametrize("col_major", [False, True], ids=["row_major", "col_major"])
@pytest.mark.parametrize("n,m,boxed,reg", rk.SYNTHETIC_CASES, ids=lambda v: str(v))
def test_synthetic_case_matches_checker(checker, n, m, boxed, reg, col_major):
    case = rk.synthetic_case(n, m, boxed, reg)
    ref = checker.backward(case)
    got = device_backward(case, col_major)
    rk.compare(got, ref, case.name + " device vs checker")
    assert (got.status == 1).all() and (got.n_backward == 1).all() and (got.fail_step == -1).all()
    if boxed and m >= 4:
        rk.assert_box_is_active(ref, case)


@pytest.mark.parametrize("col_major", [False, True], ids=["row_major", "col_major"])
@pytest.mark.parametrize("n,m,boxed,reg", rk.ONE_STEP_CASES, ids=lambda v: str(v))
def test_a_horizon_of_one_step_matches_checker(checker, n, m, boxed, reg, col_major):
    case = rk.synthetic_case(n, m, boxed, reg, T=1)
    ref = checker.backward(case)
    got = device_backward(case, col_major)
    rk.compare(got, ref, case.name + " device vs checker")
    assert (got.status == 1).all() and (got.n_backward == 1).all() and (got.fail_step == -1).all()
    if boxed and m >= 4:
        rk.assert_box_is_active(ref, case)


# ---- entries beyond a step's input dimension -------------------------------------------------------------------------------------
def assert_poison_leaves_no_trace(checker, case, col_major):
    """The device on `case` matches the checker, writes exact zeros beyond a step's input dimension, and returns the same bits with
    NaN in every input entry beyond it."""
    ref = checker.backward(case)
    got = device_backward(case, col_major)
    rk.compare(got, ref, case.name + " device vs checker")
    assert (got.status == 1).all() and (got.fail_step == -1).all()
    rk.assert_zero_beyond_dims(got, case)
    dirty = rk.poisoned(case)
    assert np.isnan(dirty.d["Fu"]).any() and np.isnan(dirty.d["Luu"]).any()
    assert same_bits(device_backward(dirty, col_major), got)
    assert not any(np.isnan(np.asarray(getattr(got, f), dtype=np.float64)).any() for f in rk.REAL_FIELDS)


@pytest.mark.parametrize("col_major", [False, True], ids=["row_major", "col_major"])
@pytest.mark.parametrize("reg", (1, 2))
@pytest.mark.parametrize("dims,boxed", rk.VARYING_CASES, ids=lambda v: "".join(map(str, v)) if isinstance(v, tuple) else ("box" if v else "free"))
def test_entries_beyond_a_steps_input_dimension_are_not_read(checker, dims, boxed, reg, col_major):
    """A (7, 6) handle whose steps have every input dimension from 0 to 6; the blocks beyond them hold ordinary numbers, then NaN."""
    assert_poison_leaves_no_trace(checker, rk.synthetic_case(*rk.VARYING_SHAPE, boxed, reg, T=rk.VARYING_T, dims=dims), col_major)


@pytest.mark.parametrize("c", rk.VARYING_MODEL_CASES, ids=rk.model_case_id)
def test_entries_beyond_a_models_input_dimension_are_not_read(checker, c):
    """The model cases with time-varying input dimension, whose padding is zeros in test_model_case_matches_checker_and_oracle."""
    assert_poison_leaves_no_trace(checker, rk.model_case(*c), False)


# ---- the retry loop --------------------------------------------------------------------------------------------------------------
def test_retry_case(checker):
    case = rk.retry_case(-0.5)
    ref = checker.backward(case)
    got = device_backward(case)
    rk.compare(got, ref, "retry case, device vs checker")
    assert got.status[0] == 1 and got.n_backward[0] == 7 and got.fail_step[0] == 1
    assert abs(got.lam[0] - 1.9342813) < 1e-7 and abs(got.dlam[0] - 16.777216) < 1e-12
    # carried lambda: a second pass from the returned values succeeds at once
    again = device_backward(case, lam=got.lam, dlam=got.dlam)
    assert again.status[0] == 1 and again.n_backward[0] == 1 and again.lam[0] == got.lam[0]
    assert np.array_equal(again.k, got.k) and np.array_equal(again.K, got.K)


@pytest.mark.parametrize("c,reg", [(c, 1) for c in rk.RETRY_CASES] + [(c, 2) for c in rk.RETRY_CASES_REG2],
                         ids=lambda v: rk.retry_id(v) if isinstance(v, tuple) else "reg%d" % v)
def test_retry_at_other_shapes_steps_and_rows(checker, c, reg):
    """Luu[row, row] = -0.5 at step `at`, the first or the last step the sweep meets or one in between, on full-size blocks: seven
    passes to lambda_6 = 1.934 with reg_type 1, eight to lambda_7 = 51.923 with reg_type 2."""
    case = rk.retry_shape_case(c, reg)
    ref = checker.backward(case)
    got = device_backward(case)
    rk.compare(got, ref, case.name + " device vs checker")
    passes, lam = (7, 1.9342813) if reg == 1 else (8, 51.923)
    assert (ref.status == 1).all() and (ref.n_backward == passes).all() and (ref.fail_step == c[3]).all()
    assert (np.abs(ref.lam - lam) < (1e-7 if reg == 1 else 1e-3)).all()
    assert (got.status == 1).all() and (got.n_backward == passes).all() and (got.fail_step == c[3]).all()
    assert np.array_equal(got.lam, ref.lam) and np.array_equal(got.dlam, ref.dlam)


def test_retry_gives_up_at_lambda_max(checker):
    case = rk.retry_case(-1e11)
    ref = checker.backward(case)
    got = device_backward(case)
    assert got.status[0] == -1 == ref.status[0] and got.n_backward[0] == 12 == ref.n_backward[0] and got.fail_step[0] == 1
    assert got.lam[0] == ref.lam[0] and got.dlam[0] == ref.dlam[0]


def test_retry_switch(checker):
    case = rk.retry_case(-0.5)
    got = device_backward(case, retry=False)
    ref = checker.backward(case, retry=False)
    assert got.status[0] == -2 == ref.status[0] and got.fail_step[0] == 1 and got.n_backward[0] == 1
    assert got.lam[0] == 1e-4 and got.dlam[0] == 1.0


# ---- independence of the instances ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(3, 2), (16, 16)])
def test_position_independence(n, m):
    """Instance s of a B = 67 batch (more instances than a wavefront has lanes) returns the bits it returns alone and elsewhere."""
    case = rk.synthetic_case(n, m, True, 1, 67)
    full = device_backward(case)
    assert (full.status == 1).all()
    for s in (0, 33, 66):
        assert same_bits(pick(full, [s]), device_backward(case.take([s]))), s
    perm = np.arange(67)[::-1].copy()
    perm[[5, 40]] = perm[[40, 5]]
    assert same_bits(pick(full, perm), device_backward(case.take(perm)))


def test_failing_neighbour_leaves_the_others_alone():
    good = [rk.retry_case(-0.5, 1, seed) for seed in (1, 2, 3, 4)]
    bad = rk.retry_case(-1e11, 1, 9)
    alone = device_backward(rk.concat(good))
    mixed = device_backward(rk.concat(good[:2] + [bad] + good[2:]))
    assert mixed.status.tolist() == [1, 1, -1, 1, 1] and mixed.n_backward[2] == 12
    assert same_bits(pick(mixed, [0, 1, 3, 4]), alone)


# ---- device tensors --------------------------------------------------------------------------------------------------------------
def test_backward_device_returns_the_bits_of_backward():
    import torch
    first, second = rk.model_case("quadrotor", 5, 0.0, 0.5, 1), rk.model_case("quadrotor", 5, 0.0, 2.0, 2)
    s = riccati.RiccatiBatch(first.n, first.m, first.T, first.B)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    for case in (first, second, first):  # the second and third call must not see what the call before left
        host = device_backward(case)
        t = {k: torch.tensor(v, dtype=torch.float64, device=dev) for k, v in case.d.items()}
        U, lo, up = (torch.tensor(np.asarray(a), dtype=torch.float64, device=dev) for a in (case.U, case.lower, case.upper))
        torch.cuda.synchronize(dev)
        s.config().reg_type = case.reg_type
        r = s.backwardDevice(U=U, lower=lo, upper=up, stream=stream, **t)
        stream.synchronize()
        got = rk.Result()
        for f in rk.REAL_FIELDS + rk.INT_FIELDS:
            a = getattr(r, f).cpu().numpy()
            setattr(got, f, a.view(np.uint32) if f == "free_mask" else a)
        assert same_bits(got, host), case.name
        # the per-instance lambda tensors of the result go back in
        r2 = s.backwardDevice(U=U, lower=lo, upper=up, lam=r.lam, dlam=r.dlam, stream=stream, **t)
        stream.synchronize()
        assert torch.equal(r2.k, r.k) and torch.equal(r2.K, r.K) and torch.equal(r2.lam, r.lam)
    with pytest.raises(ValueError):
        s.backwardDevice(U=U, lower=lo, upper=up, **{**t, "Fx": t["Fx"].to(torch.float32)})
    with pytest.raises(ValueError):
        s.backwardDevice(U=U, lower=lo, upper=up, **{**t, "Fu": t["Fu"].transpose(-1, -2)})
    with pytest.raises(ValueError):
        s.backwardDevice(U=U, lower=lo, upper=up, **{**t, "Lx": t["Lx"].cpu()})


# ---- misuse ------------------------------------------------------------------------------------------------------------------------
def test_misuse_codes():
    L = riccati.load()
    case = rk.synthetic_case(3, 2, True, 1)
    h = C.c_void_p()
    assert L.nmpc_hip_riccati_create(case.n, case.m, case.T, case.B, 0, C.byref(h)) == _capi.OK
    try:
        nb = C.c_size_t()
        assert L.nmpc_hip_riccati_field_bytes(h, riccati.FIELD_K_FB, C.byref(nb)) == _capi.OK
        assert nb.value == case.B * case.T * case.m * case.n * 8
        buf = np.zeros(nb.value // 8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.nmpc_hip_riccati_solve(h) == _capi.ERR_NOT_SOLVED  # no derivatives yet
        assert L.nmpc_hip_riccati_get(h, riccati.FIELD_K_FB, vp(buf), nb.value, 0) == _capi.ERR_NOT_SOLVED
        ms = C.c_float()
        assert L.nmpc_hip_riccati_last_ms(h, C.byref(ms)) == _capi.ERR_NOT_SOLVED
        d = {k: np.ascontiguousarray(v) for k, v in case.d.items()}
        assert L.nmpc_hip_riccati_set_derivatives(h, *[vp(d[k]) for k in riccati._DERIVATIVES], 0) == _capi.OK
        cfg = riccati.default_config()
        cfg.with_input_constraint, cfg.row_major = 1, 1
        assert L.nmpc_hip_riccati_set_config(h, C.byref(cfg)) == _capi.OK
        assert L.nmpc_hip_riccati_solve(h) == _capi.ERR_NOT_SOLVED  # constrained without set_inputs
        assert L.nmpc_hip_riccati_get(h, riccati.FIELD_K_FB, vp(buf), nb.value, 0) == _capi.ERR_NOT_SOLVED
        cfg.reg_type = 3
        assert L.nmpc_hip_riccati_set_config(h, C.byref(cfg)) == _capi.ERR_INVALID_ARGUMENT
        bad_dims = np.array([0, 1, 3, 2], dtype=np.int32)
        assert L.nmpc_hip_riccati_set_input_dims(h, vp(bad_dims)) == _capi.ERR_INVALID_ARGUMENT
        assert L.nmpc_hip_riccati_set_inputs(h, vp(np.ascontiguousarray(case.U)), vp(case.lower.copy()), vp(case.upper.copy()), 2, 0) \
            == _capi.ERR_INVALID_ARGUMENT
        assert L.nmpc_hip_riccati_set_inputs(h, vp(np.ascontiguousarray(case.U)), vp(case.lower.copy()), vp(case.upper.copy()), 0, 0) == _capi.OK
        assert L.nmpc_hip_riccati_solve(h) == _capi.OK
        assert L.nmpc_hip_riccati_get(h, riccati.FIELD_K_FB, vp(buf), nb.value - 8, 0) == _capi.ERR_INVALID_ARGUMENT
        assert L.nmpc_hip_riccati_get(h, 99, vp(buf), nb.value, 0) == _capi.ERR_INVALID_ARGUMENT
        assert L.nmpc_hip_riccati_get(h, riccati.FIELD_K_FB, vp(buf), nb.value, 0) == _capi.OK and buf.any()
    finally:
        assert L.nmpc_hip_riccati_destroy(h) == _capi.OK
    # input dimensions beyond the capacity of a handle that is smaller than the kernel's largest
    n, m = rk.VARYING_SHAPE
    s = riccati.RiccatiBatch(n, m, rk.VARYING_T, 2)
    for dims in ([m, m, m + 1, m, m], [m, -1, m, m, m], [16] * 5, [m] * 4):
        with pytest.raises(ValueError):
            s.setInputDims(dims)
    s.setInputDims([m] * 5)
