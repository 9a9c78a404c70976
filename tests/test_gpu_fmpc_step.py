"""Batched FMPC iteration on caller-supplied linearisations on the device (nmpc_amd.fmpc_step.FmpcStepBatch over the C-ABI of
include/nmpc_hip_fmpc_step.h) against the CPU checker (tests/cpp/fmpc_step_checker.cpp) and, on the oracle's models, against the
pinned oracle.

Bars: every status equal; every real output within 1e-9 (1 + |ref|) of the checker's (fp64 without FMA contraction on
both sides, the device sums in MFMA and butterfly order, the checker in ascending index order); against the oracle the bars of
tests/test_gpu_fmpc.py (rtol 1e-8, atol 1e-10; 1e-7 / 1e-9 on the delta).  The measured figures are printed before they are asserted.
The cases live in tests/fmpc_step_checker.py."""
import numpy as np
import pytest

import fmpc_step_checker as fk
from nmpc_amd import fmpc_step

pytestmark = pytest.mark.gpu

MATRICES = ("A", "B", "C", "D", "Lxx", "Luu", "Lxu", "Lxx_T")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return fk.shared_checker(tmp_path_factory.mktemp("fmpc_step_checker"))


def device_step(case: fk.Case, col_major=False, tensors=False, **config):
    """One step() of `case` on the device from its variable; the Result in the checker's layout."""
    sb = fmpc_step.FmpcStepBatch(case.n, case.m, case.g, case.T, case.B)
    assert sb.kernelName() == "fmpc_step_wave_kernel"
    cfg = sb.config()
    cfg.dt = case.dt
    for k, v in config.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    sb.setStepDims(case.mdims, case.gdims)
    lin = {k: (np.ascontiguousarray(np.swapaxes(v, -1, -2)) if col_major and k in MATRICES else v) for k, v in case.lin.items()}
    var = dict(case.var)
    keep = []
    if tensors:
        import torch
        to = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")
        lin = {k: to(v) for k, v in lin.items()}
        var = {k: to(v) for k, v in var.items()}
        keep = [lin, var]
    sb.setVariable(var["x"], var["u"], var["lam"], var["s"], var["nu"], to(case.eps) if tensors else case.eps)
    r = sb.step(*[lin[k] for k in fk.LIN], col_major=col_major)
    if col_major:
        r.K = np.ascontiguousarray(np.swapaxes(r.K, -1, -2))
        r.P = np.ascontiguousarray(np.swapaxes(r.P, -1, -2))
    assert sb.lastMs() > 0
    del keep
    return r


def assert_variable_bits(r, case, instances):
    for k, a in zip(fk.VAR, (r.x, r.u, r.lam, r.vs, r.vnu)):
        assert np.array_equal(a[instances], case.var[k][instances]), k


def assert_same_bits(a, b, instances_a, instances_b, fields=fk.REAL_FIELDS + ("status",)):
    for f in fields:
        x, y = np.asarray(getattr(a, f))[instances_a], np.asarray(getattr(b, f))[instances_b]
        assert np.array_equal(x, y, equal_nan=True), f


# ---- synthetic shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col_major", (False, True), ids=("row_major", "col_major"))
@pytest.mark.parametrize("shape", fk.SYNTHETIC_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_synthetic_shapes_match_the_checker(checker, shape, col_major):
    case = fk.synthetic_case(*shape)
    ref = checker.step(case)
    assert (ref.status == 6).all()  # every G positive definite, every step length in (0, 1]
    got = device_step(case, col_major=col_major)
    fk.compare(got, ref, case.name + (" col-major" if col_major else " row-major"))


@pytest.mark.parametrize("col_major", (False, True), ids=("row_major", "col_major"))
def test_time_varying_dimensions_match_the_checker_and_pad_with_zeros(checker, col_major):
    case = fk.synthetic_case(3, 2, 5, varying=True)
    ref = checker.step(case)
    assert (ref.status == 6).all()
    got = device_step(case, col_major=col_major)
    fk.compare(got, ref, case.name + (" col-major" if col_major else " row-major"))
    for i, (mi, gi) in enumerate(zip(case.mdims, case.gdims)):
        assert (got.k[:, i, mi:] == 0).all() and (got.K[:, i, mi:, :] == 0).all() and (got.du[:, i, mi:] == 0).all()
        assert (got.ds[:, i, gi:] == 0).all() and (got.dnu[:, i, gi:] == 0).all()
        # the variable beyond a step's dimensions is left alone
        assert np.array_equal(got.u[:, i, mi:], case.var["u"][:, i, mi:]) and np.array_equal(got.vs[:, i, gi:], case.var["s"][:, i, gi:])
        assert np.array_equal(got.vnu[:, i, gi:], case.var["nu"][:, i, gi:])


@pytest.mark.parametrize("col_major", (False, True), ids=("row_major", "col_major"))
@pytest.mark.parametrize("shape", fk.NO_INEQ_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_shapes_without_inequalities_match_the_checker(checker, shape, col_major):
    """g = 0: the equality-constrained LQ problem.  The layout has no inequality tile and no barrier parameter can be derived, so
    update_barrier_eps is off and the caller's barrier_eps comes back."""
    case = fk.synthetic_case(*shape)
    ref = checker.step(case, update_barrier_eps=0)
    assert (ref.status == 6).all()
    got = device_step(case, col_major=col_major, update_barrier_eps=0)
    fk.compare(got, ref, case.name + (" col-major" if col_major else " row-major"))
    assert (got.alpha_s_max == 1).all() and (got.alpha_nu_max == 1).all() and np.array_equal(got.barrier_eps, case.eps)
    assert got.ds.shape == (case.B, case.T, 0) and got.vnu.shape == (case.B, case.T, 0)


@pytest.mark.parametrize("col_major", (False, True), ids=("row_major", "col_major"))
@pytest.mark.parametrize("shape", fk.ONE_STEP_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_a_horizon_of_one_step_matches_the_checker(checker, shape, col_major):
    case = fk.synthetic_case(*shape, T=1)
    ref = checker.step(case)
    assert (ref.status == 6).all()
    got = device_step(case, col_major=col_major)
    fk.compare(got, ref, case.name + (" col-major" if col_major else " row-major"))


@pytest.mark.parametrize("col_major", (False, True), ids=("row_major", "col_major"))
@pytest.mark.parametrize("dims", fk.VARYING_CASES, ids=fk.varying_id)
def test_entries_beyond_a_steps_dimensions_are_neither_read_nor_written(checker, dims, col_major):
    """A two-tile handle, (7, 6, 29), whose steps fill the second inequality tile, leave it partly filled, or leave it dead.  With
    NaN in every input entry beyond a step's dimensions (check_nan on) the device returns the bits it returns without; with NaN in
    the variable beyond them too, those entries come back as they went in and everything else has the same bits."""
    case = fk.synthetic_case(*fk.VARYING_SHAPE, T=fk.VARYING_T, varying=dims)
    ref = checker.step(case)
    assert (ref.status == 6).all()
    label = case.name + (" col-major" if col_major else " row-major")
    got = device_step(case, col_major=col_major)
    fk.compare(got, ref, label)
    fk.assert_zero_beyond_dims(got, case)
    for variable in (False, True):
        dirty = device_step(fk.poisoned(case, variable), col_major=col_major)
        fk.assert_poison_left_no_trace(got, dirty, case, variable)
    # the variable beyond a step's dimensions is left alone
    mu, mg = fk.beyond_dims(case)
    for a, k, mask in ((got.u, "u", mu), (got.vs, "s", mg), (got.vnu, "nu", mg)):
        assert np.array_equal(a[:, mask], case.var[k][:, mask]), k


# ---- model cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", fk.MODELS)
def test_models_match_the_oracle_over_one_and_four_iterations(checker, model):
    var, x0, t0, params = fk.model_start(model)
    ref4 = fk.oracle_solve(model, var, x0, t0, params, 4, kkt_error_thre=0.0)
    print("max KKT error of the oracle over four iterations: %.3g" % ref4.trace[:, :, 1].max())
    got, case = fk.iterate(device_step, model, 1, kkt_error_thre=0.0)
    if model == "fmpc_vertical":
        assert len(set(case.mdims)) > 1 and len(set(case.gdims)) > 1  # the horizon crosses a contact switch
    fk.compare(got, checker.step(case, kkt_error_thre=0.0), model + " 1 iteration vs checker")
    fk.compare_with_oracle(got, fk.oracle_solve(model, var, x0, t0, params, 1, kkt_error_thre=0.0), case, model + " 1 iteration")
    got, case = fk.iterate(device_step, model, 4, kkt_error_thre=0.0)
    fk.compare_with_oracle(got, ref4, case, model + " 4 iterations", iters=4)


def test_initial_complementarity_matches_the_oracle(checker):
    model = "fmpc_cartpole"
    var, x0, t0, params = fk.model_start(model)
    got, case = fk.iterate(device_step, model, 1, kkt_error_thre=0.0, init_complementary_variable=1)
    fk.compare(got, checker.step(case, kkt_error_thre=0.0, init_complementary_variable=1), model + " init vs checker")
    ref = fk.oracle_solve(model, var, x0, t0, params, 1, kkt_error_thre=0.0, init_complementary_variable=1)
    fk.compare_with_oracle(got, ref, case, model + " init_complementary_variable")


# ---- zero pivot --------------------------------------------------------------------------------------------------------------
def test_zero_pivot_breaks_or_falls_back_to_the_lu(checker):
    case = fk.zero_pivot_case()
    got = device_step(case, break_if_llt_fails=1)
    ref = checker.step(case, break_if_llt_fails=1)
    assert list(got.status) == [6, 3, 6] == list(ref.status)
    assert_variable_bits(got, case, [1])
    without = device_step(case.take([0, 2]), break_if_llt_fails=1)  # the neighbours in a batch without it
    assert_same_bits(got, without, [0, 2], [0, 1])
    got = device_step(case, break_if_llt_fails=0)
    ref = checker.step(case, break_if_llt_fails=0)
    fk.compare(got, ref, "zero pivot, LU fallback")


# ---- exact convergence -------------------------------------------------------------------------------------------------------
def test_exact_convergence_succeeds_and_keeps_the_variable(checker):
    case = fk.converged_case()
    got = device_step(case)
    assert (got.status == 1).all() and (got.kkt_error == 0.0).all() and (got.barrier_eps == 1e-8).all()
    assert_variable_bits(got, case, slice(None))


# ---- NaN ---------------------------------------------------------------------------------------------------------------------
def test_a_nan_in_one_instance_is_reported_and_leaves_the_neighbours_alone(checker):
    base = fk.synthetic_case(3, 2, 5)
    A = base.lin["A"].copy()
    A[2, 1, 0, 1] = np.nan
    case = base.replace(lin=dict(A=A))
    ref = checker.step(case)
    got = device_step(case)
    print("status with a NaN in A of instance 2:", got.status, ref.status)
    assert np.array_equal(got.status, ref.status) and ref.status[2] == 3
    assert_variable_bits(got, case, [2])
    clean = device_step(base)
    others = [0, 1, 3, 4]
    assert_same_bits(got, clean, others, others)


# ---- apply_update = 0 --------------------------------------------------------------------------------------------------------
def test_without_the_update_the_variable_stays_and_the_delta_is_the_same(checker):
    case = fk.synthetic_case(3, 2, 5)
    moved = device_step(case)
    kept = device_step(case, apply_update=0)
    assert (kept.status == 6).all()
    assert_variable_bits(kept, case, slice(None))
    assert_same_bits(kept, moved, slice(None), slice(None),
                     ("dx", "du", "dlam", "ds", "dnu", "alpha_s_max", "alpha_nu_max", "k", "K", "s", "P", "kkt_error", "barrier_eps"))
    assert not np.array_equal(moved.x, case.var["x"])


# ---- device tensors ----------------------------------------------------------------------------------------------------------
def test_device_tensors_give_the_bits_of_the_host_path(checker):
    case = fk.synthetic_case(3, 2, 5)
    assert_same_bits(device_step(case, tensors=True), device_step(case), slice(None), slice(None))


def test_tensors_that_queued_torch_kernels_still_have_to_write_are_waited_for():
    """The advertised use: torch kernels that write the tensors are queued on torch's stream immediately before setVariable() and
    step().  The handle's own stream is non-blocking, so nothing but the mirror orders it behind them.  The tensors hold NaN until
    those kernels run, and some 25 ms of elementwise work is queued in front of them, so a call that does not wait reads NaN."""
    import torch
    case = fk.synthetic_case(3, 2, 5)
    ref = device_step(case)
    assert (ref.status == 6).all()
    dev = torch.device("cuda:0")
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)
    src_lin = {k: to(v) for k, v in case.lin.items()}
    src_var = {k: to(v) for k, v in case.var.items()}
    src_var["eps"] = to(case.eps)
    lin = {k: torch.full_like(v, float("nan")) for k, v in src_lin.items()}
    var = {k: torch.full_like(v, float("nan")) for k, v in src_var.items()}
    busy = torch.zeros(1 << 27, dtype=torch.float32, device=dev)
    sb = fmpc_step.FmpcStepBatch(case.n, case.m, case.g, case.T, case.B)
    sb.config().dt = case.dt
    sb.setStepDims(case.mdims, case.gdims)
    torch.cuda.synchronize()

    def queue_writes(src, dst):
        for _ in range(100):
            busy.add_(1.0)
        for k in src:
            torch.mul(src[k], 1.0, out=dst[k])  # x * 1.0 has the bits of x
        assert not torch.cuda.current_stream(dev).query()  # the premise: the writes are still queued when the call is made

    queue_writes(src_var, var)
    sb.setVariable(var["x"], var["u"], var["lam"], var["s"], var["nu"], var["eps"])
    queue_writes(src_lin, lin)
    got = sb.step(*[lin[k] for k in fk.LIN])
    print("status from tensors written by queued kernels:", got.status)
    assert_same_bits(got, ref, slice(None), slice(None))


# ---- batch invariance --------------------------------------------------------------------------------------------------------
def test_an_instance_alone_and_in_a_batch_of_70_returns_the_same_bits(checker):
    big = fk.synthetic_case(3, 2, 5, B=70)
    at = 37
    assert_same_bits(device_step(big.take([at])), device_step(big), [0], [at])


# ---- misuse ------------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused(checker):
    case = fk.synthetic_case(2, 0, 1)
    sb = fmpc_step.FmpcStepBatch(case.n, case.m, case.g, case.T, case.B)
    with pytest.raises(RuntimeError):  # NOT_SOLVED: no variable, no linearisation
        sb.stepDevice()
    sb.setStepDims(None, [0] * case.T)
    sb.setVariable(*[case.var[k] for k in fk.VAR])
    with pytest.raises(ValueError):  # update_barrier_eps with no inequality at any step
        sb.step(*[case.lin[k] for k in fk.LIN])
    with pytest.raises(ValueError):
        sb.setStepDims(None, [2] * case.T)
    # dimensions beyond the capacities of a handle that is smaller than the kernel's largest
    n, m, g = fk.VARYING_SHAPE
    sb = fmpc_step.FmpcStepBatch(n, m, g, fk.VARYING_T, 2)
    for md, gd in (([m] * 4 + [m + 1], None), (None, [g, 0, g + 1, 0, 0]), ([-1] + [m] * 4, None), (None, [31] * 5), ([m] * 4, None)):
        with pytest.raises(ValueError):
            sb.setStepDims(md, gd)
    sb.setStepDims([m] * 5, [g] * 5)
