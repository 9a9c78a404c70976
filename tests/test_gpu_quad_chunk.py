"""The quad kernel's backward pass at the shapes where its chunk code takes another path (ddp_kernels_quad.hpp, backwardQuad):
the guarded loop only, the straight-line chunks of 4 and of 16 timesteps, their combinations, a padded second workgroup; the three
regularisation types; n = 2 (the padding beyond n is part of the record constants that are laid once per launch); a pivot that
fails inside an unguarded chunk (the chunk's pass-failure test runs once, behind the chunk, and the guarded loop repeats it); the
box-constrained step; a handle that solves twice (the record constants outlive a solve, the input conversion reuses the chunk as
staging between them); resumable launches (every launch lays the constants itself).

Against the CPU oracle at the bar of tests/test_gpu_parity.py: status, iteration count, alpha-index history, n_backward / n_forward
bit-exact; X, U, k, K within 1e-9 (1 + |ref|), total cost within 1e-10 relative."""
import functools

import numpy as np
import pytest

import oracle
from nmpc_amd import workloads

from test_gpu_parity import INT_COLS, TOL, check_against_oracle, make_solver, oracle_batch, scaled_err

pytestmark = pytest.mark.gpu

QUAD = "ddp_solve_quad_kernel"
FIELDS = ("X", "U", "cost", "kff", "Kfb", "trace", "iters", "status", "dV")


@pytest.fixture(autouse=True)
def default_dispatch(monkeypatch):
    monkeypatch.delenv("NMPC_HIP_DDP_KERNEL", raising=False)


@functools.lru_cache(maxsize=None)
def cartpole_case(B, T, seed, max_iter, reg_type=1):
    """Workload and the oracle's answer, computed once per shape."""
    wl = workloads.cartpole_batch(B=B, T=T, seed=seed)
    return wl, oracle_batch(wl, max_iter=max_iter, reg_type=reg_type)


def outputs(s):
    return {f: np.array(getattr(s, f)()) for f in FIELDS}


# T: 3 guarded loop only; 4 the straight-line 4-step chunk; 16 the 16-step chunk; 20 = 16 + 4; 33 two full chunks and a one-step
# guarded chunk; 100 the headline's layout (six chunks of 16 and one of 4).  B: one lane, one full workgroup, a padded second one.
@pytest.mark.parametrize("T", [3, 4, 16, 20, 33, 100])
@pytest.mark.parametrize("B", [1, 16, 17])
def test_cartpole_horizons_and_batches(B, T):
    wl, ref = cartpole_case(B, T, 100 * B + T, 4)
    s = make_solver(wl, max_iter=4)
    s.solve(wl.t0, wl.x0, wl.u_init)
    assert s.kernelName() == QUAD
    check_against_oracle(wl, s, ref)


@pytest.mark.parametrize("reg_type", [0, 1, 2])
def test_regularisation_types(reg_type):
    wl, ref = cartpole_case(17, 20, 31, 4, reg_type)
    s = make_solver(wl, max_iter=4, reg_type=reg_type)
    s.solve(wl.t0, wl.x0, wl.u_init)
    assert s.kernelName() == QUAD
    check_against_oracle(wl, s, ref)


def test_bipedal_two_states():
    """n = 2: rows and columns 2, 3 of every record block are padding.  T = 28: a 12-step guarded chunk, then a full one."""
    wl = workloads.bipedal_batch(B=17, T=28, seed=32)
    s = make_solver(wl, max_iter=3)
    s.solve(wl.t0, wl.x0, wl.u_init)
    assert s.kernelName() == QUAD
    check_against_oracle(wl, s, oracle_batch(wl, max_iter=3))


@pytest.mark.parametrize("running_u, T", [(-0.05, 100), (-0.001, 96)])
def test_failed_pivot_inside_an_unguarded_chunk(running_u, T):
    """The inputs of test_gpu_parity.py's pivot-failure test (a slightly negative input weight: Quu_F is not positive until lambda
    has grown, backward passes fail inside the straight-line chunks and are retried) at 17 instances.  Compared on the instances
    whose decisions the oracle itself keeps under rounding-level perturbations of x0, as there: the problem is not convex."""
    import nmpc_amd

    wl = workloads.cartpole_batch(B=17, T=T, seed=11)
    s = nmpc_amd.DDPSolverBatch(nmpc_amd.DDPProblemCartPole(running_u=[running_u]), wl.B)
    c = s.config()
    c.print_level, c.horizon_steps, c.max_iter = 0, wl.T, 3
    s.solve(wl.t0, wl.x0, wl.u_init)
    assert s.kernelName() == QUAD
    ocfg = oracle.default_config(horizon_steps=wl.T, max_iter=3)
    params = oracle.default_params("cartpole", running_u=running_u)
    ref = oracle.solve_batch("cartpole", ocfg, wl.x0, wl.u_init, params=params, n_threads=8, want_alpha_hist=True)
    keep = np.ones(wl.B, bool)
    rng = np.random.default_rng(3)
    for eps in (1e-15, 1e-14, 1e-13, 1e-12):
        r = oracle.solve_batch("cartpole", ocfg, wl.x0 * (1 + eps * rng.uniform(-1, 1, wl.x0.shape)), wl.u_init, params=params,
                               n_threads=8, want_alpha_hist=True)
        keep &= (r.iters == ref.iters) & (r.status == ref.status) & (r.alpha_idx_hist == ref.alpha_idx_hist).all(axis=1)
        keep &= (r.trace_last[:, INT_COLS] == ref.trace_last[:, INT_COLS]).all(axis=1)
    n_bw = ref.trace_last[:, 10]
    print(f"[running_u {running_u}, T {T}] decision-stable: {int(keep.sum())} / {wl.B}; n_backward of the last iteration: {n_bw.astype(int).tolist()}")
    assert n_bw.max() >= 2, "the workload no longer makes backward passes fail"
    assert keep.mean() >= 0.8
    check_against_oracle(wl, s, ref, mask=keep)


def test_failed_pivot_of_some_instances_of_a_wave():
    """Per-instance input weights of both signs (the inputs of test_gpu_parity.py's mixed test): in every wavefront some instances
    fail a pivot and their neighbours do not; the chunk is repeated guarded for all four."""
    import nmpc_amd

    wl = workloads.cartpole_batch(B=17, T=96, seed=12)
    weights = [(-0.05, -0.01, 0.01, 0.003, -0.001, 0.02, -0.02, 0.005)[b % 8] for b in range(wl.B)]
    s = make_solver(wl, max_iter=3)
    s.setProblemBatch([nmpc_amd.DDPProblemCartPole(running_u=[w]) for w in weights])
    s.solve(wl.t0, wl.x0, wl.u_init)
    assert s.kernelName() == QUAD
    ocfg = oracle.default_config(horizon_steps=wl.T, max_iter=3)
    X, U, st, it, tl = s.X(), s.U(), s.status(), s.iters(), s.traceLast()
    retried = clean = 0
    for b in range(wl.B):
        r = oracle.solve(wl.model, ocfg, wl.x0[b], wl.u_init[b], params=oracle.default_params("cartpole", running_u=weights[b]))
        assert st[b] == r.status and it[b] == r.iters
        np.testing.assert_array_equal(tl[b, list(INT_COLS)], r.trace[-1, list(INT_COLS)])
        assert scaled_err(X[b], r.X) <= TOL and scaled_err(U[b], r.U) <= TOL
        retried += int(r.trace[-1, 10] > 1)
        clean += int(r.trace[-1, 10] == 1)
    assert retried >= 4 and clean >= 4, (retried, clean)


def test_box_constrained_step_and_records():
    """+-15 N: the BoxQP step reads its relative limits from the record; retval and free set of every timestep, every instance."""
    wl = workloads.cartpole_batch(B=17, T=20, seed=33, constrained=True)
    s = make_solver(wl, max_iter=4, with_input_constraint=True)
    s.solve(wl.t0, wl.x0, wl.u_init)
    assert s.kernelName() == QUAD
    check_against_oracle(wl, s, oracle_batch(wl, max_iter=4, with_input_constraint=True))
    ocfg = oracle.default_config(horizon_steps=wl.T, max_iter=4, with_input_constraint=1)
    qret, qfree = s.qpRetval(), s.qpFreeMask()
    for b in range(wl.B):
        r = oracle.solve(wl.model, ocfg, wl.x0[b], wl.u_init[b], lower=wl.limits[0], upper=wl.limits[1])
        if r.status >= 0:
            np.testing.assert_array_equal(qret[b], r.qp_retval)
            np.testing.assert_array_equal(qfree[b], r.qp_free_mask)


def test_second_solve_on_a_handle_equals_a_fresh_handle():
    wl_a, _ = cartpole_case(17, 20, 34, 4)
    wl_b, ref_b = cartpole_case(17, 20, 35, 4)
    s = make_solver(wl_a, max_iter=4)
    s.solve(wl_a.t0, wl_a.x0, wl_a.u_init)
    s.solve(wl_b.t0, wl_b.x0, wl_b.u_init)
    fresh = make_solver(wl_b, max_iter=4)
    fresh.solve(wl_b.t0, wl_b.x0, wl_b.u_init)
    assert s.kernelName() == QUAD
    a, b = outputs(s), outputs(fresh)
    for f in FIELDS:
        assert np.array_equal(a[f], b[f], equal_nan=True), f
    check_against_oracle(wl_b, s, ref_b)


def test_resumable_launches_lay_the_record_constants():
    """The ragged schedule at max_iter 40: three resumable launches return the bits of the whole solve and the oracle's decisions."""
    wl = workloads.cartpole_batch(B=64, T=100, seed=36)
    whole = make_solver(wl, max_iter=40, ragged_schedule=-1)
    whole.solve(wl.t0, wl.x0, wl.u_init)
    s = make_solver(wl, max_iter=40, ragged_schedule=1)
    s.solve(wl.t0, wl.x0, wl.u_init)
    assert s.kernelName() == QUAD and whole.lastSolveLaunches() == 1 and s.lastSolveLaunches() == 3
    a, b = outputs(s), outputs(whole)
    for f in FIELDS:
        assert np.array_equal(a[f], b[f], equal_nan=True), f
    check_against_oracle(wl, s, oracle_batch(wl, max_iter=40))
