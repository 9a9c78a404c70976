"""BASELINE.json config 4 as specified — quadrotor (nx 12, nu 4, T 50) in fp32 on the fp32 tile kernel
(include/nmpc_amd/hip/ddp_kernels_tile32.hpp) AND on the tile kernel's float instantiation (ddp_kernels_tile64.hpp; every test runs
on both, the f32_kernel fixture) — against the CPU oracle instantiated in float (namespace oracle_f32,
oracle/ddp_oracle.hpp compiled with Real = float).

Bar (SURVEY.md §8 c, fp32 config): X, U within 1e-3 relative, total cost within 1e-4 relative, discrete decisions (status,
iteration count, step-size index of every iteration, backward / forward pass counts) EXACT on the margin-filtered set.
The margin filter is the oracle's own decision stability at fp32 resolution: an instance is kept iff the fp32 oracle takes
the same decisions when x0 is perturbed by a few float ulps.  Every masked comparison asserts a floor on the kept fraction
and checks the dropped instances for the same optimum.
"""
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

#: the kernel an UNCONSTRAINED quadrotor_f32 solve runs on when NMPC_HIP_DDP_KERNEL forces it: the fp32 tile kernel, or the fp64 tile
#: kernel's float instantiation (ddp_kernels_tile64.hpp with v_mfma_f32_16x16x4: round 4).  Unforced the choice is per launch
#: (ModelOpsFor::plan: the float instantiation below 8192 instances, and on full chips with a cost_update_thre >= 5e-4 —
#: test_fp32_kernel_dispatch).  Box-constrained solves and cartpole_f32 (n = 4) run on ddp_solve_tile32_kernel either way.
F32_KERNEL = {"tile32": "ddp_solve_tile32_kernel", "tile64": "ddp_solve_tile64_kernel"}


@pytest.fixture(autouse=True, params=["tile32", "tile64"], ids=["tile32", "tile64f"])
def f32_kernel(request, monkeypatch):
    """Every test of this file runs on both fp32 kernels."""
    monkeypatch.setenv("NMPC_HIP_DDP_KERNEL", request.param)
    return request.param


def test_fp32_kernel_dispatch(monkeypatch):
    """Which kernel an fp32 solve runs on when nothing forces it (model_registry.hpp, ModelOpsFor::plan, measured in
    profiles/r04_c4_dispatch_sweep.txt)."""
    import nmpc_amd

    monkeypatch.delenv("NMPC_HIP_DDP_KERNEL", raising=False)
    quad = nmpc_amd.make_problem("quadrotor_f32")
    for B, max_iter, thre, constrained, want in ((64, 2, 1e-7, False, "tile64"), (4096, 2, 1e-7, False, "tile64"), (8191, 1, 1e-3, False, "tile64"),
                                                 (8192, 2, 1e-3, False, "tile64"), (8192, 8, 5e-4, False, "tile64"), (8192, 8, 1e-4, False, "tile32"),
                                                 (8192, 8, 1e-7, False, "tile32"), (16384, 8, 1e-3, False, "tile64"), (16384, 3, 1e-5, False, "tile32"),
                                                 (256, 8, 1e-3, True, "tile32")):
        s = nmpc_amd.DDPSolverBatch(quad, B)
        s.config().max_iter = max_iter
        s.config().cost_update_thre = thre
        s.config().with_input_constraint = constrained
        assert s.kernelName() == f"ddp_solve_{want}_kernel", (B, max_iter, thre, constrained)
    s = nmpc_amd.DDPSolverBatch(nmpc_amd.make_problem("cartpole_f32"), 256)
    assert s.kernelName() == "ddp_solve_tile32_kernel"
    s = nmpc_amd.DDPSolverBatch(nmpc_amd.make_problem("manipulator_f32"), 256)
    assert s.kernelName() == "ddp_solve_tile64_kernel"


TOL_XU = 1e-3
TOL_COST = 1e-4
INT_COLS = (0, 9, 10, 11)
#: a termination threshold fp32 can resolve (cost 2 .. 40, one ulp ~ 1e-6): with the reference's default 1e-7 the float
#: algorithm keeps iterating on rounding noise and rejects steps at random
FP32_COST_UPDATE_THRE = 1e-3


def make(wl, **cfg):
    import nmpc_amd

    s = nmpc_amd.DDPSolverBatch(nmpc_amd.make_problem(wl.model, **wl.params), wl.B)
    c = s.config()
    c.print_level = 0
    c.horizon_steps = wl.T
    for k, v in cfg.items():
        setattr(c, k, v)
    if wl.limits is not None:
        s.setInputLimits(*wl.limits)
    return s


def ocfg_of(wl, **cfg):
    return oracle.default_config(horizon_steps=wl.T, **{k: (list(v) if k == "alpha_list" else v) for k, v in cfg.items()})


def _limits(wl):
    return dict(lower=wl.limits[0], upper=wl.limits[1]) if wl.limits is not None else {}


def oracle_f32(wl, x0=None, **cfg):
    params = oracle.default_params(wl.model, **wl.params) if wl.params else None
    return oracle.solve_batch(wl.model, ocfg_of(wl, **cfg), wl.x0 if x0 is None else x0, wl.u_init, t0=wl.t0, params=params,
                              n_threads=8, want_alpha_hist=True, **_limits(wl))


_NATIVE_DIR = None


def oracle_f32_contracted(wl, **cfg):
    """The same fp32 oracle built -O3 -march=native (the compiler fuses a * b + c into fma, as hipcc does on the GPU): a
    second, differently rounded evaluation of the same algorithm."""
    global _NATIVE_DIR
    import tempfile
    if _NATIVE_DIR is None:
        _NATIVE_DIR = tempfile.mkdtemp(prefix="oracle_native_")
    params = oracle.default_params(wl.model, **wl.params) if wl.params else None
    return oracle.solve_batch(wl.model, ocfg_of(wl, **cfg), wl.x0, wl.u_init, t0=wl.t0, params=params, n_threads=8,
                              want_alpha_hist=True, native=True, native_dir=_NATIVE_DIR, **_limits(wl))


def resolution_mask(wl, **cfg):
    """Instances in which every accept / reject decision of the line search (DDPSolver.hpp:251-264) was taken on a cost
    difference that a float cost can resolve: |cost_update_actual| >= 64 eps |cost| in every iteration of the fp32 oracle.
    Below that the sign of J - J' is rounding noise (three ulps of the cost decided the instances this filter was added for)."""
    keep = np.ones(wl.B, bool)
    params = oracle.default_params(wl.model, **wl.params) if wl.params else None
    for b in range(wl.B):
        r = oracle.solve(wl.model, ocfg_of(wl, **cfg), wl.x0[b], wl.u_init[b], t0=float(wl.t0[b]), params=params, **_limits(wl))
        rows = r.trace[1:]
        ls = rows[:, 9] >= 0
        keep[b] = bool(np.all(np.abs(rows[ls, 6]) >= 64 * 2.0 ** -24 * np.abs(rows[ls, 1])))
    return keep


def margin_mask(wl, ref, **cfg):
    """Instances whose decisions the fp32 oracle keeps under perturbations of x0 by 1 .. 128 float ulps (relative 6e-8 ..
    8e-6, the 1e-3-of-threshold margin of SURVEY.md §8 c seen from the inputs: the kernel sums in the matrix cores' order and
    associates the triple products differently from the oracle, a deviation of a few ulps per operation)."""
    rng = np.random.default_rng(2024)
    keep = np.ones(wl.B, bool)
    for ulps in (1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 128, 128):
        x0p = wl.x0 * (1 + ulps * 2.0 ** -24 * rng.uniform(-1, 1, wl.x0.shape))
        r = oracle_f32(wl, x0=x0p, **cfg)
        keep &= (r.iters == ref.iters) & (r.status == ref.status) & (r.alpha_idx_hist == ref.alpha_idx_hist).all(axis=1)
        keep &= np.all(r.trace_last[:, INT_COLS] == ref.trace_last[:, INT_COLS], axis=1)
    r = oracle_f32_contracted(wl, **cfg)  # ... and when a * b + c is fused
    keep &= (r.iters == ref.iters) & (r.status == ref.status) & (r.alpha_idx_hist == ref.alpha_idx_hist).all(axis=1)
    return keep & resolution_mask(wl, **cfg)


def rel(got, want):
    return np.abs(got - want) / (1.0 + np.abs(want))


def check(wl, s, ref, mask, floor, label):
    frac = float(mask.mean())
    print(f"[{label}] margin-filtered set: {int(mask.sum())} / {wl.B} instances ({frac:.3f}); floor {floor}")
    assert frac >= floor, f"{label}: only {frac:.3f} of the instances are decision-stable in the fp32 oracle itself"
    mk = mask
    np.testing.assert_array_equal(s.status()[mk], ref.status[mk])
    np.testing.assert_array_equal(s.iters()[mk], ref.iters[mk])
    tr = s.trace()
    hist = np.full_like(ref.alpha_idx_hist, -2)
    for b in range(wl.B):
        n = min(int(ref.iters[b]), int(s.iters()[b]))
        hist[b, :n] = tr[b, 1:n + 1, 9].astype(np.int32)
    bad = np.flatnonzero(mk & (hist != ref.alpha_idx_hist).any(axis=1))
    for b in bad[:4]:
        print(f"[{label}] kept instance {b}: step-size indices GPU {hist[b][:16]} oracle {ref.alpha_idx_hist[b][:16]}")
    np.testing.assert_array_equal(hist[mk], ref.alpha_idx_hist[mk])
    np.testing.assert_array_equal(s.traceLast()[mk][:, INT_COLS], ref.trace_last[mk][:, INT_COLS])
    ex, eu = rel(s.X(), ref.X).reshape(wl.B, -1).max(1), rel(s.U(), ref.U).reshape(wl.B, -1).max(1)
    Jg, Jr = s.cost().sum(axis=1), ref.cost.sum(axis=1)
    ej = np.abs(Jg - Jr) / np.abs(Jr)
    print(f"[{label}] kept set: max X err {ex[mk].max():.2e}, U {eu[mk].max():.2e}, cost {ej[mk].max():.2e}")
    assert ex[mk].max() <= TOL_XU and eu[mk].max() <= TOL_XU
    assert ej[mk].max() <= TOL_COST
    ok = mk & (ref.status >= 0)
    if ok.any():
        assert rel(s.kff()[ok], ref.k[ok]).max() <= 10 * TOL_XU
        assert rel(s.Kfb()[ok], ref.K[ok]).max() <= 10 * TOL_XU
    # the dropped instances: decisions may differ (the oracle's own do, a few ulps away), the optimum may not
    if (~mk).any():
        print(f"[{label}] dropped set: max cost err {ej[~mk].max():.2e}")
        assert ej[~mk].max() <= 50 * TOL_COST


def test_reports_fp32():
    import nmpc_amd

    assert nmpc_amd.make_problem("quadrotor_f32").scalar_bytes() == 4
    assert nmpc_amd.make_problem("quadrotor").scalar_bytes() == 8


def test_c4_first_iterations_ragged_batch():
    """Default Configuration, the first three iterations (before fp32 rounding noise decides anything), 500 instances =
    15 full workgroups of 32 + one of 20."""
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=500, T=50, seed=7, fp32=True)
    s = make(wl, max_iter=3)
    s.solve(wl.t0, wl.x0, wl.u_init)
    assert s.kernelName() == F32_KERNEL[os.environ["NMPC_HIP_DDP_KERNEL"]]
    ref = oracle_f32(wl, max_iter=3)
    check(wl, s, ref, margin_mask(wl, ref, max_iter=3), 0.97, "c4 3 iterations")  # the oracle keeps 0.988


def test_c4_to_convergence_with_fp32_tolerance():
    """Solve to convergence with a cost_update_thre float arithmetic can resolve: every instance converges."""
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=384, T=50, seed=11, fp32=True)
    cfg = dict(max_iter=60, cost_update_thre=FP32_COST_UPDATE_THRE)
    s = make(wl, **cfg)
    ok = s.solve(wl.t0, wl.x0, wl.u_init)
    ref = oracle_f32(wl, **cfg)
    assert (ref.status == 1).mean() > 0.99 and ok.mean() > 0.99
    check(wl, s, ref, margin_mask(wl, ref, **cfg), 0.95, "c4 converged")  # the oracle keeps 0.971


def test_c4_default_configuration_noise_regime_reaches_the_same_optimum():
    """The reference's default thresholds in fp32: once the cost decrease is below the resolution of a float the accept test
    (DDPSolver.hpp:251-264) is decided by rounding noise — in the fp32 ORACLE as well; most instances leave the
    margin-filtered set.  What must hold for all of them: the same optimum."""
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=256, T=50, seed=3, fp32=True)
    s = make(wl, max_iter=8)
    s.solve(wl.t0, wl.x0, wl.u_init)
    ref = oracle_f32(wl, max_iter=8)
    mask = margin_mask(wl, ref, max_iter=8)
    check(wl, s, ref, mask, 0.01, "c4 default thresholds, 8 iterations")  # the oracle keeps 0.02: that is the point
    Jg, Jr = s.cost().sum(axis=1), ref.cost.sum(axis=1)
    assert (np.abs(Jg - Jr) / np.abs(Jr)).max() <= 5e-4


@pytest.mark.parametrize("B,T,max_iter", [(1, 50, 3), (31, 7, 2), (33, 2, 1), (64, 1, 1), (5, 3, 1), (96, 49, 3)])
def test_shapes(B, T, max_iter):
    """Batches that are not a multiple of 32, horizons of one and two timesteps, odd horizons.  (Short horizons converge in
    one or two iterations; max_iter stops before the noise regime so that the whole batch stays in the kept set.)"""
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=B, T=T, seed=100 + B + T, fp32=True)
    s = make(wl, max_iter=max_iter)
    s.solve(wl.t0, wl.x0, wl.u_init)
    ref = oracle_f32(wl, max_iter=max_iter)
    check(wl, s, ref, margin_mask(wl, ref, max_iter=max_iter), 0.95, f"B {B} T {T}")


@pytest.mark.parametrize("cfg", [dict(reg_type=2), dict(reg_type=2, initial_lambda=1e-2),
                                 dict(alpha_list=[1.0, 0.3, 0.1]),
                                 dict(alpha_list=list(10.0 ** np.linspace(0, -3, 25))),  # 24 fan-out trials: two fan-out rounds
                                 dict(initial_lambda=1.0, lambda_factor=2.5)])
def test_configurations(cfg):
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=96, T=30, seed=21, fp32=True)
    full = dict(max_iter=3, **cfg)
    s = make(wl, **full)
    s.solve(wl.t0, wl.x0, wl.u_init)
    ref = oracle_f32(wl, **full)
    check(wl, s, ref, margin_mask(wl, ref, **full), 0.97, str(cfg)[:60])  # the oracle keeps 0.99 .. 1.0


def test_line_search_failure_and_lambda_limit():
    """No step size is ever accepted (ratio threshold 10): every iteration runs all 11 trials, lambda climbs past lambda_max
    and the solve ends with status -1 (DDPSolver.hpp:318-328) in the same iteration as in the oracle."""
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=64, T=20, seed=5, fp32=True)
    cfg = dict(max_iter=12, cost_update_ratio_thre=10.0, lambda_max=1.0)
    s = make(wl, **cfg)
    s.solve(wl.t0, wl.x0, wl.u_init)
    ref = oracle_f32(wl, **cfg)
    assert (ref.status == -1).all()
    np.testing.assert_array_equal(s.status(), ref.status)
    np.testing.assert_array_equal(s.iters(), ref.iters)
    np.testing.assert_array_equal(s.traceLast()[:, INT_COLS], ref.trace_last[:, INT_COLS])
    # nothing was accepted: the trajectory is still the initial rollout
    assert rel(s.X(), ref.X).max() <= 1e-5


def test_backward_pass_retries():
    """A negative input weight makes Quu indefinite: the factorisation fails, lambda is raised and the backward pass is
    repeated (DDPSolver.hpp:188-214); the number of backward passes per iteration must match the oracle's."""
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=64, T=20, seed=9, fp32=True)
    wl.params = dict(w_u=-0.05)
    cfg = dict(max_iter=3)
    s = make(wl, **cfg)
    s.solve(wl.t0, wl.x0, wl.u_init)
    ref = oracle_f32(wl, **cfg)
    assert ref.trace_last[:, 10].max() > 1 or (ref.status == -1).any(), "the case does not exercise the retry path"
    mask = margin_mask(wl, ref, **cfg)
    assert mask.mean() >= 0.8
    np.testing.assert_array_equal(s.status()[mask], ref.status[mask])
    np.testing.assert_array_equal(s.iters()[mask], ref.iters[mask])
    tr = s.trace()
    for b in np.flatnonzero(mask)[:16]:
        r1 = oracle.solve(wl.model, ocfg_of(wl, **cfg), wl.x0[b], wl.u_init[b], params=oracle.default_params(wl.model, **wl.params))
        n = r1.iters
        np.testing.assert_array_equal(tr[b, 1:n + 1, 10], r1.trace[1:n + 1, 10])  # n_backward of every iteration


def test_max_iter_zero_is_the_initial_rollout():
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=40, T=50, seed=2, fp32=True)
    s = make(wl, max_iter=0)
    ok = s.solve(wl.t0, wl.x0, wl.u_init)
    ref = oracle_f32(wl, max_iter=0)
    assert not ok.any() and (s.iters() == 0).all()
    assert rel(s.X(), ref.X).max() <= 1e-5 and rel(s.cost(), ref.cost).max() <= 1e-5
    np.testing.assert_allclose(s.U(), wl.u_init.astype(np.float32), rtol=0, atol=0)


def test_deterministic_and_handle_reuse():
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=200, T=50, seed=13, fp32=True)
    s = make(wl, max_iter=6)
    s.solve(wl.t0, wl.x0, wl.u_init)
    X1, U1, it1, tr1 = s.X().copy(), s.U().copy(), s.iters().copy(), s.trace().copy()
    wl2 = workloads.quadrotor_batch(B=200, T=50, seed=14, fp32=True)
    s.solve(wl2.t0, wl2.x0, wl2.u_init)
    s.solve(wl.t0, wl.x0, wl.u_init)
    np.testing.assert_array_equal(s.X(), X1)
    np.testing.assert_array_equal(s.U(), U1)
    np.testing.assert_array_equal(s.iters(), it1)
    np.testing.assert_array_equal(s.trace(), tr1)
    # rows beyond the last iteration of an instance are zero (traceDataList() ends there)
    tr = s.trace()
    for b in range(wl.B):
        assert not tr[b, int(it1[b]) + 1:].any()


def test_box_constrained_on_the_tile():
    """with_input_constraint on the fp32 tile kernel (ddp_solve_tile32_kernel<Problem, *, true>: BoxQP.h:141-347 in float on
    the instance's gain rows) against the fp32 oracle.

    What can be asked of it: BoxQP's own termination tests (relative improvement 1e-8, gradient norm 1e-8, BoxQP.h:42-45) are
    below float resolution, so the projected Newton iteration stops on rounding noise — the kernel and the float oracle end
    it one iteration apart on ~2 % of the timesteps (retval_ 4 against 5) with solutions up to 5e-4 apart where Quu has a flat
    direction.  From there on an input that sits AT its bound in one run can be just inside it in the other: a different
    free set, discontinuously different gains.  So: (A) one iteration from the same nominal — free sets, gains and the step
    agree; (B) at convergence — the same decisions on most of the batch, and the kernel is as close to the fp64 solution as
    the float oracle itself is."""
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=96, T=50, seed=31, constrained=True, fp32=True)
    # ---- (A) the first iteration
    cfg = dict(max_iter=1, with_input_constraint=True, cost_update_thre=FP32_COST_UPDATE_THRE)
    s = make(wl, **cfg)
    s.solve(wl.t0, wl.x0, wl.u_init)
    assert s.kernelName() == "ddp_solve_tile32_kernel"
    ref = oracle_f32(wl, **cfg)
    np.testing.assert_array_equal(s.status(), ref.status)
    np.testing.assert_array_equal(s.iters(), ref.iters)
    qret, qfree, k, K = s.qpRetval(), s.qpFreeMask(), s.kff(), s.Kfb()
    free_same, ret_same, clamped, n = 0, 0, 0, 0
    for b in range(0, wl.B, 2):
        r = oracle.solve(wl.model, ocfg_of(wl, **cfg), wl.x0[b], wl.u_init[b], t0=float(wl.t0[b]), **_limits(wl))
        n += wl.T
        free_same += int((qfree[b] == r.qp_free_mask).sum())
        ret_same += int((qret[b] == r.qp_retval).sum())
        clamped += int((r.qp_free_mask != 15).sum())
        assert set(np.unique(qret[b])) <= {4, 5, 6} and np.abs(k[b] - r.k).max() <= 5e-3
        assert (np.abs(K[b] - r.K) / (1 + np.abs(r.K))).max() <= 1e-3
    print(f"[c4 box] first iteration: identical free sets on {free_same} / {n} timesteps, retval_ on {ret_same} / {n}; "
          f"{clamped} timesteps with clamped inputs; max U err {np.abs(s.U() - ref.U).max():.2e}")
    assert free_same >= 0.99 * n and ret_same >= 0.9 * n and clamped > 0.2 * n
    assert rel(s.U(), ref.U).max() <= 5e-3 and rel(s.X(), ref.X).max() <= 5e-3
    # ---- (B) to convergence
    cfg = dict(max_iter=10, with_input_constraint=True, cost_update_thre=FP32_COST_UPDATE_THRE)
    s = make(wl, **cfg)
    s.solve(wl.t0, wl.x0, wl.u_init)
    ref = oracle_f32(wl, **cfg)
    ref64 = oracle.solve_batch("quadrotor", ocfg_of(wl, **cfg), wl.x0, wl.u_init, t0=wl.t0, n_threads=8, **_limits(wl))
    J64 = ref64.cost.sum(axis=1)
    e_gpu = np.abs(s.cost().sum(axis=1) - J64) / J64
    e_o32 = np.abs(ref.cost.sum(axis=1) - J64) / J64
    same = (s.status() == ref.status) & (s.iters() == ref.iters)
    print(f"[c4 box] to convergence: same status and iteration count as the float oracle on {same.mean():.3f}; final cost against "
          f"the fp64 oracle, kernel / float oracle: median {np.median(e_gpu):.1e} / {np.median(e_o32):.1e}, 90 % "
          f"{np.quantile(e_gpu, 0.9):.1e} / {np.quantile(e_o32, 0.9):.1e}, max {e_gpu.max():.1e} / {e_o32.max():.1e}")
    assert same.mean() >= 0.85
    assert np.median(e_gpu) <= 1e-5 and np.quantile(e_gpu, 0.9) <= max(1e-4, 2 * np.quantile(e_o32, 0.9))
    assert e_gpu.max() <= max(5e-2, 2 * e_o32.max())
    eu = rel(s.U()[same], ref.U[same]).reshape(int(same.sum()), -1).max(1)
    print(f"[c4 box] U against the float oracle where the decisions agree: median {np.median(eu):.1e}, 85 % {np.quantile(eu, 0.85):.1e}")
    assert np.median(eu) <= 1e-4 and np.quantile(eu, 0.85) <= TOL_XU  # (the typical instance is inside the fp32 bar)
    inside = lambda U: float(((U >= wl.limits[0] - 1e-3) & (U <= wl.limits[1] + 1e-3)).mean())  # noqa: E731  (the rollout is not clamped, :541-556)
    assert inside(s.U()) > 0.95 and abs(inside(s.U()) - inside(ref.U)) <= 0.01


def test_second_shape_cartpole_f32():
    """The fp32 tile kernel at its smallest shape — n = 4, m = 1 ("cartpole_f32", DDPProblemCartPoleT<float>; the quadrotor is
    n = 12, m = 4): decisions and trajectories against the float oracle on the margin-filtered set; box-constrained (m = 1
    BoxQP in float): free sets and gains after one iteration; plant-pattern receding-horizon loop (TestDDPCartPole.cpp:323-346)
    on the float handle bit-identical to the same loop driven from the host."""
    import nmpc_amd
    from nmpc_amd import workloads

    assert nmpc_amd.make_problem("cartpole_f32").scalar_bytes() == 4 and nmpc_amd.make_problem("cartpole_f32").dims()[:2] == (4, 1)
    wl = workloads.cartpole_batch(B=200, T=100, seed=17, fp32=True)
    cfg = dict(max_iter=4, cost_update_thre=FP32_COST_UPDATE_THRE)
    s = make(wl, **cfg)
    s.solve(wl.t0, wl.x0, wl.u_init)
    assert s.kernelName() == "ddp_solve_tile32_kernel"
    ref = oracle_f32(wl, **cfg)
    check(wl, s, ref, margin_mask(wl, ref, **cfg), 0.6, "cartpole_f32 4 iterations")
    # ---- +-15 N box, one iteration
    wb = workloads.cartpole_batch(B=96, T=100, seed=18, constrained=True, fp32=True)
    cfgb = dict(max_iter=1, with_input_constraint=True, cost_update_thre=FP32_COST_UPDATE_THRE)
    sb = make(wb, **cfgb)
    sb.solve(wb.t0, wb.x0, wb.u_init)
    refb = oracle_f32(wb, **cfgb)
    np.testing.assert_array_equal(sb.status(), refb.status)
    qfree, k = sb.qpFreeMask(), sb.kff()
    same, n, clamped = 0, 0, 0
    for b in range(0, wb.B, 3):
        r = oracle.solve(wb.model, ocfg_of(wb, **cfgb), wb.x0[b], wb.u_init[b], t0=float(wb.t0[b]), **_limits(wb))
        n += wb.T
        same += int((qfree[b] == r.qp_free_mask).sum())
        clamped += int((r.qp_free_mask == 0).sum())
        assert np.abs(k[b] - r.k).max() <= 5e-3 * (1 + np.abs(r.k).max())
    print(f"[cartpole_f32 box] identical free sets on {same} / {n} timesteps, {clamped} clamped")
    assert same >= 0.98 * n and clamped > 0
    assert rel(sb.U(), refb.U).max() <= 5e-3
    # ---- plant pattern on the device against the host-driven loop
    B, T, ticks = 48, 60, 6
    wm = workloads.cartpole_batch(B=B, T=T, seed=19, constrained=True, fp32=True)
    cfgm = dict(max_iter=3, with_input_constraint=True, cost_update_thre=FP32_COST_UPDATE_THRE)
    sm = make(wm, **cfgm)
    log = sm.mpcRun(0.0, wm.x0, np.zeros_like(wm.u_init), ticks, shift_warm_start=False, sim_substeps=2, sim_dt=0.002)
    assert np.isfinite(log.x).all() and (np.abs(log.u0) <= 15.0 + 1e-5).all()
    h = make(wm, **cfgm)
    x, u, t = wm.x0.astype(np.float32).astype(np.float64), np.zeros_like(wm.u_init), np.zeros(B)
    h.solve(t, x, u)
    np.testing.assert_array_equal(log.x[:, 0], x)
    np.testing.assert_array_equal(log.u0[:, 0], np.clip(h.U()[:, 0], -15.0, 15.0))
    np.testing.assert_array_equal(log.iters[:, 0], h.iters())


def test_unsupported_combinations_fail_loudly():
    """What the fp32 problem type does not offer raises instead of silently running something different."""
    import nmpc_amd
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=32, T=10, seed=1, fp32=True)
    assert nmpc_amd.make_problem("quadrotor_f32").dims()[:2] == (12, 4)
    s = make(wl, max_iter=2, with_input_constraint=True)  # with_input_constraint without limits: DDPSolver.h:282-285
    with pytest.raises(RuntimeError):
        s.solve(wl.t0, wl.x0, wl.u_init)


def test_manipulator_f32_on_the_float_tile64_kernel():
    """fp32 with seven inputs and n = 14 (the reference template takes any StateDim / InputDim, DDPSolver.h:23-25; the
    fp32 tile kernel takes m <= 4, n in {4, 8, 12}): `manipulator_f32` runs on the fp64 tile kernel's float instantiation, against
    the oracle instantiated in float at the bar of this file, full groups and ragged ones; box-constrained solves of the type are
    refused, not run on something else."""
    import nmpc_amd
    from nmpc_amd import workloads

    wl = workloads.manipulator_batch(B=200, T=30, seed=13, fp32=True)
    # two iterations: from the third on the manipulator's cost differences are below 64 eps of the cost — the fp32 oracle itself
    # keeps 2 % of its decisions under ulp perturbations there (resolution_mask), 100 % up to the second
    cfg = dict(max_iter=2, cost_update_thre=FP32_COST_UPDATE_THRE)
    by_group = []
    for group in ("32", "7"):
        os.environ["NMPC_HIP_DDP_TILE64_GROUP"] = group
        try:
            s = make(wl, **cfg)
            assert s.kernelName() == "ddp_solve_tile64_kernel" and nmpc_amd.make_problem("manipulator_f32").scalar_bytes() == 4
            s.solve(wl.t0, wl.x0, wl.u_init)
        finally:
            os.environ.pop("NMPC_HIP_DDP_TILE64_GROUP")
        ref = oracle_f32(wl, **cfg)
        check(wl, s, ref, margin_mask(wl, ref, **cfg), 0.97, f"manipulator_f32 group {group}")
        by_group.append((s.X().copy(), s.U().copy(), s.Kfb().copy()))
    # the results do not depend on how the batch is cut into groups — bit for bit (the functors' code exists once per role in
    # the kernel: two copies of the linearisation once differed in their fused multiply-adds, in float only)
    assert all(np.array_equal(a, b) for a, b in zip(*by_group))
    os.environ["NMPC_HIP_DDP_TILE64_GROUP"] = "7"
    s = make(wl, **cfg)
    os.environ.pop("NMPC_HIP_DDP_TILE64_GROUP")
    s.solve(wl.t0, wl.x0, wl.u_init)
    X1 = s.X().copy()
    s.solve(wl.t0, wl.x0, wl.u_init)
    np.testing.assert_array_equal(s.X(), X1)
    # to convergence: decisions in the noise regime are not comparable, the optimum is — final costs within the tolerance of the
    # float oracle's, and of the fp64 oracle's
    sc = make(wl, max_iter=8, cost_update_thre=FP32_COST_UPDATE_THRE)
    sc.solve(wl.t0, wl.x0, wl.u_init)
    rf = oracle_f32(wl, max_iter=8, cost_update_thre=FP32_COST_UPDATE_THRE)
    r64 = oracle.solve_batch("manipulator", ocfg_of(wl, max_iter=8), wl.x0, wl.u_init, t0=wl.t0, n_threads=8)
    Jg, Jf, J64 = sc.cost().sum(axis=1), rf.cost.sum(axis=1), r64.cost.sum(axis=1)
    assert (sc.status() >= 0).all()
    assert np.max(np.abs(Jg - Jf) / np.abs(Jf)) <= 50 * TOL_COST and np.max(np.abs(Jg - J64) / np.abs(J64)) <= 50 * TOL_COST
    sb = make(wl, max_iter=2, with_input_constraint=True)
    sb.setInputLimits(np.full(7, -3.0), np.full(7, 3.0))
    with pytest.raises(RuntimeError):
        sb.solve(wl.t0, wl.x0, wl.u_init)


def test_per_instance_problem_objects():
    """nmpc_hip_ddp_set_model_params_batch on the fp32 tile kernel (ddp_solve_tile32_kernel<Problem, true>): every instance
    solves its own quadrotor (mass), instance by instance against the fp32 oracle with the same parameters; then back to the
    shared object."""
    import nmpc_amd
    from nmpc_amd import workloads

    rng = np.random.default_rng(56)
    wl = workloads.quadrotor_batch(B=45, T=50, seed=8, fp32=True)
    cfg = dict(max_iter=6, cost_update_thre=FP32_COST_UPDATE_THRE)
    masses = rng.uniform(0.8, 1.3, wl.B)
    s = make(wl, **cfg)
    s.setProblemBatch([nmpc_amd.make_problem("quadrotor_f32", mass=float(m)) for m in masses])
    s.solve(wl.t0, wl.x0, wl.u_init)
    assert s.kernelName() == F32_KERNEL[os.environ["NMPC_HIP_DDP_KERNEL"]]
    X, U, st, it = s.X(), s.U(), s.status(), s.iters()
    ocfg = ocfg_of(wl, **cfg)
    same, differs = 0, 0
    for b in range(wl.B):
        r = oracle.solve(wl.model, ocfg, wl.x0[b], wl.u_init[b], params=oracle.default_params(wl.model, mass=float(masses[b])))
        r_shared = oracle.solve(wl.model, ocfg, wl.x0[b], wl.u_init[b])
        differs += int(np.abs(r_shared.U - r.U).max() > 1e-2)
        if st[b] == r.status and it[b] == r.iters:  # (decisions at fp32 resolution: the margin filter's subject, not this test's)
            same += 1
            assert rel(X[b], r.X).max() <= TOL_XU and rel(U[b], r.U).max() <= TOL_XU
        else:
            Jg, Jr = s.cost()[b].sum(), r.cost.sum()
            assert abs(Jg - Jr) / abs(Jr) <= 50 * TOL_COST
    assert differs > wl.B // 2, "the per-instance parameters do not change the solutions"
    assert same >= int(0.8 * wl.B)
    s.setProblemBatch(None)
    s.solve(wl.t0, wl.x0, wl.u_init)
    ref = oracle_f32(wl, **cfg)
    ok = (s.status() == ref.status) & (s.iters() == ref.iters)
    assert ok.mean() >= 0.8 and rel(s.X()[ok], ref.X[ok]).max() <= TOL_XU


def test_receding_horizon_driver():
    """nmpc_hip_ddp_mpc_run on an fp32 handle (mpc_advance_kernel<Problem, float>, shift pattern): the device-resident loop
    equals the same loop driven from the host solve by solve BIT FOR BIT (the same kernel on the same float data), and follows
    the fp64 oracle's closed loop within the fp32 tolerance."""
    import nmpc_amd
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=40, T=50, seed=5, fp32=True)
    ticks = 8
    cfg = dict(max_iter=5, cost_update_thre=FP32_COST_UPDATE_THRE)
    s = make(wl, **cfg)
    log = s.mpcRun(0.0, wl.x0, np.zeros_like(wl.u_init), ticks, shift_warm_start=True)
    h = make(wl, **cfg)
    x, u, t = wl.x0.astype(np.float32).astype(np.float64), np.zeros_like(wl.u_init), np.zeros(wl.B)
    for k in range(ticks):
        h.solve(t, x, u)
        X, U = h.X(), h.U()
        np.testing.assert_array_equal(log.x[:, k], x)
        np.testing.assert_array_equal(log.u0[:, k], U[:, 0])
        np.testing.assert_array_equal(log.iters[:, k], h.iters())
        x = X[:, 1].copy()
        u = np.concatenate([U[:, 1:], U[:, -1:]], axis=1)
        t = t + np.float64(np.float32(wl.dt))  # current_t advances in double by the problem's (float) dt; rounded at ingest
    t_expected = np.concatenate([[0.0], np.cumsum(np.full(ticks - 1, np.float64(np.float32(wl.dt))))])  # (sequential additions)
    np.testing.assert_array_equal(log.t, np.broadcast_to(t_expected, (wl.B, ticks)))
    ocfg = oracle.default_config(horizon_steps=wl.T, max_iter=5, cost_update_thre=FP32_COST_UPDATE_THRE)
    for b in (0, 17, 39):
        r = oracle.mpc_run("quadrotor", ocfg, wl.x0[b], ticks, shift_warm_start=True)
        assert rel(log.x[b], r.x).max() <= 5 * TOL_XU and rel(log.u0[b], r.u0).max() <= 20 * TOL_XU


def test_full_size_c4_properties():
    """BASELINE.json's size (8192 instances): size-independent properties instead of an oracle run — costs decrease
    monotonically over accepted iterations, the stored trajectory is a rollout of the stored inputs (re-simulated by the fp32
    oracle's model), and two solves agree bit for bit."""
    from nmpc_amd import workloads

    wl = workloads.quadrotor_batch(B=8192, T=50, seed=1234, fp32=True)
    s = make(wl, max_iter=8)
    s.solve(wl.t0, wl.x0, wl.u_init)
    X, U, tr, it = s.X(), s.U(), s.trace(), s.iters()
    assert np.isfinite(X).all() and np.isfinite(U).all()
    cost = tr[:, :, 1]
    for b in range(0, wl.B, 37):
        c = cost[b, :it[b] + 1]
        c = c[c != 0]  # rows of iterations that terminated before the line search carry no cost
        assert np.all(np.diff(c) <= 1e-5 * np.abs(c[:-1]))
    # x_{i+1} = stateEq(x_i, u_i) along the stored solution, checked with the oracle's float model on a sample
    for b in range(0, wl.B, 911):
        for i in (0, 17, 49):
            ev = oracle.model_eval(wl.model, None, 0.0, X[b, i], U[b, i])
            assert rel(ev.xn, X[b, i + 1]).max() <= 2e-6
    X1 = X.copy()
    s.solve(wl.t0, wl.x0, wl.u_init)
    np.testing.assert_array_equal(s.X(), X1)
