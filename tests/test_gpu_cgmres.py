"""The batched C/GMRES solver on the MI355X against the CPU checker (tests/cpp/cgmres_checker.cpp) and the bars of the reference's
tests (nmpc_cgmres/tests/src/TestGmres.cpp, TestCgmresSolver.cpp).

Tolerances: the device translation units are compiled without FMA contraction (nmpc_amd/build.py), so the kernels and the checker
perform the same IEEE operations in the same order; what differs is the math library — the device models use nmpc_amd::sincos
(<= 1.5 ulp) and the device exp, the checker the host's libm — so results agree to rounding, amplified by the finite differences
(1 / finite_diff_delta = 500) and the closed loop."""
import math

import numpy as np
import pytest

import cgmres_checker
from nmpc_amd import cgmres

pytestmark = pytest.mark.gpu

MODELS = ("cgmres_semiactive_damper", "cgmres_cartpole", "cgmres_cartpole_with_input_bound")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return cgmres_checker.build(tmp_path_factory.mktemp("cgmres_checker"))


def cfg_dict(solver):
    c = solver.config()
    return {n: getattr(c, n) for n, _ in cgmres.CConfig._fields_}


def perturbed(model, B, seed, scale=0.1):
    rng = np.random.default_rng(seed)
    x0, u0 = cgmres_checker.initial(model)
    return np.array(x0) + scale * rng.standard_normal((B, len(x0))), np.tile(u0, (B, 1))


def make(model, B, **kw):
    return cgmres.CgmresSolverBatch(cgmres.CgmresProblem(model), B, **kw)


@pytest.mark.parametrize("n", [10, 50, 100, 500])
def test_dense_gmres_meets_the_reference_bars(checker, n):
    """TestGmres.cpp:102-160 on the device: ten random systems per size; mean |Ax - b| < 1e-10 with full k_max, with and without
    re-orthogonalisation, and < 1e2 with k_max = 20.  Iteration counts equal the checker's."""
    rng = np.random.default_rng(100 + n)
    As = rng.uniform(-1, 1, (10, n, n))
    bs = rng.uniform(-1, 1, (10, n))
    for k_max, reorth, bar in ((1000, True, 1e-10), (1000, False, 1e-10), (20, True, 1e2)):
        x, it, ro = cgmres.dense_gmres(As, bs, k_max=k_max, apply_reorth=reorth)
        errs = np.linalg.norm(np.einsum("bij,bj->bi", As, x) - bs, axis=1)
        assert errs.mean() < bar, (n, k_max, reorth, errs.mean())
        for i in range(2):
            xc, itc, roc = checker.dense_gmres(As[i], bs[i], k_max=k_max, apply_reorth=reorth)
            assert it[i] == itc and ro[i] == roc
            if k_max == 20:
                assert np.abs(x[i] - xc).max() <= 1e-9 * (1 + np.abs(xc).max())


@pytest.mark.parametrize("model", MODELS)
def test_model_eval_matches_the_checker(checker, model):
    """The four problem functions at random points: relative to the size of each output component, <= 1e-13."""
    s = make(model, 4)
    nx, nuc = s.problem_.dim_x_, s.problem_.dim_uc_
    rng = np.random.default_rng(7)
    P = 2000
    t, x, u, lmd = rng.uniform(0, 5, P), rng.uniform(-3, 3, (P, nx)), rng.uniform(-2, 2, (P, nuc)), rng.uniform(-10, 10, (P, nx))
    params = [cgmres.CgmresProblem(model) for _ in range(4)]
    if model != "cgmres_semiactive_damper":
        for i, p in enumerate(params):
            p.p[14:18] = 0.1 * i  # per-instance reference states
    s.setProblem(params)
    got = s.modelEval(t, x, u, lmd)
    for i in range(4):
        sel = np.arange(i, P, 4)
        want = checker.model_eval(model, params[i].p, t[sel], x[sel], u[sel], lmd[sel])
        for g, w in zip(got, want):
            scale = 1.0 + np.abs(w).max(axis=0)
            assert (np.abs(g[sel] - w) / scale).max() <= 1e-13


@pytest.mark.parametrize("model", MODELS)
def test_setup_matches_the_checker(checker, model):
    B = 256
    s = make(model, B)
    x0, u0 = perturbed(model, B, 1)
    s.setInitial(x0, u0)
    s.setup()
    r = checker.solve(model, cfg_dict(s), x0, u0, run=False)
    st = s.status()
    assert np.array_equal(st, r.status)
    assert (st == cgmres.Status.Succeeded).mean() > 0.9
    ok = st == cgmres.Status.Succeeded
    assert (s.err()[ok] <= 1e-6).all() and (s.err()[~ok] > 1e-6).all()
    assert np.abs(s.u_list_ - r.U).max() <= 1e-10 * (1 + np.abs(r.U).max())
    assert np.array_equal(s.delta_u_vec_, np.zeros_like(s.delta_u_vec_))


@pytest.mark.parametrize("model", MODELS)
def test_one_second_closed_loop_matches_the_checker(checker, model):
    """1 s at dump_step = 1, Euler inside the horizon and RK4 for the simulation (the reference test's solvers), 256 perturbed
    initial states: every logged x and u within 1e-9 (1 + |.|) of the checker; GMRES iteration counts and re-orthogonalisation
    flags equal on >= 99.9 % of (instance, tick).

    The semi-active damper needs more room, and the device's exp() is the cause: the damper involves no sin / cos, and every other
    operation is correctly rounded on both sides, but the horizon length steady (1 - exp(-ratio t)) goes through exp, whose device
    and host results may differ by one ulp.  The checker against ITSELF with that exp nudged up by one ulp (std::nextafter) on these
    256 instances differs by up to 2.4e-9 in x, 4.5e-6 in u and 4.8e-8 in |DhDu| (the cart-poles: 1e-14, 1e-12, 1e-11); the device measured 1.4e-9 in x.
    So the damper's bars are 1e-8 in x and 1e-5 in u and |DhDu|; the cart-poles keep 1e-9 in x and u."""
    B = 256
    s = make(model, B, ode_solver="euler", sim_ode_solver="rk4")
    s.sim_duration_ = 1.0
    s.dump_step_ = 1
    x0, u0 = perturbed(model, B, 2)
    s.setInitial(x0, u0)
    s.run()
    r = checker.solve(model, cfg_dict(s), x0, u0)
    assert r.n_ticks == len(s.log_t()) == 1000  # (t += 1e-3 in fp64 passes 1.0 after 1000 ticks)
    assert np.array_equal(s.status(), r.status)
    damper = model == "cgmres_semiactive_damper"
    for got, want, bar in ((s.log_x(), r.log_x, 1e-8 if damper else 1e-9), (s.log_u(), r.log_u, 1e-5 if damper else 1e-9)):
        assert np.isfinite(want).all()
        assert (np.abs(got - want) / (1 + np.abs(want))).max() <= bar
    assert (s.log_iters() == r.log_iters).mean() >= 0.999
    assert (s.log_reorth() == r.log_reorth).mean() >= 0.999
    # |DhDu| is a residual: terms of the size of the weights (up to 300) cancel to ~1e-3, so the one-ulp differences of sin / cos
    # (nmpc_amd::sincos against the host's libm) that stay below 1e-9 in x and u show at a few 1e-9 in it (4.9e-9 measured)
    assert (np.abs(s.log_err() - r.log_err) / (1 + np.abs(r.log_err))).max() <= (1e-5 if damper else 1e-7)


@pytest.mark.parametrize("model", ["cgmres_semiactive_damper", "cgmres_cartpole_with_input_bound"])
def test_reference_scenario(checker, model):
    """TestCgmresSolver.cpp: 20 s, Euler inside the horizon, RK4 for the simulation, from x_initial_: every instance of a 1024 batch
    ends with |x| < 0.1, within 1e-6 of the checker."""
    B = 1024
    s = make(model, B, ode_solver="euler", sim_ode_solver="rk4")
    s.sim_duration_ = 20.0
    s.dump_step_ = 0
    s.run()
    x = s.x_
    assert (s.status() == cgmres.Status.Succeeded).all()
    assert (np.linalg.norm(x, axis=1) < 0.1).all(), np.linalg.norm(x, axis=1).max()
    x0, u0 = cgmres_checker.initial(model)
    r = checker.solve(model, cfg_dict(s), np.array([x0]), np.array([u0]))
    assert np.abs(x - r.x[0]).max() <= 1e-6


def test_instances_are_independent():
    """Instance i gives the same bits at B = 1, 64 and 4096, and with shared or per-instance problem objects."""
    model = "cgmres_cartpole_with_input_bound"
    x0, u0 = perturbed(model, 4096, 3)

    def run(B, per_instance=False, idx=None):
        s = make(model, B)
        s.sim_duration_ = 0.2
        s.dump_step_ = 1
        if per_instance:
            s.setProblem([cgmres.CgmresProblem(model) for _ in range(B)])
        sel = slice(0, B) if idx is None else [idx]
        s.setInitial(x0[sel], u0[sel])
        s.run()
        return s.log_x(), s.log_u(), s.u_list_

    big = run(4096)
    mid = run(64)
    per = run(64, per_instance=True)
    for a, b, c in zip(big, mid, per):
        assert np.array_equal(a[:64], b) and np.array_equal(b, c)
    for i in (0, 37, 4095):
        one = run(1, idx=i)
        for a, b in zip(big, one):
            assert np.array_equal(a[i], b[0])


def test_control_input_from_the_host_reproduces_run():
    """Ticking calcControlInput with run()'s own states as (x, next_x) gives run()'s inputs bit for bit, from host arrays and from
    device tensors."""
    import torch
    model = "cgmres_cartpole"
    B = 64
    x0, u0 = perturbed(model, B, 4)
    s = make(model, B, ode_solver="euler", sim_ode_solver="rk4")
    s.sim_duration_ = 0.1
    s.dump_step_ = 1
    s.setInitial(x0, u0)
    s.run()
    lx, lu, ts = s.log_x(), s.log_u(), s.log_t()
    for device_path in (False, True):
        c = make(model, B, ode_solver="euler", sim_ode_solver="rk4")
        with pytest.raises(RuntimeError):
            c.calcControlInput(0.0, x0, x0)  # before setup
        c.setInitial(x0, u0)
        c.setup()
        x = x0
        for i, t in enumerate(ts):
            if device_path:
                dev = torch.device("cuda:0")
                tt = torch.full((B,), float(t), dtype=torch.float64, device=dev)
                u_t = torch.zeros((B, c.problem_.dim_uc_), dtype=torch.float64, device=dev)
                c.calcControlInputDevice(tt, torch.from_numpy(np.ascontiguousarray(x)).to(dev),
                                         torch.from_numpy(np.ascontiguousarray(lx[:, i])).to(dev), u_t)
                c.synchronize()
                u = u_t.cpu().numpy()
            else:
                u = c.calcControlInput(t, x, lx[:, i])
            assert np.array_equal(u, lu[:, i]), (device_path, i)
            x = lx[:, i]
        assert np.array_equal(c.u_list_, s.u_list_)


def test_misuse_returns_errors():
    s = make("cgmres_cartpole", 8)
    s.k_max_ = 17
    with pytest.raises(ValueError):
        s.setup()
    s.k_max_ = 5
    with pytest.raises(ValueError):
        s.setProblem([cgmres.CgmresProblem("cgmres_cartpole")] * 3)
    s.config().horizon_divide_num = 30
    with pytest.raises(ValueError):
        s.setup()
    with pytest.raises(ValueError):
        cgmres.CgmresSolverBatch(cgmres.CgmresProblem("cgmres_cartpole"), 0)


def test_non_finite_instances_stop_with_a_status():
    """An instance whose initial state is NaN gets NON_FINITE and is left alone; its neighbours run as usual."""
    model = "cgmres_cartpole"
    x0, u0 = perturbed(model, 64, 5)
    x0[3, 1] = np.nan
    s = make(model, 64)
    s.sim_duration_ = 0.05
    s.setInitial(x0, u0)
    s.run()
    st = s.status()
    assert st[3] == cgmres.Status.NonFinite and (np.delete(st, 3) == cgmres.Status.Succeeded).all()
    assert np.isfinite(np.delete(s.x_, 3, axis=0)).all()


def test_dump_writes_the_reference_files(tmp_path):
    s = make("cgmres_semiactive_damper", 2)
    s.sim_duration_ = 0.05
    s.run()
    s.dump(1, str(tmp_path))
    x = np.genfromtxt(str(tmp_path / "cgmres_x.dat"), delimiter=",")
    assert x.shape == (len(s.log_t()), 3) and x.shape[0] >= 10 and abs(x[1, 0] - 0.005) < 1e-12
    assert np.allclose(x[:, 1:], s.log_x()[1], rtol=1e-5)
    err = np.genfromtxt(str(tmp_path / "cgmres_err.dat"), delimiter=",")
    assert err.shape == (x.shape[0], 2)
    assert '"log_dt": 0.005' in (tmp_path / "cgmres_param.dat").read_text()
    assert math.isclose(np.genfromtxt(str(tmp_path / "cgmres_u.dat"), delimiter=",")[0, 1], s.log_u()[1, 0, 0], rel_tol=1e-5)
