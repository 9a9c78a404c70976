"""Parity of the HIP FMPC path (nmpc_amd.fmpc over the C-ABI of include/nmpc_hip_fmpc.h) with the CPU oracle (oracle/fmpc_oracle.hpp,
a restatement of the reference's nmpc_fmpc::FmpcSolver), SURVEY.md §8 f-4.

Bar: the discrete results (Status, iteration count) are equal; every floating-point result agrees within the tolerance written
at the comparison (fp64 on both sides; the device contracts a * b + c into FMAs and sums the horizon in slices, the oracle does
neither, so agreement is to rounding, amplified by the conditioning of the interior-point iteration — not bit-exact)."""
import numpy as np
import pytest

from nmpc_amd import fmpc as F
from oracle import fmpc as O

pytestmark = pytest.mark.gpu

MODELS = {"fmpc_oscillator": F.FmpcProblemOscillator, "fmpc_cartpole": F.FmpcProblemCartPole,
          "fmpc_pointmass": F.FmpcProblemPointMass}


def make_case(model, B, T, seed, spread=0.3):
    n, m, g, _ = O.model_info(model)
    rng = np.random.default_rng(seed)
    var = F.Variable(spread * rng.standard_normal((B, T + 1, n)), spread * rng.standard_normal((B, T, m)),
                     spread * rng.standard_normal((B, T + 1, n)), rng.uniform(0.5, 2.0, (B, T, g)),
                     rng.uniform(0.5, 2.0, (B, T, g)))
    x0 = spread * rng.standard_normal((B, n))
    t0 = rng.uniform(0, 1, B)
    return var, x0, t0


def oracle_cfg(cfg: F.Configuration):
    return O.default_config(**{k: getattr(cfg, k) for k in F.Configuration._FIELDS if k not in ("use_graph", "time_kernels")})


def oracle_batch(model, cfg, params, t0, x0, var, barrier_eps=None):
    return O.solve_batch(model, oracle_cfg(cfg), params, t0, x0, O.Variable(*var.arrays()), barrier_eps=barrier_eps, n_threads=4)


def assert_close(a, b, rtol, atol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(a)
    err = np.abs(a[ok] - b[ok])
    bound = atol + rtol * np.maximum(np.abs(a[ok]), np.abs(b[ok]))
    assert np.all(err <= bound), (what, float(np.max(err - bound)))


def compare(solver, ref, rtol=1e-8, atol=1e-10, min_stable=0.9):
    """Instances whose iteration diverges in the oracle (KKT error beyond 1e4: random starts far from a solution can do that,
    the reference has no globalisation unless enable_line_search is on) amplify rounding differences without bound; they are
    required to diverge on the device too and are left out of the value comparison."""
    stable = ref.trace[:, :, 1].max(axis=1) < 1e4
    assert stable.mean() >= min_stable, stable.mean()
    tr = solver.traceDataList()
    assert (np.nan_to_num(tr[~stable, :, 1], nan=np.inf).max(axis=1) > 1e3).all()
    st, it = solver.status(), solver.iters()
    assert np.array_equal(st[stable], ref.status[stable]), (st[:16], ref.status[:16])
    assert np.array_equal(it[stable], ref.iters[stable])
    assert np.array_equal(tr[stable, :, 0], ref.trace[stable, :, 0])
    for col, name in enumerate(F.TRACE_COLUMNS[1:], start=1):
        assert_close(tr[stable, :, col], ref.trace[stable, :, col], rtol, atol, name)
    v = solver.variable()
    for name, a, c in zip(("x", "u", "lambda", "s", "nu"), v.arrays(), ref.variable.arrays()):
        assert_close(a[stable], c[stable], rtol, atol, name)
    assert_close(solver.barrierEps()[stable], ref.barrier_eps[stable], rtol, atol, "barrier_eps")
    return v


@pytest.mark.parametrize("riccati", ["fused", "quad", "lane"])
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("B,T,max_iter", [(130, 30, 1), (70, 57, 4), (64, 8, 10)])
def test_solve_matches_oracle(model, B, T, max_iter, riccati, monkeypatch):
    """The three Riccati kernels: sixteen lanes per instance on the matrix cores with the coefficient records computed by a producer
    wave into the staging LDS ("fused": n <= 4, one input: the default for the oscillator and the cart-pole), the same with the records
    read back from HBM ("quad"), and one lane per instance (everything else; forced here through NMPC_HIP_FMPC_RICCATI, which is read
    when the handle is created)."""
    if model == "fmpc_pointmass" and riccati != "fused":
        pytest.skip("two inputs: the lane kernel is what runs anyway")
    monkeypatch.setenv("NMPC_HIP_FMPC_RICCATI", riccati)
    prob = MODELS[model]()
    var, x0, t0 = make_case(model, B, T, seed=B + T)
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = max_iter
    st = s.solve(t0, x0, var)
    want = {"fused": "fmpc_riccati_fused_kernel", "quad": "fmpc_riccati_quad_kernel", "lane": "fmpc_riccati_kernel"}[riccati]
    assert ("fmpc_riccati_kernel" if model == "fmpc_pointmass" else want) in s.kernelNames()
    ref = oracle_batch(model, s.config(), prob.p, t0, x0, var)
    # the Van der Pol problem over a short horizon diverges from about 40 % of these random starts (in the oracle just as on the
    # device); every other case converges for all instances
    compare(s, ref, min_stable=0.5 if (model == "fmpc_oscillator" and max_iter == 10) else 1.0)
    assert set(np.unique(st)) <= {1, 5}
    # gains of the last backward pass and the step it produced, against the single-instance entry of the oracle
    cl = s.coeffList()
    dv = s.deltaVariable()
    for b in (0, B - 1):
        r1 = O.solve(model, oracle_cfg(s.config()), prob.p, t0[b], x0[b], O.Variable(*(a[b] for a in var.arrays())))
        if (r1.status == 1 and r1.iters == 1) or r1.trace[:, 1].max() >= 1e4:
            continue
        for name, a, c in (("k", cl["k"][b], r1.k), ("K", cl["K"][b], r1.K), ("s", cl["s"][b], r1.s), ("P", cl["P"][b], r1.P)):
            assert_close(a, c, 1e-8, 1e-10, name)
        if r1.status == 5:  # the last iteration ran a forward pass
            for name, a, c in zip(("dx", "du", "dlambda", "ds", "dnu"), (v[b] for v in dv.arrays()), r1.delta.arrays()):
                assert_close(a, c, 1e-7, 1e-9, name)


def test_graph_replay_equals_stream_launches_and_is_deterministic():
    model = "fmpc_cartpole"
    prob = MODELS[model]()
    B, T = 200, 40
    var, x0, t0 = make_case(model, B, T, seed=7)
    results = []
    for use_graph in (True, False, True):
        s = F.FmpcSolverBatch(prob, B, T)
        s.config().max_iter = 5
        s.config().use_graph = use_graph
        s.solve(t0, x0, var)
        s.solve(t0 + 0.01, x0, None)  # second solve from the resident variable: the graph is replayed
        results.append((s.status(), s.iters(), s.traceDataList(), *s.variable().arrays()))
    for r in results[1:]:
        for a, c in zip(results[0], r):
            assert np.array_equal(a, c)


@pytest.mark.parametrize("opts", [
    dict(init_complementary_variable=True),
    dict(update_barrier_eps=False),
    dict(enable_line_search=True),
    dict(enable_line_search=True, merit_const_scale_from_lagrange_multipliers=True),
    dict(check_nan=False, break_if_llt_fails=True),
])
@pytest.mark.parametrize("model", ["fmpc_cartpole", "fmpc_pointmass"])
def test_configuration_switches_match_oracle(model, opts):
    prob = MODELS[model]()
    B, T = 96, 25
    var, x0, t0 = make_case(model, B, T, seed=11, spread=0.2)
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = 4
    for k, v in opts.items():
        setattr(s.config(), k, v)
    be = np.linspace(1e-4, 1e-1, B)
    s.setVariable(var, barrier_eps=be)
    s.solve(t0, x0)
    ref = oracle_batch(model, s.config(), prob.p, t0, x0, var, barrier_eps=be)
    compare(s, ref, rtol=1e-7, atol=1e-9)
    if opts.get("enable_line_search"):
        tr = s.traceDataList()
        assert (tr[:, :, 5] <= tr[:, :, 3] + 1e-15).all()  # alpha_s <= alpha_s_max
        m = s.meritFunc()
        r1 = O.solve(model, oracle_cfg(s.config()), prob.p, t0[3], x0[3], O.Variable(*(a[3] for a in var.arrays())), be[3])
        assert np.isfinite(m).all() and r1.status == s.status()[3]


def test_statuses_succeeded_error_and_invalid_variable():
    """Per-instance termination: an instance at the solution returns Succeeded in the first iteration, a NaN current state gives
    ErrorInForward and a NaN in the variable ErrorInBackward (check_nan, FmpcSolver.hpp:640-653,699-706), the rest of the batch runs to MaxIterationReached; a negative slack is
    checkVariable's std::runtime_error (FmpcSolver.hpp:338-353)."""
    model = "fmpc_oscillator"
    prob = MODELS[model]()
    B, T = 66, 20
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = 3
    var = F.Variable.make(prob, T, B)
    var.reset(0.0, 0.0, 0.0, 1.0, 1.0)
    x0 = np.tile([0.0, 1.0], (B, 1))
    # instance 5: converged point of a long run of the oracle, as initial guess
    cfg_long = O.default_config(horizon_steps=T, max_iter=60)
    r = O.solve(model, cfg_long, prob.p, 0.0, x0[5], O.Variable.reset(model, T))
    assert r.status == 1
    for a, c in zip(var.arrays(), r.variable.arrays()):
        a[5] = c
    be = np.full(B, 1e-4)
    be[5] = r.barrier_eps
    x0[9, 0] = np.nan  # enters through delta_x[0] = current_x - x_list[0]: forward pass (FmpcSolver.hpp:669,699-706)
    var.x_list[10, 3, 0] = np.nan  # enters through the coefficients: backward pass (:640-653)
    s.setVariable(var, barrier_eps=be)
    st = s.solve(0.0, x0)
    ref = oracle_batch(model, s.config(), prob.p, np.zeros(B), x0, var, barrier_eps=be)
    assert st[5] == 1 and st[9] == 2 and st[10] == 3 and (np.delete(st, [5, 9, 10]) == 5).all()
    assert np.array_equal(st, ref.status) and np.array_equal(s.iters(), ref.iters)
    assert s.iters()[5] == 1 and s.iters()[9] == 1 and s.iters()[10] == 1
    v = s.variable()
    assert np.array_equal(v.x_list[5], var.x_list[5])  # untouched: Succeeded before any update
    keep = np.delete(np.arange(B), [9, 10])
    for a, c in zip(v.arrays(), ref.variable.arrays()):
        assert_close(a[keep], c[keep], 1e-8, 1e-10, "variable")
    # checkVariable
    var.s_list[17, 3, 1] = -1e-3
    s.setVariable(var)
    with pytest.raises(RuntimeError, match="non-negative"):
        s.solve(0.0, x0)
    st = s.status()
    assert st[17] == F.STATUS_INVALID_VARIABLE and st[5] == 1 and st[0] == 5
    # sequence lengths: std::invalid_argument (FmpcSolver.hpp:287-311)
    bad = F.Variable.make(prob, T + 1, B)
    with pytest.raises(ValueError, match="length should be"):
        s.solve(0.0, x0, bad)


def test_per_instance_problem_objects():
    model = "fmpc_cartpole"
    B, T = 80, 30
    probs = []
    rng = np.random.default_rng(3)
    for b in range(B):
        p = F.FmpcProblemCartPole(0.02, ref_pos=float(rng.uniform(-2, 2)))
        p.p[1] = rng.uniform(0.8, 1.5)  # cart mass
        p.p[14] = rng.uniform(5.0, 20.0)  # u_max
        probs.append(p)
    var, x0, t0 = make_case(model, B, T, seed=5, spread=0.2)
    s = F.FmpcSolverBatch(probs[0], B, T)
    s.setProblem(probs, per_instance=True)
    s.config().max_iter = 5
    s.solve(t0, x0, var)
    ref = oracle_batch(model, s.config(), np.stack([p.p for p in probs]), t0, x0, var)
    compare(s, ref)
    bad = [F.FmpcProblemCartPole(0.02) for _ in range(B)]
    bad[3].p[0] = 0.03
    with pytest.raises(ValueError, match="dt"):
        s.setProblem(bad, per_instance=True)


def oscillator_plant(x, u, dt):
    return np.stack([x[:, 0] + dt * ((1.0 - x[:, 1] ** 2) * x[:, 0] - x[:, 1] + u[:, 0]), x[:, 1] + dt * x[:, 0]], axis=1)


def test_oscillator_closed_loop_reference_bounds_and_oracle_trajectory():
    """TestFmpcOscillator.cpp:137-205 for a batch: the reference's initial state in instance 0, perturbed ones elsewhere."""
    model = "fmpc_oscillator"
    horizon_dt, T = 0.01, 400
    prob = F.FmpcProblemOscillator(horizon_dt)
    B = 64
    rng = np.random.default_rng(0)
    x0 = np.tile([0.0, 1.0], (B, 1)) + np.concatenate([np.zeros((1, 2)), 0.2 * rng.standard_normal((B - 1, 2))])
    x0[:, 1] = np.maximum(x0[:, 1], 0.2)
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = 3
    var = F.Variable.make(prob, T, B)
    var.reset(0.0, 0.0, 0.0, 1e0, 1e0)
    s.setVariable(var)
    sim_dt, n_ticks = 0.005, 2000
    log = s.mpcRun(0.0, x0, n_ticks, sim_dt)
    assert np.isin(log["status"], (1, 5)).all()  # :173
    u0 = log["u0"][:, :, 0]
    g = np.stack([-log["x"][:, :, 1] - 0.05, -u0 - 1.0, u0 - 0.9], axis=-1)
    assert (g[0] <= 0).all()  # :181-183 for the reference's own start
    assert (g[:, 100:] <= 1e-9).all() and (g[:, :, 1:] <= 1e-9).all()  # perturbed starts may begin outside x1 >= -0.05
    assert (np.abs(log["x_final"]) < 1e-2).all()  # :197-198
    assert np.allclose(log["t_final"], n_ticks * sim_dt)
    # the test's result table (TestFmpcOscillator.cpp:168,186-188), readable the way the reference's users read theirs
    import os
    import tempfile

    from nmpc_amd import result_tables as RT
    path = os.path.join(tempfile.mkdtemp(), "TestFmpcOscillatorResult.txt")
    RT.write_table(path, RT.fmpc_ticks(log, 0, 0.0, sim_dt), RT.fmpc_oscillator_table())
    tab = np.genfromtxt(path, names=True)
    assert tab.dtype.names == ("time", "x0", "x1", "u0", "mpc_iter", "computation_time", "kkt_error")  # genfromtxt drops [ ]
    assert len(tab) == n_ticks and np.allclose(tab["x1"], log["x"][0, :, 1], rtol=1e-5, atol=1e-9) and tab["mpc_iter"].max() <= 3
    # the same loop through the oracle for two instances
    for b in (0, 17):
        cfg = O.default_config(horizon_steps=T, max_iter=3)
        v = O.Variable.reset(model, T)
        x, t, be = x0[b].copy(), 0.0, 1e-4
        for k in range(n_ticks):
            assert np.allclose(x, log["x"][b, k], rtol=0, atol=1e-7), (b, k)
            r = O.solve(model, cfg, prob.p, t, x, v, be)
            assert r.status == log["status"][b, k] and r.iters == log["iters"][b, k], (b, k)
            assert abs(r.variable.u[0, 0] - log["u0"][b, k, 0]) < 1e-7
            be, v = r.barrier_eps, r.variable
            x = oscillator_plant(x[None], r.variable.u[0][None], sim_dt)[0]
            t += sim_dt


def test_cartpole_closed_loop_reference_bounds():
    """TestFmpcCartPole.cpp:318-384 for a batch (nominal timer schedule: one solve per two 2 ms plant steps, K_0 feedback in
    between): swing-up from the hanging position, perturbed in the other instances."""
    horizon_dt, T = 0.01, 200
    prob = F.FmpcProblemCartPole(horizon_dt)
    B = 48
    rng = np.random.default_rng(1)
    x0 = np.tile([0.0, np.pi, 0.0, 0.0], (B, 1))
    x0[1:] += 0.05 * rng.standard_normal((B - 1, 4))
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = 5
    var = F.Variable.make(prob, T, B)
    var.reset(0.0, 0.0, 0.0, 1e0, 1e0)
    s.setVariable(var)
    log = s.mpcRun(0.0, x0, 2500, 0.002, sim_substeps=2, use_feedback=True)
    assert np.isin(log["status"], (1, 5)).all()
    assert (np.abs(log["x"][:, :, 0]) < 1e2).all()  # :362
    xf = log["x_final"]
    assert (np.abs(xf[:, 0]) < 1.0).all() and (np.abs(xf[:, 1]) < 1e-1).all()  # :377-380
    assert (np.abs(xf[:, 2]) < 1.0).all() and (np.abs(xf[:, 3]) < 1e-1).all()
    assert (np.abs(log["u0"]) <= 15.0).all()  # the force limit of ineqConst (:122-127) holds on every applied u_list[0]
    # instance 0 against the oracle's loop (tests/test_fmpc_oracle_pins.py runs the same schedule)
    model = "fmpc_cartpole"
    cfg = O.default_config(horizon_steps=T, max_iter=5)
    v = O.Variable.reset(model, T)
    x, t, be = x0[0].copy(), 0.0, 1e-4
    for k in range(400):  # the swing-up is sensitive: compare the first 1.6 s tightly
        assert np.allclose(x, log["x"][0, k], rtol=0, atol=1e-6), k
        r = O.solve(model, cfg, prob.p, t, x, v, be)
        assert r.status == log["status"][0, k] and r.iters == log["iters"][0, k]
        be, v = r.barrier_eps, r.variable
        for _ in range(2):
            u = r.variable.u[0] + r.K[0] @ (r.variable.x[0] - x)
            x = O.evaluate(model, prob.p, t, x, u, step_dt=0.002)["f"]
            t += 0.002


def test_full_size_batch_properties():
    """B = 4096, T = 200 (the bench workload): too large for the oracle in a test; size-independent properties instead — the
    KKT error falls monotonically over the iterations from a feasible start, slacks and multipliers stay positive, s matches
    -g at the solution, and a shard of the batch solved alone gives bit-identical results (instances are independent)."""
    prob = F.FmpcProblemCartPole(0.01)
    B, T = 4096, 200
    rng = np.random.default_rng(2)
    x0 = np.zeros((B, 4))
    x0[:, 0] = rng.uniform(-1, 1, B)
    x0[:, 1] = rng.uniform(-0.3, 0.3, B)
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = 8
    var = F.Variable.make(prob, T, B)
    var.reset(0.0, 0.0, 0.0, 1.0, 1.0)
    st = s.solve(0.0, x0, var)
    assert np.isin(st, (1, 5)).all()
    tr = s.traceDataList()
    it = s.iters()
    kkt = tr[:, :, 1]
    last = kkt[np.arange(B), it - 1]
    assert (last < 1e-2 * kkt[:, 0]).all()
    v = s.variable()
    assert v.s_list.min() > 0 and v.nu_list.min() > 0
    g0 = np.stack([-v.u_list[:, :, 0] - 15.0, v.u_list[:, :, 0] - 15.0, -v.x_list[:, :-1, 0] - 20.0, v.x_list[:, :-1, 0] - 20.0], -1)
    assert np.abs(g0 + v.s_list).max() < 1e-3
    sub = slice(1000, 1130)
    s2 = F.FmpcSolverBatch(prob, 130, T)
    s2.config().max_iter = 8
    v2 = F.Variable.make(prob, T, 130)
    v2.reset(0.0, 0.0, 0.0, 1.0, 1.0)
    s2.solve(0.0, x0[sub], v2)
    for a, c in zip(s2.variable().arrays(), v.arrays()):
        assert np.array_equal(a, c[sub])
    assert s.computationDuration().solve > 0
    # the split of computationDuration(): one event pair per kernel launch
    s.config().time_kernels = True
    s.solve(0.0, x0, var)
    d = s.computationDuration()
    # (fused-Riccati sequence: fmpc_tail_kernel closes an iteration and opens the next, barrier + KKT kernels run for the first only)
    tail = "fmpc_tail_kernel" in s.kernelNames()
    assert d.launches["riccati"] == 8 and d.launches["coeff"] == (1 if tail else 8) and d.launches["line_search"] == 0
    assert d.launches["update"] == 8 and d.launches["step_length"] == (0 if tail else 8) and d.launches["barrier"] == (1 if tail else 8)
    assert 0 < d.backward < d.solve and d.coeff > 0 and d.update > 0
    assert abs(sum(d.kernels.values()) - d.solve) < 0.5 * d.solve


def _solve_outputs(model, B, T, max_iter, tail, poison, line_search=False):
    import os
    os.environ["NMPC_HIP_FMPC_TAIL"] = "1" if tail else "0"  # read when the handle is created
    try:
        prob = {"fmpc_cartpole": F.FmpcProblemCartPole, "fmpc_oscillator": F.FmpcProblemOscillator}[model](0.01)
        rng = np.random.default_rng(B * 1000 + T)
        n = prob.state_dim
        x0 = np.zeros((B, n))
        x0[:, 0] = rng.uniform(-1, 1, B)
        x0[:, 1] = rng.uniform(-0.3, 0.3, B) + (np.pi if n == 4 and T % 2 else 0.0)
        if poison:  # the error paths: NaN in the state (ErrorInBackward / Forward), a huge one
            x0[::7, 0] = np.nan
            x0[3::11, 1] = 1e200
        s = F.FmpcSolverBatch(prob, B, T)
        s.config().max_iter = max_iter
        s.config().enable_line_search = line_search
        var = F.Variable.make(prob, T, B)
        var.reset(0.0, 0.0, 0.0, 1.0, 1.0)
        try:
            s.solve(0.0, x0, var)
        except RuntimeError:
            pass
        out = dict(zip(("x", "u", "lambda", "s", "nu"), s.variable().arrays()))
        out.update(zip(("dx", "du", "dlambda", "ds", "dnu"), s.deltaVariable().arrays()))
        out.update(status=s.status(), iters=s.iters(), barrier_eps=s.barrierEps(), trace=s.traceDataList(), partials=s.partials())
        out.update(("gain_" + k, v) for k, v in s.coeffList().items())
        return out, s.kernelNames()
    finally:
        os.environ.pop("NMPC_HIP_FMPC_TAIL", None)


@pytest.mark.gpu
@pytest.mark.parametrize("model,B,T,max_iter", [("fmpc_cartpole", 1024, 200, 6), ("fmpc_cartpole", 1000, 37, 8), ("fmpc_cartpole", 17, 5, 3),
                                                ("fmpc_cartpole", 100, 1, 2), ("fmpc_cartpole", 256, 130, 1), ("fmpc_cartpole", 512, 200, 40),
                                                ("fmpc_oscillator", 2048, 100, 10), ("fmpc_oscillator", 333, 64, 4),
                                                ("fmpc_cartpole", 48, 400, 4), ("fmpc_oscillator", 40, 777, 3)])  # (T > 384: s . nu terms not in LDS)
@pytest.mark.parametrize("poison", [False, True])
def test_tail_kernel_returns_the_bits_of_the_separate_kernels(model, B, T, max_iter, poison):
    """fmpc_tail_kernel (step length + update of iteration k, barrier parameter + KKT-error terms + terminal record of iteration k + 1
    in one launch; FmpcSolver.hpp:370-392, :429-436, :493-521, :713-742, :801-835) against the kernel-per-step sequence
    (NMPC_HIP_FMPC_TAIL=0): every output of the solve, the trace, the gains and the per-timestep partial sums are bit-equal — also for
    instances that leave through an error status or converge early, ragged batch sizes, T = 1 and a single iteration."""
    a, names_a = _solve_outputs(model, B, T, max_iter, False, poison)
    b, names_b = _solve_outputs(model, B, T, max_iter, True, poison)
    assert "fmpc_tail_kernel" in names_b and "fmpc_tail_kernel" not in names_a and "fmpc_update_kernel" in names_a
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True) and a[k].tobytes() == b[k].tobytes(), k
    if poison:
        assert len(np.unique(b["status"])) >= 2
    if max_iter == 40 and not poison:
        assert (b["status"] == 1).sum() > 0.9 * B and b["iters"].max() > b["iters"].min()  # converged, after different numbers of iterations


@pytest.mark.gpu
def test_tail_kernel_is_not_used_with_the_line_search():
    """The line search sits between step length and update (FmpcSolver.hpp:748-792): those solves keep the kernel-per-step sequence."""
    _, names = _solve_outputs("fmpc_cartpole", 64, 50, 3, True, False, line_search=True)
    assert "fmpc_tail_kernel" not in names and "fmpc_line_search_kernel" in names


def test_cpp_mirror_runs_the_reference_oscillator_loop(tmp_path):
    """examples/fmpc_oscillator_mpc.cpp: TestFmpcOscillator.cpp:137-205 written against nmpc_amd::FmpcSolverBatch (g++ only)."""
    import os
    import subprocess

    from nmpc_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(_capi.lib_path())
    F.load()
    exe = str(tmp_path / "fmpc_oscillator_mpc")
    cmd = ["g++", "-std=c++17", "-O2", f"-I{root}/include", os.path.join(root, "examples", "fmpc_oscillator_mpc.cpp"), f"-L{libdir}",
           "-lnmpc_hip_ddp", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "4", "10.0"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "failures 0" in r.stdout


def test_large_batch_closed_loop_fails_where_the_oracle_fails():
    """4096 perturbed cart-pole swing-ups: the interior-point iteration diverges for a handful of starts (KKT error -> inf, NaN in
    the backward pass: Status::ErrorInBackward; the reference's cart-pole test ignores solve()'s return value,
    TestFmpcCartPole.cpp:411).  Those instances must fail at the same tick with the same status in the oracle's loop, after
    tracking it until then; a sample of healthy instances is followed as well."""
    model = "fmpc_cartpole"
    B, T, n_ticks = 4096, 200, 24
    rng = np.random.default_rng(0)
    prob = F.FmpcProblemCartPole(0.01)
    x0 = np.tile([0.0, np.pi, 0.0, 0.0], (B, 1)) + 0.05 * rng.standard_normal((B, 4))
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = 5
    var = F.Variable.make(prob, T, B)
    var.reset(0.0, 0.0, 0.0, 1.0, 1.0)
    s.setVariable(var)
    log = s.mpcRun(0.0, x0, n_ticks, 0.002, sim_substeps=2, use_feedback=True)
    st = log["status"]
    failed = np.unique(np.argwhere(~np.isin(st, (1, 5)))[:, 0])
    assert 1 <= len(failed) <= 40, len(failed)  # 10 with this seed
    cfg = O.default_config(horizon_steps=T, max_iter=5)
    for b in list(failed[:6]) + [0, 1234, 4095]:
        v, x, t, be = O.Variable.reset(model, T), x0[b].copy(), 0.0, 1e-4
        kkt_prev = 0.0
        for k in range(n_ticks):
            r = O.solve(model, cfg, prob.p, t, x, v, be)
            assert r.status == st[b, k] and r.iters == log["iters"][b, k], (b, k, r.status, st[b, k])
            if r.status not in (1, 5):
                break  # the device loop keeps ticking on the broken variable; nothing to compare beyond the failure
            # an iteration on its way to divergence amplifies rounding: the state is tracked tightly while the KKT error is sane
            assert np.allclose(x, log["x"][b, k], rtol=0, atol=1e-6 if kkt_prev < 1e3 else 1e-2), (b, k)
            kkt_prev = max(kkt_prev, r.trace[:r.iters, 1].max())
            be, v = r.barrier_eps, r.variable
            for _ in range(2):
                u = r.variable.u[0] + r.K[0] @ (r.variable.x[0] - x)
                x = O.evaluate(model, prob.p, t, x, u, step_dt=0.002)["f"]
                t += 0.002
        assert (b in failed) == (r.status not in (1, 5))


def test_c_abi_from_plain_c(tmp_path):
    """examples/fmpc_c_api.c: the FMPC C-ABI used from C99 (gcc, no C++ on the caller's side) gives the Python mirror's numbers."""
    import os
    import subprocess

    from nmpc_amd import _capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(_capi.lib_path())
    F.load()
    exe = str(tmp_path / "fmpc_c_api")
    cmd = ["gcc", "-std=c99", "-O2", f"-I{root}/include", f"{root}/examples/fmpc_c_api.c", f"-L{libdir}", "-lnmpc_hip_ddp",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("solve")]
    assert len(rows) == 8
    prob = F.FmpcProblemOscillator()
    s = F.FmpcSolverBatch(prob, 4, 100)
    s.config().max_iter = 3
    var = F.Variable.make(prob, 100, 4)
    var.reset(0.0, 0.0, 0.0, 1.0, 1.0)
    x0 = np.array([[0.1 * b, 1.0] for b in range(4)])
    s.setVariable(var)
    for p in range(2):
        st = s.solve(np.zeros(4), x0)
        it, tr, u = s.iters(), s.traceDataList(), s.variable().u_list
        for b in range(4):
            row = rows[4 * p + b]
            assert [int(row[5]), int(row[6]), int(row[7])] == [2, 1, 3]  # dims
            assert int(row[9]) == st[b] and int(row[11]) == it[b]
            assert np.isclose(float(row[13]), tr[b, it[b] - 1, 1], rtol=1e-11, atol=0)  # printed with 13 digits
            assert np.isclose(float(row[15]), u[b, 0, 0], rtol=1e-11, atol=1e-300)


def test_max_iter_zero_returns_uninitialized():
    """solve() with max_iter = 0 never enters the loop (FmpcSolver.hpp:233-246): Status::Uninitialized, variable untouched."""
    model = "fmpc_oscillator"
    prob = MODELS[model]()
    B, T = 20, 12
    var, x0, t0 = make_case(model, B, T, seed=3)
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = 0
    st = s.solve(t0, x0, var)
    ref = oracle_batch(model, s.config(), prob.p, t0, x0, var)
    assert (st == 0).all() and np.array_equal(st, ref.status) and (s.iters() == 0).all() and (ref.iters == 0).all()
    for a, c in zip(s.variable().arrays(), var.arrays()):
        assert np.array_equal(a, c)


# the shipped shape, then the smallest ones at which the chunk protocol of either kernel can go wrong: (17, 3) one partial backward
# chunk, the second producer wave idle, one partial forward chunk, a second workgroup with one live lane; (1, 5) N = 2, two backward
# chunks, fifteen mirrored lanes; (33, 12) an odd number of backward chunks, two forward chunks of which the last is partial
@pytest.mark.parametrize("model,B,T,max_iter", [("fmpc_cartpole", 200, 61, 4), ("fmpc_cartpole", 17, 3, 2), ("fmpc_oscillator", 1, 5, 2),
                                                ("fmpc_oscillator", 33, 12, 2)])
def test_fused_riccati_kernel_returns_the_quad_kernels_bits(model, B, T, max_iter, monkeypatch):
    """fmpc_riccati_fused_kernel computes the coefficient records in its producer waves (fmpc::coefficients, the body of the coefficient
    kernel with another sink) and runs the quad kernel's recursion on them: the same statements on the same values — every output of a
    solve is bit-identical to the unfused path's (coefficient kernel + records through HBM + fmpc_riccati_quad_kernel).  No convergence
    is needed for that."""
    res = {}
    for riccati in ("quad", "fused"):
        monkeypatch.setenv("NMPC_HIP_FMPC_RICCATI", riccati)
        prob = MODELS[model]()
        var, x0, t0 = make_case(model, B, T, seed=7)
        s = F.FmpcSolverBatch(prob, B, T)
        s.config().max_iter = max_iter
        s.solve(t0, x0, var)
        assert ("fmpc_riccati_%s_kernel" % riccati) in s.kernelNames()
        cl = s.coeffList()
        res[riccati] = [a.copy() for a in s.variable().arrays()] + [s.traceDataList().copy(), s.iters().copy(), cl["K"].copy(), cl["P"].copy(),
                                                                    s.status().copy()]
    for a, b in zip(res["quad"], res["fused"]):
        assert np.array_equal(a, b, equal_nan=True)
