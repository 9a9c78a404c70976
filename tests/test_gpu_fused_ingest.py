"""The quad kernel's whole-solve launch converts the caller's arrays itself (QuadSolver::ingestInputs, ddp_kernels_quad.hpp; one
dispatch per solve instead of ingest_kernel + solve kernel).  Every case runs the same inputs with the launch knob on and off
(LaunchKnobs::fused_ingest, NMPC_HIP_DDP_FUSED_INGEST read when the handle is created) and compares every output field bit for bit:
the prologue has to leave the handle's t0 / x0 / U exactly as ingest_kernel does, padded lanes included."""
import numpy as np
import pytest

from nmpc_amd import workloads

from test_gpu_parity import make_solver

pytestmark = pytest.mark.gpu

FIELDS = ("X", "U", "cost", "status", "iters", "trace", "kff", "Kfb", "dV")
KNOB = "NMPC_HIP_DDP_FUSED_INGEST"


def randomised(wl, seed, t0=True):
    """The workload with random non-zero initial inputs and start times (the shipped workloads start from u = 0)."""
    rng = np.random.default_rng(seed)
    wl.u_init = rng.uniform(-0.5, 0.5, size=wl.u_init.shape)
    wl.t0 = rng.uniform(0.5, 3.0, size=wl.B) if t0 else None
    return wl


def outputs(s):
    return {f: np.array(getattr(s, f)()) for f in FIELDS}


def assert_same_bits(a, b, what):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f], equal_nan=True), (what, f, int((a[f] != b[f]).sum()))


def handle(wl, fused, monkeypatch, problems=None, **cfg):
    """A solver whose handle exists (the knob is read at create), with the environment left as it was."""
    monkeypatch.setenv(KNOB, "1" if fused else "0")
    s = make_solver(wl, **cfg)
    if problems is not None:
        s.setProblemBatch(problems)
    assert s.kernelName() == "ddp_solve_quad_kernel"  # (creates the handle)
    monkeypatch.delenv(KNOB)
    return s


def solve_device(s, wl):
    """solveDevice on device copies of the workload's arrays; the copies must come back untouched (they are inputs only)."""
    import torch

    arrays = (wl.t0, wl.x0, wl.u_init)
    d = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    before = [None if t is None else t.clone() for t in d]
    s.solveDevice(*[None if t is None else t.data_ptr() for t in d])
    s.synchronize()
    for name, t, b in zip(("current_t", "current_x", "initial_u_list"), d, before):
        assert t is None or torch.equal(t, b), f"the solve wrote to the caller's {name}"
    return outputs(s)


def one_dispatch(s):
    """Whether the last solve was the single dispatch: its kernel time is then the whole begin -> end interval (no event between
    a conversion kernel and the solve kernel), otherwise the conversion kernel lies in front of it."""
    d = s.computationDuration()
    assert d.solve >= d.opt > 0.0
    return d.setup == 0.0


def both(wl, monkeypatch, problems=None, **cfg):
    got = {}
    for fused in (True, False):
        s = handle(wl, fused, monkeypatch, problems=problems, **cfg)
        got[fused] = solve_device(s, wl)
        assert s.lastSolveLaunches() == 1 and one_dispatch(s) == fused
    assert_same_bits(got[True], got[False], "knob on against knob off")
    return got[True]


@pytest.mark.parametrize("B,T", [(1, 1), (17, 20), (40, 100)])
def test_cartpole_shapes(B, T, monkeypatch):
    """A lone lane with a one-step horizon; a partly filled second workgroup with a partial batch of rows; the benchmark's horizon
    (more rows than one pass of the four waves over 32-row batches covers: T = 100 leaves a four-row batch)."""
    out = both(randomised(workloads.cartpole_batch(B=B, T=T, seed=B + T), 7 * B + T), monkeypatch, max_iter=3)
    assert np.isfinite(out["X"]).all() and (out["iters"] >= 1).all()


def test_horizon_beyond_one_round_of_row_batches(monkeypatch):
    """T = 150: wave 0 takes a second 32-row batch (rows 128 ..), partly filled."""
    both(randomised(workloads.cartpole_batch(B=17, T=150, seed=3), 31), monkeypatch, max_iter=3)


def test_without_start_times(monkeypatch):
    both(randomised(workloads.cartpole_batch(B=17, T=20, seed=5), 11, t0=False), monkeypatch, max_iter=3)


def test_bipedal(monkeypatch):
    """n = 2 (the padded 4 x 4 blocks), time-varying dynamics: the start times matter."""
    wl = workloads.bipedal_batch(B=17, T=20, seed=5)
    t0 = wl.t0.copy()
    wl = randomised(wl, 13)
    wl.u_init *= 0.1
    wl.t0 = t0 + 0.25
    both(wl, monkeypatch, max_iter=3)


def test_box_constrained(monkeypatch):
    wl = randomised(workloads.cartpole_batch(B=17, T=20, seed=6, constrained=True), 17)
    wl.u_init *= 40.0  # (initial inputs on either side of the +- 15 N box)
    both(wl, monkeypatch, max_iter=3, with_input_constraint=True)


def test_per_instance_problem_objects(monkeypatch):
    import nmpc_amd

    wl = randomised(workloads.cartpole_batch(B=17, T=20, seed=8), 19)
    rng = np.random.default_rng(55)
    probs = [nmpc_amd.DDPProblemCartPole(cart_mass=float(rng.uniform(0.7, 1.5)), pole_length=float(rng.uniform(1.0, 2.5))) for _ in range(wl.B)]
    both(wl, monkeypatch, problems=probs, max_iter=3)


def test_second_solve_on_the_same_handle(monkeypatch):
    """Other inputs on a handle that has solved: nothing of the first solve's x0 / U / t0 survives (either half of U may hold
    the first result), and the handle agrees with a fresh one."""
    first = randomised(workloads.cartpole_batch(B=17, T=20, seed=9), 23)
    second = randomised(workloads.cartpole_batch(B=17, T=20, seed=10), 29)
    got = {}
    for fused in (True, False):
        s = handle(first, fused, monkeypatch, max_iter=3)
        solve_device(s, first)
        got[fused] = solve_device(s, second)
        assert one_dispatch(s) == fused
    assert_same_bits(got[True], got[False], "second solve, knob on against knob off")
    assert_same_bits(got[True], both(second, monkeypatch, max_iter=3), "second solve against a fresh handle")


def test_ragged_schedule_keeps_the_conversion_kernel(monkeypatch):
    """A solve cut into resumable launches does not take the new path, whatever the knob says, and agrees."""
    wl = randomised(workloads.cartpole_batch(B=64, T=20, seed=11), 37)
    got = {}
    for fused in (True, False):
        s = handle(wl, fused, monkeypatch, max_iter=500, ragged_schedule=1)
        got[fused] = solve_device(s, wl)
        assert s.lastSolveLaunches() > 1 and not one_dispatch(s)
    assert_same_bits(got[True], got[False], "ragged schedule, knob on against knob off")


def test_host_staged_solve(monkeypatch):
    """solve() stages the host arrays on the device and reaches the same launch."""
    wl = randomised(workloads.cartpole_batch(B=17, T=20, seed=12), 41)
    got = {}
    for fused in (True, False):
        s = handle(wl, fused, monkeypatch, max_iter=3)
        s.solve(wl.t0, wl.x0, wl.u_init)
        got[fused] = outputs(s)
        assert one_dispatch(s) == fused
    assert_same_bits(got[True], got[False], "solve(), knob on against knob off")
    assert_same_bits(got[True], both(wl, monkeypatch, max_iter=3), "solve() against solveDevice()")
