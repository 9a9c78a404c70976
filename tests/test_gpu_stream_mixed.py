"""A heterogeneous queue (nmpc_hip_ddp_solve_stream_ex; DDPSolverBatch.solveStream(problems=, input_limits=)): N >> B instances, each
with its OWN problem object and / or input limits, through the B slots of one handle.  Reference: a caller builds one DDPSolver per
problem, each with its problem object and its setInputLimitsFunc (DDPSolver.hpp:20-24, DDPSolver.h:282-285), and every one runs its
loop to ITS end (DDPSolver.hpp:115-123) — so every instance must return the bits of its lone solve: the queue in chunks on a plain
handle with setProblemBatch / setInputLimitsBatch, same kernel family.  Also here: the ragged-convergence schedule on a handle with
per-instance problem objects and limits (only when asked for), the refusals, and the state the handle is left in.

The queue: 600 cart-poles (T = 100), each with its own input weight, target position, pole length and input box; max_iter 40 and
rounds of 4 iterations make it ragged (the conditions on the lone solves below say how)."""
import dataclasses
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # (the worker of the wave-timing fuzz case: a process of its own, on the library NMPC_HIP_DDP_LIB names)
    sys.path.insert(0, ROOT)

import nmpc_amd
from nmpc_amd import workloads

from test_gpu_parity import make_solver
from test_gpu_stream import FIELDS

pytestmark = pytest.mark.gpu

N, T, MAX_ITER, SPAN = 600, 100, 40, 4
KERNEL_NAMES = {"quad": "ddp_solve_quad_kernel", "2w": "ddp_solve_tpi2w_kernel"}
RAGGED_FIELDS = ("X", "U", "cost", "kff", "Kfb", "status", "iters", "trace", "dV", "qpRetval", "qpFreeMask")


@dataclasses.dataclass
class Queue:
    wl: object
    running_u: np.ndarray
    ref_pos: np.ndarray
    pole_length: np.ndarray
    lower: np.ndarray  # (N, 1)
    upper: np.ndarray

    def problems(self, lo=0, hi=N):
        return [nmpc_amd.make_problem("cartpole", running_u=[self.running_u[q]], ref_pos=self.ref_pos[q], pole_length=self.pole_length[q])
                for q in range(lo, hi)]


@functools.lru_cache(maxsize=None)
def queue(constrained: bool) -> Queue:
    wl = workloads.cartpole_batch(B=N, T=T, seed=7, constrained=constrained)
    rng = np.random.default_rng(7)
    running_u = rng.uniform(0.0005, 0.02, N)
    ref_pos = rng.uniform(-1.0, 1.0, N)
    pole_length = rng.uniform(1.5, 2.5, N)
    half = rng.uniform(5.0, 20.0, N)
    return Queue(wl, running_u, ref_pos, pole_length, -half[:, None], half[:, None])


def config(constrained):
    return dict(max_iter=MAX_ITER, with_input_constraint=constrained, trace_level=0)


@functools.lru_cache(maxsize=None)
def lone_solves(kernel, slots, constrained, own_problems, own_limits):
    """ "want": the queue in chunks of `slots` on a plain handle with setProblemBatch / setInputLimitsBatch, one whole-solve launch each
    (the pattern of test_gpu_stream.lone_solves)."""
    q = queue(constrained)
    out = {f: [] for f in FIELDS}
    for lo in range(0, N, slots):
        hi = min(lo + slots, N)
        part = dataclasses.replace(q.wl, B=hi - lo, x0=q.wl.x0[lo:hi], u_init=q.wl.u_init[lo:hi], t0=q.wl.t0[lo:hi])
        s = make_solver(part, ragged_schedule=-1, **config(constrained))
        s.setKernel(kernel)
        s.setDispatchBatch(slots)
        if own_problems:
            s.setProblemBatch(q.problems(lo, hi))
        if own_limits:
            s.setInputLimitsBatch(q.lower[lo:hi], q.upper[lo:hi])
        s.solve(part.t0, part.x0, part.u_init)
        got = {"X": s.X(), "U": s.U(), "cost": s.cost(), "status": s.status(), "iters": s.iters(), "trace_last": s.traceLast(), "dV": s.dV()}
        for f in FIELDS:
            out[f].append(np.array(got[f]))
    return {f: np.concatenate(v) for f, v in out.items()}


def stream_solver(kernel, slots, constrained):
    s = make_solver(dataclasses.replace(queue(constrained).wl, B=slots), **config(constrained))
    s.setKernel(kernel)
    return s


def stream_mixed(s, constrained, own_problems, own_limits):
    q = queue(constrained)
    return s.solveStream(q.wl.t0, q.wl.x0, q.wl.u_init, span=SPAN, problems=q.problems() if own_problems else None,
                         input_limits=(q.lower, q.upper) if own_limits else None)


def assert_fields_equal(r, want, what=""):
    for f in FIELDS:
        got = getattr(r, f) if not isinstance(r, dict) else r[f]
        assert np.array_equal(got, want[f], equal_nan=True), (what, f, int((got != want[f]).sum()),
                                                               np.flatnonzero((got != want[f]).reshape(N, -1).any(axis=1))[:8])


def assert_ragged(want, constrained, rounds, slots):
    """The conditions on the lone solves that keep the comparison from passing vacuously."""
    it = want["iters"]
    print("iters min %d median %d max %d, <= span: %d, at the cap with status 0: %d, status -1: %d, rounds %d" % (
        it.min(), np.median(it), it.max(), (it <= SPAN).sum(), ((it == MAX_ITER) & (want["status"] == 0)).sum(), (want["status"] == -1).sum(), rounds))
    assert (it <= SPAN).sum() >= 0.1 * N  # instances that leave after their first round
    assert it.max() > 2 * SPAN  # ... next to ones that stay for several
    if not constrained:
        assert ((it == MAX_ITER) & (want["status"] == 0)).any()  # an instance's own max_iter-th iteration
    assert rounds > math.ceil(N / slots)  # slots are refilled in mid-queue


@pytest.mark.parametrize("kernel,slots,constrained,own_problems,own_limits", [
    ("quad", 256, False, True, False),
    ("quad", 256, True, True, True),
    ("2w", 128, False, True, False),
    ("2w", 128, True, False, True),  # limits only: the shared problem object
])
def test_every_instance_returns_the_bits_of_its_lone_solve(kernel, slots, constrained, own_problems, own_limits):
    want = lone_solves(kernel, slots, constrained, own_problems, own_limits)
    s = stream_solver(kernel, slots, constrained)
    r = stream_mixed(s, constrained, own_problems, own_limits)
    assert s.kernelName() == KERNEL_NAMES[kernel]
    assert_fields_equal(r, want)
    assert_ragged(want, constrained, r.rounds, slots)


def test_the_problem_objects_reach_the_kernel():
    s = stream_solver("quad", 256, False)
    own = stream_mixed(s, False, True, False)
    shared = stream_mixed(stream_solver("quad", 256, False), False, False, False)
    moved = np.abs(own.U - shared.U).reshape(N, -1).max(axis=1) > 1e-3
    print("instances whose inputs differ from the shared problem's by more than 1e-3:", int(moved.sum()))
    assert moved.sum() >= N / 2


def test_streamed_mixed_queue_agrees_with_the_oracle():
    """Every instance against the CPU oracle on ITS parameter vector: equal iteration counts and verdicts, X within 1e-9 scaled (the
    tolerance and form of tests/test_gpu_stream.py)."""
    from concurrent.futures import ThreadPoolExecutor

    import oracle
    q = queue(False)
    r = stream_mixed(stream_solver("quad", 256, False), False, True, False)
    ocfg = oracle.default_config(horizon_steps=T, max_iter=MAX_ITER)

    def one(i):
        p = oracle.default_params("cartpole", running_u=q.running_u[i], ref_pos=q.ref_pos[i], pole_length=q.pole_length[i])
        return oracle.solve("cartpole", ocfg, q.wl.x0[i], q.wl.u_init[i], t0=float(q.wl.t0[i]), params=p)

    with ThreadPoolExecutor(8) as pool:
        refs = list(pool.map(one, range(N)))
    ref_iters = np.array([x.iters for x in refs])
    ref_status = np.array([x.status for x in refs])
    ref_X = np.stack([x.X for x in refs])
    assert np.array_equal(r.iters, ref_iters) and np.array_equal(r.status, ref_status)
    err = (np.abs(r.X - ref_X) / (1.0 + np.abs(ref_X))).max()
    print("X against the oracle, scaled:", err)
    assert err < 1e-9


def test_the_handle_is_left_with_its_shared_problem_and_limits():
    q = queue(False)
    want = lone_solves("quad", 256, False, True, False)
    s = stream_solver("quad", 256, False)
    assert_fields_equal(stream_mixed(s, False, True, False), want, "first queue")
    assert_fields_equal(stream_mixed(s, False, True, False), want, "the same handle again")
    # ... a shared-object queue through the old entry point: the bits of a fresh handle
    fresh = stream_mixed(stream_solver("quad", 256, False), False, False, False)
    assert_fields_equal(stream_mixed(s, False, False, False), {f: getattr(fresh, f) for f in FIELDS}, "plain solveStream afterwards")
    # ... and a plain solve() of 256 instances: a fresh handle with the shared problem
    part = dataclasses.replace(q.wl, B=256, x0=q.wl.x0[:256], u_init=q.wl.u_init[:256], t0=q.wl.t0[:256])
    t = make_solver(part, ragged_schedule=-1, **config(False))
    t.setKernel("quad")
    t.solve(part.t0, part.x0, part.u_init)
    s.config().ragged_schedule = -1
    s.solve(part.t0, part.x0, part.u_init)
    for f, a, b in (("X", s.X(), t.X()), ("U", s.U(), t.U()), ("cost", s.cost(), t.cost()), ("status", s.status(), t.status()),
                    ("iters", s.iters(), t.iters()), ("trace_last", s.traceLast(), t.traceLast()), ("dV", s.dV(), t.dV())):
        assert np.array_equal(a, b, equal_nan=True), ("plain solve afterwards", f)
    assert not np.array_equal(s.U(), want["U"][:256])  # (the shared problem's solution, not the queue's)


def test_refusals_say_what_to_do():
    q, qc = queue(False), queue(True)
    # per-instance objects that belong to the handle's slots
    s = stream_solver("quad", 256, False)
    s.setProblemBatch(q.problems(0, 256))
    with pytest.raises(RuntimeError, match=r"nmpc_hip_ddp -2\].*belong to its slots.*nmpc_hip_ddp_solve_stream_ex"):
        stream_mixed(s, False, True, False)
    with pytest.raises(RuntimeError, match=r"nmpc_hip_ddp -2\].*belong to its slots"):
        stream_mixed(s, False, False, False)
    # a blob with another dt
    s = stream_solver("quad", 256, False)
    problems = q.problems()
    problems[17].set("dt", 0.02)
    with pytest.raises(ValueError, match=r"instance 17 of the queue has a different dt\(\)"):
        s.solveStream(q.wl.t0, q.wl.x0, q.wl.u_init, span=SPAN, problems=problems)
    # lower without upper
    s = stream_solver("quad", 256, True)
    with pytest.raises(ValueError, match="only one of lower / upper"):
        s.solveStream(qc.wl.t0, qc.wl.x0, qc.wl.u_init, span=SPAN, input_limits=(qc.lower, None))
    # limits while the solver is unconstrained
    s = stream_solver("quad", 256, False)
    with pytest.raises(ValueError, match="with_input_constraint is off"):
        s.solveStream(q.wl.t0, q.wl.x0, q.wl.u_init, span=SPAN, input_limits=(q.lower, q.upper))
    # a family without resumable launches
    wl = workloads.manipulator_batch(B=64, T=20, seed=3)
    s = make_solver(wl, max_iter=10)
    with pytest.raises(RuntimeError, match="resumable"):
        s.solveStream(wl.t0, wl.x0, wl.u_init, problems=[nmpc_amd.make_problem(wl.model) for _ in range(wl.B)])


@pytest.mark.parametrize("kernel,box", [("quad", 1.0), ("2w", 1.0), ("quad", 2.0), ("2w", 2.0)])
def test_ragged_schedule_with_own_problems_and_limits(kernel, box):
    """One handle of 600 instances with setProblemBatch + setInputLimitsBatch, box-constrained: the schedule — only when asked for —
    returns the bits of the whole-solve launch.

    box 1: the queue's own boxes (half-width U(5, 20)).  On those every instance is done within the schedule's first launch — the CPU
    oracle gives 2 .. 15 iterations, 19 instances with status -1 — so the compaction finds nothing to move.  box 2: the same
    instances with boxes twice as wide (half-width U(10, 40), still binding); the CPU oracle gives 2 .. 26 iterations, five
    instances above 16, 11 with status -1.  The condition that the data IS ragged across the first boundary is asserted there."""
    q = queue(True)

    def run(mode):
        s = make_solver(q.wl, max_iter=MAX_ITER, with_input_constraint=True, ragged_schedule=mode)
        s.setKernel(kernel)
        s.setProblemBatch(q.problems())
        s.setInputLimitsBatch(box * q.lower, box * q.upper)
        s.solve(q.wl.t0, q.wl.x0, q.wl.u_init)
        assert s.kernelName() == KERNEL_NAMES[kernel]
        return s.lastSolveLaunches(), {f: np.array(getattr(s, f)()) for f in RAGGED_FIELDS}

    n_on, on = run(1)
    n_off, off = run(-1)
    n_auto, _ = run(0)
    assert n_on > 1 and n_off == 1 and n_auto == 1, (n_on, n_off, n_auto)
    for f in RAGGED_FIELDS:
        assert np.array_equal(on[f], off[f], equal_nan=True), (f, int((on[f] != off[f]).sum()))
    it = off["iters"]
    print("box x%g: iters min %d max %d, above 16: %d, status -1: %d, launches %d" % (box, it.min(), it.max(), (it > 16).sum(), (off["status"] == -1).sum(), n_on))
    if box > 1.0:
        assert (it < 16).any() and (it > 16).any()  # the compaction has something to do


def fuzz_worker(out_path):
    r = stream_mixed(stream_solver("quad", 256, True), True, True, True)
    np.savez(out_path, **{f: getattr(r, f) for f in FIELDS})


def test_mixed_queue_on_the_wave_timing_fuzz_build(tmp_path):
    """The problems + limits case on the library whose workgroup barriers are wrapped in per-wave pseudo-random sleeps
    (include/nmpc_amd/hip/fuzz_sched.hpp): the product library's bits.  One seed, one run."""
    from nmpc_amd import build as hip_build
    lib = hip_build.fuzz_path(1)
    if not os.path.exists(lib):
        pytest.skip("nmpc_amd/lib/fuzz1 is not built")
    want = lone_solves("quad", 256, True, True, True)
    out = str(tmp_path / "fuzz.npz")
    env = dict(os.environ)
    env["NMPC_HIP_DDP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", out], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = dict(np.load(out))
    assert_fields_equal(got, want, "fuzz seed 1")


def test_cpp_mixed_stream_matches_lone_solves(tmp_path):
    """include/nmpc_amd/DDPSolverBatch.hpp: the solveStream overload with one problem object per instance —
    examples/cartpole_stream_mixed.cpp runs 600 cart-poles through 256 slots and compares every one bit for bit with solve() on chunks
    with setProblemBatch."""
    from nmpc_amd import build as hip_build
    exe = str(tmp_path / "cartpole_stream_mixed")
    libdir = os.path.dirname(hip_build.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O2", f"-I{ROOT}/include", f"{ROOT}/examples/cartpole_stream_mixed.cpp", f"-L{libdir}", "-lnmpc_hip_ddp",
           f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "600", "256"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "STREAM_MIXED_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__":
    assert sys.argv[1] == "worker"
    fuzz_worker(sys.argv[2])
