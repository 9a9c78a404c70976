"""Streamed solve (nmpc_hip_ddp_solve_stream): N cart-pole instances to convergence (default Configuration) through the 4096 slots of ONE
handle; batch-iterations/s-equivalent = instance-iterations / 4096 / device time.   python scripts/stream_throughput.py [N] [slots] [spans ...]

python scripts/stream_throughput.py mixed [N] [slots] [reps]: the HETEROGENEOUS queue (nmpc_hip_ddp_solve_stream_ex) — every cart-pole with
its own input weight, target position and pole length — as (a) the heterogeneous stream, (b) the same queue on the shared problem
object through nmpc_hip_ddp_solve_stream, (b') that shared-object queue through the heterogeneous entry point, every instance
bringing a copy of the shared object (b' / b: what the own-problem instantiation and its refill cost at equal work — (a) and (b) solve
different problems and iterate differently) and (c) chunked solve() calls with setProblemBatch, each chunk to convergence.  Warm handles, the variants alternate, median and range of `reps` repetitions."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import nmpc_amd  # noqa: E402
from nmpc_amd import workloads  # noqa: E402



def mixed(N, S, reps):
    wl = workloads.cartpole_batch(B=N, T=100, seed=1234)
    rng = np.random.default_rng(7)
    running_u, ref_pos, pole_length = rng.uniform(0.0005, 0.02, N), rng.uniform(-1.0, 1.0, N), rng.uniform(1.5, 2.5, N)
    problems = [nmpc_amd.make_problem(wl.model, running_u=[running_u[q]], ref_pos=ref_pos[q], pole_length=pole_length[q]) for q in range(N)]

    def solver():
        s = nmpc_amd.DDPSolverBatch(nmpc_amd.make_problem(wl.model), S)
        c = s.config(); c.print_level, c.horizon_steps, c.max_iter, c.trace_level = 0, wl.T, 500, 0
        return s

    copies = [nmpc_amd.make_problem(wl.model)] * N

    def stream(s, own):
        t0 = time.perf_counter()
        r = s.solveStream(wl.t0, wl.x0, wl.u_init, problems=own)
        return int(r.iters.sum()), r.device_ms, 1e3 * (time.perf_counter() - t0), r.rounds

    def chunks(s):
        it, dev, t0 = 0, 0.0, time.perf_counter()
        for lo in range(0, N, S):
            hi = min(lo + S, N)
            pad = list(range(lo, hi)) + [lo] * (S - (hi - lo))  # (solve() takes whole batches)
            s.setProblemBatch([problems[q] for q in pad])
            s.solve(wl.t0[pad], wl.x0[pad], wl.u_init[pad])
            it += int(s.iters()[: hi - lo].sum())
            dev += s.computationDuration().solve
        return it, dev, 1e3 * (time.perf_counter() - t0), (N + S - 1) // S

    variants = (("a: heterogeneous stream", solver(), lambda s: stream(s, problems)), ("b: shared-object stream", solver(), lambda s: stream(s, None)),
                ("c: chunked solve() + setProblemBatch", solver(), chunks),
                ("b': shared objects as per-instance copies", solver(), lambda s: stream(s, copies)))
    rates = {name: [] for name, _, _ in variants}
    last = {}
    for rep in range(reps + 1):  # (repetition 0 warms the handles up and is not counted)
        for name, s, run in variants:
            it, dev, wall, launches = run(s)
            if rep:
                rates[name].append(it / S / (dev * 1e-3))
            last[name] = (it, dev, wall, launches)
    print(f"N {N} cart-poles (T 100, default Configuration, per-instance running_u / ref_pos / pole_length) through {S} slots, {reps} repetitions")
    for name, _, _ in variants:
        r = np.array(rates[name])
        it, dev, wall, launches = last[name]
        print(f"  {name:38s}: median {np.median(r):8.0f} batch-it/s-equivalent (min {r.min():.0f}, max {r.max():.0f}); last run: {it} instance-iterations, "
              f"device {dev:.2f} ms, wall {wall:.2f} ms, {launches} rounds / chunks", flush=True)
    med = {name: float(np.median(rates[name])) for name in rates}
    names = [v[0] for v in variants]
    print(f"  a / b = {med[names[0]] / med[names[1]]:.3f}   b' / b = {med[names[3]] / med[names[1]]:.3f}   a / c = {med[names[0]] / med[names[2]]:.2f}")


if len(sys.argv) > 1 and sys.argv[1] == "mixed":
    mixed(int(sys.argv[2]) if len(sys.argv) > 2 else 32768, int(sys.argv[3]) if len(sys.argv) > 3 else 4096, int(sys.argv[4]) if len(sys.argv) > 4 else 5)
    sys.exit(0)
N = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
S = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
spans = [int(a) for a in sys.argv[3:]] or [16]
wl = workloads.cartpole_batch(B=N, T=100, seed=1234)
for span in spans:
    s = nmpc_amd.DDPSolverBatch(nmpc_amd.make_problem(wl.model), S)
    c = s.config(); c.print_level, c.horizon_steps, c.max_iter, c.trace_level = 0, wl.T, 500, 0
    best = None
    for rep in range(3):
        t0 = time.perf_counter()
        r = s.solveStream(wl.t0, wl.x0, wl.u_init, span=span)
        wall = time.perf_counter() - t0
        it = int(r.iters.sum())
        rate = it / S / (r.device_ms * 1e-3)
        best = max(best or 0, rate)
    st = {int(k): int(v) for k, v in zip(*np.unique(r.status, return_counts=True))}
    print(f"N {N} slots {S} span {span:3d}: {r.rounds} rounds, device {r.device_ms:8.2f} ms (wall {1e3 * wall:8.2f}), {it} instance-iterations "
          f"(mean {it / N:.2f}) -> {best:8.0f} batch-it/s-equivalent; status {st}", flush=True)
