#!/usr/bin/env python3
"""Two builds of the library on the FMPC path, on one GPU box: do they return the same BITS, and is one slower?  Public Python API
only (nmpc_amd.fmpc), so the same file drives any earlier build; a fresh child process per library (NMPC_HIP_DDP_LIB), one at a time.

  python scripts/fmpc_lib_ab.py bits <libA> <libB> [out_dir]
      every case below on each library; every returned array (x, u, lambda, s, nu, the step, status, iters, trace, barrier_eps, merit,
      partials, gains k / K / s / P, the mpc_run logs) compared byte for byte, NaN positions included.  Exit status 1 on any difference
      (the first differing entry of every differing array is printed).  The cases reach the fixed-dimension and the dims-aware variant
      of every kernel of the iteration: oscillator / cart-pole / point-mass / vertical motion, lane / quad / fused Riccati with and
      without the tail kernel, line search, init_complementary_variable, update_barrier_eps off, ragged batches, closed loops with
      and without feedback, the error statuses; for the quad and the fused Riccati kernel also the smallest horizons at which their
      chunk loops take another path (tests/test_gpu_fmpc.py::test_fused_riccati_kernel_returns_the_quad_kernels_bits).
  python scripts/fmpc_lib_ab.py time <libA> <libB> <out.json> [repetitions]
      4096 x T 200 cart-pole, max_iter 5 (the bench workload) as shipped (fused + tail), with NMPC_HIP_FMPC_RICCATI=quad (the
      unfused matrix-core sequence) and =lane (the kernel-per-step sequence) and with the line search: the libraries alternate,
      `repetitions` (default 5) processes each; per kernel class (config.time_kernels) and for the graph-replayed solve: median and
      spread (max - min) over the repetitions.
      Verdict per row: B's median <= A's median + A's spread.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POISON = 1e300  # entries beyond a step's dimensions (vertical motion): never read


def fixed_case(F, model, B, T, seed, spread=0.2):
    prob = {"fmpc_oscillator": F.FmpcProblemOscillator, "fmpc_cartpole": F.FmpcProblemCartPole, "fmpc_pointmass": F.FmpcProblemPointMass}[model]()
    n, m, g = prob.state_dim, prob.input_dim, prob.ineq_dim
    rng = np.random.default_rng(seed)
    var = F.Variable(spread * rng.standard_normal((B, T + 1, n)), spread * rng.standard_normal((B, T, m)),
                     spread * rng.standard_normal((B, T + 1, n)), rng.uniform(0.5, 2.0, (B, T, g)), rng.uniform(0.5, 2.0, (B, T, g)))
    return prob, var, spread * rng.standard_normal((B, n)), rng.uniform(0, 1, B)


def vertical_case(F, B, T, seed):
    rng = np.random.default_rng(seed)
    prob = F.FmpcProblemVerticalMotion()
    t0 = rng.uniform(0.0, 6.0, B)
    x = np.tile([1.0, 0.0], (B, T + 1, 1)) + 0.05 * rng.standard_normal((B, T + 1, 2))
    u = 9.80665 + rng.uniform(-2.0, 2.0, (B, T, 2))
    lam = 0.1 * rng.standard_normal((B, T + 1, 2))
    s, nu = rng.uniform(0.5, 2.0, (B, T, 4)), rng.uniform(0.5, 2.0, (B, T, 4))
    x0 = np.stack([1.0 + 0.1 * rng.standard_normal(B), 0.1 * rng.standard_normal(B)], axis=1)
    for b in range(B):
        for i in range(T):
            m, g = prob.dimsAt(t0[b] + i * prob.dt())
            u[b, i, m:] = POISON
            s[b, i, g:] = POISON
            nu[b, i, g:] = POISON
    return prob, F.Variable(x, u, lam, s, nu), x0, t0


def outputs(s):
    out = dict(zip(("x", "u", "lambda", "s", "nu"), s.variable().arrays()))
    out.update(zip(("dx", "du", "dlambda", "ds", "dnu"), s.deltaVariable().arrays()))
    out.update(status=s.status(), iters=s.iters(), barrier_eps=s.barrierEps(), trace=s.traceDataList(), merit=s.meritFunc(),
               partials=s.partials())
    out.update(("gain_" + k, v) for k, v in s.coeffList().items())
    return out


def solve_case(F, prob, var, x0, t0, max_iter, barrier_eps=None, expect=(), second_iteration=True, **opts):
    B, T = var.u_list.shape[0], var.u_list.shape[1]
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = max_iter
    for k, v in opts.items():
        setattr(s.config(), k, v)
    s.setVariable(var, barrier_eps=barrier_eps)
    try:
        s.solve(t0, x0)
    except RuntimeError:  # (checkVariable's verdict: the arrays are compared all the same)
        pass
    names = s.kernelNames()
    for e in expect:
        assert e in names, (e, names)
    out = outputs(s)
    # the update and barrier bodies must have run on live data: most instances went into a second iteration
    assert not second_iteration or (out["iters"] >= 2).mean() > 0.5, out["iters"]
    return out


def loop_case(F, prob, B, T, max_iter, x0, t0, n_ticks, sim_dt, substeps, feedback, init, **opts):
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = max_iter
    for k, v in opts.items():
        setattr(s.config(), k, v)
    v = F.Variable.make(prob, T, B)
    v.reset(*init)
    s.setVariable(v)
    log = s.mpcRun(t0, x0, n_ticks, sim_dt, sim_substeps=substeps, use_feedback=feedback)
    out = {"log_" + k: a for k, a in log.items()}
    out.update(outputs(s))
    return out


def statuses_case(F):
    """The inputs of tests/test_gpu_fmpc.py::test_statuses_succeeded_error_and_invalid_variable (instance 5's converged point comes
    from a long solve on the library under test), then the negative slack of its checkVariable part."""
    prob = F.FmpcProblemOscillator()
    B, T = 66, 20
    var = F.Variable.make(prob, T, B)
    var.reset(0.0, 0.0, 0.0, 1.0, 1.0)
    x0 = np.tile([0.0, 1.0], (B, 1))
    one = F.FmpcSolverBatch(prob, 1, T)
    one.config().max_iter = 60
    v1 = F.Variable.make(prob, T, 1)
    v1.reset(0.0, 0.0, 0.0, 1.0, 1.0)
    assert one.solve(0.0, x0[5:6], v1)[0] == 1
    for a, c in zip(var.arrays(), one.variable().arrays()):
        a[5] = c[0]
    be = np.full(B, 1e-4)
    be[5] = one.barrierEps()[0]
    x0[9, 0] = np.nan
    var.x_list[10, 3, 0] = np.nan
    a = solve_case(F, prob, var, np.array(x0), 0.0, 3, barrier_eps=be)
    assert a["status"][5] == 1 and a["status"][9] == 2 and a["status"][10] == 3, a["status"]
    var.s_list[17, 3, 1] = -1e-3
    b = solve_case(F, prob, var, x0, 0.0, 3)
    assert b["status"][17] == F.STATUS_INVALID_VARIABLE
    return {"first_" + k: v for k, v in a.items()} | {"negative_" + k: v for k, v in b.items()}


def cases(F):
    """(name, thunk) of every case; environment switches are read when a handle is created."""
    out = []

    def add(name, fn, env=None):
        def run():
            for k in ("NMPC_HIP_FMPC_RICCATI", "NMPC_HIP_FMPC_TAIL"):
                os.environ.pop(k, None)
            os.environ.update(env or {})
            return fn()
        out.append((name, run))

    sequences = (("lane", {"NMPC_HIP_FMPC_RICCATI": "lane"}, "fmpc_riccati_kernel"), ("quad", {"NMPC_HIP_FMPC_RICCATI": "quad"}, "fmpc_riccati_quad_kernel"),
                 ("fused_tail", {"NMPC_HIP_FMPC_RICCATI": "fused", "NMPC_HIP_FMPC_TAIL": "1"}, "fmpc_tail_kernel"),
                 ("fused_separate", {"NMPC_HIP_FMPC_RICCATI": "fused", "NMPC_HIP_FMPC_TAIL": "0"}, "fmpc_riccati_fused_kernel"))
    switches = (("line_search", dict(enable_line_search=True)),
                ("line_search_lagrange", dict(enable_line_search=True, merit_const_scale_from_lagrange_multipliers=True)),
                ("init_complementary", dict(init_complementary_variable=True)), ("fixed_barrier_eps", dict(update_barrier_eps=False)))
    for k, model in enumerate(("fmpc_oscillator", "fmpc_cartpole", "fmpc_pointmass")):
        for B, T, max_iter in ((130, 30, 4), (70, 57, 5)):  # (neither batch is a multiple of 64)
            for seq, env, kernel in sequences:
                if model == "fmpc_pointmass" and seq != "lane":
                    continue  # (two inputs: the lane kernel is what runs anyway)
                add(f"{model}/{seq}/B{B}T{T}", lambda model=model, B=B, T=T, max_iter=max_iter, kernel=kernel, k=k: solve_case(
                    F, *fixed_case(F, model, B, T, seed=B + T + k), max_iter, expect=(kernel,)), env)
        for name, opts in switches:
            for seq, env, _ in sequences[:1] + sequences[2:3]:
                if model == "fmpc_pointmass" and seq != "lane":
                    continue
                add(f"{model}/{seq}/{name}", lambda model=model, opts=opts, k=k: solve_case(
                    F, *fixed_case(F, model, 96 + 5, 25, seed=11 + k), 4, barrier_eps=np.linspace(1e-4, 1e-1, 101), **opts), env)
    # one partial backward chunk and an idle second producer wave / two backward chunks in a batch of one / an odd number of backward
    # chunks and a partial last forward chunk
    for model, B, T in (("fmpc_cartpole", 17, 3), ("fmpc_oscillator", 1, 5), ("fmpc_oscillator", 33, 12)):
        for seq, env, kernel in sequences[1:]:
            add(f"{model}/{seq}/B{B}T{T}", lambda model=model, B=B, T=T, kernel=kernel: solve_case(
                F, *fixed_case(F, model, B, T, seed=7), 2, expect=(kernel,), second_iteration=False), env)
    add("statuses", lambda: statuses_case(F))
    rng = np.random.default_rng(0)
    x_osc = np.tile([0.0, 1.0], (70, 1)) + 0.2 * rng.standard_normal((70, 2))
    x_osc[:, 1] = np.maximum(x_osc[:, 1], 0.2)
    x_cp = np.tile([0.0, np.pi, 0.0, 0.0], (48, 1)) + 0.05 * rng.standard_normal((48, 4))
    x_pm = 0.3 * rng.standard_normal((33, F.FmpcProblemPointMass().state_dim))
    for fb in (False, True):
        add(f"loop/oscillator/feedback{int(fb)}", lambda fb=fb: loop_case(F, F.FmpcProblemOscillator(0.01), 70, 100, 3, x_osc, 0.0, 300, 0.005, 1, fb,
                                                                          (0.0, 0.0, 0.0, 1.0, 1.0)))
        add(f"loop/cartpole/feedback{int(fb)}", lambda fb=fb: loop_case(F, F.FmpcProblemCartPole(0.01), 48, 100, 5, x_cp, 0.0, 300, 0.002, 2, fb,
                                                                        (0.0, 0.0, 0.0, 1.0, 1.0)))
        add(f"loop/pointmass/feedback{int(fb)}", lambda fb=fb: loop_case(F, F.FmpcProblemPointMass(), 33, 40, 4, x_pm, 0.0, 100, 0.01, 2, fb,
                                                                         (0.0, 0.0, 0.0, 1.0, 1.0), enable_line_search=fb))
    for B, T, max_iter in ((63, 100, 6), (130, 37, 4)):
        add(f"vertical/B{B}T{T}", lambda B=B, T=T, max_iter=max_iter: solve_case(F, *vertical_case(F, B, T, seed=B + T), max_iter,
                                                                                 expect=("fmpc_update_dims_kernel",)))
    for name, opts in switches:
        add(f"vertical/{name}", lambda opts=opts: solve_case(F, *vertical_case(F, 101, 60, seed=21), 4, **opts))
    x_v = np.tile([1.0, 0.0], (16, 1)) + np.linspace(0, 0.05, 16)[:, None] * np.array([1.0, 0.0])
    for fb in (False, True):
        add(f"loop/vertical/feedback{int(fb)}", lambda fb=fb: loop_case(F, F.FmpcProblemVerticalMotion(), 16, 100, 10, x_v, np.zeros(16), 600, 0.01, 1,
                                                                        fb, (1.0, 9.80665, 0.0, 1.0, 1.0), kkt_error_thre=1e-6))
    return out


def bits_worker(path):
    from nmpc_amd import fmpc as F
    arrays = {}
    for name, run in cases(F):
        for k, v in run().items():
            arrays[name + "|" + k] = np.asarray(v)
        print("ran", name, flush=True)
    np.savez(path, **arrays)


def time_worker(which):
    from nmpc_amd import fmpc as F
    if which in ("quad", "lane"):
        os.environ["NMPC_HIP_FMPC_RICCATI"] = which
    B, T, max_iter = 4096, 200, 5
    prob = F.FmpcProblemCartPole(0.01)
    rng = np.random.default_rng(12345)
    x0 = np.zeros((B, 4))
    x0[:, 0] = rng.uniform(-1, 1, B)
    x0[:, 1] = np.pi + rng.uniform(-0.3, 0.3, B)
    s = F.FmpcSolverBatch(prob, B, T)
    s.config().max_iter = max_iter
    s.config().enable_line_search = which == "line_search"
    var = F.Variable.make(prob, T, B)
    var.reset(0.0, 0.0, 0.0, 1.0, 1.0)
    be = np.full(B, 1e-4)

    def solves(n):
        rows = []
        for _ in range(n):
            s.setVariable(var, barrier_eps=be)
            s.solve(0.0, x0)
            d = s.computationDuration()
            rows.append(dict(d.kernels or {}, solve=d.solve))
        return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}

    solves(3)
    graph = solves(7)["solve"]  # the hipGraph of the solve, replayed
    s.config().time_kernels = True
    solves(2)
    row = solves(7)
    row["solve_events"] = row.pop("solve")  # (stream launches with an event pair around each)
    row["solve"] = graph
    row["kernels"] = ",".join(s.kernelNames())
    print("RESULT " + json.dumps(row), flush=True)


def child(lib, args, timeout):
    env = dict(os.environ, NMPC_HIP_DDP_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=timeout)
    if r.returncode != 0:  # (a fault included: nothing more is started on the GPU)
        sys.stdout.write(r.stdout)
        raise SystemExit("child failed with status %d on %s" % (r.returncode, lib))
    return r.stdout


def bits(lib_a, lib_b, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    paths = [os.path.join(out_dir, "bits_%s.npz" % t) for t in "ab"]
    for lib, p in zip((lib_a, lib_b), paths):
        text = child(lib, ["bits-worker", p], 900)
        print(lib, ":", text.count("\nran ") + text.startswith("ran "), "cases ran")
    a, b = np.load(paths[0]), np.load(paths[1])
    assert sorted(a.files) == sorted(b.files), "the libraries returned different sets of arrays"
    differing = 0
    for k in a.files:
        x, y = a[k], b[k]
        if x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes():
            continue
        differing += 1
        if x.shape != y.shape:
            print("DIFFERENT", k, "shapes", x.shape, y.shape)
            continue
        word = {8: np.uint64, 4: np.uint32}[x.itemsize]
        neq = np.flatnonzero(np.ascontiguousarray(x).reshape(-1).view(word) != np.ascontiguousarray(y).reshape(-1).view(word))
        j = np.unravel_index(int(neq[0]), x.shape)
        print("DIFFERENT", k, "%d of %d entries, first at" % (len(neq), x.size), j, repr(x[j]), repr(y[j]))
    cases_n = len({k.split("|")[0] for k in a.files})
    print("%d cases, %d arrays, %d differ" % (cases_n, len(a.files), differing))
    return 1 if differing else 0


def timing(lib_a, lib_b, out_path, reps):
    table = {}
    for which in ("shipped", "quad", "lane", "line_search"):
        rows = {"a": [], "b": []}
        for _ in range(reps):
            for tag, lib in (("a", lib_a), ("b", lib_b)):
                text = child(lib, ["time-worker", which], 300)
                rows[tag].append(json.loads(next(ln for ln in text.splitlines() if ln.startswith("RESULT "))[7:]))
        res = {"kernels": rows["a"][0]["kernels"], "rows": {}}
        for k in rows["a"][0]:
            if k == "kernels" or max(r[k] for r in rows["a"]) == 0.0:
                continue
            va, vb = [r[k] for r in rows["a"]], [r[k] for r in rows["b"]]
            spread = max(va) - min(va)
            res["rows"][k] = {"a_median_ms": float(np.median(va)), "a_spread_ms": spread, "b_median_ms": float(np.median(vb)),
                              "b_spread_ms": max(vb) - min(vb), "b_not_slower": bool(np.median(vb) <= np.median(va) + spread), "a_ms": va, "b_ms": vb}
            print("%-12s %-12s A %9.4f (spread %.4f)  B %9.4f (spread %.4f)  %s" % (
                which, k, np.median(va), spread, np.median(vb), max(vb) - min(vb), "ok" if res["rows"][k]["b_not_slower"] else "SLOWER"), flush=True)
        table[which] = res
    out = {"what": "FMPC cart-pole 4096 x T 200, max_iter 5, fp64: milliseconds per solve and per kernel class (config.time_kernels, sum over the "
                   "solve's launches); per process the median of 7 solves, %d processes per library, alternating; spread = max - min over the "
                   "processes; solve = hipGraph replay, solve_events = stream launches with event pairs" % reps,
           "a": lib_a, "b": lib_b, "repetitions": reps, "configurations": table}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)
    return 0 if all(r["b_not_slower"] for c in table.values() for r in c["rows"].values()) else 1


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "bits-worker":
        bits_worker(sys.argv[2])
    elif mode == "time-worker":
        time_worker(sys.argv[2])
    elif mode == "bits":
        sys.exit(bits(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else tempfile.mkdtemp(prefix="fmpc_lib_ab_")))
    elif mode == "time":
        sys.exit(timing(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]) if len(sys.argv) > 5 else 5))
    else:
        raise SystemExit(__doc__)
