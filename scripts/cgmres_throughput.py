"""C/GMRES closed-loop throughput on one MI355X: the reference's 20 s cart-pole scenario (bounded input, Euler inside the horizon,
RK4 simulation, logging off) at B = 1024, 4096, 16384, 65536, in instance-ticks per second (wall time of run(): setup + every
tick launch); the CPU checker (tests/cpp/cgmres_checker.cpp) on 16 threads as the CPU column; the latency of one
calcControlInput tick through nmpc_hip_cgmres_control_input_device at B = 4096.  Writes one JSON object.

  python scripts/cgmres_throughput.py [--sizes 1024,4096,...] [--no-cpu] [--no-latency] [--out profiles/r07_cgmres_throughput.json]

Each invocation is one process; run it under `timeout -k 10 <s>`.  Result of the committed run: profiles/r07_cgmres_throughput.json,
kernel trace of the B = 4096 leg: profiles/r07_cgmres_kernel_stats.csv."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from nmpc_amd import cgmres  # noqa: E402

MODEL = "cgmres_cartpole_with_input_bound"


def gpu_leg(B: int, sim: float):
    s = cgmres.CgmresSolverBatch(cgmres.CgmresProblemCartPole(with_input_bound=True), B, ode_solver="euler", sim_ode_solver="rk4")
    s.sim_duration_ = sim
    s.dump_step_ = 0
    s.run()  # warm-up (module load, first-touch)
    t0 = time.perf_counter()
    s.run()
    wall = time.perf_counter() - t0
    n_ticks = 0
    t = 0.0
    while t <= sim:
        n_ticks += 1
        t += s.dt_
    x = s.x_
    return {"B": B, "ticks": n_ticks, "wall_s": wall, "event_ms": s.lastDurationMs(), "instance_ticks_per_s": B * n_ticks / wall,
            "max_final_norm_x": float(np.linalg.norm(x, axis=1).max()), "all_succeeded": bool((s.status() == 1).all())}


def cpu_leg(B: int, sim: float, threads: int):
    import cgmres_checker
    chk = cgmres_checker.build(tempfile.mkdtemp(prefix="cgmres_chk_"))
    cfg = {n: getattr(cgmres.default_config(), n) for n, _ in cgmres.CConfig._fields_}
    cfg.update(sim_duration=sim, dump_step=0, ode_solver=0, sim_ode_solver=1)
    x0, u0 = cgmres_checker.initial(MODEL)
    t0 = time.perf_counter()
    r = chk.solve(MODEL, cfg, np.tile(x0, (B, 1)), np.tile(u0, (B, 1)), n_threads=threads)
    wall = time.perf_counter() - t0
    return {"B": B, "threads": threads, "ticks": r.n_ticks, "wall_s": wall, "instance_ticks_per_s": B * r.n_ticks / wall}


def latency_leg(B: int, reps: int):
    """Wall time of one nmpc_hip_cgmres_control_input_device call on device arrays (launch + kernel + synchronize), t = 1 s."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    s = cgmres.CgmresSolverBatch(cgmres.CgmresProblemCartPole(with_input_bound=True), B, ode_solver="euler", sim_ode_solver="rk4")
    s.setup()
    nx, nuc = s.problem_.dim_x_, s.problem_.dim_uc_
    host = {"t": np.full(B, 1.0), "x": np.tile(s.problem_.x_initial_, (B, 1)), "u": np.zeros((B, nuc))}
    dev = {}
    for k, a in host.items():
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0  # host to device
        dev[k] = p
    L = cgmres.load()
    out = []
    for i in range(reps + 5):
        t0 = time.perf_counter()
        cgmres.check(L.nmpc_hip_cgmres_control_input_device(s._h, dev["t"], dev["x"], dev["x"], dev["u"], None))
        s.synchronize()
        if i >= 5:
            out.append(1e3 * (time.perf_counter() - t0))
    for p in dev.values():
        hip.hipFree(p)
    out.sort()
    return {"B": B, "reps": reps, "median_ms": out[len(out) // 2], "min_ms": out[0], "max_ms": out[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,16384,65536")
    ap.add_argument("--sim", type=float, default=20.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=64)
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"scenario": "%s, %g s, dt 1e-3, N 25, k_max 5, Euler horizon, RK4 simulation, logging off" % (MODEL, a.sim), "gpu": []}
    for B in [int(v) for v in a.sizes.split(",") if v]:
        leg = gpu_leg(B, a.sim)
        print(json.dumps(leg), flush=True)
        res["gpu"].append(leg)
    if not a.no_cpu:
        res["cpu"] = cpu_leg(a.cpu_batch, a.sim, 16)
        print(json.dumps(res["cpu"]), flush=True)
        best = max(g["instance_ticks_per_s"] for g in res["gpu"]) if res["gpu"] else 0.0
        res["gpu_over_cpu_best"] = best / res["cpu"]["instance_ticks_per_s"]
    if not a.no_latency:
        res["control_input_latency"] = latency_leg(4096, 50)
        print(json.dumps(res["control_input_latency"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
