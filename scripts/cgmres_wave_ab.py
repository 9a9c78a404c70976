"""C/GMRES: the wave kernel (one wavefront per controller, the tick in LDS) against the lane kernel (one lane per controller) on one
MI355X, in ONE process: two handles of the same fleet of bounded cart-poles (N 25, k_max 5, Euler horizon, RK4 plant, logging off,
perturbed swing-up starts), warmed up, alternated (which kernel goes first flips every repetition), five repetitions, medians and
spread.  For B = 1, 64, 256, 1024, 4096, 16384:

  (a) one control_input_device tick, HIP events around the call: both handles are set up and fed the same 250 recorded closed-loop
      states (x, next_x, t of a lane run), so that GMRES does the work of a real tick; median of ticks 50 .. 249 per repetition.
  (b) wall time of run() over 2 s of simulation (2001 ticks; setup and the final synchronise included).

The results of the two kernels are equal bit for bit (tests/test_gpu_cgmres_wave.py); the script checks the inputs of its last tick.

  python scripts/cgmres_wave_ab.py [--sizes 1,64,...] [--reps 5] [--sim 2] [--no-run] [--no-tick] [--out profiles/cgmres_wave_ab.json]
  rocprofv3 --kernel-trace --stats ... -- python scripts/cgmres_wave_ab.py --trace-leg 1024     (the wave run kernel alone, 2 s)

Each invocation is one process; run it under `timeout -k 10 <s>`.  Committed result: profiles/cgmres_wave_ab.json, kernel trace of
the B = 1024 leg: profiles/cgmres_wave_kernel_stats.csv."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nmpc_amd import cgmres  # noqa: E402

MODEL = "cgmres_cartpole_with_input_bound"
KERNELS = ("lane", "wave")
WARM, TICKS = 50, 250


def fleet(B, kernel):
    s = cgmres.CgmresSolverBatch(cgmres.CgmresProblemCartPole(with_input_bound=True), B, ode_solver="euler", sim_ode_solver="rk4")
    s.setKernel(kernel)
    rng = np.random.default_rng(0)
    s.setInitial(s.problem_.x_initial_ + 0.1 * rng.standard_normal((B, s.problem_.dim_x_)))
    s.dump_step_ = 0
    return s


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "reps": list(v)}


class Hip:
    """The few HIP runtime calls the tick leg needs, through ctypes on the runtime the library itself uses."""

    def __init__(self):
        import ctypes as C
        self.C = C
        self.rt = C.CDLL("libamdhip64.so")

    def ok(self, rc):
        assert rc == 0, "HIP error %d" % rc

    def upload(self, a):
        C = self.C
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = C.c_void_p()
        self.ok(self.rt.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)))
        self.ok(self.rt.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1))  # host to device
        return p

    def download(self, p, shape):
        C = self.C
        a = np.zeros(shape)
        self.ok(self.rt.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, C.c_size_t(a.nbytes), 2))  # device to host
        return a

    def handle(self, create):
        p = self.C.c_void_p()
        self.ok(create(self.C.byref(p)))
        return p


def tick_leg(B, reps):
    import ctypes as C
    hip = Hip()
    h = {k: fleet(B, k) for k in KERNELS}
    rec = h["lane"]
    rec.sim_duration_ = (TICKS - 1) * rec.dt_ + 0.5 * rec.dt_
    rec.dump_step_ = 1
    rec.run()
    ts, lx = rec.log_t(), rec.log_x()
    assert len(ts) == TICKS
    rec.dump_step_ = 0
    nx, nuc = rec.problem_.dim_x_, rec.problem_.dim_uc_
    xs = hip.upload(np.concatenate([rec.x_initial_[None], np.moveaxis(lx, 1, 0)]))  # [TICKS + 1][B][NX]
    tt = hip.upload(np.repeat(ts[:, None], B, axis=1))  # [TICKS][B]
    u = {k: hip.upload(np.zeros((B, nuc))) for k in KERNELS}
    stream = hip.handle(hip.rt.hipStreamCreate)
    ev = [(hip.handle(hip.rt.hipEventCreate), hip.handle(hip.rt.hipEventCreate)) for _ in range(TICKS)]
    L = cgmres.load()
    at = lambda p, off: C.c_void_p(p.value + 8 * off)  # noqa: E731
    med = {k: [] for k in KERNELS}
    for r in range(reps + 1):  # repetition 0 warms both kernels up and is dropped
        for k in (KERNELS if r % 2 == 0 else KERNELS[::-1]):
            s = h[k]
            s.setup()
            for i in range(TICKS):
                hip.ok(hip.rt.hipEventRecord(ev[i][0], stream))
                cgmres.check(L.nmpc_hip_cgmres_control_input_device(s._h, at(tt, i * B), at(xs, i * B * nx), at(xs, (i + 1) * B * nx), u[k], stream))
                hip.ok(hip.rt.hipEventRecord(ev[i][1], stream))
            hip.ok(hip.rt.hipStreamSynchronize(stream))
            if r > 0:
                ms = []
                for i in range(WARM, TICKS):
                    f = C.c_float()
                    hip.ok(hip.rt.hipEventElapsedTime(C.byref(f), ev[i][0], ev[i][1]))
                    ms.append(f.value)
                med[k].append(statistics.median(ms))
    same = np.array_equal(hip.download(u["lane"], (B, nuc)), hip.download(u["wave"], (B, nuc))) and np.array_equal(h["lane"].u_list_, h["wave"].u_list_)
    for p in [xs, tt] + list(u.values()):
        hip.rt.hipFree(p)
    for e0, e1 in ev:
        hip.rt.hipEventDestroy(e0)
        hip.rt.hipEventDestroy(e1)
    hip.rt.hipStreamDestroy(stream)
    same = bool(same)
    out = {"B": B, "same_bits": same, "lane_ms": spread(med["lane"]), "wave_ms": spread(med["wave"])}
    out["lane_over_wave"] = out["lane_ms"]["median"] / out["wave_ms"]["median"]
    out["difference_ms"] = out["lane_ms"]["median"] - out["wave_ms"]["median"]
    out["lane_spread_ms"] = out["lane_ms"]["max"] - out["lane_ms"]["min"]
    out["wave_faster_beyond_lane_spread"] = out["difference_ms"] > out["lane_spread_ms"]
    return out


def run_leg(B, reps, sim):
    h = {k: fleet(B, k) for k in KERNELS}
    wall = {k: [] for k in KERNELS}
    for s in h.values():
        s.sim_duration_ = sim
    for r in range(reps + 1):
        for k in (KERNELS if r % 2 == 0 else KERNELS[::-1]):
            t0 = time.perf_counter()
            h[k].run()
            if r > 0:
                wall[k].append(time.perf_counter() - t0)
    n_ticks, t = 0, 0.0
    while t <= sim:  # as run() counts them
        n_ticks += 1
        t += h["lane"].dt_
    same = np.array_equal(h["lane"].x_, h["wave"].x_) and np.array_equal(h["lane"].u_list_, h["wave"].u_list_)
    out = {"B": B, "sim_s": sim, "ticks": n_ticks, "same_bits": bool(same), "lane_wall_s": spread(wall["lane"]), "wave_wall_s": spread(wall["wave"])}
    for k in KERNELS:
        out[k + "_ms_per_tick"] = 1e3 * out[k + "_wall_s"]["median"] / n_ticks
    out["lane_over_wave"] = out["lane_wall_s"]["median"] / out["wave_wall_s"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,256,1024,4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sim", type=float, default=2.0)
    ap.add_argument("--no-run", action="store_true")
    ap.add_argument("--no-tick", action="store_true")
    ap.add_argument("--trace-leg", type=int, default=0, help="only run() of the wave kernel at this batch (for rocprofv3)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.trace_leg:
        s = fleet(a.trace_leg, "wave")
        s.sim_duration_ = a.sim
        s.run()
        print(json.dumps({"B": a.trace_leg, "kernel": s.kernelName(), "event_ms": s.lastDurationMs()}))
        return
    res = {"scenario": "%s, dt 1e-3, N 25, k_max 5, Euler horizon, RK4 simulation, logging off, perturbed starts" % MODEL,
           "wave_lds_bytes": cgmres.wave_lds_bytes(MODEL, 25, 5), "reps": a.reps, "tick": [], "run": []}
    for B in [int(v) for v in a.sizes.split(",") if v]:
        if not a.no_tick:
            leg = tick_leg(B, a.reps)
            print(json.dumps(leg), flush=True)
            res["tick"].append(leg)
        if not a.no_run:
            leg = run_leg(B, a.reps, a.sim)
            print(json.dumps(leg), flush=True)
            res["run"].append(leg)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
