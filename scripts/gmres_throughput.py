"""Batched GMRES throughput on one MI355X: systems per second of nmpc_hip_gmres_solve_device on device-resident inputs
(gmres_wave_kernel, one wavefront per system), and on the same systems the lane-per-system diagnostic nmpc_hip_cgmres_dense_gmres
through its own entry point.

Shapes: n in {10, 50, 100, 500} x B in {10, 256, 4096}, full k_max (= n), eps 1e-10, systems with entries uniform in [-1, 1] from a
zero start (seeded, generated on the device); the Givens variant everywhere, the Householder variant where its k_max bound allows
(n <= 128).  Wave legs: HIP events around each solve_device (nmpc_hip_gmres_last_ms), solves repeated until a leg has accumulated
`--min-seconds` (0.5) of device time; between two solves the system is handed over again (set_system with the transposed image on
the device: nothing but b and x is copied), because a second solve would otherwise restart from the first's solution.  Lane legs:
the diagnostic takes HOST arrays and allocates, copies and frees in every call, so what is timed is the wall time of the call —
that is what a caller of that entry point pays; calls are repeated until 0.5 s or `--lane-max-calls`.

  python scripts/gmres_throughput.py [--shapes 10x10,500x4096,...] [--skip-lane] [--out profiles/gmres_throughput.json]

One process; run it under `timeout -k 10 <s>`.  Result of the committed run: profiles/gmres_throughput.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nmpc_amd import cgmres, gmres  # noqa: E402

SHAPES = ",".join("%dx%d" % (n, B) for n in (10, 50, 100, 500) for B in (10, 256, 4096))


def wave_leg(n, B, At, b, make_triangular, min_seconds):
    s = gmres.GmresBatch(n, B, k_max_capacity=n)
    s.make_triangular_ = make_triangular
    ms = []
    while len(ms) < 2 or sum(ms[1:]) < 1e3 * min_seconds:  # the first solve is the warm-up
        s.set_system_device(At, b, None, a_col_major=True)
        s.solve_device(k_max=n, eps=1e-10)
        ms.append(s.lastMs())
    timed = ms[1:]
    status = s.status()
    return s, {"solves": len(timed), "timed_seconds": 1e-3 * sum(timed), "ms_per_solve": float(np.mean(timed)), "ms_per_solve_min": min(timed),
               "ms_per_solve_max": max(timed), "systems_per_s": B * len(timed) / (1e-3 * sum(timed)), "mean_iters": float(s.iters().mean()),
               "status_counts": {str(v): int((status == v).sum()) for v in np.unique(status)}}


def lane_leg(n, B, A_host, b_host, min_seconds, max_calls):
    secs = []
    x = None
    while len(secs) < 2 or (sum(secs[1:]) < min_seconds and len(secs) - 1 < max_calls):
        t = time.perf_counter()
        x, iters, _ = cgmres.dense_gmres(A_host, b_host, k_max=n, apply_reorth=True, eps=1e-10)
        secs.append(time.perf_counter() - t)
        if len(secs) == 1 and secs[0] > 20 * min_seconds:
            break  # one call already took many times the leg's time: it is the measurement
    timed = secs[1:] or secs
    return x, {"calls": len(timed), "timed_seconds": sum(timed), "ms_per_call": 1e3 * float(np.mean(timed)), "ms_per_call_min": 1e3 * min(timed),
               "systems_per_s": B * len(timed) / sum(timed), "mean_iters": float(np.mean(iters)), "timing": "wall time of the host call"}


def run_shape(n, B, a):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(1000 * n + B % 997)
    A = 2 * torch.rand(B, n, n, generator=gen, device="cuda", dtype=torch.float64) - 1
    b = 2 * torch.rand(B, n, generator=gen, device="cuda", dtype=torch.float64) - 1
    At = A.transpose(1, 2).contiguous()
    torch.cuda.synchronize()
    out = {"n": n, "B": B, "k_max": n}
    s, out["wave_triangular"] = wave_leg(n, B, At, b, True, a.min_seconds)
    x_wave = s.x()
    del s
    if n <= gmres.HOUSEHOLDER_MAX_K:
        _, out["wave_householder"] = wave_leg(n, B, At, b, False, a.min_seconds)
    if not a.skip_lane:
        del At
        A_host, b_host = A.cpu().numpy(), b.cpu().numpy()
        del A
        torch.cuda.empty_cache()
        x_lane, out["lane"] = lane_leg(n, B, A_host, b_host, a.min_seconds, a.lane_max_calls)
        out["wave_over_lane"] = out["wave_triangular"]["systems_per_s"] / out["lane"]["systems_per_s"]
        ok = np.isfinite(x_lane).all(axis=1) & np.isfinite(x_wave).all(axis=1)
        out["max_rel_x_diff_wave_vs_lane"] = float((np.abs(x_wave - x_lane)[ok] / (1 + np.abs(x_lane)[ok])).max()) if ok.any() else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--lane-max-calls", type=int, default=50)
    ap.add_argument("--skip-lane", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s]
    res = {"what": "systems per second, full k_max = n, eps 1e-10, uniform [-1, 1] systems from a zero start; wave legs: solve_device on resident "
                   "inputs (HIP events per solve); lane legs: nmpc_hip_cgmres_dense_gmres on host arrays (wall time of the call, which "
                   "allocates, copies and frees)", "shapes": []}
    for n, B in shapes:
        leg = run_shape(n, B, a)
        print(json.dumps(leg), flush=True)
        res["shapes"].append(leg)
        if a.out:  # (written after every shape: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
