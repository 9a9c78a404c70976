"""BoxQP throughput on one MI355X: QPs per second of nmpc_hip_boxqp_solve_device on device-resident inputs, per kernel.

Shapes (n, B): (2, 65536), (8, 65536), (16, 65536) — full chips; (8, 256), (16, 256) — the small batches at which a lane-per-QP
kernel leaves most compute units idle (the crossover of the automatic choice); (32, 4096), (64, 4096) — wave kernel only.  Every shape
runs on every kernel that supports it.  The QPs are random SPD problems with generic boxes, started from zero (seeded, generated on
the device).  Timing: HIP events on a torch stream around `reps` back-to-back solve_device calls; every (shape, kernel) is warmed
up, the kernels of a shape ALTERNATE over at least `--rounds` rounds in this one process, and rounds are added until each (shape,
kernel) has accumulated `--min-seconds` (0.5) of device time.  Reported: QPs/s over all rounds, and the slowest / fastest round.  The time of a lane solve
includes its ingest kernels (the layout conversion is part of handing the device a QP).

  python scripts/boxqp_throughput.py [--shapes 2x65536,8x256,...] [--rounds 5] [--out profiles/boxqp_throughput.json]

One process; run it under `timeout -k 10 <s>`.  Result of the committed run: profiles/boxqp_throughput.json."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nmpc_amd import boxqp  # noqa: E402

SHAPES = "2x65536,8x65536,16x65536,8x256,16x256,32x4096,64x4096"


def make_inputs(n: int, B: int, seed: int):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *shape: torch.rand(*shape, generator=gen, device="cuda", dtype=torch.float64)  # noqa: E731
    A = torch.randn(B, n, n, generator=gen, device="cuda", dtype=torch.float64)
    H = (A @ A.transpose(1, 2) + 0.3 * torch.eye(n, device="cuda", dtype=torch.float64)).contiguous()
    H = (0.5 * (H + H.transpose(1, 2))).contiguous()
    g = 2 * torch.randn(B, n, generator=gen, device="cuda", dtype=torch.float64)
    lower = -(0.1 + 1.4 * rnd(B, n))
    upper = 0.1 + 1.4 * rnd(B, n)
    return H, g, lower, upper


def timed(qp, inputs, stream, reps: int) -> float:
    """Device seconds of `reps` solves."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        qp.solve_device(*inputs, stream=stream)
    e1.record(stream)
    e1.synchronize()
    return 1e-3 * e0.elapsed_time(e1)


def run_shape(n: int, B: int, rounds: int, min_seconds: float):
    import torch
    inputs = make_inputs(n, B, seed=1000 * n + B % 997)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    kernels = (["lane"] if n <= boxqp.LANE_MAX_DIM else []) + ["wave"]
    legs = {}
    auto = boxqp.BoxQPBatch(n, B).kernelName()
    for k in kernels:
        qp = boxqp.BoxQPBatch(n, B)
        qp.setKernel(k)
        timed(qp, inputs, stream, 2)  # warm-up: code object load, first touch of the workspace
        t1 = timed(qp, inputs, stream, 3) / 3
        reps = max(1, math.ceil(min_seconds / rounds / t1))
        ret = qp.retval_
        legs[k] = {"qp": qp, "reps": reps, "seconds": [], "retval": ret, "x": qp.x(),
                   "mean_iter": float(qp.iter().mean()), "retval_counts": {str(r): int((ret == r).sum()) for r in np.unique(ret)}}
    done = 0
    while done < rounds or min(sum(legs[k]["seconds"]) for k in kernels) < min_seconds:  # the kernels alternate
        for k in kernels:
            legs[k]["seconds"].append(timed(legs[k]["qp"], inputs, stream, legs[k]["reps"]))
        done += 1
    out = {"n": n, "B": B, "automatic_choice": auto, "kernels": {}}
    for k in kernels:
        leg = legs[k]
        per_round = [B * leg["reps"] / s for s in leg["seconds"]]
        out["kernels"][k] = {"reps_per_round": leg["reps"], "rounds": done, "timed_seconds": sum(leg["seconds"]),
                             "qps_per_s": B * leg["reps"] * done / sum(leg["seconds"]), "qps_per_s_slowest_round": min(per_round),
                             "qps_per_s_fastest_round": max(per_round), "ms_per_solve": 1e3 * sum(leg["seconds"]) / (leg["reps"] * done),
                             "mean_iter": leg["mean_iter"], "retval_counts": leg["retval_counts"]}
    if len(kernels) == 2:  # faster and different is not faster
        a, b = legs["lane"], legs["wave"]
        out["kernels_agree"] = {"retval_equal_frac": float((a["retval"] == b["retval"]).mean()),
                                "max_abs_x_diff": float(np.abs(a["x"] - b["x"]).max())}
        out["wave_over_lane"] = out["kernels"]["wave"]["qps_per_s"] / out["kernels"]["lane"]["qps_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s]
    res = {"what": "QPs per second of solve_device on resident inputs (HIP events, kernels alternating per round), random SPD box QPs "
                   "from a zero start, default configuration", "shapes": []}
    for n, B in shapes:
        leg = run_shape(n, B, a.rounds, a.min_seconds)
        print(json.dumps(leg), flush=True)
        res["shapes"].append(leg)
        if a.out:  # (written after every shape: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
