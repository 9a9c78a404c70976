#!/usr/bin/env python3
"""Generates tests/golden/fmpc_vertical_golden.npz: input -> output vectors of the CPU FMPC oracle on fmpc_vertical, the problem
with time-varying input / inequality dimensions.

The committed file was written by the per-step-dimension checker that tests/ held before oracle/fmpc_oracle.hpp took each step's
dimensions from the model; the oracle has to reproduce every array of it bit for bit (tests/test_fmpc_dynamic_host_cpu.py).  No
transcendental function is involved, so the vectors do not depend on the host's libm.  Data only; regenerate with

    python tests/golden/make_fmpc_vertical_golden.py

Cases (dt 0.01, T 20, B 8): horizons that start at T0 cover the 1 -> 2, 2 -> 1, 1 -> 0 and 0 -> 1 input switches, a horizon with
two inputs throughout, one without any inequality row (barrier parameter 0 / 0) and the reference-position switch at 8.0; the
entries beyond each step's dimensions hold POISON.  Five option sets on one shared problem object, one solve with a problem object
(contact schedule) per instance, and 30 ticks of the closed loop of one instance from the nominal start.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import fmpc as O  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fmpc_vertical_golden.npz")
MODEL = "fmpc_vertical"
POISON = -1234.5
T0 = (1.9, 2.5, 2.9, 4.4, 4.6, 4.9, 5.5, 7.9)
T, MAX_ITER, KKT = 20, 8, 1e-4
OPTION_SETS = {
    "default": {},
    "line_search": dict(enable_line_search=1),
    "init_complementary": dict(init_complementary_variable=1),
    "fixed_barrier": dict(update_barrier_eps=0),
    "line_search_multiplier_scale": dict(enable_line_search=1, merit_const_scale_from_lagrange_multipliers=1),
}
SOLVES = tuple(OPTION_SETS) + ("per_instance",)
LOOP = dict(T=20, max_iter=5, t0=1.9, n_ticks=30, sim_dt=0.01)
VAR = ("x", "u", "lam", "s", "nu")


def make_inputs():
    """The start of make_case(B, T, seed=11) of tests/test_gpu_fmpc_dynamic.py (same draws in the same order) at the times T0."""
    B = len(T0)
    rng = np.random.default_rng(11)
    rng.uniform(0.0, 6.0, B)  # (make_case draws t0 first)
    t0 = np.array(T0)
    x = np.tile([1.0, 0.0], (B, T + 1, 1)) + 0.05 * rng.standard_normal((B, T + 1, 2))
    u = 9.80665 + rng.uniform(-2.0, 2.0, (B, T, 2))
    lam = 0.1 * rng.standard_normal((B, T + 1, 2))
    s = rng.uniform(0.5, 2.0, (B, T, 4))
    nu = rng.uniform(0.5, 2.0, (B, T, 4))
    x0 = np.stack([1.0 + 0.1 * rng.standard_normal(B), 0.1 * rng.standard_normal(B)], axis=1)
    shared = O.default_params(MODEL)
    per_instance = np.tile(shared, (B, 1))
    for b in range(B):  # image: [dt, running_x 2, running_u, terminal_x 2, mass, f_min, f_max, ref_switch_t, ds 2, flight 2]
        per_instance[b, 8] = 30.0 - b
        per_instance[b, 10:14] = [2.0 + 0.05 * b, 3.0 - 0.05 * b, 4.5 + 0.02 * b, 5.0 - 0.02 * b]
    inputs = {"t0": t0, "x0": x0, "params": shared, "per_instance_params": per_instance}
    for name, params in (("in", np.tile(shared, (B, 1))), ("per_instance_in", per_instance)):
        v = [a.copy() for a in (x, u, lam, s, nu)]
        for b in range(B):
            for i in range(T):
                m, g = O.dims_at(MODEL, t0[b] + i * params[b, 0], params[b])
                v[1][b, i, m:] = POISON
                v[3][b, i, g:] = POISON
                v[4][b, i, g:] = POISON
        for k, a in zip(VAR, v):
            inputs[f"{name}_{k}"] = a
    return inputs


def run_solve(name, inputs):
    """Every output of the batched solve `name` (one of SOLVES) from the stored inputs."""
    per = name == "per_instance"
    cfg = O.default_config(horizon_steps=T, max_iter=MAX_ITER, kkt_error_thre=KKT, **OPTION_SETS.get(name, {}))
    prefix = "per_instance_in_" if per else "in_"
    var = O.Variable(*(inputs[prefix + k] for k in VAR))
    r = O.solve_batch_full(MODEL, cfg, inputs["per_instance_params" if per else "params"], inputs["t0"], inputs["x0"], var)
    out = {"status": r.status, "iters": r.iters, "trace": r.trace, "barrier_eps": r.barrier_eps, "k": r.k, "K": r.K,
           "s_gain": r.s, "P": r.P, "merit": r.merit}
    for k, a, d in zip(VAR, r.variable.arrays(), r.delta.arrays()):
        out[k] = a
        out["d" + k] = d
    return out


def run_loop(inputs):
    """The closed loop solve -> log -> plant step of one instance from the nominal, unpoisoned start."""
    Tl = LOOP["T"]
    cfg = O.default_config(horizon_steps=Tl, max_iter=LOOP["max_iter"], kkt_error_thre=KKT)
    var = O.Variable.reset(MODEL, Tl, 1.0, 9.80665, 0.0, 1.0, 1.0, batch=1)
    r = O.closed_loop(MODEL, cfg, inputs["params"], np.array([LOOP["t0"]]), np.array([[1.0, 0.0]]), var, LOOP["n_ticks"],
                           LOOP["sim_dt"])
    return {"x_log": r.x_log, "u0_log": r.u0_log, "status_log": r.status_log, "iter_log": r.iter_log}


def build_store():
    store = dict(make_inputs())
    for name in SOLVES:
        for k, a in run_solve(name, store).items():
            store[f"{name}/{k}"] = a
    for k, a in run_loop(store).items():
        store[f"loop/{k}"] = a
    return store


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(out, **build_store())
    print(len(SOLVES), "solves and one closed loop ->", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
