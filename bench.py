#!/usr/bin/env python3
"""Benchmark of the MI355X DDP hot path.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Metric (BASELINE.json): DDP iterations/s (whole node), batch = 4096 cart-pole instances (nx=4, nu=1, T=100,
fp64) per GPU.  One STEP = one batched `solve()` through the C-ABI with the reference's default
DDPSolver::Configuration except max_iter = --iters-per-solve (default 8, the pre-convergence regime in which an
iteration is nominal: 1 backward + ~1.1 forward passes; the MPC callers of the reference run max_iter = 3).  A DDP
iteration is one DDPSolver::procOnce (DDPSolver.hpp:143-340: linearise + regularised backward pass + line-search
forward pass); instances that meet the reference's termination tests earlier stop earlier, and only iterations that
were actually executed are counted (sum of traceDataList().back().iter over the batch / 4096).  Inputs are already
resident in HBM.  value = n_gpus * K * (executed instance-iterations per solve / 4096) / t, t = max over ranks of the
wall time of the K steps (from a barrier + device-synchronise bracket to the stream synchronise after the last step).  Weak
scaling: every rank owns its own 4096 instances; the only collective is ONE all_gather of the packed results (X | U | cost |
status | iters per shard; RCCL over xGMI) after the timed steps, reported as config.final_gather_ms.  --global-batch G cuts
ONE batch of G instances into contiguous balanced shards instead (strong split, uneven shards padded to one fixed-size
all-gather), --verify-gather compares the gathered records with the unsharded solve.
The CPU baseline leg runs first, the GPU legs last; the timed job is exactly --steps steps after --warmup untimed ones, and
ms_per_step is its wall time / --steps.  --dump-outputs DIR writes what the last timed step returned (X, U, cost, status, iters;
the FMPC workload: its variable, status, iters) as DIR/<name>.npy, for comparing two builds on the same inputs.

After the timed job the default (c2, nominal) run also measures SURVEY.md 8(d)'s two timing modes with the same handle —
m1 (termination tests disabled, N = 50 iterations forced) and m2 (solve to convergence, max_iter 500) — and reports them as
config.m1_value / config.m2_value (batch-iterations/s): outside the timed region, a few solves each; with the CPU oracle's rate in the
same mode beside each (config.m1.cpu_value / config.m2.cpu_value), M2 with eight batches in flight on a pool of handles
(config.m2_overlapped_value) and M2 as a STREAM of 32768 / 262144 instances through the 4096 slots of one handle
(config.m2_stream_value / config.m2_stream_sustained_value: nmpc_hip_ddp_solve_stream).

Multi-GPU: `python bench.py --gpus N` with N > 1 outside a launcher starts the N ranks itself (torch.distributed.run on 127.0.0.1) and
refuses a job with fewer visible devices than ranks (--share-devices: test boxes).  BASELINE config 5 (manipulator, 65536 instances
over 8 GPUs, one RCCL all-gather of the results):   python bench.py --gpus 8 --workload c5 --global-batch 65536

The default line finally carries `secondary`: the other workloads of DESIGN.md 5's table (c3, c4, c4f64, c5, fmpc, centroidal), each
on its own handle, >= --secondary-seconds of back-to-back solves after the c2 job, with value, ms_per_step, kernel and roofline
(contract fraction + the PMC traffic of profiles/hbm_traffic.json when it was measured on these device sources).

The JSON line also carries
  roofline     HBM-roofline accounting of the solve kernel: algorithmic bytes (SURVEY.md §8 d formula with the
               measured backward / forward pass counts) / HIP-event kernel time measured on the launch stream;
  cpu_baseline the CPU oracle ("port" of the reference's Eigen path, oracle/) timed on this host's cores on a
               bounded sample of the same workload.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
LANE_MAPPINGS = {
    "ddp_solve_quad_kernel": "quad: 16 instances per workgroup of 4 wavefronts; backward pass on the fp64 matrix cores "
                             "(16 lanes per instance, v_mfma_f64_4x4x4), linearisation parallel over the horizon, "
                             "forward pass one lane per instance (master + helper wavefront)",
    "ddp_solve_tpi2w_kernel": "one lane per instance, 64 instances per workgroup, master + helper wavefront",
    "ddp_solve_tpi_kernel": "one lane per instance, 64 instances per single-wavefront workgroup",
    "ddp_solve_wpi_kernel": "one wavefront per instance: lane = timestep / matrix entry (v_mfma_f64_16x16x4) / step size",
    "ddp_solve_tile64_kernel": "fp64 tile: groups of up to 32 instances per persistent workgroup of 8 wavefronts; model code one lane "
                               "per instance (linearisation into zero-compacted LDS records, rollouts fed from an LDS ring of the "
                               "nominal), backward pass lane = matrix entry on v_mfma_f64_16x16x4 in natural layout (X^T Y products "
                               "chained in registers), derivatives never in HBM",
    "ddp_solve_tile32_kernel": "fp32 tile: 32 instances per workgroup of 12 wavefronts; model code one lane per instance "
                               "(linearisation into LDS records, rollouts; every step size of the line search at once on the "
                               "other wavefronts), backward pass one 16x16 augmented block per instance on v_mfma_f32_16x16x4",
}


# name -> (generator in nmpc_amd.workloads, per-GPU batch, horizon, description)
WORKLOADS = {
    "c2": ("cartpole_batch", 4096, 100,
           "C2 batched cart-pole swing-up: nx=4, nu=1, T=%d, batch=%d per GPU, fp64, "
           "x0~U([-1,1]x[-pi,pi]x[-1,1]x[-1,1]) splitmix64 seed %d, u_init=0, unconstrained"),
    "c3": ("bipedal_batch", 1024, 300,
           "C3 bipedal CoM-ZMP: nx=2, nu=1, T=%d, batch=%d per GPU, fp64, t0~U[0,17] s on the reference's ref_zmp / "
           "omega^2 schedule, splitmix64 seed %d, u_init=0"),
    "c4": ("quadrotor_batch", 8192, 50,
           "C4 quadrotor: nx=12, nu=4, T=%d, batch=%d per GPU, fp32 (problem type quadrotor_f32), hover-perturbed x0 "
           "splitmix64 seed %d, u_init=hover"),
    "c4f64": ("quadrotor_batch", 8192, 50,
              "C4-shape quadrotor in the reference's arithmetic: nx=12, nu=4, T=%d, batch=%d per GPU, fp64, hover-perturbed "
              "x0 splitmix64 seed %d, u_init=hover"),
    "c5": ("manipulator_batch", 8192, 30,
           "C5-shape manipulator: nx=14, nu=7, T=%d, batch=%d per GPU (65536 over 8 GPUs), fp64, splitmix64 seed %d"),
    "centroidal": ("centroidal_batch", 4096, 100,
                   "centroidal motion (TestDDPCentroidalMotion.cpp: the reference's largest model): nx=9, nu in {16, 0} along the horizon, "
                   "T=%d, batch=%d per GPU, fp64, splitmix64 seed %d"),
}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1,
                    help="ranks of the job, one per GPU.  Under torch.distributed.run (WORLD_SIZE set) it must equal the world size; a plain "
                         "`python bench.py --gpus N` with N > 1 launches the N ranks itself (torch.distributed.run, 127.0.0.1 rendezvous)")
    ap.add_argument("--share-devices", action="store_true",
                    help="allow more ranks than visible devices (rank r on device r %% n_devices, the final gather over gloo because RCCL "
                         "wants one device per rank): the one-GPU test box.  Without it a job with fewer devices than ranks is refused")
    ap.add_argument("--steps", type=int, default=200, help="timed steps (one batched solve each); ms_per_step is their mean")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["fmpc"], default="c2",
                    help="c2 (default) is BASELINE.json's metric configuration; c3 / c4 / c5 are the other configs "
                         "(parity-test cases) measured with the same harness")
    ap.add_argument("--batch", type=int, default=0, help="instances per GPU (0: the workload's own)")
    ap.add_argument("--horizon", type=int, default=0, help="horizon_steps (0: the workload's own)")
    ap.add_argument("--iters-per-solve", type=int, default=8)
    ap.add_argument("--mode", choices=("nominal", "m1", "m2"), default="nominal",
                    help="nominal (default): reference defaults with max_iter = --iters-per-solve.  m1 / m2 are the two "
                         "timing modes of SURVEY.md 8(d): m1 = termination tests disabled (k_rel_norm_thre = 0, "
                         "cost_update_thre = -inf), every instance executes exactly --iters-per-solve iterations unless "
                         "lambda exceeds lambda_max; m2 = solve to convergence with the reference defaults (max_iter 500)")
    ap.add_argument("--cost-update-thre", type=float, default=None,
                    help="override Configuration::cost_update_thre.  c4 (fp32) defaults to 1e-3: the reference's 1e-7 is below the "
                         "resolution of an fp32 cost, where the accept test is rounding noise in the fp32 ORACLE itself (DESIGN.md "
                         "3a); the rate with the reference's default rides along as config.default_threshold_value")
    ap.add_argument("--min-seconds", type=float, default=None,
                    help="no effect: the timed job is exactly --steps steps (accepted so that older command lines still parse)")
    ap.add_argument("--no-extra-modes", action="store_true", help="skip the m1 / m2 (c2) and fp32-tolerance (c4) extra legs")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the secondary legs of the default line (c3, c4, c4f64, c5, fmpc, centroidal: >= --secondary-seconds each, "
                         "after the c2 job and outside its timed region)")
    ap.add_argument("--secondary-seconds", type=float, default=0.6)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=6.0,
                    help="sizing target of the CPU baseline sample (the sustained all-core rate is ~3x below the probe: ~20 s)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed job, write what its last step returned to the caller as DIR/<name>.npy (float32 / float64, "
                         "at most 64 MB in all: a fixed sample of instances beyond that, their indices in instances.npy).  The inputs "
                         "depend on the arguments only, so two builds can be compared output for output")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="strong split: ONE batch of this many instances (the workload's generator, --seed) cut into contiguous, "
                         "balanced shards over the ranks (nmpc_amd.sharding.shard_range: sizes differ by at most one) instead of "
                         "every rank owning its own --batch instances; reports scaling = strong")
    ap.add_argument("--verify-gather", action="store_true",
                    help="after the job rank 0 solves the whole (unsharded) batch on its device and compares the gathered records "
                         "with it bit for bit: config.gather_verified (needs --global-batch)")
    return ap.parse_args()


def mode_config(mode: str, iters_per_solve: int, cost_update_thre=None) -> dict:
    """Configuration overrides of the three timing modes (same for the GPU solver and the CPU oracle)."""
    if mode == "m1":
        return dict(max_iter=iters_per_solve, k_rel_norm_thre=0.0, cost_update_thre=-1e300)
    cfg = dict(max_iter=500 if mode == "m2" else iters_per_solve)
    if cost_update_thre is not None:
        cfg["cost_update_thre"] = cost_update_thre
    return cfg


def host_cores():
    """CPUs this process may actually use: the affinity mask, capped by the cgroup CPU quota when there is one."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = float(q) / float(per)
    except Exception:
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except Exception:
            pass
    return n, quota


def cpu_baseline(wl, mode: str, iters_per_solve: int, target_seconds: float, cost_update_thre=None, extra_modes=()):
    """Time the CPU oracle (kind "port") on a bounded sample of the same workload: a thread sweep (1, 16, 64, all usable
    cores; threads pinned, instances handed out dynamically), the best rate is the baseline.  The first 256 instances' iteration
    counts / statuses are kept (`check_*`): main() compares the GPU's last solve with them (the checker's usual role)."""
    import oracle
    affinity, quota = host_cores()
    usable = affinity if quota is None else max(1, min(affinity, int(quota + 0.5)))
    build_dir = tempfile.mkdtemp(prefix="oracle_native_")
    cfg = oracle.default_config(horizon_steps=wl.T, **mode_config(mode, iters_per_solve, cost_update_thre))

    def run(nb, threads):
        # the sample is the workload's own instances, repeated cyclically when more than one batch is needed
        idx = np.arange(nb) % wl.B
        r = oracle.solve_batch(wl.model, cfg, wl.x0[idx], wl.u_init[idx], t0=wl.t0[idx], n_threads=threads,
                               want_gains=False, native=True, native_dir=build_dir)
        return r.total_iters, r.seconds

    it1, sec1 = run(64, 1)  # probe: one core
    rate1 = it1 / max(sec1, 1e-9)  # instance-iterations / s / core
    per_solve = it1 / 64.0
    sweep = {}
    legs = sorted({1, min(16, usable), min(64, usable), usable})
    budget = target_seconds / len(legs)
    for th in legs:
        guess = rate1 * th * (0.5 if th > 1 else 1.0)  # all-core rates are well below threads x one-core
        nb = int(max(8 * th, 64, guess * budget / max(per_solve, 1.0)))
        it, sec = run(nb, th)
        sweep[th] = {"instance_iterations_per_s": it / sec, "solves": nb, "seconds": sec}
    best = max(sweep, key=lambda k: sweep[k]["instance_iterations_per_s"])
    n_chk = min(256, wl.B)
    chk = oracle.solve_batch(wl.model, cfg, wl.x0[:n_chk], wl.u_init[:n_chk], t0=wl.t0[:n_chk], n_threads=usable, want_gains=False,
                             native=True, native_dir=build_dir)
    # "same M1 / M2 modes" on the CPU — the whole batch once per mode (twice when the first pass took under a second) on the
    # thread count that won the sweep, from the very inputs the GPU legs solve
    modes = {}
    for m_name, m_iters in extra_modes:
        m_cfg = oracle.default_config(horizon_steps=wl.T, **mode_config(m_name, m_iters))
        it_m, sec_m, reps = 0, 0.0, 0
        while reps < 2 and (reps == 0 or sec_m < 1.0):
            r = oracle.solve_batch(wl.model, m_cfg, wl.x0, wl.u_init, t0=wl.t0, n_threads=best, want_gains=False, native=True,
                                   native_dir=build_dir)
            it_m, sec_m, reps = it_m + r.total_iters, sec_m + r.seconds, reps + 1
        modes[m_name] = {"cpu_value": it_m / sec_m / wl.B, "cpu_cores": best, "cpu_seconds": sec_m, "cpu_solves": reps * wl.B,
                         "cpu_mean_iterations": it_m / float(reps * wl.B),
                         "cpu_status_counts": {str(k): int(v) for k, v in zip(*np.unique(r.status, return_counts=True))}}
    return {
        "modes": modes,
        "check_iters": [int(v) for v in chk.iters], "check_status": [int(v) for v in chk.status],
        "value": sweep[best]["instance_iterations_per_s"] / wl.B,  # batch-iterations / s
        "unit": "DDP iterations/s (batch=%d)" % wl.B,
        "cores": best,
        "kind": "port",
        "sample": "oracle/ (%s) built -O3 -march=native on this host; the workload's %d instances cycled, mode %s, max_iter %d; "
                  "thread sweep %s, threads pinned, dynamic chunks; best: %d threads, %d solves in %.1f s.  Host: %d CPUs in the "
                  "affinity mask, cgroup quota %s, os.cpu_count() %d"
                  % (wl.model, wl.B, mode, cfg.max_iter, legs, best, sweep[best]["solves"], sweep[best]["seconds"], affinity,
                     "none" if quota is None else "%.1f CPUs" % quota, os.cpu_count() or 0),
        "instance_iterations_per_s": sweep[best]["instance_iterations_per_s"],
        "instance_iterations_per_s_1core": sweep[1]["instance_iterations_per_s"],
        "thread_sweep": {str(k): round(v["instance_iterations_per_s"], 1) for k, v in sweep.items()},
        "host_cpus_affinity": affinity,
        "host_cpu_quota": quota,
    }


# The other workloads of DESIGN.md 5's table, timed as SECONDARY legs of the default (c2) line so that the driver's record holds them:
# name -> (generator, generator kwargs, batch, horizon, cost_update_thre override)
SECONDARY = {
    "c3": ("bipedal_batch", {}, 1024, 300, None),
    "c4": ("quadrotor_batch", {"fp32": True}, 8192, 50, 1e-3),
    "c4f64": ("quadrotor_batch", {}, 8192, 50, None),
    "c5": ("manipulator_batch", {}, 8192, 30, None),
    "centroidal": ("centroidal_batch", {}, 4096, 100, None),
}


def measured_traffic(name: str, batch: int, iters_per_solve: int, cost_update_thre):
    """(HBM bytes per launch, source, note) of profiles/hbm_traffic.json's entry `name`: used only when it was measured on the device
    sources of this tree (source hash) at this batch / iteration count / threshold."""
    traffic_file = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    try:
        entry = json.load(open(traffic_file)).get(name)
        if not isinstance(entry, dict) or entry.get("batch") != batch or entry.get("iterations_per_step") != iters_per_solve:
            return None, None, None
        if (entry.get("cost_update_thre") or None) != (cost_update_thre or None):
            return None, None, None
        from nmpc_amd import build as hip_build
        src_hash = hip_build.source_hash()
        if entry.get("source_hash") != src_hash:
            return None, None, ("profiles/hbm_traffic.json holds a measurement of other device sources (hash %s, now %s): not used"
                                % (entry.get("source_hash"), src_hash))
        return entry.get("hbm_bytes_per_launch"), entry.get("source"), None
    except Exception:
        return None, None, None


def ddp_secondary_leg(name: str, device_index: int, seed: int, iters_per_solve: int, min_seconds: float):
    """One secondary workload: its own handle, the nominal configuration (reference defaults, max_iter = iters_per_solve), three
    warm-up solves, then >= min_seconds of back-to-back solves with the inputs resident; roofline as for the headline."""
    import torch
    import nmpc_amd
    from nmpc_amd import _capi, workloads
    gen, gen_kw, batch, horizon, thre = SECONDARY[name]
    wl = getattr(workloads, gen)(B=batch, T=horizon, seed=seed, **gen_kw)
    problem = nmpc_amd.make_problem(wl.model)
    elem = float(problem.scalar_bytes())
    solver = nmpc_amd.DDPSolverBatch(problem, wl.B, device=device_index)
    cfg = solver.config()
    cfg.print_level = 0
    cfg.horizon_steps = wl.T
    cfg.max_iter = iters_per_solve
    cfg.trace_level = 1
    if thre is not None:
        cfg.cost_update_thre = thre
    dev = torch.device("cuda", device_index)
    d_x0, d_u0, d_t0 = (torch.from_numpy(a).to(dev) for a in (wl.x0, wl.u_init, wl.t0))

    def step():
        solver.solveDevice(d_t0.data_ptr(), d_x0.data_ptr(), d_u0.data_ptr())

    for _ in range(3):
        step()
    solver.synchronize()
    t0 = time.perf_counter()
    step()
    solver.synchronize()
    n_steps = int(max(4, np.ceil(min_seconds / max(time.perf_counter() - t0, 1e-6))))
    solver.timingStats(reset=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_steps):
        step()
    solver.synchronize()
    dt = time.perf_counter() - t0
    n_l, _, k_ms_sum = solver.timingStats()
    it = solver.iters()
    st = solver.status()
    rows = solver.trace()[:, 1:, :]
    ex = rows[:, :, 0] > 0
    n_ex = max(int(ex.sum()), 1)
    bw = float(rows[:, :, _capi.TRACE_COLUMNS.index("n_backward")][ex].sum()) / n_ex
    fw = float(rows[:, :, _capi.TRACE_COLUMNS.index("n_forward")][ex].sum()) / n_ex
    inst_it = float(it.sum())
    words = workloads.algorithmic_words_per_instance_iteration(wl.n, wl.m, wl.T, bw, fw)
    fused = workloads.fused_words_per_instance_iteration(wl.n, wl.m, wl.T, bw, fw)
    k_ms = k_ms_sum / max(n_l, 1)
    ach = words * elem * inst_it / (k_ms * 1e-3) / 1e9
    traffic, src, note = measured_traffic(name, wl.B, iters_per_solve, thre)
    roof = {"bound": "hbm", "kernel": solver.kernelName() + "<%s>" % wl.model, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": ach / HBM_PEAK_GBS, "traffic": traffic, "kernel_ms_avg": k_ms, "launches_timed": int(n_l),
            "backward_passes_per_iteration": bw, "forward_passes_per_iteration": fw,
            "algorithmic_bytes_per_launch": words * elem * inst_it, "fused_lower_bound_bytes_per_launch": fused * elem * inst_it}
    if traffic:
        roof["traffic_source"] = src
        roof["traffic_over_fused_bound"] = traffic / roof["fused_lower_bound_bytes_per_launch"]
        roof["hbm_frac_measured"] = traffic / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
    elif note:
        roof["traffic_note"] = note
    out = {"workload": "%s: nx=%d, nu=%d, T=%d, batch=%d, %s, seed %d, default Configuration with max_iter = %d%s"
                       % (wl.model, wl.n, wl.m, wl.T, wl.B, "fp32" if elem == 4 else "fp64", seed, iters_per_solve,
                          "" if thre is None else ", cost_update_thre = %g" % thre),
           "metric": "DDP iterations/s (batch=%d, T=%d)" % (wl.B, wl.T), "value": n_steps * (inst_it / wl.B) / dt,
           "ms_per_step": 1e3 * dt / n_steps, "timed_steps": n_steps, "timed_seconds": dt, "dtype": "f32" if elem == 4 else "f64",
           "kernel": roof["kernel"], "mean_iterations": float(it.mean()),
           "status_counts": {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
           "roofline": roof, "traffic": traffic}
    del solver
    if name == "c3":
        # 1024 bipedal instances are 64 quad workgroups on 256 CUs: a single batch is a latency chain (T = 300 timesteps x ~1.1 k
        # cycles per iteration) that leaves three quarters of the chip idle.  Eight batches in flight on eight handles / streams
        # (DDPSolverPool) is how a caller with more than one batch fills it: the pooled rate and its contract fraction ride along.
        pool = nmpc_amd.DDPSolverPool(problem, wl.B, n_handles=8, device=device_index)
        pc = pool.config()
        pc.print_level, pc.horizon_steps, pc.max_iter = 0, wl.T, iters_per_solve
        pool.applyConfig()
        for _ in range(16):
            pool.submit(d_t0.data_ptr(), d_x0.data_ptr(), d_u0.data_ptr())
        pool.synchronize()
        torch.cuda.synchronize()
        n_pool = max(64, 8 * n_steps // 2)
        t0 = time.perf_counter()
        for _ in range(n_pool):
            pool.submit(d_t0.data_ptr(), d_x0.data_ptr(), d_u0.data_ptr())
        pool.synchronize()
        dtp = time.perf_counter() - t0
        it_p = float(pool.solvers[-1].iters().sum())
        out["pooled"] = {"value": n_pool * (it_p / wl.B) / dtp, "handles": 8, "batches": n_pool, "ms_per_solve": 1e3 * dtp / n_pool,
                         "contract_frac": words * elem * it_p * n_pool / dtp / 1e9 / HBM_PEAK_GBS}
        del pool
    return out


def secondary_legs(device_index: int, seed: int, iters_per_solve: int, min_seconds: float):
    out = {}
    t0 = time.perf_counter()
    for name in ("c3", "c4", "c4f64", "c5", "fmpc", "centroidal"):
        try:
            if name == "fmpc":
                import bench_fmpc
                out[name] = bench_fmpc.secondary_leg(device_index, seed, min_seconds)
            else:
                out[name] = ddp_secondary_leg(name, device_index, seed, iters_per_solve, min_seconds)
        except Exception as e:  # the headline stands on its own; say which leg is missing and why
            out[name] = {"value": None, "error": repr(e)}
    out["seconds_total"] = time.perf_counter() - t0
    return out


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """--dump-outputs: write each array as <out_dir>/<name>.npy, float32 / float64 as they are and integer fields as float64.  The arrays
    share a leading instance axis; when they come to more than 64 MB together, the same fixed sample of instances (seed 0, sorted) is
    taken from every one and its indices go to instances.npy."""
    arrs = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        arrs[name] = a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)
    n_inst = next(iter(arrs.values())).shape[0]
    assert all(a.shape[0] == n_inst for a in arrs.values()), {k: a.shape for k, a in arrs.items()}
    total = sum(a.nbytes for a in arrs.values())
    if total > DUMP_MAX_BYTES:
        per_inst = total / n_inst + 8  # (+ its index)
        keep = int((DUMP_MAX_BYTES - 128 * 1024) // per_inst)  # (room for the .npy headers)
        idx = np.sort(np.random.default_rng(0).choice(n_inst, size=keep, replace=False))
        arrs = {name: a[idx] for name, a in arrs.items()}
        arrs["instances"] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrs.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def launch_ranks(n: int) -> None:
    """`python bench.py --gpus N` outside a launcher: become the launcher of N ranks of this very command line (one process per GPU,
    rendezvous on 127.0.0.1, a free port) — the form the driver itself uses for N > 1.  Runs them as a child process and exits with
    its status: does not return."""
    import subprocess
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    rc = subprocess.run(cmd).returncode
    # a launcher killed by signal s has returncode -s: exit with 128 + s, the status a shell reports for it (134 abort, 139 fault)
    sys.exit(128 - rc if rc < 0 else rc)


def check_world(args, world: int, n_dev: int) -> None:
    """--gpus is the number of ranks that must have joined, each on its own device (the flag used to be parsed and never read)."""
    if args.gpus != world:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d rank(s) (WORLD_SIZE): refusing to report a job of another size"
                         % (args.gpus, world))
    if n_dev < world and not args.share_devices:
        raise SystemExit("bench.py: %d rank(s) but only %d visible device(s); one process per GPU is the contract "
                         "(--share-devices runs them on the devices there are, gather over gloo: test boxes only)" % (world, n_dev))


def main():
    args = parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        launch_ranks(args.gpus)
    if args.workload == "fmpc":  # the FMPC path has its own script behind the same contract
        import bench_fmpc
        return bench_fmpc.main(args, host_cores)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    import torch  # device memory for the inputs + torch.distributed (RCCL); imported before the HIP library
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: torch.cuda.is_available() is False (no CPU fallback)")
    n_dev = torch.cuda.device_count()
    check_world(args, world, n_dev)
    device_index = local_rank % n_dev  # (--share-devices: tests run two ranks on a one-GPU box, both on device 0)
    torch.cuda.set_device(device_index)
    dev = torch.device("cuda", device_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RCCL needs one device per rank; two ranks sharing a GPU (the one-GPU test box) gather over gloo instead
        backend = "nccl" if n_dev >= world else "gloo"
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend="gloo")
    else:
        backend = None

    import nmpc_amd
    from nmpc_amd import _capi, workloads

    # per-rank shard: rank r owns instances [r*B, (r+1)*B) of the global splitmix64 stream
    gen, wl_batch, wl_horizon, wl_text = WORKLOADS[args.workload]
    gen_kw = dict(fp32=True) if args.workload == "c4" else {}
    wl_full = None
    if args.global_batch > 0:
        import dataclasses
        from nmpc_amd import sharding
        wl_full = getattr(workloads, gen)(B=args.global_batch, T=args.horizon or wl_horizon, seed=args.seed, **gen_kw)
        lo_, hi_ = sharding.shard_range(args.global_batch, rank, world)
        wl = dataclasses.replace(wl_full, B=hi_ - lo_, x0=wl_full.x0[lo_:hi_], u_init=wl_full.u_init[lo_:hi_], t0=wl_full.t0[lo_:hi_])
    else:
        wl = getattr(workloads, gen)(B=args.batch or wl_batch, T=args.horizon or wl_horizon, seed=args.seed + 7919 * rank, **gen_kw)
    problem = nmpc_amd.make_problem(wl.model)
    elem = problem.scalar_bytes()
    solver = nmpc_amd.DDPSolverBatch(problem, wl.B, device=device_index)
    if args.global_batch > 0:
        solver.setDispatchBatch(args.global_batch)  # the kernel family of the WHOLE batch: shards == the unsharded solve, bit for bit

    def configure(mode, iters, cost_update_thre=None):
        cfg = solver.config()
        dflt = nmpc_amd.Configuration()
        for key in ("max_iter", "k_rel_norm_thre", "cost_update_thre"):
            setattr(cfg, key, getattr(dflt, key))
        cfg.print_level = 0
        cfg.horizon_steps = wl.T
        for key, val in mode_config(mode, iters, cost_update_thre).items():
            setattr(cfg, key, val)
        cfg.trace_level = 1

    fp32_headline = args.workload == "c4" and args.cost_update_thre is None and args.mode == "nominal"
    if fp32_headline:
        args.cost_update_thre = 1e-3  # the threshold an fp32 cost can resolve is the c4 headline (see --cost-update-thre)
    configure(args.mode, args.iters_per_solve, args.cost_update_thre)

    # The CPU leg runs FIRST (on rank 0's host cores): the GPU legs then come last and back to back, where an outside
    # observer sampling the device sees them (the driver's sampler saw an idle GPU behind a 16 s CPU tail).
    cpu_leg = None
    want_extra_modes = not args.no_extra_modes and args.mode == "nominal" and args.workload == "c2"
    if rank == 0 and not args.no_cpu_baseline:  # rank 0 at every world size (the other ranks wait at the barrier below)
        try:
            cpu_leg = cpu_baseline(wl, args.mode, args.iters_per_solve, args.cpu_seconds, args.cost_update_thre,
                                   extra_modes=(("m1", 50), ("m2", 500)) if want_extra_modes else ())
        except Exception as e:  # the GPU number stands on its own; say why the baseline is missing
            cpu_leg = {"value": None, "unit": "DDP iterations/s", "cores": os.cpu_count(), "kind": "port", "sample": "failed: %r" % (e,)}
    if world > 1 and not args.no_cpu_baseline:
        dist.barrier()

    d_x0 = torch.from_numpy(wl.x0).to(dev)
    d_u0 = torch.from_numpy(wl.u_init).to(dev)
    d_t0 = torch.from_numpy(wl.t0).to(dev)
    # the packed per-shard result the one collective moves: [X | U | cost | status, iters (int32 pairs)] — sharding.pack_results'
    # fields, field-major here (one device-side pack per field)
    n_x = wl.B * (wl.T + 1) * wl.n
    n_u = wl.B * wl.T * max(wl.m, 1)
    n_c = wl.B * (wl.T + 1)
    n_rec = n_x + n_u + n_c + wl.B
    # (uneven shards of a strong split: every rank sends a buffer of the largest shard's size, one fixed-size all-gather)
    per_inst = (wl.T + 1) * wl.n + wl.T * max(wl.m, 1) + (wl.T + 1) + 1
    n_send = n_rec if args.global_batch <= 0 else per_inst * (-(-args.global_batch // world))
    d_res = torch.zeros(n_send, dtype=torch.float64, device=dev)
    gather_dev = dev if backend == "nccl" else torch.device("cpu")
    d_all = torch.empty(world * n_send, dtype=torch.float64, device=gather_dev) if world > 1 else None

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def step():
        solver.solveDevice(d_t0.data_ptr(), d_x0.data_ptr(), d_u0.data_ptr())

    for _ in range(args.warmup):
        step()
    solver.synchronize()
    solver.timingStats(reset=True)
    red_dev = dev if backend == "nccl" else torch.device("cpu")

    # The timed job: exactly --steps steps, from a barrier + device synchronise to the stream synchronise after the last one; no
    # collective and no host round trip inside it.
    barrier()
    t_begin = time.perf_counter()
    for _ in range(args.steps):
        step()
    solver.synchronize()
    total_steps = args.steps
    t_solve = time.perf_counter()
    # the one collective of the job: gather the packed results of every shard
    off = 0
    for field, count in ((_capi.FIELD_X, n_x), (_capi.FIELD_U, n_u), (_capi.FIELD_COST, n_c)):
        solver.getDevice(field, d_res.data_ptr() + off * 8, count * 8)
        off += count
    solver.getDevice(_capi.FIELD_STATUS, d_res.data_ptr() + off * 8, wl.B * 4)
    solver.getDevice(_capi.FIELD_ITERS, d_res.data_ptr() + off * 8 + wl.B * 4, wl.B * 4)
    solver.synchronize()
    if world > 1:
        dist.all_gather_into_tensor(d_all, d_res if backend == "nccl" else d_res.cpu())
    barrier()
    t_end = time.perf_counter()
    if args.dump_outputs:  # what the caller of the timed path receives from its last step (before the extra legs reuse the handle)
        dumped = {"X": solver.X(), "U": solver.U(), "cost": solver.cost(), "status": solver.status(), "iters": solver.iters()}
        dump_outputs(args.dump_outputs if world == 1 else os.path.join(args.dump_outputs, "rank%d" % rank), dumped)

    mine = torch.tensor([t_end - t_begin, t_end - t_solve, t_solve - t_begin], dtype=torch.float64, device=red_dev)
    per_rank = [mine.clone() for _ in range(world)]
    elapsed_t = mine.clone()
    if world > 1:
        dist.all_gather(per_rank, mine)
        dist.all_reduce(elapsed_t, op=dist.ReduceOp.MAX)
    elapsed, gather_s = float(elapsed_t[2]), float(elapsed_t[1])  # (the timed steps; the gather after them is reported on its own)

    n_solves, total_ms, kernel_ms = solver.timingStats()
    tr = solver.trace()  # (B, max_iter+1, 12) of the last solve; rows beyond an instance's last iteration are zero
    iters = solver.iters()
    rows = tr[:, 1:, :]
    executed = rows[:, :, 0] > 0
    n_it = int(executed.sum())
    n_bw = float(rows[:, :, _capi.TRACE_COLUMNS.index("n_backward")][executed].sum()) / max(n_it, 1)
    n_fw = float(rows[:, :, _capi.TRACE_COLUMNS.index("n_forward")][executed].sum()) / max(n_it, 1)
    inst_it_per_solve = float(iters.sum())  # this rank's shard
    # whole-job count: every rank solves its own instances (different seeds), so sum the executed iterations over ranks
    job_it = torch.tensor([inst_it_per_solve], dtype=torch.float64, device=red_dev)
    if world > 1:
        dist.all_reduce(job_it, op=dist.ReduceOp.SUM)
    job_it_per_solve = float(job_it[0])
    status = solver.status()
    kernel_name = solver.kernelName()
    headline_iters, headline_status = iters.copy(), status.copy()
    hist = {str(k): int(v) for k, v in zip(*np.unique(iters, return_counts=True))}
    status_counts = {str(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))}

    # ---- the gathered records against the unsharded solve (strong split, --verify-gather): rank 0, after the timed job
    gather_verified, shard_sizes = None, None
    if args.global_batch > 0:
        from nmpc_amd import sharding
        shard_sizes = sharding.shard_sizes(args.global_batch, world)
    if args.verify_gather and args.global_batch > 0 and rank == 0:
        whole = nmpc_amd.DDPSolverBatch(problem, wl_full.B, device=device_index)
        wc, sc = whole.config(), solver.config()
        for key, val in vars(sc).items():
            setattr(wc, key, val.copy() if isinstance(val, np.ndarray) else val)
        whole.solve(wl_full.t0, wl_full.x0, wl_full.u_init)
        want = (whole.X(), whole.U(), whole.cost(), whole.status(), whole.iters())
        got_all = (d_all if world > 1 else d_res).cpu().numpy()
        ok, lo_ = True, 0
        for r_, sz in enumerate(shard_sizes):
            rec = got_all[r_ * n_send:(r_ + 1) * n_send]
            o = 0
            for arr, per in ((want[0], (wl.T + 1) * wl.n), (want[1], wl.T * max(wl.m, 1)), (want[2], wl.T + 1)):
                ok = ok and np.array_equal(rec[o:o + sz * per], arr[lo_:lo_ + sz].reshape(-1))
                o += sz * per
            ints = rec[o:o + sz].view(np.int32)
            ok = ok and np.array_equal(ints[:sz], want[3][lo_:lo_ + sz]) and np.array_equal(ints[sz:2 * sz], want[4][lo_:lo_ + sz])
            lo_ += sz
        gather_verified = bool(ok)
        del whole

    # ---- extra legs, outside the timed job (every rank runs them; rank 0 reports its own)
    def pass_counts():
        """(executed instance-iterations, backward passes per iteration, forward trials per iteration) of the last solve's trace."""
        tr_ = solver.trace()[:, 1:, :]
        ex = tr_[:, :, 0] > 0
        n = int(ex.sum())
        return (n, float(tr_[:, :, _capi.TRACE_COLUMNS.index("n_backward")][ex].sum()) / max(n, 1),
                float(tr_[:, :, _capi.TRACE_COLUMNS.index("n_forward")][ex].sum()) / max(n, 1))

    def roofline_of(kernel_ms_avg, n_launches, inst_it, bw, fw):
        """SURVEY.md 8(d) contract accounting of one launch with the measured pass counts."""
        words_ = workloads.algorithmic_words_per_instance_iteration(wl.n, wl.m, wl.T, bw, fw)
        fused_ = workloads.fused_words_per_instance_iteration(wl.n, wl.m, wl.T, bw, fw)
        bytes_ = words_ * float(elem) * inst_it
        ach = bytes_ / (kernel_ms_avg * 1e-3) / 1e9
        return {"bound": "hbm", "kernel": solver.kernelName() + "<%s>" % wl.model, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": ach / HBM_PEAK_GBS, "traffic": None, "kernel_ms_avg": kernel_ms_avg, "launches_timed": int(n_launches),
                "backward_passes_per_iteration": bw, "forward_passes_per_iteration": fw,
                "algorithmic_bytes_per_launch": bytes_, "algorithmic_bytes_per_instance_iteration": words_ * float(elem),
                "fused_lower_bound_bytes_per_instance_iteration": fused_ * float(elem),
                "fused_lower_bound_bytes_per_launch": fused_ * float(elem) * inst_it}

    def leg(mode, iters, n_steps, cost_update_thre=None):
        configure(mode, iters, cost_update_thre)
        for _ in range(2):
            step()
        solver.synchronize()
        torch.cuda.synchronize()
        solver.timingStats(reset=True)
        t0 = time.perf_counter()
        for _ in range(n_steps):
            step()
        solver.synchronize()
        dt = time.perf_counter() - t0
        n_l, _, k_ms_sum = solver.timingStats()
        it = solver.iters()
        st = solver.status()
        n_exec, bw, fw = pass_counts()
        return {"value": n_steps * (float(it.sum()) / wl.B) / dt, "ms_per_solve": 1e3 * dt / n_steps,
                "solves_per_s": n_steps * wl.B / dt, "mean_iterations": float(it.mean()), "max_iterations": int(it.max()),
                "status_counts": {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
                "roofline": roofline_of(k_ms_sum / max(n_l, 1), n_l, float(it.sum()), bw, fw)}

    extras = {}
    if not args.no_extra_modes and args.mode == "nominal":
        if args.workload == "c2":
            extras["m1"] = leg("m1", 50, 10)
            extras["m2"] = leg("m2", 500, 10)
            # M2 again with consecutive batches overlapped: 32 batches dealt round-robin to eight handles (DDPSolverPool), each
            # with its own stream.  Under the ragged-convergence schedule (automatic at max_iter 500) a converged instance gives
            # up its workgroup slot within sixteen iterations, so the batches in flight share the chip instead of queueing for
            # the CUs that whole-solve workgroups hold until their slowest instance is done (per-batch results are those of a
            # lone handle, tests/test_gpu_ragged.py); the same pool with whole-solve launches rides along for comparison.
            def pooled_m2(ragged):
                pool = nmpc_amd.DDPSolverPool(problem, wl.B, n_handles=8, device=device_index)
                pc = pool.config()
                pc.print_level = 0
                pc.horizon_steps = wl.T
                pc.ragged_schedule = ragged
                for key, val in mode_config("m2", 500).items():
                    setattr(pc, key, val)
                pool.applyConfig()
                for _ in range(8):
                    pool.submit(d_t0.data_ptr(), d_x0.data_ptr(), d_u0.data_ptr())
                pool.synchronize()
                torch.cuda.synchronize()
                t0p = time.perf_counter()
                for _ in range(32):
                    pool.submit(d_t0.data_ptr(), d_x0.data_ptr(), d_u0.data_ptr())
                pool.synchronize()
                dtp = time.perf_counter() - t0p
                it_p = pool.solvers[-1].iters()
                res = {"value": 32 * (float(it_p.sum()) / wl.B) / dtp, "solves_per_s": 32 * wl.B / dtp, "ms_per_solve": 1e3 * dtp / 32,
                       "handles": 8, "batches": 32, "launches_per_solve": pool.solvers[-1].lastSolveLaunches(),
                       "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")}
                del pool
                return res

            extras["m2_overlapped"] = pooled_m2(0)
            extras["m2_overlapped"]["whole_solve_launches_value"] = pooled_m2(-1)["value"]

            # M2 as a STREAM: a queue of N >> 4096 instances through the 4096 slots of ONE handle (nmpc_hip_ddp_solve_stream): the slot of
            # an instance that has converged takes the next one of the queue at the next round boundary (the successor of the pool: no
            # batch boundaries at all; every instance returns the bits of its lone solve, tests/test_gpu_stream.py).  The rate is
            # instance-iterations / 4096 / device time (HIP events around the whole schedule, staging copies excluded).  32768 instances:
            # the queue holds ~36 that never converge, and ONE such instance is a chain of 500 iterations x ~47 us = 23.5 ms that
            # nothing shortens — 157 batch-iterations of work cannot take less, i.e. <= 6.7 k whatever the schedule; 262144 instances
            # amortise that tail: the sustained rate.
            def stream_leg(n_inst, span):
                wl_s = workloads.cartpole_batch(B=n_inst, T=wl.T, seed=args.seed)
                st = nmpc_amd.DDPSolverBatch(problem, wl.B, device=device_index)
                sc = st.config()
                sc.print_level, sc.horizon_steps, sc.trace_level = 0, wl.T, 0
                for key, val in mode_config("m2", 500).items():
                    setattr(sc, key, val)
                best = None
                for _ in range(2):
                    r = st.solveStream(wl_s.t0, wl_s.x0, wl_s.u_init, span=span)
                    if best is None or r.device_ms < best.device_ms:
                        best = r
                it_s = float(best.iters.sum())
                res = {"value": it_s / wl.B / (best.device_ms * 1e-3), "instances": n_inst, "slots": wl.B, "span": span, "rounds": best.rounds,
                       "device_ms": best.device_ms, "mean_iterations": it_s / n_inst, "solves_per_s": n_inst / (best.device_ms * 1e-3),
                       "status_counts": {str(k): int(v) for k, v in zip(*np.unique(best.status, return_counts=True))}}
                del st
                return res

            extras["m2_stream"] = stream_leg(32768, 8)
            extras["m2_stream"]["sustained"] = stream_leg(262144, 8)
        if args.workload == "c3":
            # 1024 bipedal instances are 64 quad workgroups on 256 CUs: the single-batch rate is a latency, not the chip's rate.
            # Four batches in flight on four handles / streams (DDPSolverPool) is how a caller with more than one batch fills it.
            pool = nmpc_amd.DDPSolverPool(problem, wl.B, n_handles=4, device=device_index)
            pc = pool.config()
            pc.print_level = 0
            pc.horizon_steps = wl.T
            for key, val in mode_config("nominal", args.iters_per_solve).items():
                setattr(pc, key, val)
            pool.applyConfig()
            for _ in range(8):
                pool.submit(d_t0.data_ptr(), d_x0.data_ptr(), d_u0.data_ptr())
            pool.synchronize()
            torch.cuda.synchronize()
            n_pool = 200
            t0p = time.perf_counter()
            for _ in range(n_pool):
                pool.submit(d_t0.data_ptr(), d_x0.data_ptr(), d_u0.data_ptr())
            pool.synchronize()
            dtp = time.perf_counter() - t0p
            it_p = pool.solvers[-1].iters()
            extras["pooled"] = {"value": n_pool * (float(it_p.sum()) / wl.B) / dtp, "solves_per_s": n_pool * wl.B / dtp,
                                "ms_per_solve": 1e3 * dtp / n_pool, "handles": 4, "batches": n_pool}
            del pool
        if fp32_headline:
            extras["default_threshold"] = leg("nominal", args.iters_per_solve, 20, cost_update_thre=1e-7)
            extras["fp32_tolerance_m2"] = leg("m2", 500, 10, cost_update_thre=1e-3)

    secondary = None
    if (rank == 0 and world == 1 and args.workload == "c2" and args.mode == "nominal" and not args.no_secondary
            and args.batch == 0 and args.horizon == 0 and args.global_batch <= 0):
        secondary = secondary_legs(device_index, args.seed, args.iters_per_solve, args.secondary_seconds)

    if rank == 0:
        words = workloads.algorithmic_words_per_instance_iteration(wl.n, wl.m, wl.T, n_bw, n_fw)
        fused = workloads.fused_words_per_instance_iteration(wl.n, wl.m, wl.T, n_bw, n_fw)
        k_ms = kernel_ms / max(n_solves, 1)
        bytes_per_launch = words * float(elem) * inst_it_per_solve
        achieved = bytes_per_launch / (k_ms * 1e-3) / 1e9
        # one "DDP iteration" of the metric = procOnce over a batch: the per-GPU batch (weak scaling: every rank owns one), or the
        # one global batch of a strong split
        batch_unit = args.global_batch if args.global_batch > 0 else wl.B
        value = total_steps * (job_it_per_solve / batch_unit) / elapsed
        config = {
            "workload": (wl_text % (wl.T, wl.B, args.seed))
                        + ", default DDPSolver::Configuration with max_iter = iterations_per_step"
                        + ("" if args.cost_update_thre is None else ", cost_update_thre = %g" % args.cost_update_thre),
            "mode": args.mode,
            "iterations_per_step": args.iters_per_solve if args.mode != "m2" else 500,
            "solves_per_s": (args.global_batch if args.global_batch > 0 else world * wl.B) * total_steps / elapsed,
            "timed_steps_total": total_steps,
            "timed_seconds": elapsed,
            "gathered_record": "per shard, field-major: X | U | cost | status, iters (int32)",
            "iteration_histogram": hist,
            "instance_iterations_per_step": job_it_per_solve,
            "backward_passes_per_iteration": n_bw,
            "forward_passes_per_iteration": n_fw,
            "status_counts": status_counts,
            "lane_mapping": (LANE_MAPPINGS.get(kernel_name, kernel_name) if not (kernel_name == "ddp_solve_tile64_kernel" and gen_kw.get("fp32"))
                             else LANE_MAPPINGS[kernel_name].replace("fp64 tile:", "tile kernel, float instantiation:").replace(
                                 "v_mfma_f64_16x16x4", "v_mfma_f32_16x16x4")),
            "final_gather_ms": 1e3 * gather_s,
            "gather_backend": backend,
            "per_rank_solve_ms": [1e3 * float(t[2]) / total_steps for t in per_rank],
            "per_rank_gather_ms": [1e3 * float(t[1]) for t in per_rank],
        }
        if "m1" in extras:
            config["m1_value"] = extras["m1"]["value"]
            config["m1"] = dict(extras["m1"], note="SURVEY 8(d) M1: termination tests disabled, max_iter = N = 50; batch-iterations/s")
            config["m2_value"] = extras["m2"]["value"]
            config["m2"] = dict(extras["m2"], note="SURVEY 8(d) M2: default Configuration, solve to convergence (max_iter 500)")
            for m_name in ("m1", "m2"):  # the CPU oracle in the same mode on the same inputs (cpu_baseline()'s extra modes)
                config[m_name].update((cpu_leg or {}).get("modes", {}).get(m_name, {}))
            config["m2_overlapped_value"] = extras["m2_overlapped"]["value"]
            config["m2_overlapped"] = dict(extras["m2_overlapped"], note="M2 with 32 consecutive batches on eight handles / streams "
                                           "(nmpc_amd.DDPSolverPool) under the ragged-convergence schedule: sustained rate with the convergence "
                                           "tails overlapped; whole_solve_launches_value: the same pool with one launch per solve")
        if "m2_stream" in extras:
            config["m2_stream_value"] = extras["m2_stream"]["value"]
            config["m2_stream_sustained_value"] = extras["m2_stream"]["sustained"]["value"]
            config["m2_stream"] = dict(extras["m2_stream"], note="M2 as a stream: 32768 instances to convergence through the 4096 slots of ONE "
                                       "handle, freed slots refilled at round boundaries (nmpc_hip_ddp_solve_stream); batch-iterations/s-equivalent = "
                                       "instance-iterations / 4096 / device time.  Bounded by the 23.5 ms chain of an instance that runs to max_iter "
                                       "500; `sustained`: 262144 instances (the tail amortised)")
        if "pooled" in extras:
            config["pooled_value"] = extras["pooled"]["value"]
            config["pooled"] = dict(extras["pooled"], note="the same workload with four batches in flight on four handles / streams "
                                    "(nmpc_amd.DDPSolverPool): one batch of %d instances occupies %d of the chip's 256 CUs" % (wl.B, -(-wl.B // 16)))
        if gather_verified is not None:
            config["gather_verified"] = gather_verified
            config["global_batch"] = args.global_batch
            config["shard_sizes"] = shard_sizes
        if "default_threshold" in extras:
            config["cost_update_thre"] = 1e-3
            config["default_threshold_value"] = extras["default_threshold"]["value"]
            config["default_threshold"] = dict(extras["default_threshold"], note="same workload with the reference's default "
                                               "cost_update_thre = 1e-7, below the resolution of an fp32 cost: the accept test is "
                                               "rounding noise there in the fp32 oracle itself (DESIGN.md 3a) — secondary number")
            config["fp32_tolerance_m2"] = dict(extras["fp32_tolerance_m2"], note="cost_update_thre = 1e-3, solve to convergence")
        out = {
            "metric": "DDP iterations/s (whole node), batch=%d, T=%d" % (args.global_batch if args.global_batch > 0 else wl.B, wl.T)
                      + (", cost_update_thre=1e-3 (the threshold an fp32 cost resolves)" if fp32_headline else ""),
            "value": value,
            "unit": ("DDP iterations/s (one iteration = procOnce over the global batch of %d instances, sharded)" % batch_unit)
                    if args.global_batch > 0 else "DDP iterations/s (one iteration = procOnce over a batch of %d instances per GPU)" % wl.B,
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / total_steps,
            "higher_is_better": True,
            "scaling": "strong" if args.global_batch > 0 else "weak",
            "vs_baseline": None,
            "dtype": "f64" if elem == 8 else "f32",
            "data": "synthetic",
            "config": config,
            "instance_iterations_per_s": value * batch_unit,
            "roofline": {
                "bound": "hbm",
                "kernel": kernel_name + "<%s>" % wl.model,
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": None,
                "accounting": "SURVEY.md 8(d) contract bytes (the reference's materialised dataflow), NOT measured traffic: the "
                              "kernel keeps the derivatives on chip; `traffic` is the rocprofv3 PMC measurement",
                "kernel_ms_avg": k_ms,
                "launches_timed": int(n_solves),
                "algorithmic_bytes_per_launch": bytes_per_launch,
                "algorithmic_bytes_per_instance_iteration": words * float(elem),
                "fused_lower_bound_bytes_per_instance_iteration": fused * float(elem),
                "fused_lower_bound_bytes_per_launch": fused * float(elem) * inst_it_per_solve,
            },
        }
        if secondary is not None:
            out["secondary"] = secondary
        if "m1" in extras:
            out["roofline_m1"] = extras["m1"]["roofline"]
            out["roofline_m2"] = extras["m2"]["roofline"]
        if cpu_leg is not None:
            # the oracle's first 256 instances against the GPU's last timed solve: how many took the same decisions (iteration count
            # and status).  fp64: all of them but instances at a decision boundary; fp32 (c4): the margin-filtered parity of
            # tests/test_gpu_fp32.py in one number — the oracle here is the -march=native build (contracted), one of the perturbed runs
            # the tests accept
            chk_it, chk_st = cpu_leg.pop("check_iters", None), cpu_leg.pop("check_status", None)
            cpu_leg.pop("modes", None)  # (reported under config.m1 / config.m2)
            if chk_it is not None and headline_iters is not None:
                k = len(chk_it)
                agree = (headline_iters[:k] == np.asarray(chk_it)) & (headline_status[:k] == np.asarray(chk_st))
                cpu_leg["gpu_decisions_agree_frac"] = float(agree.mean())
                cpu_leg["gpu_decisions_checked"] = k
                config["oracle_agree_frac"] = float(agree.mean())
            out["cpu_baseline"] = cpu_leg
        traffic_file = os.path.join(ROOT, "profiles", "hbm_traffic.json")
        if os.path.exists(traffic_file):
            try:
                tf = json.load(open(traffic_file))
                entry = tf.get(args.workload) if isinstance(tf.get(args.workload), dict) else (tf if args.workload == "c2" else None)
                from nmpc_amd import build as hip_build
                src_hash = hip_build.source_hash()
                thre_ok = (args.cost_update_thre is None) or (fp32_headline and entry and entry.get("cost_update_thre") == 1e-3)
                if (entry and args.mode == "nominal" and thre_ok and entry.get("batch") == wl.B
                        and entry.get("iterations_per_step") == args.iters_per_solve and entry.get("source_hash") != src_hash):
                    out["roofline"]["traffic_note"] = ("profiles/hbm_traffic.json holds a measurement of other device sources (hash %s, "
                                                       "now %s): not used" % (entry.get("source_hash"), src_hash))
                elif (entry and args.mode == "nominal" and thre_ok and entry.get("batch") == wl.B
                        and entry.get("iterations_per_step") == args.iters_per_solve):
                    out["roofline"]["traffic"] = entry.get("hbm_bytes_per_launch")
                    out["roofline"]["traffic_source"] = entry.get("source")
                    out["roofline"]["traffic_source_hash"] = src_hash
                    if out["roofline"]["traffic"]:
                        out["roofline"]["traffic_over_fused_bound"] = (out["roofline"]["traffic"]
                                                                       / out["roofline"]["fused_lower_bound_bytes_per_launch"])
                        out["roofline"]["hbm_frac_measured"] = out["roofline"]["traffic"] / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
            except Exception:
                pass
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
