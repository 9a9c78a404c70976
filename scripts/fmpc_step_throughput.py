"""Throughput of the batched FMPC iteration on caller-supplied linearisations on one MI355X: iterations (instance steps) per second
and ms per call of nmpc_hip_fmpc_step_step_device on device-resident inputs (fmpc_step_wave_kernel, one wavefront per instance),
against

  (1) the CPU checker (tests/cpp/fmpc_step_checker.cpp) on 16 threads: wall time of the call on host arrays;
  (2) the same iteration written as a torch loop on the same device: the residuals and the slack step as batched einsum calls, the
      backward and forward sweeps per step as batched matmul, linalg.cholesky and cholesky_solve, which is what a caller without this
      solver writes (G is positive definite on these inputs, so Cholesky stands in for the pivoted LDLT).

Shapes (n, m, g, T) x B as in DESIGN.md 2.12, the seeded synthetic linearisations of tests/fmpc_step_checker.py generated on the host
and made resident.  apply_update = 0, so that every timed call runs the same iteration from the same variable (the update's stores are
not in the figure).  HIP events around every call; the GPU legs alternate in one process, `--rounds` rounds of `--min-seconds / rounds`
each, and the figures are medians over all timed calls with the quartiles and the extremes beside them.

  python scripts/fmpc_step_throughput.py [--shapes 4x1x4x200x64,...] [--out profiles/fmpc_step_throughput.json]

One process; run it under `timeout -k 10 <s>`.  Result of the committed run: profiles/fmpc_step_throughput.json."""
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

import fmpc_step_checker as fk  # noqa: E402
from nmpc_amd import fmpc_step  # noqa: E402

SHAPES = ",".join(["%dx%dx%dx%dx%d" % (n, m, g, T, B) for n, m, g, T in ((4, 1, 4, 200), (12, 4, 8, 50), (16, 16, 32, 30))
                   for B in (64, 1024, 8192)] + ["4x1x4x200x4096"])


def lds_bytes(n, m, g):
    gt = (g + 15) // 16
    return ((8 + 2 * gt) * 17 * n + (5 + 2 * gt) * 17 * m + 6 * n + 6 * m + 3 * g + 16) * 8


def torch_step(d, v, eps_in, dt, T):
    """One iteration (update_barrier_eps on, no update) as batched torch calls; returns (K [B, T, m, n], dx, du, alpha_s, alpha_nu)."""
    import torch
    x, lam, s, nu = v["x"], v["lam"], v["s"], v["nu"]
    A, Bm, Cm, Dm = d["A"], d["B"], d["C"], d["D"]
    eps = (0.5 * (s * nu).sum((1, 2)) / (s.shape[1] * s.shape[2])).clamp(1e-8, 1e6).view(-1, 1, 1)
    xbar = d["f"] - x[:, 1:]
    gbar = d["g"] + s
    lxbar = -lam[:, :-1] + dt * d["Lx"] + torch.einsum("btkr,btk->btr", A, lam[:, 1:]) + torch.einsum("btjr,btj->btr", Cm, nu)
    lubar = dt * d["Lu"] + torch.einsum("btkr,btk->btr", Bm, lam[:, 1:]) + torch.einsum("btjr,btj->btr", Dm, nu)
    nus = nu / s
    tsub = nus * gbar - nu + eps / s
    SC, SD = nus.unsqueeze(-1) * Cm, nus.unsqueeze(-1) * Dm
    Qxx = dt * d["Lxx"] + Cm.mT @ SC
    Quu = dt * d["Luu"] + Dm.mT @ SD
    Qxu = dt * d["Lxu"] + Cm.mT @ SD
    lxt = lxbar + torch.einsum("btjr,btj->btr", Cm, tsub)
    lut = lubar + torch.einsum("btjr,btj->btr", Dm, tsub)
    sv = -(d["Lx_T"] - lam[:, -1]).unsqueeze(-1)
    P = d["Lxx_T"]
    Ks, ks, Ps, ss = [None] * T, [None] * T, [None] * (T + 1), [None] * (T + 1)
    Ps[T], ss[T] = P, sv
    for i in range(T - 1, -1, -1):
        Ai, Bi = A[:, i], Bm[:, i]
        PA = P @ Ai
        F = Qxx[:, i] + Ai.mT @ PA
        H = Qxu[:, i] + PA.mT @ Bi
        G = Quu[:, i] + Bi.mT @ P @ Bi
        w = P @ xbar[:, i].unsqueeze(-1) - sv
        rhs = torch.cat([Bi.mT @ w + lut[:, i].unsqueeze(-1), H.mT], -1)
        kK = -torch.cholesky_solve(rhs, torch.linalg.cholesky(G))
        k, K = kK[..., :1], kK[..., 1:]
        sv = -Ai.mT @ w - lxt[:, i].unsqueeze(-1) - H @ k
        P = F - K.mT @ G @ K
        P = 0.5 * (P + P.mT)
        Ks[i], ks[i], Ps[i], ss[i] = K, k, P, sv
    dx = (d["current_x"] - x[:, 0]).unsqueeze(-1)
    dxs, dus = [dx], []
    for i in range(T):
        du = Ks[i] @ dx + ks[i]
        dx = A[:, i] @ dx + Bm[:, i] @ du + xbar[:, i].unsqueeze(-1)
        dus.append(du)
        dxs.append(dx)
    dX, dU = torch.stack(dxs, 1).squeeze(-1), torch.stack(dus, 1).squeeze(-1)
    dlam = (torch.stack(Ps, 1) @ dX.unsqueeze(-1) - torch.stack(ss, 1)).squeeze(-1)
    ds = -(torch.einsum("btjk,btk->btj", Cm, dX[:, :-1]) + torch.einsum("btjk,btk->btj", Dm, dU) + gbar)
    dnu = -(nu * (ds + s) - eps) / s
    big = torch.full_like(ds, 1.0)
    a_s = torch.where(ds < 0, -0.995 * s / ds, big).amin((1, 2)).clamp(max=1.0)
    a_nu = torch.where(dnu < 0, -0.995 * nu / dnu, big).amin((1, 2)).clamp(max=1.0)
    return torch.stack(Ks, 1), dX, dU, dlam, a_s, a_nu


def summary(ms, B, T):
    ms = np.asarray(ms)
    q = np.percentile(ms, [0, 25, 50, 75, 100])
    return {"calls": int(ms.size), "ms_per_call": float(q[2]), "ms_quartiles": [float(q[1]), float(q[3])], "ms_min_max": [float(q[0]), float(q[4])],
            "instances_per_s": float(B / (1e-3 * q[2])), "steps_per_s": float(B * T / (1e-3 * q[2]))}


def run_shape(n, m, g, T, B, a, checker):
    import torch
    case = fk.synthetic_case(n, m, g, B=B, T=T)
    to = lambda x: torch.from_numpy(np.array(x)).to("cuda:0")
    d = {k: to(v) for k, v in case.lin.items()}
    v = {k: to(x) for k, x in case.var.items()}
    sb = fmpc_step.FmpcStepBatch(n, m, g, T, B)
    sb.config().dt = case.dt
    sb.config().apply_update = 0
    sb.setVariable(v["x"], v["u"], v["lam"], v["s"], v["nu"], to(case.eps))
    r = sb.step(*[d[k] for k in fk.LIN], fields=("status", "K", "dx", "du", "alpha_s_max"))  # hands the tensors over; read in place
    out = {"n": n, "m": m, "g": g, "T": T, "B": B, "status_continued": int((r.status == 6).sum()), "lds_bytes": lds_bytes(n, m, g)}
    legs = {"fmpc_step_wave_kernel": [], "torch_loop": []}
    K_t, dX_t, dU_t, _, a_s, _ = torch_step(d, v, None, case.dt, T)  # warm-up, and the agreement of the two
    torch.cuda.synchronize()
    rel = lambda got, ref: float((np.abs(got - ref) / (1 + np.abs(ref))).max()) if ref.size else 0.0
    out["max_rel_diff_vs_torch_loop"] = max(rel(r.K, K_t.cpu().numpy()), rel(r.dx, dX_t.cpu().numpy()), rel(r.du, dU_t.cpu().numpy()),
                                            rel(r.alpha_s_max, a_s.cpu().numpy()))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per_round = a.min_seconds / a.rounds
    for _ in range(a.rounds):
        for name, ms in legs.items():
            spent = 0.0
            while spent < 1e3 * per_round:
                if name == "torch_loop":
                    e0.record()
                    torch_step(d, v, None, case.dt, T)
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                else:
                    sb.stepDevice()
                    ms.append(sb.lastMs())
                spent += ms[-1]
    for name, ms in legs.items():
        out[name] = summary(ms, B, T)
    out["kernel_over_torch_loop"] = out["fmpc_step_wave_kernel"]["steps_per_s"] / out["torch_loop"]["steps_per_s"]
    if checker is not None:
        secs = []
        while not secs or (sum(secs) < a.min_seconds and len(secs) < 20):
            t = time.perf_counter()
            ref = checker.step(case, n_threads=16, apply_update=0)
            secs.append(time.perf_counter() - t)
        out["cpu_checker_16_threads"] = summary([1e3 * x for x in secs], B, T)
        out["kernel_over_cpu_checker"] = out["fmpc_step_wave_kernel"]["steps_per_s"] / out["cpu_checker_16_threads"]["steps_per_s"]
        out["max_rel_diff_vs_checker"] = max(fk.rel_err(r.K, ref.K), fk.rel_err(r.dx, ref.dx), fk.rel_err(r.du, ref.du))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    checker = None if a.skip_cpu else fk.build(tempfile.mkdtemp(prefix="fmpc_step_checker_"))
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s]
    res = {"what": "one iteration per instance (update_barrier_eps on, apply_update off) on the seeded synthetic linearisations of "
                   "tests/fmpc_step_checker.py; GPU legs: HIP events per call on resident inputs, alternating in one process, medians; CPU "
                   "leg: wall time of the checker on 16 threads",
           "shapes": []}
    for n, m, g, T, B in shapes:
        leg = run_shape(n, m, g, T, B, a, checker)
        fk.synthetic_case.cache_clear()  # the largest case holds gigabytes
        print(json.dumps(leg), flush=True)
        res["shapes"].append(leg)
        if a.out:  # (written after every leg: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
