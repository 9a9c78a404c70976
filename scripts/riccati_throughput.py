"""Throughput of the batched Riccati backward pass on one MI355X: passes per second and ms per solve of nmpc_hip_riccati_solve_device
on device-resident inputs (riccati_wave_kernel, one wavefront per instance), against

  (1) the CPU checker (tests/cpp/riccati_checker.cpp) on 16 threads: wall time of the call on host arrays;
  (2) the same pass written as a torch loop on the same device: per step batched matmul, linalg.cholesky and cholesky_solve, which
      is what a caller without this solver writes (unconstrained legs only: torch has no BoxQP).

Shapes (n, m, T) x B as in DESIGN.md 2.11, seeded synthetic derivatives (Fx = I + 0.1 U, Fu = 0.3 U, Lxx = I, Luu = I, U uniform in
[-1, 1]) generated on the device, reg_type 1 from lambda 1e-4, one pass per instance; the box-constrained leg adds u = 0.2 U and limits
+-0.4.  HIP events around every solve; the GPU legs alternate in one process, `--rounds` rounds of `--min-seconds / rounds` each, and
the figures are medians over all timed solves with the quartiles and the extremes beside them.

  python scripts/riccati_throughput.py [--shapes 4x1x100x64,...] [--out profiles/riccati_throughput.json]

One process; run it under `timeout -k 10 <s>`.  Result of the committed run: profiles/riccati_throughput.json."""
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

from nmpc_amd import riccati  # noqa: E402

SHAPES = ",".join("%dx%dx%dx%d" % (n, m, T, B) for n, m, T in ((4, 1, 100), (12, 4, 50), (14, 7, 30), (16, 16, 30)) for B in (64, 1024, 8192))
BOXED = (12, 4, 50)
LAMBDA = 1e-4


def inputs(n, m, T, B, boxed):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(1000 * n + 10 * m + B % 997)
    u = lambda *shape: 2 * torch.rand(*shape, generator=gen, device="cuda", dtype=torch.float64) - 1
    eye = lambda k, *lead: torch.eye(k, device="cuda", dtype=torch.float64).expand(*lead, k, k).contiguous()
    d = dict(Fx=eye(n, B, T) + 0.1 * u(B, T, n, n), Fu=0.3 * u(B, T, n, m), Lx=u(B, T, n), Lu=u(B, T, m), Lxx=eye(n, B, T), Luu=eye(m, B, T),
             Lxu=0.1 * u(B, T, n, m), Vx_T=u(B, n), Vxx_T=eye(n, B))
    if boxed:
        d.update(U=0.2 * u(B, T, m), lower=torch.full((m,), -0.4, device="cuda", dtype=torch.float64),
                 upper=torch.full((m,), 0.4, device="cuda", dtype=torch.float64))
    torch.cuda.synchronize()
    return d


def torch_pass(d, T, m):
    """The unconstrained pass at LAMBDA (reg_type 1) as a loop of batched torch calls; returns k [B, T, m], K [B, T, m, n]."""
    import torch
    Vx, Vxx = d["Vx_T"].unsqueeze(-1), d["Vxx_T"]
    lamI = LAMBDA * torch.eye(m, device="cuda", dtype=torch.float64)
    ks, Ks = [None] * T, [None] * T
    for i in range(T - 1, -1, -1):
        Fx, Fu = d["Fx"][:, i], d["Fu"][:, i]
        FxT, FuT = Fx.mT, Fu.mT
        Qx = d["Lx"][:, i].unsqueeze(-1) + FxT @ Vx
        Qu = d["Lu"][:, i].unsqueeze(-1) + FuT @ Vx
        FuTV = FuT @ Vxx
        Qxx = d["Lxx"][:, i] + FxT @ Vxx @ Fx
        Qux = d["Lxu"][:, i].mT + FuTV @ Fx
        Quu = d["Luu"][:, i] + FuTV @ Fu
        L = torch.linalg.cholesky(Quu + lamI)
        kK = -torch.cholesky_solve(torch.cat([Qu, Qux], -1), L)
        k, K = kK[..., :1], kK[..., 1:]
        KT = K.mT
        Vx = Qx + KT @ Quu @ k + KT @ Qu + Qux.mT @ k
        Vxx = Qxx + KT @ Quu @ K + KT @ Qux + Qux.mT @ K
        Vxx = 0.5 * (Vxx + Vxx.mT)
        ks[i], Ks[i] = k.squeeze(-1), K
    return torch.stack(ks, 1), torch.stack(Ks, 1)


def summary(ms, B):
    ms = np.asarray(ms)
    q = np.percentile(ms, [0, 25, 50, 75, 100])
    return {"solves": int(ms.size), "ms_per_solve": float(q[2]), "ms_quartiles": [float(q[1]), float(q[3])], "ms_min_max": [float(q[0]), float(q[4])],
            "passes_per_s": float(B / (1e-3 * q[2]))}


def run_shape(n, m, T, B, boxed, a, checker):
    import torch
    d = inputs(n, m, T, B, boxed)
    s = riccati.RiccatiBatch(n, m, T, B)
    r = s.backwardDevice(**d)  # hands the tensors over; the timed solves read them in place
    s.synchronize()
    out = {"n": n, "m": m, "T": T, "B": B, "boxed": boxed, "status_ok": int((r.status == 1).sum()), "lds_bytes": (173 * n + 122 * m) * 8}
    legs = {"riccati_wave_kernel": []}
    if not boxed:
        legs["torch_loop"] = []
        k_t, K_t = torch_pass(d, T, m)  # warm-up, and the agreement of the two
        torch.cuda.synchronize()
        out["max_rel_diff_vs_torch_loop"] = float(max(((r.k - k_t).abs() / (1 + k_t.abs())).max(), ((r.K - K_t).abs() / (1 + K_t.abs())).max()))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per_round = a.min_seconds / a.rounds
    for _ in range(a.rounds):
        for name, ms in legs.items():
            spent = 0.0
            while spent < 1e3 * per_round:
                if name == "torch_loop":
                    e0.record()
                    torch_pass(d, T, m)
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                else:
                    s.solveDevice()
                    ms.append(s.lastMs())
                spent += ms[-1]
    for name, ms in legs.items():
        out[name] = summary(ms, B)
    if "torch_loop" in legs:
        out["kernel_over_torch_loop"] = out["riccati_wave_kernel"]["passes_per_s"] / out["torch_loop"]["passes_per_s"]
    if checker is not None:
        import riccati_checker as rk
        host = {k: v.cpu().numpy() for k, v in d.items()}
        case = rk.Case("throughput", n, m, T, {k: host[k] for k in riccati._DERIVATIVES}, None, host.get("U"), host.get("lower"), host.get("upper"), 1)
        secs = []
        while not secs or (sum(secs) < a.min_seconds and len(secs) < 20):
            t = time.perf_counter()
            ref = checker.backward(case, n_threads=16)
            secs.append(time.perf_counter() - t)
        out["cpu_checker_16_threads"] = summary([1e3 * v for v in secs], B)
        out["kernel_over_cpu_checker"] = out["riccati_wave_kernel"]["passes_per_s"] / out["cpu_checker_16_threads"]["passes_per_s"]
        out["max_rel_diff_vs_checker"] = float(max(rk.rel_err(r.k.cpu().numpy(), ref.k), rk.rel_err(r.K.cpu().numpy(), ref.K)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    checker = None
    if not a.skip_cpu:
        import riccati_checker as rk
        checker = rk.build(tempfile.mkdtemp(prefix="riccati_checker_"))
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s]
    res = {"what": "one backward pass per instance (reg_type 1, lambda 1e-4, no retry needed) on seeded synthetic derivatives; GPU legs: HIP events "
                   "per solve on resident inputs, alternating in one process, medians; CPU leg: wall time of the checker on 16 threads",
           "shapes": []}
    for n, m, T, B in shapes:
        for boxed in ((False, True) if (n, m, T) == BOXED else (False,)):
            leg = run_shape(n, m, T, B, boxed, a, checker)
            print(json.dumps(leg), flush=True)
            res["shapes"].append(leg)
            if a.out:  # (written after every leg: a run that is cut short leaves what it measured)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
