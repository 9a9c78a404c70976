"""Kernel time of the headline (c2) or bipedal (c3) batch on the quad kernel and its backward / forward split
(nmpc_hip_ddp_last_solve_phases), medians over 50 solves behind 10 warm-up solves.  The library is the tree's own or the one
NMPC_HIP_DDP_LIB names (scripts/quad_chunk_ab.sh runs it once per side).
    python scripts/quad_phases.py c2|c3 [label]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import nmpc_amd  # noqa: E402
from nmpc_amd import workloads  # noqa: E402

name = sys.argv[1]
label = sys.argv[2] if len(sys.argv) > 2 else os.path.basename(os.environ.get("NMPC_HIP_DDP_LIB", "tree"))
wl = workloads.cartpole_batch(B=4096, T=100, seed=1234) if name == "c2" else workloads.bipedal_batch(B=1024, T=300, seed=1234)
s = nmpc_amd.DDPSolverBatch(nmpc_amd.make_problem(wl.model), wl.B)
c = s.config()
c.print_level, c.horizon_steps, c.max_iter = 0, wl.T, 8
ms, bw, fw = [], [], []
for k in range(60):
    s.solve(wl.t0, wl.x0, wl.u_init)
    d = s.computationDuration()
    if k >= 10:
        ms.append(d.opt)
        bw.append(d.backward)
        fw.append(d.forward)
print(f"{name} {label:7s} kernel ms median {np.median(ms):.4f} (min {min(ms):.4f})  backward {np.median(bw):.4f}  forward {np.median(fw):.4f}  "
      f"{s.kernelName()}, iterations {int(s.iters().sum())}")
