"""A torque-limited pendulum written in torch, solved with nmpc_amd.FmpcStepBatch: the model lives in this file as three torch
functions (dynamics, inequality constraints, costs), torch.func linearises them at the solver's variable, and every interior-point
iteration (barrier update, KKT residuals, Riccati recursion with the pivoted LDLT, forward sweep, fraction-to-boundary rule, update)
runs on the device in one launch for the whole batch.  No problem class is compiled in.

State [theta, omega] (theta = 0 hangs down), input: a torque with |u| <= U_MAX.  Instance b starts at rest at a different angle and
has to be brought to rest at the bottom; the limit binds at the start of the horizon.

  python scripts/torch_fmpc_pendulum.py [--batch 16] [--steps 40]

Prints one line per iteration and ends with "ok" once every instance reports Succeeded (kkt_error <= kkt_error_thre)."""
import argparse
import os
import sys

import numpy as np
import torch
from torch.func import hessian, jacrev, vmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = 0.05
U_MAX = 1.5
GRAVITY, DAMPING = 9.81, 0.1
N, M, G = 2, 1, 2


def state_eq(x, u):
    """x_{i+1}: explicit Euler of theta'' = -g sin(theta) - c theta' + u."""
    th, om = x[0], x[1]
    return torch.stack([th + DT * om, om + DT * (-GRAVITY * torch.sin(th) - DAMPING * om + u[0])])


def ineq_const(x, u):
    """g(x, u) <= 0."""
    return torch.stack([u[0] - U_MAX, -u[0] - U_MAX])


def running_cost(x, u):
    return 0.5 * (4.0 * x[0] ** 2 + 0.2 * x[1] ** 2 + 0.05 * u[0] ** 2)


def terminal_cost(x):
    return 0.5 * (20.0 * x[0] ** 2 + 2.0 * x[1] ** 2)


def linearise(x, u, current_x):
    """The fourteen arrays FmpcStepBatch.step takes, at x [B, T+1, n], u [B, T, m], by torch.func over the batch and the horizon."""
    over = lambda fn: vmap(vmap(fn))
    xs = x[:, :-1]
    A, Bm = over(jacrev(state_eq, (0, 1)))(xs, u)
    C, D = over(jacrev(ineq_const, (0, 1)))(xs, u)
    Lx, Lu = over(jacrev(running_cost, (0, 1)))(xs, u)
    (Lxx, Lxu), (_, Luu) = over(hessian(running_cost, (0, 1)))(xs, u)
    xT = x[:, -1]
    return (A, Bm, C, D, Lx, Lu, Lxx, Luu, Lxu, over(state_eq)(xs, u), over(ineq_const)(xs, u), vmap(jacrev(terminal_cost))(xT),
            vmap(hessian(terminal_cost))(xT), current_x)


def solve(stepper, B, T, device, max_iter=60, verbose=True):
    """Iterate `stepper` (an FmpcStepBatch, or anything with its config / setVariable / step / variable) to its KKT threshold."""
    f64 = dict(dtype=torch.float64, device=device)
    current_x = torch.zeros(B, N, **f64)
    current_x[:, 0] = torch.linspace(0.6, 1.4, B, **f64)
    x = current_x.unsqueeze(1).repeat(1, T + 1, 1).contiguous()
    u, lam = torch.zeros(B, T, M, **f64), torch.zeros(B, T + 1, N, **f64)
    s, nu = torch.ones(B, T, G, **f64), torch.ones(B, T, G, **f64)
    cfg = stepper.config()
    cfg.dt = DT
    cfg.init_complementary_variable = 1  # the first iteration sets s and nu from g
    stepper.setVariable(x, u, lam, s, nu)
    for it in range(1, max_iter + 1):
        lin = [t.contiguous() for t in linearise(x, u, current_x)]
        r = stepper.step(*lin, fields=("status", "kkt_error", "barrier_eps", "alpha_s_max"))
        cfg.init_complementary_variable = 0
        if verbose:
            print("iter %2d: max kkt_error %.3e, barrier_eps %.2e, min alpha_s %.3f, status %s" % (
                it, r.kkt_error.max(), r.barrier_eps.max(), r.alpha_s_max.min(), sorted(set(int(v) for v in r.status))))
        if (r.status == 1).all():
            return it, r, x, u
        if not np.isin(r.status, (1, 6)).all():
            raise RuntimeError("an instance failed: status %s" % r.status)
        xv, uv = stepper.variable()[:2]
        x, u = torch.from_numpy(xv).to(device), torch.from_numpy(uv).to(device)
    raise RuntimeError("not converged in %d iterations" % max_iter)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=40)
    a = ap.parse_args()
    from nmpc_amd import FmpcStepBatch
    stepper = FmpcStepBatch(N, M, G, a.steps, a.batch)
    it, r, x, u = solve(stepper, a.batch, a.steps, "cuda:0")
    umax = float(u.abs().max())
    print("kernel %s: %d iterations, last call %.3f ms; max |u| %.4f (limit %.1f), final |theta| <= %.3f" % (
        stepper.kernelName(), it, stepper.lastMs(), umax, U_MAX, float(x[:, -1, 0].abs().max())))
    assert umax <= U_MAX
    print("ok")


if __name__ == "__main__":
    main()
