"""iLQR on a damped, torque-limited pendulum whose dynamics and cost are plain torch functions: nothing of the model is compiled
into the library.  Per iteration the B trajectories are linearised with torch.func (vmap over instances and steps), the backward
pass (Riccati recursion, lambda retries, BoxQP feed-forward) runs in one launch of nmpc_amd.RiccatiBatch on the tensors as they are,
and the line search rolls the candidates out in torch.  `lam` / `dlam` of every instance are carried across the iterations
(DDPSolver.hpp:302-333).

  python scripts/torch_ilqr_pendulum.py [--batch 64] [--steps 60] [--iters 30]"""
import argparse
import os
import sys

import torch
from torch.func import hessian, jacrev, vmap

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nmpc_amd import RiccatiBatch  # noqa: E402

DT, U_MAX = 0.05, 4.0
GOAL = torch.tensor([torch.pi, 0.0], dtype=torch.float64)
ALPHAS = [10.0 ** (-0.3 * i) for i in range(11)]  # the reference's alpha_list
FACTOR, LAM_MIN, LAM_MAX = 1.6, 1e-6, 1e10


def step(x, u):
    """One Euler step of theta'' = -g / l sin(theta) - c theta' + u."""
    acc = -9.81 * torch.sin(x[0]) - 0.1 * x[1] + u[0]
    return torch.stack([x[0] + DT * x[1], x[1] + DT * acc])


def running(x, u):
    e = x - GOAL.to(x.device)
    return DT * (0.5 * (e[0] ** 2 + 0.1 * e[1] ** 2) + 0.005 * u[0] ** 2)


def terminal(x):
    e = x - GOAL.to(x.device)
    return 50.0 * e[0] ** 2 + 5.0 * e[1] ** 2


def over_steps(fn):
    return vmap(vmap(fn))  # [B, T, ...]


def rollout(x0, policy):
    """X [B, T + 1, 2], U [B, T, 1] and the cost [B] of u_i = policy(i, x_i), clamped to the limits."""
    X, U = [x0], []
    for i in range(policy.T):
        u = policy(i, X[-1]).clamp(-U_MAX, U_MAX)
        U.append(u)
        X.append(vmap(step)(X[-1], u))
    X, U = torch.stack(X, 1), torch.stack(U, 1)
    return X, U, over_steps(running)(X[:, :-1], U).sum(1) + vmap(terminal)(X[:, -1])


class Policy:
    def __init__(self, T, U, X=None, k=None, K=None, alpha=0.0):
        self.T, self.U, self.X, self.k, self.K, self.alpha = T, U, X, k, K, alpha

    def __call__(self, i, x):
        if self.k is None:
            return self.U[:, i]
        return self.U[:, i] + self.alpha * self.k[:, i] + (self.K[:, i] @ (x - self.X[:, i]).unsqueeze(-1)).squeeze(-1)


def linearise(X, U):
    """The Derivative blocks [B, T, rows, cols] and the terminal pair, contiguous."""
    xs, c = X[:, :-1], lambda t: t.contiguous()
    Fx, Fu = over_steps(jacrev(step, (0, 1)))(xs, U)
    Lx, Lu = over_steps(jacrev(running, (0, 1)))(xs, U)
    (Lxx, Lxu), (_, Luu) = over_steps(hessian(running, (0, 1)))(xs, U)
    return dict(Fx=c(Fx), Fu=c(Fu), Lx=c(Lx), Lu=c(Lu), Lxx=c(Lxx), Luu=c(Luu), Lxu=c(Lxu), Vx_T=c(vmap(jacrev(terminal))(X[:, -1])),
                Vxx_T=c(vmap(hessian(terminal))(X[:, -1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    B, T = a.batch, a.steps
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.zeros(B, 2, dtype=torch.float64, device=dev)
    x0[:, 0] = 0.5 * (2 * torch.rand(B, generator=gen, device=dev, dtype=torch.float64) - 1)  # hanging, +- 0.5 rad
    solver = RiccatiBatch(2, 1, T, B)
    lower = torch.full((1,), -U_MAX, dtype=torch.float64, device=dev)
    upper = -lower
    lam = torch.full((B,), 1e-4, dtype=torch.float64, device=dev)
    dlam = torch.ones(B, dtype=torch.float64, device=dev)
    X, U, J = rollout(x0, Policy(T, 0.1 * torch.ones(B, T, 1, dtype=torch.float64, device=dev)))
    print("iter 0: mean cost %.4f" % J.mean().item())
    for it in range(1, a.iters + 1):
        r = solver.backwardDevice(U=U, lower=lower, upper=upper, lam=lam, dlam=dlam, **linearise(X, U))
        ok = r.status == 1
        lam, dlam = r.lam, r.dlam  # after the retries of this pass
        # line search: per instance the first step size that lowers the cost
        done = ~ok  # an instance whose pass gave up keeps its trajectory
        Xn, Un, Jn = X.clone(), U.clone(), J.clone()
        for alpha in ALPHAS:
            Xc, Uc, Jc = rollout(x0, Policy(T, U, X, r.k, r.K, alpha))
            take = ~done & (Jc < J)
            Xn[take], Un[take], Jn[take] = Xc[take], Uc[take], Jc[take]
            done |= take
            if done.all():
                break
        improved = Jn < J
        gain = (J - Jn).max().item()
        X, U, J = Xn, Un, Jn
        # the reference's lambda schedule (DDPSolver.hpp:302-333), per instance
        down = torch.minimum(dlam / FACTOR, torch.full_like(dlam, 1 / FACTOR))
        up = torch.maximum(dlam * FACTOR, torch.full_like(dlam, FACTOR))
        dlam = torch.where(improved, down, up)
        lam = torch.where(improved, torch.where(lam >= LAM_MIN, lam * dlam, torch.zeros_like(lam)), torch.maximum(lam * dlam, torch.full_like(lam, LAM_MIN)))
        lam = lam.clamp(max=LAM_MAX).contiguous()
        dlam = dlam.contiguous()
        print("iter %d: mean cost %.4f, passes %d..%d, improved %d / %d, backward %.3f ms" % (
            it, J.mean().item(), int(r.n_backward.min()), int(r.n_backward.max()), int(improved.sum()), B, solver.lastMs()))
        if gain < 1e-7:
            break
    err = (X[:, -1] - GOAL.to(dev)).abs().max().item()
    print("final: mean cost %.4f, worst |x_T - goal| %.3f, %s" % (J.mean().item(), err, solver.kernelName()))


if __name__ == "__main__":
    main()
