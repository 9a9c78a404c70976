// CPU checker of the batched C/GMRES solver (test infrastructure, not product code): a plain C++17 statement of the algorithm
// (C/GMRES, Ohtsuka 2004; GMRES with Givens rotations, Kelley Alg. 3.5.1) and of the shipped problems, without Eigen, built by the
// tests with g++ -O2 -ffp-contract=off and loaded through ctypes.  Independent of the device code: its own vectors, its own
// model functions (std::sin / std::cos / std::exp of the host libm), the operation order of the reference solver.
#pragma once

extern "C"
{
  /** model: 0 = cgmres_semiactive_damper, 1 = cgmres_cartpole, 2 = cgmres_cartpole_with_input_bound.  Returns 0 or -1. */
  int chk_model_dims(int model, int * nx, int * nuc);

  /** The four problem functions at P points with one parameter block (the doubles of the problem object). */
  int chk_model_eval(int model, const double * params, int P, const double * t, const double * x, const double * u, const double * lmd,
                     double * dotx, double * dotlmd, double * dphidx, double * dhdu);

  /** GMRES on one dense system (A row-major n x n); x is the initial guess in, the solution out. */
  void chk_dense_gmres(int n, const double * A, const double * b, double * x, int k_max, int apply_reorth, double eps, int * iters,
                       int * reorth_fired);

  /** cfg: sim_duration, steady_horizon_duration, horizon_divide_num, horizon_increase_ratio, dt, eq_zeta, k_max, finite_diff_delta,
      dump_step, ode_solver, sim_ode_solver (0 Euler, 1 RK4).  params: one block (per_instance = 0) or B blocks.
      do_run = 0: setup only.  Outputs [B][...]; logs [B][log_rows][...] (may be NULL when dump_step = 0).  Returns the number of
      ticks run. */
  int chk_solve(int model, const double * params, int per_instance, const double * cfg, int B, const double * x0, const double * u0,
                int do_run, int n_threads, double * x_out, double * u_out, double * U_out, int * status, double * err_out,
                double * log_x, double * log_u, double * log_err, int * log_iters, int * log_reorth, int log_rows);
}
