// Host-side C++ mirror of the reference's nmpc_cgmres::Gmres (nmpc_cgmres/include/nmpc_cgmres/Gmres.h:21-204) for a BATCH of
// independent dense systems A x = b of one size on one MI355X.  Same public surface (make_triangular_, apply_reorth_,
// solve(A, b, x, k_max, eps), H, g, err list, basis) with a batch index where the reference has one solver.
//
// Plain C++17 (no HIP runtime, no Eigen): everything numeric happens behind the C-ABI of <nmpc_hip_gmres.h> in libnmpc_hip_ddp.so.
#pragma once

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include <nmpc_hip_gmres.h>

namespace nmpc_amd
{
/** \brief Batched GMRES method to solve linear equations (Kelley 1995, Algorithms 3.5.1 and 3.4.2). */
class GmresBatch
{
public:
  static constexpr int MaxDim = 512; // NMPC_HIP_GMRES_MAX_DIM
  static constexpr int HouseholderMaxK = 128; // NMPC_HIP_GMRES_HOUSEHOLDER_MAX_K
  static_assert(MaxDim == NMPC_HIP_GMRES_MAX_DIM && HouseholderMaxK == NMPC_HIP_GMRES_HOUSEHOLDER_MAX_K, "mirror and header disagree");

  /** Gmres() (Gmres.h:31) for `batch` systems of size n; k_max_capacity sizes the device buffers (clamped to n). */
  GmresBatch(int n, int batch, int k_max_capacity = 100, int device = 0) : n_(n), batch_(batch)
  {
    check(nmpc_hip_gmres_create(n, batch, k_max_capacity, device, &h_));
  }

  ~GmresBatch()
  {
    nmpc_hip_gmres_destroy(h_);
  }

  GmresBatch(const GmresBatch &) = delete;
  GmresBatch & operator=(const GmresBatch &) = delete;

  /** solve(A, b, x, k_max, eps) (Gmres.h:42-51) for every system: A [B][n][n] row-major, b [B][n]; x [B][n] is the initial guess
      and is overwritten by the solution. */
  void solve(const std::vector<double> & A, const std::vector<double> & b, std::vector<double> & x, int k_max = 100, double eps = 1e-10)
  {
    const size_t bn = static_cast<size_t>(batch_) * n_;
    if(A.size() != bn * n_ || b.size() != bn || x.size() != bn)
    {
      throw std::invalid_argument("[Gmres] A must hold batch * n * n entries, b and x batch * n");
    }
    check(nmpc_hip_gmres_set_system(h_, A.data(), b.data(), x.data(), 0, 0));
    pushConfig(k_max, eps);
    check(nmpc_hip_gmres_solve(h_));
    x = get<double>(NMPC_HIP_GMRES_FIELD_X);
  }

  /** The systems of the last solve again, from the x it returned (restarted GMRES). */
  std::vector<double> solveAgain(int k_max = 100, double eps = 1e-10)
  {
    pushConfig(k_max, eps);
    check(nmpc_hip_gmres_solve(h_));
    return get<double>(NMPC_HIP_GMRES_FIELD_X);
  }

  /** Device arrays (layouts of nmpc_hip_gmres.h), asynchronous on `stream` (a hipStream_t; nullptr = the solver's own). */
  void setSystemDevice(const double * d_A, const double * d_b, const double * d_x0, bool a_col_major)
  {
    check(nmpc_hip_gmres_set_system(h_, d_A, d_b, d_x0, 1, a_col_major ? 1 : 0));
  }
  void solveDevice(int k_max = 100, double eps = 1e-10, void * stream = nullptr)
  {
    pushConfig(k_max, eps);
    check(nmpc_hip_gmres_solve_device(h_, stream));
  }
  void synchronize()
  {
    check(nmpc_hip_gmres_synchronize(h_));
  }

  /** H_ (Gmres.h:198) of system b: (k_max + 1) x k_max row-major, k_max as clamped by the last solve. */
  std::vector<double> H(int b) const
  {
    return slice(get<double>(NMPC_HIP_GMRES_FIELD_H), b);
  }
  /** g_ (Gmres.h:199) of system b. */
  std::vector<double> g(int b) const
  {
    return slice(get<double>(NMPC_HIP_GMRES_FIELD_G), b);
  }
  /** err_list_ (Gmres.h:201) of system b: iters(b) + 1 entries. */
  std::vector<double> errList(int b) const
  {
    std::vector<double> e = slice(get<double>(NMPC_HIP_GMRES_FIELD_ERR_LIST), b);
    e.resize(std::min<size_t>(e.size(), static_cast<size_t>(iters(b)) + 1));
    return e;
  }
  /** basis_ (Gmres.h:203) of system b: iters(b) + 1 vectors of n entries; needs keep_basis_ = true at the solve. */
  std::vector<std::vector<double>> basis(int b) const
  {
    const std::vector<double> all = slice(get<double>(NMPC_HIP_GMRES_FIELD_BASIS), b);
    std::vector<std::vector<double>> out;
    for(int j = 0; j <= iters(b); j++)
    {
      out.emplace_back(all.begin() + static_cast<size_t>(j) * n_, all.begin() + static_cast<size_t>(j + 1) * n_);
    }
    return out;
  }
  int iters(int b) const
  {
    return get<int>(NMPC_HIP_GMRES_FIELD_ITERS)[at(b)];
  }
  int reorth(int b) const
  {
    return get<int>(NMPC_HIP_GMRES_FIELD_REORTH)[at(b)];
  }
  /** nmpc_hip_gmres_status of system b. */
  int status(int b) const
  {
    return get<int>(NMPC_HIP_GMRES_FIELD_STATUS)[at(b)];
  }
  std::string kernelName() const
  {
    const char * name = nullptr;
    check(nmpc_hip_gmres_kernel_name(h_, &name));
    return name;
  }
  float lastMs() const
  {
    float ms = 0;
    check(nmpc_hip_gmres_last_ms(h_, &ms));
    return ms;
  }
  int batch() const
  {
    return batch_;
  }

public:
  bool make_triangular_ = true;
  bool apply_reorth_ = true;
  bool keep_basis_ = false;

protected:
  static void check(int rc)
  {
    if(rc == NMPC_HIP_OK)
    {
      return;
    }
    const std::string msg = nmpc_hip_gmres_last_error();
    if(rc == NMPC_HIP_ERR_INVALID_ARGUMENT)
    {
      throw std::invalid_argument(msg);
    }
    throw std::runtime_error(msg);
  }

  int at(int b) const
  {
    if(b < 0 || b >= batch_)
    {
      throw std::out_of_range("[Gmres] batch index out of range");
    }
    return b;
  }

  void pushConfig(int k_max, double eps)
  {
    nmpc_hip_gmres_config c;
    c.k_max = k_max;
    c.eps = eps;
    c.make_triangular = make_triangular_ ? 1 : 0;
    c.apply_reorth = apply_reorth_ ? 1 : 0;
    c.keep_basis = keep_basis_ ? 1 : 0;
    check(nmpc_hip_gmres_set_config(h_, &c));
  }

  template<class T>
  std::vector<T> get(int field) const
  {
    size_t bytes = 0;
    check(nmpc_hip_gmres_field_bytes(h_, field, &bytes));
    std::vector<T> out(bytes / sizeof(T));
    check(nmpc_hip_gmres_get(h_, field, out.data(), bytes, 0));
    return out;
  }

  std::vector<double> slice(const std::vector<double> & all, int b) const
  {
    const size_t per = all.size() / batch_;
    return std::vector<double>(all.begin() + at(b) * per, all.begin() + (at(b) + 1) * per);
  }

  int n_ = 0;
  int batch_ = 0;
  nmpc_hip_gmres_handle h_ = nullptr;
};
} // namespace nmpc_amd
