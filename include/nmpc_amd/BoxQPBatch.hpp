// Host-side C++ mirror of the reference's nmpc_ddp::BoxQP<VarDim> (nmpc_ddp/include/nmpc_ddp/BoxQP.h:18-397) for a BATCH of
// independent box-constrained QPs of one size on one MI355X.  Same public members (config(), solve(), retval, retstr, free indices,
// traceDataList()) with a batch index where the reference has one solver; VarDim may be nmpc_amd::Dynamic with the size given at
// run time, as with Eigen::Dynamic there.
//
// Plain C++17 (no HIP runtime, no Eigen): everything numeric happens behind the C-ABI of <nmpc_hip_boxqp.h> in libnmpc_hip_ddp.so.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include <nmpc_amd/linalg.hpp> // nmpc_amd::Dynamic
#include <nmpc_hip_boxqp.h>

namespace nmpc_amd
{
/** \brief Batched solver for quadratic programming problems with box constraints.
    \tparam VarDim dimension of decision variables (1 .. 64, or nmpc_amd::Dynamic) */
template<int VarDim>
class BoxQPBatch
{
public:
  /*! \brief Configuration (BoxQP.h:33-55); trace_capacity = rows of traceDataList() kept per QP (0 = none). */
  struct Configuration
  {
    int print_level = 1;
    int max_iter = 500;
    double grad_thre = 1e-8;
    double rel_improve_thre = 1e-8;
    double step_factor = 0.6;
    double min_step = 1e-22;
    double armijo_param = 0.1;
    int trace_capacity = 0;
  };

  /*! \brief The scalar members of BoxQP::TraceData (BoxQP.h:58-82); clamped_flag as a mask (bit j = clamped_flag[j]). */
  struct TraceData
  {
    int iter = 0;
    double obj = 0;
    int factorization_num = 0;
    int step_num = 0;
    std::uint64_t clamped_flag = 0;
    double grad_norm = 0; //!< grad_norm of BoxQP.h:244-248 (a sum of squares)
  };

  /** BoxQP(var_dim) (BoxQP.h:101-118) for `batch` QPs. */
  explicit BoxQPBatch(int batch, int var_dim = VarDim, int device = 0) : var_dim_(var_dim), batch_(batch)
  {
    if(var_dim_ <= 0)
    {
      throw std::runtime_error("var_dim must be positive: " + std::to_string(var_dim_) + " <= 0");
    }
    if(VarDim != Dynamic && var_dim_ != VarDim)
    {
      throw std::runtime_error("var_dim is inconsistent with template parameter: " + std::to_string(var_dim_)
                               + " != " + std::to_string(VarDim));
    }
    check(nmpc_hip_boxqp_create(var_dim_, batch_, device, &h_));
  }

  ~BoxQPBatch()
  {
    nmpc_hip_boxqp_destroy(h_);
  }

  BoxQPBatch(const BoxQPBatch &) = delete;
  BoxQPBatch & operator=(const BoxQPBatch &) = delete;

  /** solve(H, g, lower, upper[, initial_x]) (BoxQP.h:126-347) for every QP: H [B][n][n] (symmetric, row-major), the vectors [B][n];
      initial_x may be nullptr (zeros).  Returns x [B][n]. */
  std::vector<double> solve(const double * H, const double * g, const double * lower, const double * upper, const double * initial_x = nullptr)
  {
    pushConfig();
    check(nmpc_hip_boxqp_solve(h_, H, g, lower, upper, initial_x));
    if(config_.print_level >= 2)
    {
      const std::vector<int> ret = get<int>(NMPC_HIP_BOXQP_FIELD_RETVAL), it = get<int>(NMPC_HIP_BOXQP_FIELD_ITER),
                             nf = get<int>(NMPC_HIP_BOXQP_FIELD_FACTORIZATION_NUM);
      const std::vector<double> obj = get<double>(NMPC_HIP_BOXQP_FIELD_OBJ);
      for(int b = 0; b < batch_; b++)
      {
        std::cout << "[BoxQP] " << b << ": result: " << ret[b] << " (" << retstr_.at(ret[b]) << "), iter: " << it[b] << ", obj: " << obj[b]
                  << ", factorization_num: " << nf[b] << std::endl;
      }
    }
    return get<double>(NMPC_HIP_BOXQP_FIELD_X);
  }
  std::vector<double> solve(const std::vector<double> & H, const std::vector<double> & g, const std::vector<double> & lower,
                            const std::vector<double> & upper)
  {
    checkSizes(H, g, lower, upper);
    return solve(H.data(), g.data(), lower.data(), upper.data(), nullptr);
  }
  std::vector<double> solve(const std::vector<double> & H, const std::vector<double> & g, const std::vector<double> & lower,
                            const std::vector<double> & upper, const std::vector<double> & initial_x)
  {
    checkSizes(H, g, lower, upper);
    if(initial_x.size() != g.size())
    {
      throw std::invalid_argument("[BoxQP] initial_x must hold batch * var_dim entries");
    }
    return solve(H.data(), g.data(), lower.data(), upper.data(), initial_x.data());
  }

  /** Same with device arrays, asynchronous on `stream` (a hipStream_t; nullptr = the solver's own stream). */
  void solveDevice(const double * d_H, const double * d_g, const double * d_lower, const double * d_upper, const double * d_initial_x = nullptr,
                   void * stream = nullptr)
  {
    pushConfig();
    check(nmpc_hip_boxqp_solve_device(h_, d_H, d_g, d_lower, d_upper, d_initial_x, stream));
  }

  void synchronize()
  {
    check(nmpc_hip_boxqp_synchronize(h_));
  }

  /** Accessor to configuration (BoxQP.h:350-359); read at the next solve. */
  Configuration & config()
  {
    return config_;
  }
  const Configuration & config() const
  {
    return config_;
  }

  /** x of QP b (the value solve() of the reference returns). */
  std::vector<double> x(int b) const
  {
    const std::vector<double> all = get<double>(NMPC_HIP_BOXQP_FIELD_X);
    return std::vector<double>(all.begin() + static_cast<size_t>(at(b)) * var_dim_, all.begin() + static_cast<size_t>(b + 1) * var_dim_);
  }

  /** retval_ (BoxQP.h:372) of QP b. */
  int retval(int b) const
  {
    return get<int>(NMPC_HIP_BOXQP_FIELD_RETVAL)[at(b)];
  }

  /** retstr_.at(retval_) of QP b. */
  const std::string & retstr(int b) const
  {
    return retstr_.at(retval(b));
  }

  int iter(int b) const
  {
    return get<int>(NMPC_HIP_BOXQP_FIELD_ITER)[at(b)];
  }

  /** free_idxs_ (BoxQP.h:389) of QP b. */
  std::vector<int> freeIdxs(int b) const
  {
    const std::uint64_t mask = get<std::uint64_t>(NMPC_HIP_BOXQP_FIELD_FREE_MASK)[at(b)];
    std::vector<int> idxs;
    for(int j = 0; j < var_dim_; j++)
    {
      if((mask >> j) & 1u)
      {
        idxs.push_back(j);
      }
    }
    return idxs;
  }

  /** llt_free_ (BoxQP.h:386) of QP b: the lower factor of H[free, free], nf x nf row-major, nf = freeIdxs(b).size(). */
  std::vector<double> factor(int b) const
  {
    const std::vector<double> all = get<double>(NMPC_HIP_BOXQP_FIELD_FACTOR);
    const size_t n = var_dim_, nf = freeIdxs(b).size();
    std::vector<double> L(nf * nf, 0.0);
    for(size_t r = 0; r < nf; r++)
    {
      for(size_t c = 0; c <= r; c++)
      {
        L[r * nf + c] = all[(static_cast<size_t>(at(b)) * n + r) * n + c];
      }
    }
    return L;
  }

  /** traceDataList() (BoxQP.h:362) of QP b, as far as config().trace_capacity reached: the initial entry, then one per iteration. */
  std::vector<TraceData> traceDataList(int b) const
  {
    const std::vector<std::uint64_t> raw = get<std::uint64_t>(NMPC_HIP_BOXQP_FIELD_TRACE);
    const int cap = static_cast<int>(raw.size() / (static_cast<size_t>(batch_) * NMPC_HIP_BOXQP_TRACE_COLUMNS));
    const int rows = std::min(cap, iter(b) + 1);
    std::vector<TraceData> out(rows);
    for(int r = 0; r < rows; r++)
    {
      const std::uint64_t * w = raw.data() + (static_cast<size_t>(at(b)) * cap + r) * NMPC_HIP_BOXQP_TRACE_COLUMNS;
      out[r].iter = static_cast<int>(asDouble(w[0]));
      out[r].obj = asDouble(w[1]);
      out[r].factorization_num = static_cast<int>(asDouble(w[2]));
      out[r].step_num = static_cast<int>(asDouble(w[3]));
      out[r].clamped_flag = w[4];
      out[r].grad_norm = asDouble(w[5]);
    }
    return out;
  }

  /** "boxqp_lane_kernel" or "boxqp_wave_kernel": what the next solve launches. */
  std::string kernelName() const
  {
    const char * name = nullptr;
    check(nmpc_hip_boxqp_kernel_name(h_, &name));
    return name;
  }

  /** "lane", "wave" or nullptr (the automatic choice). */
  void setKernel(const char * kernel)
  {
    check(nmpc_hip_boxqp_set_kernel(h_, kernel));
  }

  float lastSolveMs() const
  {
    float ms = 0;
    check(nmpc_hip_boxqp_last_solve_ms(h_, &ms));
    return ms;
  }

  int batch() const
  {
    return batch_;
  }

public:
  //! Dimension of decision variables
  const int var_dim_ = 0;

  //! Return string (BoxQP.h:375-383)
  const std::unordered_map<int, std::string> retstr_ = {{-2, "Gradient of search direction is positive"},
                                                        {-1, "Hessian is not positive definite"},
                                                        {0, "Computation is not finished"},
                                                        {1, "Maximum main iterations exceeded"},
                                                        {2, "Maximum line-search iterations exceeded"},
                                                        {3, "No bounds, returning Newton point"},
                                                        {4, "Improvement smaller than tolerance"},
                                                        {5, "Gradient norm smaller than tolerance"},
                                                        {6, "All dimensions are clamped"}};

protected:
  static void check(int rc)
  {
    if(rc == NMPC_HIP_OK)
    {
      return;
    }
    const std::string msg = nmpc_hip_boxqp_last_error();
    if(rc == NMPC_HIP_ERR_INVALID_ARGUMENT)
    {
      throw std::invalid_argument(msg);
    }
    throw std::runtime_error(msg);
  }

  static double asDouble(std::uint64_t w)
  {
    double d;
    static_assert(sizeof(d) == sizeof(w), "8-byte words");
    std::memcpy(&d, &w, sizeof(d));
    return d;
  }

  int at(int b) const
  {
    if(b < 0 || b >= batch_)
    {
      throw std::out_of_range("[BoxQP] batch index out of range");
    }
    return b;
  }

  void checkSizes(const std::vector<double> & H, const std::vector<double> & g, const std::vector<double> & lower,
                  const std::vector<double> & upper) const
  {
    const size_t bn = static_cast<size_t>(batch_) * var_dim_;
    if(H.size() != bn * var_dim_ || g.size() != bn || lower.size() != bn || upper.size() != bn)
    {
      throw std::invalid_argument("[BoxQP] H must hold batch * var_dim * var_dim entries, g / lower / upper batch * var_dim");
    }
  }

  void pushConfig()
  {
    nmpc_hip_boxqp_config c;
    c.max_iter = config_.max_iter;
    c.grad_thre = config_.grad_thre;
    c.rel_improve_thre = config_.rel_improve_thre;
    c.step_factor = config_.step_factor;
    c.min_step = config_.min_step;
    c.armijo_param = config_.armijo_param;
    c.trace_capacity = config_.trace_capacity;
    check(nmpc_hip_boxqp_set_config(h_, &c));
  }

  template<class T>
  std::vector<T> get(int field) const
  {
    size_t bytes = 0;
    check(nmpc_hip_boxqp_field_bytes(h_, field, &bytes));
    std::vector<T> out(bytes / sizeof(T));
    check(nmpc_hip_boxqp_get(h_, field, out.data(), bytes, 0));
    return out;
  }

  int batch_ = 0;
  nmpc_hip_boxqp_handle h_ = nullptr;
  Configuration config_;
};
} // namespace nmpc_amd
