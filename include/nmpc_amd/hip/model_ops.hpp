// Type-erased description of one registered problem type: what the C-ABI (nmpc_amd/csrc/capi.hip) knows about a problem
// class compiled into gfx950 code.  model_registry.hpp (ModelOpsFor) fills it for every kernel family.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <cstring>

#include <hip/hip_runtime.h>

#include <nmpc_amd/hip/ddp_kernels.hpp>
#include <nmpc_amd/hip/mpc_args.hpp>

namespace nmpc_amd
{
namespace hip
{
/** The kernel families of the DDP solve.  Every name the library reports or accepts for one — the short name of
    nmpc_hip_ddp_set_kernel / NMPC_HIP_DDP_KERNEL, the __global__ symbol nmpc_hip_ddp_kernel_name reports — comes from kFamilies. */
enum class Family : int
{
  Auto = -1, //!< (LaunchKnobs::pin only: no family forced)
  Lane, //!< ddp_kernels.hpp: one wavefront, one instance per lane
  TwoWave, //!< ddp_kernels_2w.hpp: master + helper wavefront, LDS-staged records
  Quad, //!< ddp_kernels_quad.hpp: matrix-core backward pass, 16 instances per workgroup (n <= 4, one input)
  Wpi, //!< ddp_kernels_wpi.hpp: one wavefront per instance (9 <= n <= 16)
  Tile64, //!< ddp_kernels_tile64.hpp: groups of instances per workgroup (5 <= n <= 15), fp64 and float
  Tile32, //!< ddp_kernels_tile32.hpp: the fp32 tile kernel (n in {4, 8, 12}, m <= 4)
};
struct FamilyInfo
{
  Family family;
  const char * pin; //!< short name
  const char * kernel; //!< __global__ symbol, as rocprofv3 lists it
  bool workspace; //!< the kernel needs the handle's per-instance workspace (DeviceBuffers::wpi_ws)
  int gain_layout; //!< ModelOps: 0 = tile-major kff / Kfb, 1 = instance-major records [B][T][MM + MM N] in the workspace
  int swap_group; //!< instances per workgroup of its resumable launches (the ragged compaction swaps whole workgroups)
  bool own_problems; //!< it has instantiations with one problem object per instance (set_model_params_batch)
};
inline constexpr FamilyInfo kFamilies[] = {
    {Family::Lane, "1w", "ddp_solve_tpi_kernel", false, 0, 64, false},
    {Family::TwoWave, "2w", "ddp_solve_tpi2w_kernel", false, 0, 64, true},
    {Family::Quad, "quad", "ddp_solve_quad_kernel", false, 0, 16, true},
    {Family::Wpi, "wpi", "ddp_solve_wpi_kernel", true, 0, 64, true},
    {Family::Tile64, "tile64", "ddp_solve_tile64_kernel", true, 1, 64, true},
    {Family::Tile32, "tile32", "ddp_solve_tile32_kernel", true, 1, 64, true},
};
constexpr const FamilyInfo & familyInfo(Family f)
{
  return kFamilies[static_cast<int>(f)];
}
//! the family of a short name or a kernel symbol ("auto": Family::Auto); false for anything else
inline bool familyByName(const char * name, Family * out)
{
  if(std::strcmp(name, "auto") == 0)
  {
    *out = Family::Auto;
    return true;
  }
  for(const FamilyInfo & f : kFamilies)
  {
    if(std::strcmp(name, f.pin) == 0 || std::strcmp(name, f.kernel) == 0)
    {
      *out = f.family;
      return true;
    }
  }
  return false;
}

/** What picks a kernel family and its launch schedule besides the problem's shape, the batch size and the Configuration — per
    HANDLE, fixed when the handle is created or through the C-ABI (nmpc_hip_ddp_set_kernel, nmpc_hip_ddp_set_dispatch_batch), never
    read from the environment on the launch path.  The environment variables (NMPC_HIP_DDP_KERNEL, NMPC_HIP_DDP_TILE64_GROUP / _CHUNK /
    _PAIR / _ADOPT / _WIDE, NMPC_HIP_DDP_FAN_SCRATCH, NMPC_HIP_DDP_FAN_AUTO, NMPC_HIP_DDP_RAGGED, NMPC_HIP_DDP_NO_WORKSPACE,
    NMPC_HIP_DDP_FUSED_INGEST) are
    developer overrides for A/B measurements and tests: fromEnvironment() reads them ONCE, when a handle is created. */
struct LaunchKnobs
{
  Family pin = Family::Auto; //!< a forced kernel family (families the problem type does not have are ignored)
  int tile64_group = 0; //!< > 0: at most this many instances per group of the tile kernel
  int tile64_chunk = 0; //!< > 0: at most this many timesteps per pass of its model code
  int tile64_pair = 1, tile64_adopt = 1, tile64_wide = 1; //!< 0: that part of its line-search schedule off (A/B)
  int fan_scratch = 1; //!< 0: the quad kernel's fan-out scratch is not allocated
  int fan_auto = 0; //!< valid if has_fan_auto: ModelOpsFor::kQuadFanOutAutoMaxIter overridden
  int has_fan_auto = 0;
  int ragged = 0; //!< 1 forces the ragged-convergence schedule on, -1 off, 0: Configuration::ragged_schedule decides
  int have_workspace = 1; //!< the handle's per-instance workspace was allocated (0: the kernels that need it are not chosen)
  int n_cu = 256; //!< compute units of the handle's device (the handle sets it at create)
  //! > 0: the batch size the kernel family is chosen FOR — a shard of a larger solve takes the family the whole batch would get,
  //! so that its results are the unsharded solve's bit for bit (families differ in the last bits; DDPSolverSharded, bench.py)
  int dispatch_batch = 0;
  //! 1: a whole-solve launch of the quad kernel reads the caller's arrays itself (QuadSolver::ingestInputs) — one dispatch per
  //! solve_device, no ingest_kernel and no event between the two; 0: ingest_kernel first, as every other family (A/B, tests)
  int fused_ingest = 1;

  int batchFor(int batch) const
  {
    return dispatch_batch > 0 ? dispatch_batch : batch;
  }
  static LaunchKnobs fromEnvironment()
  {
    LaunchKnobs k;
    if(const char * e = std::getenv("NMPC_HIP_DDP_KERNEL"))
    {
      for(const FamilyInfo & f : kFamilies) // (short names only; anything else: automatic)
      {
        if(std::strcmp(e, f.pin) == 0)
        {
          k.pin = f.family;
        }
      }
    }
    if(const char * e = std::getenv("NMPC_HIP_DDP_TILE64_GROUP"))
    {
      k.tile64_group = std::atoi(e) & 0xffff;
    }
    if(const char * e = std::getenv("NMPC_HIP_DDP_TILE64_CHUNK"))
    {
      k.tile64_chunk = std::atoi(e) & 0x1fff;
    }
    if(const char * e = std::getenv("NMPC_HIP_DDP_TILE64_PAIR"))
    {
      k.tile64_pair = std::atoi(e) != 0;
    }
    if(const char * e = std::getenv("NMPC_HIP_DDP_TILE64_ADOPT"))
    {
      k.tile64_adopt = std::atoi(e) != 0;
    }
    if(const char * e = std::getenv("NMPC_HIP_DDP_TILE64_WIDE"))
    {
      k.tile64_wide = std::atoi(e) != 0;
    }
    if(const char * e = std::getenv("NMPC_HIP_DDP_FAN_SCRATCH"))
    {
      k.fan_scratch = std::strcmp(e, "0") != 0;
    }
    if(const char * e = std::getenv("NMPC_HIP_DDP_FAN_AUTO"))
    {
      k.fan_auto = std::atoi(e);
      k.has_fan_auto = 1;
    }
    if(const char * e = std::getenv("NMPC_HIP_DDP_RAGGED"))
    {
      k.ragged = std::strcmp(e, "0") == 0 ? -1 : 1;
    }
    if(const char * e = std::getenv("NMPC_HIP_DDP_NO_WORKSPACE")) // (tests of the path a failed workspace allocation takes)
    {
      k.have_workspace = std::strcmp(e, "0") == 0;
    }
    if(const char * e = std::getenv("NMPC_HIP_DDP_FUSED_INGEST"))
    {
      k.fused_ingest = std::strcmp(e, "0") != 0;
    }
    return k;
  }
};

/** The kernel one solve launches: chosen once per solve by ModelOps::plan, then handed to ModelOps::launch_solve and read by the
    C-ABI for everything that depends on the family (gain layout, ragged / streamed eligibility, swap tables). */
struct KernelPlan
{
  Family family = Family::Lane;
  bool constrained = false; //!< Configuration::with_input_constraint: the BoxQP instantiation
  bool own_problems = false; //!< one problem object per instance (set_model_params_batch): the kOwnProblem instantiation
  bool fan_out = false; //!< the quad kernel's step-size-parallel line search
  bool resumable = false; //!< the family has a resumable instantiation for this solve (ragged schedule, streamed solves)

  const char * kernelName() const
  {
    return familyInfo(family).kernel;
  }
  bool needsWorkspace() const
  {
    return familyInfo(family).workspace;
  }
  int gainLayout() const
  {
    return familyInfo(family).gain_layout;
  }
  int swapGroup() const
  {
    return familyInfo(family).swap_group;
  }
};

//! bumped whenever ModelOps changes layout: nmpc_hip_ddp_register_model refuses a table compiled against another header
constexpr int kModelOpsAbi = 3;

/** Type-erased operations of one registered problem type. */
struct ModelOps
{
  int abi = kModelOpsAbi; //!< leading layout word (kModelOpsAbi)
  const char * name;
  int state_dim;
  int input_dim_max;
  int dynamic_input;
  size_t param_bytes;
  //! placement-constructs a default problem object into out
  void (*default_params)(void * out);
  //! the kernel a solve of `batch` instances under `cfg` runs on, with the handle's knobs; own_problems: one problem object per
  //! instance (a pure host function: no environment, no device queries)
  KernelPlan (*plan)(const LaunchKnobs & knobs, int batch, const nmpc_hip_ddp_config & cfg, bool own_problems);
  //! launches the kernel of `plan`; params points to a host copy of the problem object; buf.iter_end > 0: a resumable launch
  hipError_t (*launch_solve)(const void * params,
                             const KernelPlan & plan,
                             const LaunchKnobs & knobs,
                             const nmpc_hip_ddp_config & cfg,
                             const DeviceBuffers & buf,
                             hipStream_t stream);
  //! host-side inputDim(t0 + i dt) for i < T (validation of initial_u_list, DDPSolver.hpp:46-58)
  void (*input_dims)(const void * params, double t0, int T, int * out);
  //! dt() of the problem object
  double (*dt)(const void * params);
  //! launches the receding-horizon advance step (mpc_kernels.hpp) between two solves
  hipError_t (*launch_mpc_advance)(const void * params,
                                   const DeviceBuffers & buf,
                                   const MpcAdvanceArgs & args,
                                   hipStream_t stream);
  //! 1 if the problem has the plant step stateEq(t, x, u, dt) the plant pattern integrates with
  int has_plant_step;
  //! elements (of the problem's scalar type) of per-instance workspace the model's kernels need for horizon T (0: none)
  size_t (*wpi_workspace_doubles)(const LaunchKnobs & knobs, int T);
  //! sizeof(Problem::Scalar): 8 for the reference's arithmetic, 4 for the fp32 problem types (every Scalar device array
  //! of the handle has this element size; the C-ABI exchanges doubles either way)
  int scalar_bytes;
};

} // namespace hip
} // namespace nmpc_amd

extern "C" int nmpc_hip_ddp_register_model(const nmpc_amd::hip::ModelOps * ops);

/** Registers the problem type under ProblemType::kName with the operations `OpsMaker::make()` returns. */
#define NMPC_AMD_REGISTER_PROBLEM_WITH(ProblemType, OpsMaker)                                         \
  namespace                                                                                           \
  {                                                                                                   \
  struct ProblemType##Registrar                                                                       \
  {                                                                                                   \
    ProblemType##Registrar()                                                                          \
    {                                                                                                 \
      static const nmpc_amd::hip::ModelOps ops = OpsMaker::make();                                    \
      nmpc_hip_ddp_register_model(&ops);                                                              \
    }                                                                                                 \
  } g_##ProblemType##_registrar;                                                                      \
  }
