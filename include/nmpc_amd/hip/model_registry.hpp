// Registry that connects a problem TYPE (a functor class derived from nmpc_amd::DDPProblem, compiled into
// gfx950 code together with the solver kernel) to the NAME the C-ABI of include/nmpc_hip_ddp.h uses.
//
// A user model is added without touching the library: write the problem header, then in one .hip file
//     #include <nmpc_amd/hip/model_registry.hpp>
//     #include "MyProblem.hpp"
//     NMPC_AMD_REGISTER_PROBLEM(MyProblem);          // needs: static constexpr const char * kName
// compile it with hipcc --offload-arch=gfx950 and link (or dlopen) it next to libnmpc_hip_ddp.so.  fp64 and fp32 problem
// types register the same way: ModelOpsFor picks the kernel families of the problem's Scalar type and shape.
#pragma once

#include <atomic>
#include <initializer_list>

#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>

#include <nmpc_amd/hip/model_ops.hpp>
#include <nmpc_amd/hip/ddp_kernels.hpp>
#include <nmpc_amd/hip/ddp_kernels_2w.hpp>
#include <nmpc_amd/hip/ddp_kernels_quad.hpp>
#include <nmpc_amd/hip/ddp_kernels_wpi.hpp>
#include <nmpc_amd/hip/ddp_kernels_tile64.hpp>
#include <nmpc_amd/hip/ddp_kernels_tile32.hpp>
#include <nmpc_amd/hip/mpc_kernels.hpp>

namespace nmpc_amd
{
namespace hip
{
/** The handle allocates every Scalar array with sizeof(Problem::Scalar) (ModelOps::scalar_bytes): an fp32 problem type's kernels
    see the same pointers as float arrays. */
inline DeviceBuffersT<float> floatView(const DeviceBuffers & buf64)
{
  DeviceBuffersT<float> buf;
  buf.B = buf64.B;
  buf.Bp = buf64.Bp;
  buf.T = buf64.T;
  buf.trace_rows = buf64.trace_rows;
  buf.t0 = reinterpret_cast<const float *>(buf64.t0);
  buf.x0 = reinterpret_cast<const float *>(buf64.x0);
  buf.X = reinterpret_cast<float *>(buf64.X);
  buf.U = reinterpret_cast<float *>(buf64.U);
  buf.cost = reinterpret_cast<float *>(buf64.cost);
  buf.kff = reinterpret_cast<float *>(buf64.kff);
  buf.Kfb = reinterpret_cast<float *>(buf64.Kfb);
  buf.trace = reinterpret_cast<float *>(buf64.trace);
  buf.trace_last = reinterpret_cast<float *>(buf64.trace_last);
  buf.dV = reinterpret_cast<float *>(buf64.dV);
  buf.status = buf64.status;
  buf.iters = buf64.iters;
  buf.sel = buf64.sel;
  buf.qp_ret = buf64.qp_ret;
  buf.qp_free = buf64.qp_free;
  buf.input_dim = buf64.input_dim;
  buf.wpi_ws = reinterpret_cast<float *>(buf64.wpi_ws);
  buf.phase_ticks = buf64.phase_ticks;
  buf.params_batch = buf64.params_batch;
  buf.lim_batch = buf64.lim_batch; // (the limits are read by the receding-horizon driver's clamp: doubles in every handle)
  buf.lim_steps = buf64.lim_steps;
  buf.lim_steps_per_instance = buf64.lim_steps_per_instance;
  buf.lim_mm = buf64.lim_mm;
  buf.lim_rows = buf64.lim_rows;
  buf.lim_offset = buf64.lim_offset;
  for(int i = 0; i < kMaxInputDim; i++)
  {
    buf.lim_lo[i] = buf64.lim_lo[i];
    buf.lim_hi[i] = buf64.lim_hi[i];
  }
  return buf;
}

/** More than 64 KB of dynamic LDS has to be requested per kernel and device: once per device ordinal for the kernels of one Owner
    (several host threads may launch at once; the setup is idempotent). */
template<class Owner>
inline hipError_t requestDynamicLds(std::initializer_list<const void *> kernels, size_t bytes)
{
  static std::atomic<bool> requested[64] = {};
  int dev = 0;
  if(hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
  {
    return hipErrorInvalidDevice;
  }
  if(!requested[dev].load(std::memory_order_acquire))
  {
    for(const void * fn : kernels)
    {
      const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
      if(e != hipSuccess)
      {
        return e;
      }
    }
    requested[dev].store(true, std::memory_order_release);
  }
  return hipSuccess;
}

template<class Problem>
struct ModelOpsFor
{
  using Scalar = typename Problem::Scalar;
  static constexpr bool kF64 = std::is_same<Scalar, double>::value;
  static_assert(kF64 || std::is_same<Scalar, float>::value, "a DDP problem computes in double or float");
  static constexpr int N = Problem::kStateDim, M = Problem::kInputDimMax;

  // ---- the kernel families this problem type has (fp64: lane, two-wave, quad, wave-per-instance, tile64; fp32: tile32, tile64) ----
  //! two-wave kernel: both record layouts (the box-constrained one is the larger: it carries the input limits) have to fit in LDS
  static constexpr bool kTwoWaveFits = [] {
    if constexpr(kF64)
    {
      return PairSolver<Problem, false>::kFits && PairSolver<Problem, true>::kFits;
    }
    return false;
  }();
  //! quad kernel (matrix-core backward pass, 16 instances per workgroup): n <= 4, one input
  static constexpr bool kQuadShape = [] {
    if constexpr(kF64)
    {
      return QuadSolver<Problem, false>::kShape;
    }
    return false;
  }();
  //! wave-per-instance (matrix-core) kernel: the shapes whose blocks fill a 16 x 16 tile
  static constexpr bool kWpiShape = kF64 && N >= 9 && N <= 16 && M >= 1 && M <= 16;
  //! box-constrained solves on the wave-per-instance kernel: register-path shapes only (static m <= 8)
  static constexpr bool kWpiBoxQP = kWpiShape && !Problem::kDynamicInput && M <= 8;
  /** Tile kernel (ddp_kernels_tile64.hpp: groups of up to 32 instances per workgroup, derivatives LDS-resident, backward pass on
      v_mfma_f64_16x16x4 in natural layout, BoxQP included): 5 <= n <= 15, m <= 16, static or inputDim(t).  Its float instantiation
      (v_mfma_f32_16x16x4, the lanes of a row holding the tile's columns in the order that makes the f32 instruction's result layout
      the f64 one): static m <= 8, unconstrained solves. */
  static constexpr bool kTile64Shape = N >= 5 && N <= 15 && M >= 1 && M <= 16 && (kF64 || (!Problem::kDynamicInput && M <= 8));
  //! m > 8 or inputDim(t) (the reference's centroidal-motion problem, 16 / 0): the gains are computed in natural layout across
  //! the wave (TileSolver64::stepGainsNatural, round 4); unconstrained solves only — their BoxQP stays on the lane kernel
  static constexpr bool kTile64Big = kF64 && kTile64Shape && (Problem::kDynamicInput || M > 8);
  static constexpr bool kTile64BoxQP = kF64 && kTile64Shape && !kTile64Big;
  //! the fp32 tile kernel (ddp_kernels_tile32.hpp: TileSolver32): n in {4, 8, 12}, static m <= 4, BoxQP included
  static constexpr bool kTile32Shape = !kF64 && (N == 4 || N == 8 || N == 12) && !Problem::kDynamicInput && M >= 1 && M <= 4;
  static_assert(kF64 || kTile32Shape || kTile64Shape, "an fp32 problem type needs the shape of the fp32 tile kernel (n in {4, 8, 12}, "
                                                      "m <= 4) or of the tile kernel's float instantiation (5 <= n <= 15, m <= 8)");

  // ---- the measured thresholds (plan() is their one user) ----
  /** Quad kernel: it wins while its workgroups fit on the chip in one round (one per CU: 16 * 256 instances); larger batches go to
      the 2-wave kernel, whose 64-instance workgroups keep the latency flat up to 16384 instances. */
  static constexpr int kQuadMaxBatch = 4096;
  //! Configuration::line_search_fan_out = 0 (automatic): solves with max_iter above this use the step-size-parallel search.
  //! -1 = always: since the lane groups fan out from the first pass on and an accepted rollout is adopted from the fan-out
  //! scratch (PairSolver::adoptFanOut), the parallel search is the faster one in the nominal regime too.
  //! NMPC_HIP_DDP_FAN_AUTO=<max_iter> overrides (A/B measurements).
  static constexpr int kQuadFanOutAutoMaxIter = -1;
  //! Below this batch the wave-per-instance kernel is still the (marginally) faster one where both exist (n >= 9).  Until round
  //! 4 the threshold was 1025: a group's sweep could not go faster than its model wave linearises ONE timestep per pass
  //! (33 k cycles for the manipulator, whatever the group size).  The model wave now linearises a CHUNK of timesteps per pass
  //! — as many (slot, timestep) pairs as its 64 lanes and the record area hold (backwardSweepModel) — and the two kernels
  //! are level up to 512 instances, the tile kernel ahead from there (scripts/tile64_chunk_ab.py,
  //! profiles/r04_tile64_chunk_ab.txt: manipulator 1.38 against 1.37 ms at 256, 1.41 / 1.42 at 512, 1.45 / 1.57 at 1024,
  //! 1.82 / 3.04 at 2048).
  //! Round 4, second half (the later step sizes ride along with the first, slot-major ring): ahead from 64 instances on
  //! (profiles/r04*_tile64_chunk_ab.txt: manipulator tile64 / wave-per-instance 1.07 at 16 instances, 0.96 at 64, 0.91 at 256,
  //! 0.31 at 8192; quadrotor 0.96 / 0.89 / 0.81 / 0.40).
  static constexpr int kTile64MinBatch = 64;
  //! box-constrained solves: round 3's threshold (the QP dominates their timestep; small batches have not been re-measured)
  static constexpr int kTile64MinBatchBoxQP = 1025;
  //! ... and for m > 4 (the QP grows with m^3; measured at 8192 instances only: profiles/r05_constrained_tile64_ab.txt)
  static constexpr int kTile64MinBatchBoxQPWide = 4096;
  //! Small models: the lane kernels keep a timestep's blocks in registers (n (n + m) <= 48 — planar VTOL: 70 - 80 scratch
  //! instructions; the quadrotor's 192 make 1500) and hold 64 instances per wavefront, several wavefronts per SIMD, so their
  //! time barely grows with the batch, while the tile kernel's (<= 35 instances per CU and round) grows linearly.  Measured
  //! (scripts/lane_vs_tile_ab.py, profiles/r05_lane_vs_tile_ab.txt; planar VTOL, T 60, 6 iterations; tile / lane ms):
  //! unconstrained 0.94 / 0.98 at 1024, 1.42 / 1.00 at 2048, 2.87 / 1.04 at 8192, 11.0 / 1.62 at 32768; box 3.78 / 4.81 at
  //! 4096, 6.04 / 4.74 at 8192, 23.2 / 5.75 at 32768.  Above these batches such shapes go back to the lane kernels.
  static constexpr bool kLaneKeepsUp = !Problem::kDynamicInput && N * (N + M) <= 48;
  static constexpr int kTile64MaxBatchSmall = 1024;
  static constexpr int kTile64MaxBatchSmallBoxQP = 6143;
  /** fp32, on the shapes both tile kernels take (unconstrained solves of n in {8, 12}, m <= 4; BoxQP in float is the fp32 tile
      kernel's only), measured on the quadrotor (profiles/r04_c4_dispatch_sweep.txt, scripts/c4_dispatch_sweep*.py):
        * the fp32 tile kernel is the leaner one per full sweep (16 MFMAs + 125 other instructions a step against 10 + 250), but a
          workgroup is 32 instances whatever the batch, its model wave linearises all 32 lanes of every timestep and its matrix
          waves step all their slots — a sweep costs the same however few instances still iterate, and batches below 8192 leave
          CUs idle (64 .. 4096 instances: 0.77 - 0.86 ms per 2 iterations);
        * the float instantiation of the tile kernel sizes its groups to the batch and deals a sweep's work by ACTIVE index: 1.3 -
          2.6 x faster up to 4096 instances at any iteration count and threshold; on full chips (8192, 16384 instances) level for
          one to four iterations and ahead from there (c4, max_iter 8: 1.95 k against 1.46 k it/s — the iteration counts of a batch
          are ragged, the late sweeps nearly empty) AS LONG AS most line searches end at the first or second step size (its search
          is passes over the horizon: the first two step sizes in one, the later ones in a second, the taken one in a third; the
          fp32 tile kernel rolls every step size out at once).  They do not once an fp32 solve iterates below the resolution of a
          float cost: 0.7 - 0.9 x at cost_update_thre = 1e-4 and below (the reference's default 1e-7: 0.6 x), level at 3e-4, 1.0 -
          1.3 x at 1e-3.
      Hence: the float instantiation below a full chip's batch (32 x the number of CUs: 8192 on MI355X, where the fp32 tile kernel's
      fixed 32-instance workgroups fill the chip), and on full chips with cost_update_thre >= 5e-4. */
  static constexpr double kTile64FloatFromThreshold = 5e-4;

  /** THE kernel choice: the family a solve of `batch` instances under `cfg` runs on, given the handle's knobs (a pinned family the
      problem type has; the batch the family is chosen for; whether the per-instance workspace exists; the CU count). */
  static Family family(const LaunchKnobs & knobs, int batch, const nmpc_hip_ddp_config & cfg)
  {
    const bool con = cfg.with_input_constraint != 0;
    const Family pin = knobs.pin;
    batch = knobs.batchFor(batch); // (a shard of a larger solve takes the family the WHOLE batch would get)
    if constexpr(!kF64)
    {
      if(!kTile32Shape || (kTile64Shape && !con && pin != Family::Tile32
                           && (pin == Family::Tile64 || batch < 32 * knobs.n_cu || cfg.cost_update_thre >= kTile64FloatFromThreshold)))
      {
        return Family::Tile64;
      }
      return Family::Tile32;
    }
    // fp64.  NMPC_HIP_DDP_KERNEL / nmpc_hip_ddp_set_kernel pins: 1w the single-wave lane kernel; 2w the two-wave kernel; quad the
    // quad kernel at any batch; wpi the wave-per-instance kernel over the tile kernel; tile64 the tile kernel at any batch (A/B).
    const int padded = (batch + kLanesPerBlock - 1) / kLanesPerBlock * kLanesPerBlock;
    if(kQuadShape && pin != Family::Lane && pin != Family::TwoWave && (padded <= kQuadMaxBatch || pin == Family::Quad))
    {
      return Family::Quad;
    }
    // (without the per-instance workspace — the allocation failed at create — the gain records and the candidate scratch have
    // nowhere to live: the lane kernels, which need none, take the solve)
    if(kTile64Shape && knobs.have_workspace != 0 && pin != Family::Lane && pin != Family::Wpi && !(pin == Family::TwoWave && kTwoWaveFits))
    {
      bool tile = true;
      if(kTile64Big)
      {
        tile = !con; // (every batch size: the wave-per-instance kernel takes these gains through LDS, 3 - 4 x slower)
      }
      else if(pin != Family::Tile64)
      {
        if(kLaneKeepsUp && batch > (con ? kTile64MaxBatchSmallBoxQP : kTile64MaxBatchSmall))
        {
          tile = false;
        }
        else if(kWpiShape && batch < (con ? kTile64MinBatchBoxQP : kTile64MinBatch))
        {
          tile = false;
        }
        // Box-constrained solves: every lane of a wave runs the BoxQP of its instance (boxQPMasked), a matrix wave of the tile
        // kernel one after the other for its up to five instances.  Measured (scripts/constrained_tile64_ab.py, 8192 instances, 4
        // iterations): quadrotor (m = 4) tile 7.2 ms against 11.1 ms on the wave-per-instance kernel, manipulator (m = 7) 23.7
        // against 17.1 — the QP grows with m^3 and the wave-per-instance kernel hides it behind more waves per SIMD.  So the tile
        // kernel takes the constrained solves up to m = 4 (and all of 5 <= n <= 8, where no other matrix-core kernel exists).
        // Round 5: the QPs of a matrix wave's five slots are solved together, lane = slot (TileSolver64::qpBatch) — manipulator box
        // 24.3 -> 12.2 ms (wave-per-instance kernel 15.1), quadrotor box 7.2 -> 4.8 (11.1): m > 4 goes to the tile kernel on full
        // chips too.
        else if(con && kWpiBoxQP && M > 4 && batch < kTile64MinBatchBoxQPWide)
        {
          tile = false;
        }
      }
      if(tile)
      {
        return Family::Tile64;
      }
    }
    if(kWpiShape && (!con || kWpiBoxQP) && knobs.have_workspace != 0 && pin != Family::Lane)
    {
      return Family::Wpi;
    }
    // lane mapping: the 2-wave (master + helper, LDS-staged) kernel whenever its records fit in LDS, else the single-wave kernel
    return (kTwoWaveFits && pin != Family::Lane) ? Family::TwoWave : Family::Lane;
  }
  static KernelPlan plan(const LaunchKnobs & knobs, int batch, const nmpc_hip_ddp_config & cfg, bool own_problems)
  {
    KernelPlan p;
    p.family = family(knobs, batch, cfg);
    p.constrained = cfg.with_input_constraint != 0;
    p.own_problems = own_problems;
    // step-size-parallel line search of the quad kernel's unconstrained solves: on request, or (0 = automatic) for long solves
    const int fan_auto = knobs.has_fan_auto ? knobs.fan_auto : kQuadFanOutAutoMaxIter;
    p.fan_out = p.family == Family::Quad && (cfg.line_search_fan_out == 1 || (cfg.line_search_fan_out == 0 && cfg.max_iter > fan_auto));
    // resumable launches (the ragged-convergence schedule, streamed solves): the quad kernel with the step-size-parallel line search
    // and the two-wave kernel, with one problem object for all instances or one per instance
    p.resumable = (p.family == Family::Quad && (p.constrained || p.fan_out)) || p.family == Family::TwoWave;
    return p;
  }
  static size_t workspaceElems(const LaunchKnobs & knobs, int T)
  {
    size_t n = 0;
    auto atLeast = [&n](size_t k) { n = k > n ? k : n; };
    if constexpr(kWpiShape)
    {
      atLeast(WaveSolver<Problem>::workspaceDoubles(T));
    }
    if constexpr(kTile64Shape)
    {
      atLeast(TileSolver64<Problem>::workspaceDoubles(T)); // (elements of Scalar: gain records + candidate trajectories)
    }
    if constexpr(kTile32Shape)
    {
      atLeast(TileSolver32<Problem>::workspaceElems(T));
    }
    if constexpr(kQuadShape)
    {
      // fan-out scratch of the quad kernel's line search (PairSolver::FanDest): three more candidate trajectories.
      // NMPC_HIP_DDP_FAN_SCRATCH=0: none (A/B measurements, tests of the path taken when the allocation fails)
      if(knobs.fan_scratch != 0)
      {
        atLeast(3 * (static_cast<size_t>(T + 1) * (N + 1) + static_cast<size_t>(T) * M));
      }
    }
    return n;
  }
  /** Launches exactly the instantiation of the plan (hipErrorNotSupported for a combination the family does not have). */
  static hipError_t launchSolve(const void * params,
                                const KernelPlan & plan,
                                const LaunchKnobs & knobs,
                                const nmpc_hip_ddp_config & cfg,
                                const DeviceBuffers & buf64,
                                hipStream_t stream)
  {
    if((plan.needsWorkspace() && buf64.wpi_ws == nullptr) || (buf64.iter_end > 0 && !plan.resumable))
    {
      return hipErrorNotSupported; // (the gain records live in the workspace; capi.hip asks plan.resumable first)
    }
    Problem problem;
    std::memcpy(static_cast<void *>(&problem), params, sizeof(Problem));
    DeviceBuffersT<Scalar> buf;
    if constexpr(kF64)
    {
      buf = buf64;
    }
    else
    {
      buf = floatView(buf64);
    }
    const bool con = plan.constrained, own = plan.own_problems;
    switch(plan.family)
    {
      case Family::Tile64:
        if constexpr(kTile64Shape)
        {
          if(con)
          {
            if constexpr(kTile64BoxQP)
            {
              return own ? launchTile64<Problem, true, true>(problem, cfg, buf, knobs, stream)
                         : launchTile64<Problem, true, false>(problem, cfg, buf, knobs, stream);
            }
            return hipErrorNotSupported;
          }
          return own ? launchTile64<Problem, false, true>(problem, cfg, buf, knobs, stream)
                     : launchTile64<Problem, false, false>(problem, cfg, buf, knobs, stream);
        }
        break;
      case Family::Tile32:
        if constexpr(kTile32Shape)
        {
          constexpr size_t lds = TileSolver32<Problem>::kLdsBytes;
          const hipError_t e = requestDynamicLds<TileSolver32<Problem>>(
              {reinterpret_cast<const void *>(&ddp_solve_tile32_kernel<Problem, false, false>),
               reinterpret_cast<const void *>(&ddp_solve_tile32_kernel<Problem, true, false>),
               reinterpret_cast<const void *>(&ddp_solve_tile32_kernel<Problem, false, true>),
               reinterpret_cast<const void *>(&ddp_solve_tile32_kernel<Problem, true, true>)},
              lds);
          if(e != hipSuccess)
          {
            return e;
          }
          const dim3 g((buf.B + kTileInstances - 1) / kTileInstances), blk(kTileThreads);
          if(own && con)
          {
            hipLaunchKernelGGL((ddp_solve_tile32_kernel<Problem, true, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else if(own)
          {
            hipLaunchKernelGGL((ddp_solve_tile32_kernel<Problem, true, false>), g, blk, lds, stream, problem, cfg, buf);
          }
          else if(con)
          {
            hipLaunchKernelGGL((ddp_solve_tile32_kernel<Problem, false, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else
          {
            hipLaunchKernelGGL((ddp_solve_tile32_kernel<Problem, false, false>), g, blk, lds, stream, problem, cfg, buf);
          }
          return hipGetLastError();
        }
        break;
      case Family::Wpi:
        if constexpr(kWpiShape)
        {
          constexpr size_t lds = WaveSolver<Problem, false>::kLdsBytes; // same layout with and without BoxQP
          const dim3 g(buf.B), blk(kLanesPerBlock);
          if(con)
          {
            if constexpr(kWpiBoxQP)
            {
              if(own)
              {
                hipLaunchKernelGGL((ddp_solve_wpi_kernel<Problem, true, true>), g, blk, lds, stream, problem, cfg, buf);
              }
              else
              {
                hipLaunchKernelGGL((ddp_solve_wpi_kernel<Problem, true, false>), g, blk, lds, stream, problem, cfg, buf);
              }
              return hipGetLastError();
            }
            return hipErrorNotSupported;
          }
          if(own)
          {
            hipLaunchKernelGGL((ddp_solve_wpi_kernel<Problem, false, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else
          {
            hipLaunchKernelGGL((ddp_solve_wpi_kernel<Problem, false, false>), g, blk, lds, stream, problem, cfg, buf);
          }
          return hipGetLastError();
        }
        break;
      case Family::Quad:
        if constexpr(kQuadShape)
        {
          constexpr size_t lds = QuadSolver<Problem, false>::kLdsBytes;
          const hipError_t e = requestDynamicLds<QuadSolver<Problem, false>>(
              {reinterpret_cast<const void *>(&ddp_solve_quad_kernel<Problem, false, false, true, true>),
               reinterpret_cast<const void *>(&ddp_solve_quad_kernel<Problem, true, false, true, true>),
               reinterpret_cast<const void *>(&ddp_solve_quad_kernel<Problem, false, true, true, true>),
               reinterpret_cast<const void *>(&ddp_solve_quad_kernel<Problem, true, true, true, true>),
               reinterpret_cast<const void *>(&ddp_solve_quad_kernel<Problem, false, false>),
               reinterpret_cast<const void *>(&ddp_solve_quad_kernel<Problem, true, false>),
               reinterpret_cast<const void *>(&ddp_solve_quad_kernel<Problem, false, true>),
               reinterpret_cast<const void *>(&ddp_solve_quad_kernel<Problem, true, true>),
               reinterpret_cast<const void *>(&ddp_solve_quad_kernel<Problem, false, false, true>),
               reinterpret_cast<const void *>(&ddp_solve_quad_kernel<Problem, false, true, true>)},
              lds);
          if(e != hipSuccess)
          {
            return e;
          }
          const dim3 g(buf.Bp / kQuadInstances), blk(kQuadWaves * 64);
          if(buf.iter_end > 0 && own && con) // (a resumable launch, plan.resumable: one problem object per instance ...)
          {
            hipLaunchKernelGGL((ddp_solve_quad_kernel<Problem, true, true, true, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else if(buf.iter_end > 0 && own)
          {
            hipLaunchKernelGGL((ddp_solve_quad_kernel<Problem, false, true, true, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else if(buf.iter_end > 0 && con) // (... or the shared one)
          {
            hipLaunchKernelGGL((ddp_solve_quad_kernel<Problem, true, false, true, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else if(buf.iter_end > 0)
          {
            hipLaunchKernelGGL((ddp_solve_quad_kernel<Problem, false, false, true, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else if(con && own)
          {
            hipLaunchKernelGGL((ddp_solve_quad_kernel<Problem, true, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else if(con)
          {
            hipLaunchKernelGGL((ddp_solve_quad_kernel<Problem, true, false>), g, blk, lds, stream, problem, cfg, buf);
          }
          else if(plan.fan_out && own)
          {
            hipLaunchKernelGGL((ddp_solve_quad_kernel<Problem, false, true, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else if(plan.fan_out)
          {
            hipLaunchKernelGGL((ddp_solve_quad_kernel<Problem, false, false, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else if(own)
          {
            hipLaunchKernelGGL((ddp_solve_quad_kernel<Problem, false, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else
          {
            hipLaunchKernelGGL((ddp_solve_quad_kernel<Problem, false, false>), g, blk, lds, stream, problem, cfg, buf);
          }
          return hipGetLastError();
        }
        break;
      case Family::TwoWave:
        if constexpr(kTwoWaveFits)
        {
          // the box-constrained record also carries the input limits (PairSolver::kBwdRec): LDS is sized per instantiation
          constexpr size_t lds = PairSolver<Problem, false>::kLdsBytes, lds_con = PairSolver<Problem, true>::kLdsBytes;
          static_assert(lds <= 64 * 1024 && lds_con <= 64 * 1024,
                        "kTwoWaveFits keeps the records of both layouts within the default dynamic LDS limit");
          const dim3 g(buf.Bp / kLanesPerBlock), blk(2 * kLanesPerBlock);
          if(buf.iter_end > 0 && own && con)
          {
            hipLaunchKernelGGL((ddp_solve_tpi2w_kernel<Problem, true, true, true>), g, blk, lds_con, stream, problem, cfg, buf);
          }
          else if(buf.iter_end > 0 && own)
          {
            hipLaunchKernelGGL((ddp_solve_tpi2w_kernel<Problem, false, true, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else if(buf.iter_end > 0 && con)
          {
            hipLaunchKernelGGL((ddp_solve_tpi2w_kernel<Problem, true, false, true>), g, blk, lds_con, stream, problem, cfg, buf);
          }
          else if(buf.iter_end > 0)
          {
            hipLaunchKernelGGL((ddp_solve_tpi2w_kernel<Problem, false, false, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else if(con && own)
          {
            hipLaunchKernelGGL((ddp_solve_tpi2w_kernel<Problem, true, true>), g, blk, lds_con, stream, problem, cfg, buf);
          }
          else if(con)
          {
            hipLaunchKernelGGL((ddp_solve_tpi2w_kernel<Problem, true, false>), g, blk, lds_con, stream, problem, cfg, buf);
          }
          else if(own)
          {
            hipLaunchKernelGGL((ddp_solve_tpi2w_kernel<Problem, false, true>), g, blk, lds, stream, problem, cfg, buf);
          }
          else
          {
            hipLaunchKernelGGL((ddp_solve_tpi2w_kernel<Problem, false, false>), g, blk, lds, stream, problem, cfg, buf);
          }
          return hipGetLastError();
        }
        break;
      case Family::Lane:
        if constexpr(kF64)
        {
          if(own)
          {
            return hipErrorNotSupported; // the single-wavefront kernel has no per-instance-problem instantiation
          }
          const dim3 g(buf.Bp / kLanesPerBlock), blk(kLanesPerBlock);
          if(con)
          {
            hipLaunchKernelGGL((ddp_solve_tpi_kernel<Problem, true>), g, blk, 0, stream, problem, cfg, buf);
          }
          else
          {
            hipLaunchKernelGGL((ddp_solve_tpi_kernel<Problem, false>), g, blk, 0, stream, problem, cfg, buf);
          }
          return hipGetLastError();
        }
        break;
      case Family::Auto:
        break;
    }
    return hipErrorNotSupported; // (a family this problem type does not have: plan() never picks one)
  }
  static hipError_t launchMpcAdvance(const void * params,
                                     const DeviceBuffers & buf64,
                                     const MpcAdvanceArgs & args,
                                     hipStream_t stream)
  {
    Problem problem;
    std::memcpy(static_cast<void *>(&problem), params, sizeof(Problem));
    if constexpr(kF64)
    {
      hipLaunchKernelGGL((mpc_advance_kernel<Problem>), dim3(buf64.Bp / kLanesPerBlock), dim3(kLanesPerBlock), 0, stream, problem, buf64,
                         args);
    }
    else
    {
      const DeviceBuffersT<float> buf = floatView(buf64);
      hipLaunchKernelGGL((mpc_advance_kernel<Problem>), dim3(buf.Bp / kLanesPerBlock), dim3(kLanesPerBlock), 0, stream, problem, buf, args);
    }
    return hipGetLastError();
  }
  static void defaultParams(void * out)
  {
    new(out) Problem();
  }
  static void inputDims(const void * params, double t0, int T, int * out)
  {
    Problem problem;
    std::memcpy(static_cast<void *>(&problem), params, sizeof(Problem));
    for(int i = 0; i < T; i++)
    {
      if constexpr(Problem::kDynamicInput)
      {
        out[i] = problem.inputDim(t0 + i * problem.dt());
      }
      else
      {
        out[i] = M;
      }
    }
  }
  static double dt(const void * params)
  {
    Problem problem;
    std::memcpy(static_cast<void *>(&problem), params, sizeof(Problem));
    return static_cast<double>(problem.dt());
  }
  static ModelOps make()
  {
    static_assert(std::is_trivially_copyable<Problem>::value,
                  "a DDP problem must be trivially copyable (no std::function / heap members): it is passed to "
                  "the GPU by value");
    static_assert(std::is_default_constructible<Problem>::value, "a DDP problem must be default constructible");
    ModelOps ops;
    ops.name = Problem::kName;
    ops.state_dim = N;
    ops.input_dim_max = M;
    ops.dynamic_input = Problem::kDynamicInput ? 1 : 0;
    ops.param_bytes = sizeof(Problem);
    ops.default_params = &defaultParams;
    ops.plan = &plan;
    ops.launch_solve = &launchSolve;
    ops.input_dims = &inputDims;
    ops.dt = &dt;
    ops.launch_mpc_advance = &launchMpcAdvance;
    ops.has_plant_step = HasPlantStep<Problem>::value ? 1 : 0;
    ops.wpi_workspace_doubles = &workspaceElems;
    ops.scalar_bytes = static_cast<int>(sizeof(Scalar));
    return ops;
  }
};
} // namespace hip
} // namespace nmpc_amd

#define NMPC_AMD_REGISTER_PROBLEM(ProblemType) NMPC_AMD_REGISTER_PROBLEM_WITH(ProblemType, nmpc_amd::hip::ModelOpsFor<ProblemType>)
//! the names INTEGRATION.md published for fp32 problem types (NMPC_AMD_REGISTER_PROBLEM serves them)
#define NMPC_AMD_REGISTER_PROBLEM_TILE32(ProblemType) NMPC_AMD_REGISTER_PROBLEM(ProblemType)
#define NMPC_AMD_REGISTER_PROBLEM_TILE64_FLOAT(ProblemType) NMPC_AMD_REGISTER_PROBLEM(ProblemType)
