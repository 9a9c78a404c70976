// The BoxQP probe problems (boxqp_probe.hpp) compiled for gfx950 into a TEST library, libnmpc_test_models.so
// (nmpc_amd/build.py: build_test_models).  It registers nothing itself: it exports the operations tables, and the test hands each
// one to nmpc_hip_ddp_register_model of whichever DDP library it has loaded (tests/test_gpu_boxqp_known_answers.py).  Each shape is
// chosen to reach particular BoxQP code: the run-time m boxQP of the lane / two-wave kernels, boxQPMasked of the wave-per-instance
// and tile kernels (qpBatch on the tile kernel), the quad kernel's constrained variant and the fp32 tile kernel's float boxQP.
//
// One translation unit per probe so that they compile in parallel: -DNMPC_TEST_PROBE=<i> instantiates probe i's kernels and exports
// nmpc_test_probe_ops_<i> / nmpc_test_probe_two_wave_fits_<i>; without it the file is the index the test calls.
#define NMPC_TEST_PROBE_COUNT 5

#ifdef NMPC_TEST_PROBE
#  include <nmpc_amd/hip/model_registry.hpp>

#  include "boxqp_probe.hpp"

#  define NMPC_TEST_CAT2(a, b) a##b
#  define NMPC_TEST_CAT(a, b) NMPC_TEST_CAT2(a, b)

namespace
{
using nmpc_amd::Dynamic;
using nmpc_amd::test::BoxQPProbe;

#  if NMPC_TEST_PROBE == 0
struct Probe : BoxQPProbe<double, 4, 2>
{
  static constexpr const char * kName = "boxqp_probe_d4m2";
};
#  elif NMPC_TEST_PROBE == 1
struct Probe : BoxQPProbe<double, 4, 1>
{
  static constexpr const char * kName = "boxqp_probe_d4m1";
};
#  elif NMPC_TEST_PROBE == 2
struct Probe : BoxQPProbe<double, 9, 2>
{
  static constexpr const char * kName = "boxqp_probe_d9m2";
};
#  elif NMPC_TEST_PROBE == 3
struct Probe : BoxQPProbe<double, 9, Dynamic, 16>
{
  static constexpr const char * kName = "boxqp_probe_d9dyn16";
};
#  elif NMPC_TEST_PROBE == 4
struct Probe : BoxQPProbe<float, 4, 2>
{
  static constexpr const char * kName = "boxqp_probe_f4m2";
};
#  else
#    error "NMPC_TEST_PROBE out of range"
#  endif
} // namespace

extern "C"
{
  const void * NMPC_TEST_CAT(nmpc_test_probe_ops_, NMPC_TEST_PROBE)(void)
  {
    static const nmpc_amd::hip::ModelOps ops = nmpc_amd::hip::ModelOpsFor<Probe>::make();
    return &ops;
  }
  int NMPC_TEST_CAT(nmpc_test_probe_two_wave_fits_, NMPC_TEST_PROBE)(void)
  {
    return nmpc_amd::hip::ModelOpsFor<Probe>::kTwoWaveFits ? 1 : 0;
  }
}

#else // the index

extern "C"
{
  const void * nmpc_test_probe_ops_0(void);
  const void * nmpc_test_probe_ops_1(void);
  const void * nmpc_test_probe_ops_2(void);
  const void * nmpc_test_probe_ops_3(void);
  const void * nmpc_test_probe_ops_4(void);
  int nmpc_test_probe_two_wave_fits_0(void);
  int nmpc_test_probe_two_wave_fits_1(void);
  int nmpc_test_probe_two_wave_fits_2(void);
  int nmpc_test_probe_two_wave_fits_3(void);
  int nmpc_test_probe_two_wave_fits_4(void);

  int nmpc_test_model_count(void)
  {
    return NMPC_TEST_PROBE_COUNT;
  }
  //! the operations table of probe i (NULL out of range): pass it to nmpc_hip_ddp_register_model
  const void * nmpc_test_model_ops(int i)
  {
    const void * (*const ops[NMPC_TEST_PROBE_COUNT])(void) = {&nmpc_test_probe_ops_0, &nmpc_test_probe_ops_1, &nmpc_test_probe_ops_2,
                                                              &nmpc_test_probe_ops_3, &nmpc_test_probe_ops_4};
    return (i >= 0 && i < NMPC_TEST_PROBE_COUNT) ? ops[i]() : nullptr;
  }
  //! ModelOpsFor<probe i>::kTwoWaveFits: whether the two-wave kernel exists for its shape (-1 out of range)
  int nmpc_test_model_two_wave_fits(int i)
  {
    int (*const fits[NMPC_TEST_PROBE_COUNT])(void) = {&nmpc_test_probe_two_wave_fits_0, &nmpc_test_probe_two_wave_fits_1,
                                                      &nmpc_test_probe_two_wave_fits_2, &nmpc_test_probe_two_wave_fits_3,
                                                      &nmpc_test_probe_two_wave_fits_4};
    return (i >= 0 && i < NMPC_TEST_PROBE_COUNT) ? fits[i]() : -1;
  }
}
#endif
