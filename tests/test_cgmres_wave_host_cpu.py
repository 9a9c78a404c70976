"""The wave kernel family of the C/GMRES solver (one wavefront per controller, include/nmpc_amd/hip/cgmres_wave_kernels.hpp): what can
be checked without a GPU — the three new entry points, the LDS budget function, the mirrors."""
import os
import re
import subprocess

import pytest

from nmpc_amd import _capi, cgmres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("cgmres_semiactive_damper", "cgmres_cartpole", "cgmres_cartpole_with_input_bound")
NEW = ("nmpc_hip_cgmres_set_kernel", "nmpc_hip_cgmres_kernel_name", "nmpc_hip_cgmres_wave_lds_bytes")


def test_new_entry_points_are_declared_exported_and_listed():
    text = open(os.path.join(ROOT, "include", "nmpc_hip_cgmres.h")).read()
    declared = set(re.findall(r"\b(nmpc_hip_cgmres_\w+)\s*\(", text))
    L = cgmres.load()
    for name in NEW:
        assert name in declared and name in cgmres.EXPORTS
        getattr(L, name)
    getattr(L, "nmpc_hip_cgmres_register_wave_model")  # the registration hook of NMPC_AMD_REGISTER_CGMRES_WAVE_PROBLEM


def test_wave_lds_bytes():
    """The formula of the header: 8 (4 n + 3 ((2 N + 1) dim_x + N) + (K + 3) n + K K + 3 K + 1), n = N dim_uc."""
    dims = {"cgmres_semiactive_damper": (2, 3), "cgmres_cartpole": (4, 1), "cgmres_cartpole_with_input_bound": (4, 3)}
    for m in MODELS:
        nx, nuc = dims[m]
        for N, K in ((25, 5), (25, 16)):
            got = cgmres.wave_lds_bytes(m, N, K)
            n = N * nuc
            assert got == 8 * (4 * n + 3 * ((2 * N + 1) * nx + N) + (K + 3) * n + K * K + 3 * K + 1)
            assert 0 < got <= 65536
        for K in (1, 5, 16):
            sizes = [cgmres.wave_lds_bytes(m, N, K) for N in (1, 2, 3, 25, 26, 100, 400)]
            assert sizes == sorted(sizes)
        for N in (1, 25, 400):
            sizes = [cgmres.wave_lds_bytes(m, N, K) for K in range(1, 17)]
            assert sizes == sorted(sizes)
    assert cgmres.wave_lds_bytes("cgmres_cartpole_with_input_bound", 400, 16) > 65536
    # the shapes of the refusal tests on the GPU: N = 100 fits at k_max = 5 and not at 16
    assert cgmres.wave_lds_bytes("cgmres_cartpole_with_input_bound", 100, 5) <= 65536 < cgmres.wave_lds_bytes(
        "cgmres_cartpole_with_input_bound", 100, 16)
    with pytest.raises(ValueError):
        cgmres.wave_lds_bytes("no_such_problem", 25, 5)
    for N, K in ((0, 5), (25, 0), (25, 17)):
        with pytest.raises(ValueError):
            cgmres.wave_lds_bytes("cgmres_cartpole", N, K)


def test_python_mirror_has_the_kernel_choice():
    assert callable(cgmres.CgmresSolverBatch.setKernel) and callable(cgmres.CgmresSolverBatch.kernelName)
    assert callable(cgmres.wave_lds_bytes)


def mirror_exe(directory):
    """tests/cpp/cgmres_wave_mirror.cpp against the C++ mirror, g++ only."""
    libdir = os.path.dirname(_capi.lib_path())
    cgmres.load()
    exe = os.path.join(str(directory), "cgmres_wave_mirror")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT}/include", os.path.join(ROOT, "tests", "cpp", "cgmres_wave_mirror.cpp"),
           f"-L{libdir}", "-lnmpc_hip_ddp", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_cpp_mirror_compiles(tmp_path):
    assert os.path.exists(mirror_exe(tmp_path))
