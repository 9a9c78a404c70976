"""Batched BoxQP solver: what can be checked without a GPU — the C-ABI's exports, the reference's defaults, the mirrors' constants
against the header, argument validation ahead of the device probe, a host-only compile of the C++ mirror, and the case set of
tests/boxqp_cases.py itself: that it holds the exits, line searches and refactorisations the GPU tests rely on, and that every
decision of oracle.ddp_numpy.boxqp on it is stable under 1e-13 relative perturbations (so the GPU tests compare them on all cases)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import boxqp_cases as bc
from nmpc_amd import _capi, boxqp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nmpc_hip_boxqp.h")


def test_every_declared_entry_point_is_exported():
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(nmpc_hip_boxqp_\w+)\s*\(", text))
    assert declared == set(boxqp.EXPORTS)
    L = boxqp.load()
    for name in declared:
        getattr(L, name)


def test_nothing_is_declared_in_the_ddp_header():
    assert "nmpc_hip_boxqp" not in open(os.path.join(ROOT, "include", "nmpc_hip_ddp.h")).read()


def test_default_config_is_the_references():
    c = boxqp.default_config()
    assert (c.max_iter, c.grad_thre, c.rel_improve_thre, c.step_factor, c.min_step, c.armijo_param) == (500, 1e-8, 1e-8, 0.6, 1e-22, 0.1)
    assert c.trace_capacity == 0
    # the struct of the header, field for field
    body = re.search(r"typedef struct\s*\{(.*?)\}\s*nmpc_hip_boxqp_config;", open(HEADER).read(), re.S).group(1)
    fields = re.findall(r"^\s*(int|double)\s+(\w+);", body, re.M)
    assert [(n, {"int": C.c_int, "double": C.c_double}[t]) for t, n in fields] == boxqp.CConfig._fields_


def test_mirror_constants_are_the_headers():
    text = open(HEADER).read()
    fields = dict(re.findall(r"NMPC_HIP_BOXQP_FIELD_(\w+) = (\d+)", text))
    assert {k: int(v) for k, v in fields.items()} == {
        "X": boxqp.FIELD_X, "RETVAL": boxqp.FIELD_RETVAL, "ITER": boxqp.FIELD_ITER, "FACTORIZATION_NUM": boxqp.FIELD_FACTORIZATION_NUM,
        "FREE_MASK": boxqp.FIELD_FREE_MASK, "OBJ": boxqp.FIELD_OBJ, "FACTOR": boxqp.FIELD_FACTOR, "TRACE": boxqp.FIELD_TRACE}
    rets = {int(v): s for v, s in re.findall(r"NMPC_HIP_BOXQP_RET_\w+ = (-?\d+),? /\* \"(.*?)\" \*/", text)}
    assert rets == boxqp.RETSTR and sorted(rets) == list(range(-2, 7))
    defines = dict(re.findall(r"#define NMPC_HIP_BOXQP_(\w+) (\d+)", text))
    assert int(defines["MAX_DIM"]) == boxqp.MAX_DIM == 64 and int(defines["LANE_MAX_DIM"]) == boxqp.LANE_MAX_DIM == 16
    assert int(defines["TRACE_COLUMNS"]) == len(boxqp.TRACE_COLUMNS) == 6 and boxqp.TRACE_DTYPE.itemsize == 48
    assert (int(defines["AUTO_LANE_MAX_DIM"]), int(defines["AUTO_LANE_MIN_BATCH"])) == (boxqp.AUTO_LANE_MAX_DIM, boxqp.AUTO_LANE_MIN_BATCH)
    assert boxqp.AUTO_LANE_MAX_DIM <= boxqp.LANE_MAX_DIM
    # the C++ mirror's strings
    mirror = open(os.path.join(ROOT, "include", "nmpc_amd", "BoxQPBatch.hpp")).read()
    assert {int(v): s for v, s in re.findall(r"\{(-?\d+), \"(.*?)\"\}", mirror)} == boxqp.RETSTR


@pytest.mark.parametrize("var_dim,batch", [(0, 4), (65, 4), (-1, 4), (8, 0), (8, -3)])
def test_create_validates_before_it_probes_the_device(var_dim, batch):
    L = boxqp.load()
    h = C.c_void_p()
    assert L.nmpc_hip_boxqp_create(var_dim, batch, 0, C.byref(h)) == _capi.ERR_INVALID_ARGUMENT
    assert not h.value and L.nmpc_hip_boxqp_last_error()
    with pytest.raises(ValueError):
        boxqp.BoxQPBatch(var_dim, batch)


def test_create_needs_a_device_or_gives_a_handle():
    L = boxqp.load()
    h = C.c_void_p()
    rc = L.nmpc_hip_boxqp_create(8, 4, 0, C.byref(h))
    assert rc in (_capi.OK, _capi.ERR_NO_DEVICE)
    if rc == _capi.OK:
        assert L.nmpc_hip_boxqp_destroy(h) == _capi.OK
    else:
        assert b"no CPU fallback" in L.nmpc_hip_boxqp_last_error()
    assert L.nmpc_hip_boxqp_create(8, 4, 0, None) == _capi.ERR_INVALID_ARGUMENT
    assert L.nmpc_hip_boxqp_default_config(None) == _capi.ERR_INVALID_ARGUMENT


def test_cpp_mirror_compiles_with_a_host_compiler_alone(tmp_path):
    """tests/cpp/boxqp_mirror.cpp against BoxQPBatch.hpp (fixed and nmpc_amd::Dynamic var_dim): g++, no HIP headers.  Run, it either
    solves the known answers (a device is there) or reports the library's no-device error as std::runtime_error."""
    boxqp.load()
    libdir = os.path.dirname(_capi.lib_path())
    exe = str(tmp_path / "boxqp_mirror")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT}/include", os.path.join(ROOT, "tests", "cpp", "boxqp_mirror.cpp"),
           f"-L{libdir}", "-lnmpc_hip_ddp", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    last = r.stdout.splitlines()[-1]
    assert last == "ok boxqp_lane_kernel boxqp_wave_kernel" or (last.startswith("runtime_error: no HIP device available") and "qp 0" not in r.stdout), last


# ---- the case set ----------------------------------------------------------------------------------------------------------
def test_case_generator_is_the_known_answer_files_body():
    """The first case of size 8 drawn here equals the first case random_cases(rng, n, 8, 8, ...) of
    tests/test_gpu_boxqp_known_answers.py draws from the same generator state (its coupling matrix C is not part of a bare QP and is
    not drawn here, so only the first case can be compared)."""
    import test_gpu_boxqp_known_answers as ka
    H, g, _, lo, up, kind = ka.random_cases(np.random.default_rng(108), 3, 8, 8, 1)[0]
    cs = bc.cases(8)
    assert kind == cs.kind[0] == 0
    assert np.array_equal(H, cs.H[0]) and np.array_equal(g, cs.g[0]) and np.array_equal(lo, cs.lower[0]) and np.array_equal(up, cs.upper[0])
    assert [int(k) for k in cs.kind[:7]] == [0, 1, 2, 3, 4, 0, 1] and cs.H.shape == (70, 8, 8) and cs.x0.shape == (70, 8)


@pytest.mark.parametrize("n", bc.SIZES)
def test_case_set_holds_what_the_gpu_tests_rely_on(n):
    cs, o = bc.cases(n), bc.oracle(n)
    assert set(o.retval.tolist()) == {5, 6}
    assert (o.retval[cs.kind == 0] == 6).all() and (o.free_mask[cs.kind == 0] == 0).all()
    outside = ((cs.x0 < cs.lower) | (cs.x0 > cs.upper)).any(axis=1)
    assert outside.sum() >= 35
    backtrack = refactorise = 0
    for b in range(bc.COUNT):
        rows, ret, it = bc.replay(cs.H[b], cs.g[b], cs.lower[b], cs.upper[b], cs.x0[b])
        assert (ret, it) == (o.retval[b], o.iters[b])
        backtrack += any(r[3] > 0 for r in rows)
        refactorise += bool(rows) and rows[-1][1] > 1
    assert 14 <= backtrack <= 30 and refactorise <= 56
    assert refactorise > 0 or n == 1
    # the twins: improvement-based exits (retval 4) at every size, at n >= 16 for every case that is not all clamped
    t = bc.oracle(n, scaled=True)
    assert (t.retval == 4).any() and np.array_equal(t.retval == 6, o.retval == 6) and set(t.retval.tolist()) <= {4, 5, 6}
    assert np.array_equal(t.free_mask, o.free_mask)
    if n >= 16:
        assert (t.retval[o.retval != 6] == 4).all()


def test_iteration_counts_reach_eight():
    assert max(int(bc.oracle(n).iters.max()) for n in bc.SIZES) >= 8


@pytest.mark.parametrize("n", bc.SIZES)
def test_every_decision_is_stable_under_perturbation(n):
    """H and g perturbed by 1e-13 relative, four seeds: no case changes retval, iteration count or free set, and x moves by less than
    1e-10 relative (measured: 9e-12) — two orders inside the GPU tests' 1e-9 bar, which therefore fits a reordered sum."""
    cs, o = bc.cases(n), bc.oracle(n)
    worst = 0.0
    for seed in range(4):
        rng = np.random.default_rng(1000 + seed)
        E = rng.uniform(-1, 1, cs.H.shape)
        E = (E + E.transpose(0, 2, 1)) / 2
        p = bc.Cases(cs.H * (1 + 1e-13 * E), cs.g * (1 + 1e-13 * rng.uniform(-1, 1, cs.g.shape)), cs.lower, cs.upper, cs.x0, cs.kind)
        r = bc.solve_oracle(p)
        assert np.array_equal(r.retval, o.retval) and np.array_equal(r.iters, o.iters) and np.array_equal(r.free_mask, o.free_mask)
        worst = max(worst, float((np.abs(r.x - o.x).max(axis=1) / (1 + np.abs(o.x).max(axis=1))).max()))
    assert worst < 1e-10, worst
