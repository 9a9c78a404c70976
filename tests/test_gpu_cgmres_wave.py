"""The wave kernels of the batched C/GMRES solver (one wavefront per controller, the tick in LDS) against the lane kernels in the
same process.  The contract is equality of bits, not a tolerance: both translation units are compiled without FMA contraction, the
wave kernel calls the lane kernel's own device functions for the model steps and keeps the element order of every sum
(include/nmpc_amd/hip/cgmres_wave_kernels.hpp), so every comparison here is np.array_equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cgmres_checker
from nmpc_amd import _capi, cgmres
from test_cgmres_wave_host_cpu import mirror_exe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("cgmres_semiactive_damper", "cgmres_cartpole", "cgmres_cartpole_with_input_bound")
BOUNDED = "cgmres_cartpole_with_input_bound"
B = 67  # more than one wavefront of the lane kernel, no multiple of 64
SEED = 11
# (horizon_divide_num, k_max, horizon ODE): n = 75 > 64 lanes for dim_uc = 3 at N = 25; ragged iteration counts at k_max = 16; k_max = 1;
# N = 3 and N = 1 (k_max clamped to n, the re-orthogonalisation fires); RK4 inside the horizon
CASES = ((25, 5, "euler"), (25, 16, "euler"), (25, 1, "euler"), (3, 5, "euler"), (1, 5, "euler"), (22, 5, "rk4"))
FIELDS = ("log_x", "log_u", "log_err", "log_iters", "log_reorth", "log_t", "x_", "u_", "u_list_", "delta_u_vec_", "status", "err")


def perturbed(model, batch, seed, scale=0.1):
    """As perturbed() of tests/test_gpu_cgmres.py."""
    rng = np.random.default_rng(seed)
    x0, u0 = cgmres_checker.initial(model)
    return np.array(x0) + scale * rng.standard_normal((batch, len(x0))), np.tile(u0, (batch, 1))


def make(model, batch, N=25, ode="euler", kernel="lane", problems=None):
    s = cgmres.CgmresSolverBatch(problems if problems is not None else cgmres.CgmresProblem(model), batch, horizon_divide_num=N,
                                 ode_solver=ode, sim_ode_solver="rk4")
    s.setKernel(kernel)
    return s


def fields(s):
    out = {}
    for f in FIELDS:
        v = getattr(s, f)
        out[f] = v() if callable(v) else v
    return out


def closed_loop(model, kernel, N, k_max, ode, batch=B, x0u0=None, problems=None, sim_duration=0.2):
    s = make(model, batch, N, ode, kernel, problems)
    s.k_max_ = k_max
    s.sim_duration_ = sim_duration
    s.dump_step_ = 1
    x0, u0 = x0u0 if x0u0 is not None else perturbed(model, batch, SEED)
    s.setInitial(x0, u0)
    s.run()
    assert s.kernelName() == ("cgmres_wave_run_kernel" if kernel == "wave" else "cgmres_run_kernel")
    return fields(s)


def assert_same(lane, wave):
    for f in FIELDS:
        assert lane[f].shape == wave[f].shape, f
        assert np.array_equal(lane[f], wave[f], equal_nan=lane[f].dtype.kind == "f"), (
            f, int((lane[f] != wave[f]).sum()), np.argwhere(lane[f] != wave[f])[:3].tolist())


@pytest.mark.parametrize("N,k_max,ode", CASES)
@pytest.mark.parametrize("model", MODELS)
def test_closed_loop_equals_the_lane_kernel(model, N, k_max, ode):
    """200 ticks, 67 perturbed starts (seed 11), every tick logged: every log and every state of the handle bit for bit.  (NaN rows of
    an instance that stopped compare equal: both kernels leave the fill value there.)  The coverage facts are asserted on the LANE
    result, so that the comparison is known to have gone through the branch it is here for."""
    lane = closed_loop(model, "lane", N, k_max, ode)
    assert lane["log_t"].shape == (200,)
    it = lane["log_iters"][lane["log_iters"] >= 0]
    print(model, (N, k_max, ode), "iterations", np.unique(it).tolist(), "reorth ticks", int((lane["log_reorth"] == 1).sum()), "of",
          lane["log_reorth"].size, "status", np.unique(lane["status"]).tolist())
    if N == 1:
        assert (lane["log_reorth"] == 1).any()  # the re-orthogonalisation branch
    if k_max == 16:
        assert len(np.unique(it)) > 1  # ragged iteration counts
    if model == "cgmres_semiactive_damper" and (N, k_max) == (25, 1):
        st = set(np.unique(lane["status"]).tolist())
        assert cgmres.Status.Succeeded in st and cgmres.Status.NonFinite in st  # stopped controllers beside running ones
    wave = closed_loop(model, "wave", N, k_max, ode)
    assert_same(lane, wave)


def test_switching_kernels_between_ticks():
    """setup(), then 60 calcControlInput ticks fed with a lane run()'s logged states, the kernel alternating lane / wave every tick:
    the inputs and the final u_list_ / delta_u_vec_ are those of the all-lane sequence.  Once from host arrays, once from device
    tensors (where the odd ticks go through the wave kernel's device path)."""
    import torch
    x0, u0 = perturbed(BOUNDED, B, SEED)
    r = make(BOUNDED, B)
    r.sim_duration_ = 0.0595
    r.dump_step_ = 1
    r.setInitial(x0, u0)
    r.run()
    lx, ts = r.log_x(), r.log_t()
    assert len(ts) == 60

    def ticks(kernel_of_tick, device_path):
        c = make(BOUNDED, B)
        c.setInitial(x0, u0)
        c.setup()
        x, us = x0, []
        for i, t in enumerate(ts):
            c.setKernel(kernel_of_tick(i))
            if device_path:
                dev = torch.device("cuda:0")
                tt = torch.full((B,), float(t), dtype=torch.float64, device=dev)
                u_t = torch.zeros((B, c.problem_.dim_uc_), dtype=torch.float64, device=dev)
                c.calcControlInputDevice(tt, torch.from_numpy(np.ascontiguousarray(x)).to(dev),
                                         torch.from_numpy(np.ascontiguousarray(lx[:, i])).to(dev), u_t)
                c.synchronize()
                us.append(u_t.cpu().numpy())
            else:
                us.append(c.calcControlInput(t, x, lx[:, i]))
            x = lx[:, i]
        return np.array(us), c.u_list_, c.delta_u_vec_, c.u_, c.err(), c.status()

    want = ticks(lambda i: "lane", False)
    assert np.array_equal(want[0], np.moveaxis(r.log_u(), 1, 0))  # (the lane sequence is run()'s, as test_gpu_cgmres.py shows)
    for device_path in (False, True):
        got = ticks(lambda i: "wave" if i % 2 else "lane", device_path)
        for a, b in zip(want, got):
            assert np.array_equal(a, b), device_path
    all_wave = ticks(lambda i: "wave", True)
    for a, b in zip(want, all_wave):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("model", MODELS)
def test_per_instance_problem_objects(model):
    """One problem object per instance (the cart-poles: per-instance reference states, as test_model_eval_matches_the_checker sets
    them; the damper: per-instance weights): wave equals lane at B = 67, and instance 37 alone at B = 1 gives its bits of the batch."""
    def problems(idx):
        out = []
        for i in idx:
            p = cgmres.CgmresProblem(model)
            if model == "cgmres_semiactive_damper":
                p.p[3] *= 1 + 0.05 * (i % 4)
            else:
                p.p[14:18] = 0.1 * (i % 4)
            out.append(p)
        return out

    x0, u0 = perturbed(model, B, SEED)
    lane = closed_loop(model, "lane", 25, 5, "euler", problems=problems(range(B)), sim_duration=0.05)
    wave = closed_loop(model, "wave", 25, 5, "euler", problems=problems(range(B)), sim_duration=0.05)
    assert_same(lane, wave)
    shared = closed_loop(model, "lane", 25, 5, "euler", sim_duration=0.05)
    assert not np.array_equal(shared["log_u"][37], lane["log_u"][37])  # the per-instance object is in use
    one = closed_loop(model, "wave", 25, 5, "euler", batch=1, x0u0=(x0[37:38], u0[37:38]), problems=problems([37]), sim_duration=0.05)
    for f in FIELDS:
        if f != "log_t":
            assert np.array_equal(one[f][0], lane[f][37], equal_nan=True), f


def handle_k_max(s):
    cfg = cgmres.CConfig()
    cgmres.check(cgmres.load().nmpc_hip_cgmres_get_config(s._h, C.byref(cfg)))
    return cfg.k_max


def test_refusals():
    """The LDS budget (64 KiB per workgroup) and unknown names.  N = 400 does not fit at any k_max (the GMRES basis alone is
    (k_max + 3) * 1200 doubles), so the refusal of a k_max raised AFTER setKernel("wave") is shown on N = 100, which fits at k_max = 5
    (50 824 B) and not at 16 (79 336 B)."""
    s = cgmres.CgmresSolverBatch(cgmres.CgmresProblem(BOUNDED), 4, horizon_divide_num=400)
    assert s.kernelName() == "cgmres_run_kernel"
    s.k_max_ = 16
    with pytest.raises(ValueError, match=str(cgmres.wave_lds_bytes(BOUNDED, 400, 16))):
        s.setKernel("wave")
    assert s.kernelName() == "cgmres_run_kernel"
    with pytest.raises(ValueError):
        s.setKernel("nope")
    assert s.kernelName() == "cgmres_run_kernel"
    L = cgmres.load()
    assert L.nmpc_hip_cgmres_set_kernel(s._h, None) == _capi.ERR_INVALID_ARGUMENT

    s = cgmres.CgmresSolverBatch(cgmres.CgmresProblem(BOUNDED), 4, horizon_divide_num=100)
    s.setKernel("wave")
    assert s.kernelName() == "cgmres_wave_run_kernel" and handle_k_max(s) == 5
    s.k_max_ = 16
    with pytest.raises(ValueError, match=str(cgmres.wave_lds_bytes(BOUNDED, 100, 16))):
        s.setup()
    assert handle_k_max(s) == 5 and s.kernelName() == "cgmres_wave_run_kernel"
    s.setKernel("lane")  # (pushes k_max = 16, which the lane kernel takes)
    assert s.kernelName() == "cgmres_run_kernel" and handle_k_max(s) == 16
    with pytest.raises(ValueError):
        s.setKernel("wave")
    s.k_max_ = 5
    s.setKernel("wave")
    s.sim_duration_ = 0.003
    s.run()
    assert (s.status() == cgmres.Status.Succeeded).all()


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return cgmres_checker.build(tmp_path_factory.mktemp("cgmres_checker"))


@pytest.mark.parametrize("model", MODELS)
def test_closed_loop_matches_the_checker(checker, model):
    """The comparison of test_one_second_closed_loop_matches_the_checker (tests/test_gpu_cgmres.py) at its bars, with the wave kernel,
    64 instances and 0.3 s: a cross-check against the CPU restatement that does not go through the lane kernel."""
    batch = 64
    s = make(model, batch, kernel="wave")
    s.sim_duration_ = 0.3
    s.dump_step_ = 1
    x0, u0 = perturbed(model, batch, 2)
    s.setInitial(x0, u0)
    s.run()
    cfg = {n: getattr(s.config(), n) for n, _ in cgmres.CConfig._fields_}
    r = checker.solve(model, cfg, x0, u0)
    assert r.n_ticks == len(s.log_t())
    assert np.array_equal(s.status(), r.status)
    damper = model == "cgmres_semiactive_damper"
    for got, want, bar in ((s.log_x(), r.log_x, 1e-8 if damper else 1e-9), (s.log_u(), r.log_u, 1e-5 if damper else 1e-9)):
        assert np.isfinite(want).all()
        assert (np.abs(got - want) / (1 + np.abs(want))).max() <= bar
    assert (s.log_iters() == r.log_iters).mean() >= 0.999
    assert (s.log_reorth() == r.log_reorth).mean() >= 0.999
    assert (np.abs(s.log_err() - r.log_err) / (1 + np.abs(r.log_err))).max() <= (1e-5 if damper else 1e-7)


def test_cpp_mirror_program_runs(tmp_path):
    """tests/cpp/cgmres_wave_mirror.cpp: setKernel / kernelName of the C++ mirror, wave == lane from C++."""
    r = subprocess.run([mirror_exe(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "wave == lane" in r.stdout


def test_example_runs_on_the_wave_kernel(tmp_path):
    """examples/cgmres_cartpole.cpp --kernel wave: 16 controllers ticked through control_input_device for 0.1 s."""
    libdir = os.path.dirname(_capi.lib_path())
    exe = str(tmp_path / "cgmres_cartpole")
    cmd = ["g++", "-std=c++17", "-O2", f"-I{ROOT}/include", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "examples", "cgmres_cartpole.cpp"), f"-L{libdir}", "-lnmpc_hip_ddp", "-L/opt/rocm/lib", "-lamdhip64",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "16", "0.1", "--kernel", "wave"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "cgmres_wave_run_kernel" in r.stdout and " 0 non-finite" in r.stdout
