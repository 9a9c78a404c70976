"""Kernel choice through the API: nmpc_hip_ddp_set_kernel / set_dispatch_batch / kernel_name_for_batch and their
mirrors.  The environment variables are developer overrides read ONCE, when a handle is created — not on the launch path."""
import os

import numpy as np
import pytest

import nmpc_amd
from nmpc_amd import workloads

from test_gpu_parity import make_solver, oracle_batch, scaled_err

pytestmark = pytest.mark.gpu


def test_set_kernel_pins_the_family_and_environment_is_read_at_create(monkeypatch):
    wl = workloads.cartpole_batch(B=512, T=60, seed=1)
    s = make_solver(wl, max_iter=6)
    assert s.kernelName() == "ddp_solve_quad_kernel"
    monkeypatch.setenv("NMPC_HIP_DDP_KERNEL", "1w")  # after the handle exists: no effect on it
    assert s.kernelName() == "ddp_solve_quad_kernel"
    s.solve(wl.t0, wl.x0, wl.u_init)
    quad = (s.X().copy(), s.iters().copy(), s.status().copy())
    t = make_solver(wl, max_iter=6)  # a handle created under the override takes it
    assert t.kernelName() == "ddp_solve_tpi_kernel"
    monkeypatch.delenv("NMPC_HIP_DDP_KERNEL")
    assert t.kernelName() == "ddp_solve_tpi_kernel"
    t.setKernel("auto")
    assert t.kernelName() == "ddp_solve_quad_kernel"
    for name, kernel in (("2w", "ddp_solve_tpi2w_kernel"), ("1w", "ddp_solve_tpi_kernel"), ("ddp_solve_tpi2w_kernel", "ddp_solve_tpi2w_kernel"),
                         ("tile64", "ddp_solve_quad_kernel"), ("auto", "ddp_solve_quad_kernel")):  # (no tile kernel for n = 4: ignored)
        s.setKernel(name)
        assert s.kernelName() == kernel, name
        s.solve(wl.t0, wl.x0, wl.u_init)
        # across families: the same decisions, values to rounding (INTEGRATION.md "what is reproducible")
        assert np.array_equal(s.iters(), quad[1]) and np.array_equal(s.status(), quad[2]) and scaled_err(s.X(), quad[0]) < 1e-11
    assert np.array_equal(s.X(), quad[0])  # back on the quad kernel: the same bits
    with pytest.raises((ValueError, RuntimeError)):
        s.setKernel("warp32")
    # a choice made before the (lazily created) handle exists is applied when it is created
    u = nmpc_amd.DDPSolverBatch(nmpc_amd.make_problem(wl.model), wl.B)
    u.config().horizon_steps = wl.T
    u.setKernel("2w")
    assert u.kernelName() == "ddp_solve_tpi2w_kernel"


def test_dispatch_batch_gives_a_shard_the_whole_batchs_family():
    wl = workloads.cartpole_batch(B=2048, T=40, seed=3)
    s = make_solver(wl, max_iter=5)
    assert s.kernelName() == "ddp_solve_quad_kernel" and s.kernelNameForBatch(8192) == "ddp_solve_tpi2w_kernel"
    s.setDispatchBatch(8192)
    assert s.kernelName() == "ddp_solve_tpi2w_kernel"
    s.setDispatchBatch(0)
    assert s.kernelName() == "ddp_solve_quad_kernel"
    # fp32: the family depends on the batch size at the reference's default threshold (tile64<float> below 8192, tile32 from there)
    wl = workloads.quadrotor_batch(B=256, T=20, seed=3, fp32=True)
    s = make_solver(wl, max_iter=2)
    assert s.kernelName() == "ddp_solve_tile64_kernel" and s.kernelNameForBatch(8192) == "ddp_solve_tile32_kernel"
    whole = workloads.quadrotor_batch(B=8192, T=20, seed=3, fp32=True)
    w = make_solver(whole, max_iter=2)
    w.solve(whole.t0, whole.x0, whole.u_init)
    assert w.kernelName() == "ddp_solve_tile32_kernel"
    for lo, hi in ((0, 4096), (4096, 8192)):
        sh = workloads.quadrotor_batch(B=8192, T=20, seed=3, fp32=True)
        sh.B, sh.x0, sh.u_init, sh.t0 = hi - lo, sh.x0[lo:hi], sh.u_init[lo:hi], sh.t0[lo:hi]
        h = make_solver(sh, max_iter=2)
        h.setDispatchBatch(8192)
        h.solve(sh.t0, sh.x0, sh.u_init)
        assert h.kernelName() == "ddp_solve_tile32_kernel"
        assert np.array_equal(h.X(), w.X()[lo:hi]) and np.array_equal(h.U(), w.U()[lo:hi]) and np.array_equal(h.iters(), w.iters()[lo:hi])


def test_without_the_workspace_the_lane_kernels_take_the_solve(monkeypatch):
    """centroidal / manipulator batches go to the tile kernel, whose gain records live in the per-instance workspace; when
    that allocation fails at create the handle has to fall back to a kernel that needs none — and say so in kernelName()."""
    wl = workloads.manipulator_batch(B=96, T=20, seed=4)
    monkeypatch.setenv("NMPC_HIP_DDP_NO_WORKSPACE", "1")
    s = make_solver(wl, max_iter=4)
    assert s.kernelName() == "ddp_solve_tpi_kernel"  # (the Python mirror creates its handle lazily: here)
    monkeypatch.delenv("NMPC_HIP_DDP_NO_WORKSPACE")
    assert s.kernelName() == "ddp_solve_tpi_kernel"
    s.solve(wl.t0, wl.x0, wl.u_init)
    ref = oracle_batch(wl, max_iter=4)
    assert np.array_equal(s.iters(), ref.iters) and np.array_equal(s.status(), ref.status)
    assert scaled_err(s.X(), ref.X) < 1e-9 and scaled_err(s.Kfb(), ref.K) < 1e-8
    t = make_solver(wl, max_iter=4)
    assert t.kernelName() == "ddp_solve_tile64_kernel"


# ---- the dispatch table: every registered DDP problem type, every pin, with and without the workspace ----------------------------------
# tests/golden/kernel_choice.txt was recorded from the library before the kernel choice moved into one plan per solve
# (ModelOpsFor::plan, include/nmpc_amd/hip/model_registry.hpp); the decision must not have moved for any combination.
TABLE_MODELS = ("cartpole", "bipedal", "vertical", "centroidal", "quadrotor", "manipulator", "planar_vtol", "cartpole_f32",
                "quadrotor_f32", "manipulator_f32")
TABLE_BATCHES = (16, 63, 64, 512, 1024, 1025, 4096, 4097, 6143, 6144, 8191, 8192, 16384)
TABLE_PINS = ("auto", "1w", "2w", "quad", "wpi", "tile64", "tile32")
TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_choice.txt")


def dispatch_table():
    """One line per (model, constrained, cost_update_thre, pin, workspace): whether set_model_params_batch is accepted at the handle's
    batch (64), then the family kernel_name_for_batch reports for every batch of TABLE_BATCHES (ddp_solve_<family>_kernel)."""
    import ctypes as C

    from nmpc_amd import _capi
    L = _capi.load()
    lines = []
    for ws in (1, 0):
        for model in TABLE_MODELS:
            if ws:
                os.environ.pop("NMPC_HIP_DDP_NO_WORKSPACE", None)
            else:
                os.environ["NMPC_HIP_DDP_NO_WORKSPACE"] = "1"
            try:
                prob = nmpc_amd.make_problem(model)
                s = nmpc_amd.DDPSolverBatch(prob, 64)
                s.config().print_level = 0
                s.config().horizon_steps = 20
                s.kernelName()  # (creates the handle: the environment is read here)
            finally:
                os.environ.pop("NMPC_HIP_DDP_NO_WORKSPACE", None)
            for con in (0, 1):
                for thre in ((1e-7, 1e-3) if model.endswith("_f32") else (None,)):
                    for pin in TABLE_PINS:
                        s.config().with_input_constraint = bool(con)
                        if thre is not None:
                            s.config().cost_update_thre = thre
                        s.setKernel(pin)
                        names = [s.kernelNameForBatch(b)[len("ddp_solve_"):-len("_kernel")] for b in TABLE_BATCHES]
                        raw = bytes(prob.blob) * 64
                        own = L.nmpc_hip_ddp_set_model_params_batch(s._h, raw, C.sizeof(prob.blob)) == _capi.OK
                        _capi.check(L.nmpc_hip_ddp_set_model_params_batch(s._h, None, 0))
                        key = f"{model} con={con} thre={'-' if thre is None else f'{thre:g}'} pin={pin} ws={ws}"
                        lines.append(f"{key} own={int(own)} : {' '.join(names)}")
            s.close()
    return lines


def test_dispatch_table_matches_the_recorded_one():
    with open(TABLE_PATH) as f:
        want = [ln.rstrip("\n") for ln in f if ln.strip() and not ln.startswith("#")]
    assert dispatch_table() == want


def test_stream_check_uses_the_handles_knobs(monkeypatch):
    """solve_stream asks the handle's own plan whether its family has resumable launches: a handle pinned to the single-wavefront
    kernel is refused up front, and a variable set after create does not change an unpinned handle's answer."""
    wl = workloads.cartpole_batch(B=300, T=30, seed=5)
    s = make_solver(wl, max_iter=20)
    s.setKernel("1w")
    with pytest.raises(RuntimeError, match=r"nmpc_hip_ddp -2\].*resumable"):
        s.solveStream(wl.t0, wl.x0, wl.u_init)
    t = make_solver(wl, max_iter=20)
    t.kernelName()  # (creates the handle)
    monkeypatch.setenv("NMPC_HIP_DDP_KERNEL", "1w")
    r = t.solveStream(wl.t0, wl.x0, wl.u_init)
    assert r.iters.shape == (wl.B,) and (r.iters > 0).all()
