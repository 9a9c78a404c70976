"""The shipped DDP problem functors (include/nmpc_amd/models/*.hpp), compiled on the host by tests/cpp/model_functor_checker.cpp,
checked directly rather than only through solve parity:

  * finite differences of stateEq, the running cost and the terminal cost against the analytic derivatives the device uses
    (TestDDPCartPole.cpp:609-649, TestDDPCentroidalMotion.cpp:367-411, and the same for every other shipped fp64 model);
  * every output against the oracle's separately written functors (oracle.model_eval) at ~100 random points per model;
  * the fp32 types against their fp64 twins;
  * the default problem objects against the oracle's default parameters and the library's nmpc_hip_ddp_model_default_params;
  * the test-only BoxQP probe (tests/cpp/boxqp_probe.hpp) means what tests/test_gpu_boxqp_known_answers.py relies on.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64_MODELS = ("cartpole", "bipedal", "vertical", "centroidal", "quadrotor", "manipulator", "planar_vtol")
FP32_TWINS = {"cartpole_f32": "cartpole", "quadrotor_f32": "quadrotor", "manipulator_f32": "manipulator"}


class Eval:
    pass


class Checker:
    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.mfc_eval.argtypes = [C.c_char_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)] + [C.c_void_p] * 12

    def info(self, name):
        n, m, dyn, sb, pb = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
        assert self.L.mfc_info(name.encode(), C.byref(n), C.byref(m), C.byref(dyn), C.byref(sb), C.byref(pb)) == 0, name
        return n.value, m.value, bool(dyn.value), sb.value, pb.value

    def default_blob(self, name):
        nbytes = self.info(name)[4]
        buf = C.create_string_buffer(nbytes)
        assert self.L.mfc_default_params(name.encode(), buf, C.c_size_t(nbytes)) == 0
        return buf.raw

    def eval(self, name, t, x, u, blob=None):
        n, mmax, _, _, _ = self.info(name)
        mm = max(mmax, 1)
        x = np.ascontiguousarray(x, dtype=np.float64)
        ub = np.zeros(mm)
        u = np.asarray(u, dtype=np.float64).ravel()
        ub[: min(u.size, mm)] = u[:mm]
        o = {k: np.zeros(s) for k, s in (("xn", n), ("L", 1), ("phi", 1), ("Fx", n * n), ("Fu", n * mm), ("Lx", n), ("Lu", mm),
                                          ("Lxx", n * n), ("Luu", mm * mm), ("Lxu", n * mm), ("Vx", n), ("Vxx", n * n))}
        m = C.c_int()
        pb = None if blob is None else C.create_string_buffer(bytes(blob), len(blob))
        keys = ("xn", "L", "phi", "Fx", "Fu", "Lx", "Lu", "Lxx", "Luu", "Lxu", "Vx", "Vxx")
        rc = self.L.mfc_eval(name.encode(), pb, float(t), x.ctypes.data, ub.ctypes.data, C.byref(m), *[o[k].ctypes.data for k in keys])
        assert rc == 0
        mi = m.value
        e = Eval()
        e.m = mi
        e.xn, e.Lx, e.Vx = o["xn"], o["Lx"], o["Vx"]
        e.running_cost, e.terminal_cost = float(o["L"][0]), float(o["phi"][0])
        e.Fx, e.Lxx, e.Vxx = (o[k].reshape(n, n) for k in ("Fx", "Lxx", "Vxx"))
        e.Fu, e.Lxu = (o[k][: n * mi].reshape(n, mi) for k in ("Fu", "Lxu"))
        e.Lu, e.Luu = o["Lu"][:mi].copy(), o["Luu"][: mi * mi].reshape(mi, mi)
        return e


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    out = tmp_path_factory.mktemp("mfc")
    lib = os.path.join(str(out), "libmodel_functor_checker.so")
    src = os.path.join(ROOT, "tests", "cpp", "model_functor_checker.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", f"-I{os.path.join(ROOT, 'include')}", src, "-o", lib],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return Checker(lib)


def blob_from(chk, name, params):
    """A problem object's memory image from the oracle's parameter vector (same order; the oracle's vectors of the builder models
    end in unused entries)."""
    nbytes = chk.info(name)[4]
    return np.asarray(params, dtype=np.float64)[: nbytes // 8].tobytes()


def fd_jacobians(chk, name, t, x, u, blob=None, eps=1e-6):
    n, m = x.size, u.size
    Fx, Fu = np.zeros((n, n)), np.zeros((n, m))
    for i in range(n):
        e = np.zeros(n)
        e[i] = eps
        Fx[:, i] = (chk.eval(name, t, x + e, u, blob).xn - chk.eval(name, t, x - e, u, blob).xn) / (2 * eps)
    for i in range(m):
        e = np.zeros(m)
        e[i] = eps
        Fu[:, i] = (chk.eval(name, t, x, u + e, blob).xn - chk.eval(name, t, x, u - e, blob).xn) / (2 * eps)
    return Fx, Fu


def fd_cost(f, z0, eps=1e-5):
    k = z0.size
    g, Hh = np.zeros(k), np.zeros((k, k))
    for i in range(k):
        e = np.zeros(k)
        e[i] = eps
        g[i] = (f(z0 + e) - f(z0 - e)) / (2 * eps)
        for j in range(k):
            d = np.zeros(k)
            d[j] = eps
            Hh[i, j] = (f(z0 + e + d) - f(z0 + e - d) - f(z0 - e + d) + f(z0 - e - d)) / (4 * eps * eps)
    return g, Hh


# ---------------------------------------------------------------------------------------------------
# finite differences of the shipped functors
# ---------------------------------------------------------------------------------------------------
def test_cartpole_check_derivative(chk):
    """TestDDPCartPole.cpp:609-649 on the shipped functor: x = (1, -2, 3, -4), u = 10, dt = 0.01."""
    x, u = np.array([1.0, -2.0, 3.0, -4.0]), np.array([10.0])
    ev = chk.eval("cartpole", 0.0, x, u)
    Fx, Fu = fd_jacobians(chk, "cartpole", 0.0, x, u)
    assert np.linalg.norm(ev.Fx - Fx) < 1e-6
    assert np.linalg.norm(ev.Fu - Fu) < 1e-6


def test_centroidal_check_derivative(chk):
    """TestDDPCentroidalMotion.cpp:367-411 on the shipped functor: constant stance, dt = 0.01, random x, u in [-1, 1]."""
    rng = np.random.default_rng(3)
    blob = blob_from(chk, "centroidal", oracle.default_params("centroidal", dt=0.01, flight_t0=1e9, flight_t1=2e9, ref_switch_t=1e9))
    for t in (0.0, 2.0):
        for _ in range(5):
            x, u = rng.uniform(-1, 1, 9), rng.uniform(-1, 1, 16)
            ev = chk.eval("centroidal", t, x, u, blob)
            assert ev.m == 16
            Fx, Fu = fd_jacobians(chk, "centroidal", t, x, u, blob)
            assert np.linalg.norm(ev.Fx - Fx) < 1e-6
            assert np.linalg.norm(ev.Fu - Fu) < 1e-6


@pytest.mark.parametrize("model", FP64_MODELS)
def test_shipped_jacobians_and_cost_derivatives(chk, model):
    """Every shipped fp64 model at the points tests/test_oracle_pins.py uses for the oracle's functors: state-equation Jacobians to
    1e-6 (Frobenius), cost gradient and Hessian blocks and the terminal cost's against central differences."""
    rng = np.random.default_rng(11)
    n = chk.info(model)[0]
    t = {"vertical": 2.5, "bipedal": 7.4}.get(model, 0.3)
    for _ in range(3):
        x = rng.uniform(-0.7, 0.7, n)
        m = chk.eval(model, t, x, np.zeros(16)).m
        u = rng.uniform(-1, 1, m) * (5.0 if model in ("cartpole", "quadrotor", "planar_vtol") else 1.0)
        ev = chk.eval(model, t, x, u)
        Fx, Fu = fd_jacobians(chk, model, t, x, u)
        assert np.linalg.norm(ev.Fx - Fx) < 1e-6
        assert np.linalg.norm(ev.Fu - Fu) < 1e-6
        g, Hh = fd_cost(lambda z: chk.eval(model, t, z[:n], z[n:]).running_cost, np.concatenate([x, u]))
        scale = 1.0 + np.abs(Hh).max()
        np.testing.assert_allclose(np.concatenate([ev.Lx, ev.Lu]), g, rtol=1e-6, atol=1e-7 * scale)
        np.testing.assert_allclose(ev.Lxx, Hh[:n, :n], rtol=1e-4, atol=2e-5 * scale)
        np.testing.assert_allclose(ev.Luu, Hh[n:, n:], rtol=1e-4, atol=2e-5 * scale)
        np.testing.assert_allclose(ev.Lxu, Hh[:n, n:], rtol=1e-4, atol=2e-5 * scale)
        gv, Hv = fd_cost(lambda z: chk.eval(model, t, z, u).terminal_cost, x)
        scale = 1.0 + np.abs(Hv).max()
        np.testing.assert_allclose(ev.Vx, gv, rtol=1e-6, atol=1e-7 * scale)
        np.testing.assert_allclose(ev.Vxx, Hv, rtol=1e-4, atol=2e-5 * scale)


# ---------------------------------------------------------------------------------------------------
# shipped functors against the oracle's, and the fp32 types against their fp64 twins
# ---------------------------------------------------------------------------------------------------
FIELDS = ("xn", "running_cost", "terminal_cost", "Fx", "Fu", "Lx", "Lu", "Lxx", "Luu", "Lxu", "Vx", "Vxx")


def _sample(rng, model, n, m):
    x = rng.uniform(-1.0, 1.0, n)
    u = rng.uniform(-1.0, 1.0, m) * (5.0 if model in ("cartpole", "quadrotor", "planar_vtol") else 1.0)
    return x, u


@pytest.mark.parametrize("model", FP64_MODELS)
def test_shipped_functors_match_the_oracle(chk, model):
    """~100 random (t, x, u) per model, default parameters: every output of the shipped functor against the oracle's restatement
    within 1e-12 (1 + |oracle|), the input dimension exactly.  No model needs a looser bar although the shipped models take sin / cos
    from sincosFast (linalg.hpp) and the oracle from libm: the worst difference seen is 1.1e-16."""
    rng = np.random.default_rng(2024)
    n = chk.info(model)[0]
    tol = 1e-12
    t_hi = {"bipedal": 20.0, "vertical": 10.0, "centroidal": 2.5}.get(model, 1.0)
    worst = 0.0
    for _ in range(100):
        t = float(rng.uniform(0.0, t_hi))
        m = chk.eval(model, t, np.zeros(n), np.zeros(16)).m
        assert m == int(oracle.input_dims(model, None, t, 1)[0])
        x, u = _sample(rng, model, n, m)
        a, b = chk.eval(model, t, x, u), oracle.model_eval(model, None, t, x, u)
        assert a.m == b.m
        for f in FIELDS:
            got, want = np.asarray(getattr(a, f), float), np.asarray(getattr(b, f), float)
            assert got.shape == want.shape, f
            err = float((np.abs(got - want) / (1.0 + np.abs(want))).max()) if got.size else 0.0
            worst = max(worst, err)
            assert err <= tol, f"{model} {f} at t = {t}: {err:.3e}"
    print(f"[{model}] worst scaled difference to the oracle: {worst:.2e}")


@pytest.mark.parametrize("f32,f64", sorted(FP32_TWINS.items()))
def test_fp32_types_match_their_fp64_twins(chk, f32, f64):
    """The float instantiations compute the same statements in float: every output within 2e-4 (1 + |fp64|) of the fp64 twin at
    ~100 random points (inputs representable in float; a few dozen float roundings of O(1) quantities, worst seen ~1e-5)."""
    rng = np.random.default_rng(5)
    n, m = chk.info(f64)[0], chk.info(f64)[1]
    for _ in range(100):
        t = float(np.float32(rng.uniform(0.0, 1.0)))
        x, u = _sample(rng, f64, n, m)
        x, u = x.astype(np.float32).astype(np.float64), u.astype(np.float32).astype(np.float64)
        a, b = chk.eval(f32, t, x, u), chk.eval(f64, t, x, u)
        for f in FIELDS:
            got, want = np.asarray(getattr(a, f), float), np.asarray(getattr(b, f), float)
            err = float((np.abs(got - want) / (1.0 + np.abs(want))).max())
            assert err <= 2e-4, f"{f32} {f}: {err:.3e}"


@pytest.mark.parametrize("model", FP64_MODELS + tuple(sorted(FP32_TWINS)))
def test_default_problem_objects(chk, model):
    """The default problem object of each shipped type equals the oracle's default parameters (the same vector the solve tests hand
    the oracle), and the library's nmpc_hip_ddp_model_default_params writes that same object."""
    from nmpc_amd import _capi
    blob = chk.default_blob(model)
    scalar = chk.info(model)[3]
    vals = np.frombuffer(blob, dtype=np.float64 if scalar == 8 else np.float32).astype(np.float64)
    ref = oracle.default_params(model)
    assert vals.size <= ref.size
    want = ref[: vals.size] if scalar == 8 else ref[: vals.size].astype(np.float32).astype(np.float64)
    np.testing.assert_array_equal(vals, want)
    assert not ref[vals.size:].any()  # (the oracle's vectors of the builder models end in unused zeros)
    L = _capi.load()
    buf = C.create_string_buffer(len(blob))
    _capi.check(L.nmpc_hip_ddp_model_default_params(model.encode(), buf, C.c_size_t(len(blob))))
    assert buf.raw == blob


# ---------------------------------------------------------------------------------------------------
# the BoxQP probe of tests/test_gpu_boxqp_known_answers.py
# ---------------------------------------------------------------------------------------------------
def probe_blob(dtype, n, mm, dt, H, g, Cm, m_steps=None):
    """Memory image of BoxQPProbe<Real, n, M, mm> (tests/cpp/boxqp_probe.hpp): dt, H (mm x mm), g (mm), C (mm x n), all column-major,
    then 16 ints of inputDim per timestep, padded to the alignment of Real."""
    Hb, gb, Cb = np.zeros((mm, mm)), np.zeros(mm), np.zeros((mm, n))
    H, g, Cm = np.asarray(H, float), np.asarray(g, float), np.asarray(Cm, float)
    Hb[: H.shape[0], : H.shape[1]] = H
    gb[: g.size] = g
    Cb[: Cm.shape[0], :] = Cm
    body = np.concatenate([[dt], Hb.T.ravel(), gb, Cb.T.ravel()]).astype(dtype).tobytes()
    steps = np.full(16, mm, np.int32) if m_steps is None else np.asarray(m_steps, np.int32)
    raw = body + steps.tobytes()
    align = np.dtype(dtype).itemsize
    return raw + b"\0" * ((-len(raw)) % align)


@pytest.mark.parametrize("name,dtype,n,mm", [("boxqp_probe_d4m2", np.float64, 4, 2), ("boxqp_probe_d9dyn16", np.float64, 9, 16),
                                             ("boxqp_probe_f4m2", np.float32, 4, 2)])
def test_boxqp_probe_means_what_it_claims(chk, name, dtype, n, mm):
    """Fu = 0 and Fx = I (the input never moves the state), Luu = H, Lu = g + Hu + Cx, Lxu = C', Lx = C'u, Lxx = 0, Vx = x, Vxx = I,
    the running cost's derivatives against central differences, and inputDim(t) read from the table — what makes the backward pass
    hand BoxQP exactly H, g and C.  The probe's blob layout (size, field offsets) is the one the GPU test writes."""
    rng = np.random.default_rng(17)
    nbytes = chk.info(name)[4]
    default = probe_blob(dtype, n, mm, 0.1, np.eye(mm), np.zeros(mm), np.zeros((mm, n)))
    assert len(default) == nbytes and chk.default_blob(name) == default
    steps = [16, 16, 0, 0, 16, 4, 2, 2] + [16] * 8 if mm == 16 else None
    tol = 1e-12 if dtype == np.float64 else 1e-5
    for it in range(6):
        A = rng.normal(size=(mm, mm))
        H = A @ A.T + np.eye(mm)
        g, Cm = rng.normal(size=mm), rng.normal(size=(mm, n))
        if dtype == np.float32:
            H, g, Cm = (v.astype(np.float32).astype(np.float64) for v in (H, g, Cm))
        blob = probe_blob(dtype, n, mm, 0.1, H, g, Cm, steps)
        t = 0.1 * it
        x = rng.uniform(-1, 1, n)
        m = mm if steps is None else steps[it]
        u = rng.uniform(-1, 1, m)
        if dtype == np.float32:
            x, u = x.astype(np.float32).astype(np.float64), u.astype(np.float32).astype(np.float64)
        ev = chk.eval(name, t, x, u, blob)
        assert ev.m == m
        Hm, gm, Cmm = H[:m, :m], g[:m], Cm[:m]
        np.testing.assert_allclose(ev.xn, x, rtol=0, atol=tol)
        np.testing.assert_array_equal(ev.Fx, np.eye(n))
        assert ev.Fu.shape == (n, m) and not ev.Fu.any()
        np.testing.assert_allclose(ev.Luu, Hm, rtol=0, atol=tol * 10)
        np.testing.assert_allclose(ev.Lu, gm + Hm @ u + Cmm @ x, rtol=0, atol=tol * 100)
        np.testing.assert_allclose(ev.Lxu, Cmm.T, rtol=0, atol=tol * 10)
        np.testing.assert_allclose(ev.Lx, Cmm.T @ u, rtol=0, atol=tol * 100)
        assert not ev.Lxx.any()
        np.testing.assert_allclose(ev.Vx, x, rtol=0, atol=tol)
        np.testing.assert_array_equal(ev.Vxx, np.eye(n))
        Lref = 0.5 * u @ Hm @ u + gm @ u + u @ Cmm @ x
        assert abs(ev.running_cost - Lref) <= tol * 100 * (1 + abs(Lref))
        if dtype == np.float64 and m > 0:
            gr, Hh = fd_cost(lambda z: chk.eval(name, t, z[:n], z[n:], blob).running_cost, np.concatenate([x, u]))
            scale = 1.0 + np.abs(Hh).max()
            np.testing.assert_allclose(np.concatenate([ev.Lx, ev.Lu]), gr, rtol=1e-6, atol=1e-7 * scale)
            np.testing.assert_allclose(ev.Luu, Hh[n:, n:], rtol=1e-4, atol=2e-5 * scale)
            np.testing.assert_allclose(ev.Lxu, Hh[:n, n:], rtol=1e-4, atol=2e-5 * scale)
            np.testing.assert_allclose(Hh[:n, :n], 0.0, atol=2e-5 * scale)
            Fx, Fu = fd_jacobians(chk, name, t, x, u, blob)
            assert np.linalg.norm(Fu) == 0.0 and np.linalg.norm(Fx - np.eye(n)) < 1e-9
