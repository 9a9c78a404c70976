"""Batched GMRES solver: what can be checked without a GPU — the C-ABI's exports and the mirrors' constants against the header,
argument validation, the CPU checker (tests/cpp/gmres_checker.cpp) against the reference's bars, a NumPy restatement and
numpy.linalg.lstsq, and the stability of every decision of the GPU cases (tests/gmres_checker.py) under the two sum orders.

The argument checks that need a handle (k_max above the capacity or the Householder bound, BASIS without keep_basis, a wrong byte
count) run wherever create() gives one, i.e. on a machine with a device; tests/test_gpu_gmres.py repeats them under the gpu mark."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gmres_checker as gc
from nmpc_amd import _capi, gmres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nmpc_hip_gmres.h")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return gc.shared_checker(tmp_path_factory.mktemp("gmres_checker"))


# ---- mirror consistency ------------------------------------------------------------------------------------------------------
def test_every_declared_entry_point_is_exported():
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(nmpc_hip_gmres_\w+)\s*\(", text))
    assert declared == set(gmres.EXPORTS)
    L = gmres.load()
    for name in declared:
        getattr(L, name)


def test_default_config_and_struct_are_the_headers():
    c = gmres.default_config()
    assert (c.k_max, c.eps, c.make_triangular, c.apply_reorth, c.keep_basis) == (100, 1e-10, 1, 1, 0)
    body = re.search(r"typedef struct\s*\{(.*?)\}\s*nmpc_hip_gmres_config;", open(HEADER).read(), re.S).group(1)
    fields = re.findall(r"^\s*(int|double)\s+(\w+);", body, re.M)
    assert [(n, {"int": C.c_int, "double": C.c_double}[t]) for t, n in fields] == gmres.CConfig._fields_


def test_mirror_constants_are_the_headers():
    text = open(HEADER).read()
    fields = dict(re.findall(r"NMPC_HIP_GMRES_FIELD_(\w+) = (\d+)", text))
    assert {k: int(v) for k, v in fields.items()} == {
        "X": gmres.FIELD_X, "ITERS": gmres.FIELD_ITERS, "REORTH": gmres.FIELD_REORTH, "ERR_LIST": gmres.FIELD_ERR_LIST, "H": gmres.FIELD_H,
        "G": gmres.FIELD_G, "BASIS": gmres.FIELD_BASIS, "STATUS": gmres.FIELD_STATUS}
    status = {k: int(v) for k, v in re.findall(r"NMPC_HIP_GMRES_(CONVERGED|K_MAX|NON_FINITE) = (\d+)", text)}
    assert status == {"CONVERGED": gmres.STATUS_CONVERGED, "K_MAX": gmres.STATUS_K_MAX, "NON_FINITE": gmres.STATUS_NON_FINITE}
    assert sorted(status.values()) == [1, 2, 3]
    defines = dict(re.findall(r"#define NMPC_HIP_GMRES_(\w+) (\d+)", text))
    assert int(defines["MAX_DIM"]) == gmres.MAX_DIM == 512
    assert int(defines["HOUSEHOLDER_MAX_K"]) == gmres.HOUSEHOLDER_MAX_K >= 100
    # the C++ mirror (it also static_asserts them against the header) and the kernels' header
    mirror = open(os.path.join(ROOT, "include", "nmpc_amd", "GmresBatch.hpp")).read()
    assert int(re.search(r"MaxDim = (\d+);", mirror).group(1)) == gmres.MAX_DIM
    assert int(re.search(r"HouseholderMaxK = (\d+);", mirror).group(1)) == gmres.HOUSEHOLDER_MAX_K
    kernels = open(os.path.join(ROOT, "include", "nmpc_amd", "hip", "gmres_kernels.hpp")).read()
    assert int(re.search(r"kMaxDim = (\d+);", kernels).group(1)) == gmres.MAX_DIM
    assert int(re.search(r"kHouseholderMaxK = (\d+);", kernels).group(1)) == gmres.HOUSEHOLDER_MAX_K
    # the Householder bound's reasoning: its LDS fits the 160 KiB of a gfx950 workgroup, and the next multiple of 16 would not
    lds = lambda n, K: (2 * n + 3 * (K + 1) + 4 * K + (K + 1) ** 2) * 8
    assert lds(512, gmres.HOUSEHOLDER_MAX_K) <= 160 * 1024 < lds(512, gmres.HOUSEHOLDER_MAX_K + 16)


# ---- argument checks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch,cap", [(0, 4, 10), (513, 4, 10), (-1, 4, 10), (8, 0, 8), (8, -3, 8), (8, 4, 0)])
def test_create_validates_before_it_probes_the_device(n, batch, cap):
    L = gmres.load()
    h = C.c_void_p()
    assert L.nmpc_hip_gmres_create(n, batch, cap, 0, C.byref(h)) == _capi.ERR_INVALID_ARGUMENT
    assert not h.value and L.nmpc_hip_gmres_last_error()
    with pytest.raises(ValueError):
        gmres.GmresBatch(n, batch, cap)


def handle_argument_checks(L, h):
    """The checks that need a handle (n = 200, capacity 150); shared with tests/test_gpu_gmres.py."""
    cfg = gmres.default_config()
    bad = _capi.ERR_INVALID_ARGUMENT
    cfg.k_max = 151  # above the capacity
    assert L.nmpc_hip_gmres_set_config(h, C.byref(cfg)) == bad and b"capacity" in L.nmpc_hip_gmres_last_error()
    cfg.k_max = 150
    assert L.nmpc_hip_gmres_set_config(h, C.byref(cfg)) == _capi.OK
    cfg.make_triangular = 0  # Householder: 150 > 128
    assert L.nmpc_hip_gmres_set_config(h, C.byref(cfg)) == bad and b"Householder" in L.nmpc_hip_gmres_last_error()
    cfg.k_max = gmres.HOUSEHOLDER_MAX_K
    assert L.nmpc_hip_gmres_set_config(h, C.byref(cfg)) == _capi.OK
    cfg.k_max = 0
    assert L.nmpc_hip_gmres_set_config(h, C.byref(cfg)) == bad
    n = C.c_size_t()
    assert L.nmpc_hip_gmres_field_bytes(h, gmres.FIELD_BASIS, C.byref(n)) == bad and b"keep_basis" in L.nmpc_hip_gmres_last_error()
    assert L.nmpc_hip_gmres_field_bytes(h, 99, C.byref(n)) == bad
    assert L.nmpc_hip_gmres_field_bytes(h, gmres.FIELD_X, C.byref(n)) == _capi.OK and n.value == 3 * 200 * 8
    buf = np.zeros(3 * 200 + 1)
    assert L.nmpc_hip_gmres_get(h, gmres.FIELD_X, buf.ctypes.data_as(C.c_void_p), n.value + 8, 0) == bad
    assert b"bytes" in L.nmpc_hip_gmres_last_error()
    assert L.nmpc_hip_gmres_get(h, gmres.FIELD_BASIS, buf.ctypes.data_as(C.c_void_p), 8, 0) == bad
    assert L.nmpc_hip_gmres_get(h, gmres.FIELD_X, buf.ctypes.data_as(C.c_void_p), n.value, 0) == _capi.ERR_NOT_SOLVED
    assert L.nmpc_hip_gmres_solve(h) == _capi.ERR_NOT_SOLVED  # no system yet
    assert L.nmpc_hip_gmres_set_system(h, None, None, None, 0, 0) == bad


def test_create_needs_a_device_or_gives_a_handle():
    """Without a device (the CPU machine): NMPC_HIP_ERR_NO_DEVICE and its message.  With one: the handle-bound argument checks."""
    L = gmres.load()
    h = C.c_void_p()
    rc = L.nmpc_hip_gmres_create(200, 3, 150, 0, C.byref(h))
    assert rc in (_capi.OK, _capi.ERR_NO_DEVICE)
    if rc == _capi.OK:
        handle_argument_checks(L, h)
        assert L.nmpc_hip_gmres_destroy(h) == _capi.OK
    else:
        assert not h.value and b"no CPU fallback" in L.nmpc_hip_gmres_last_error()
        with pytest.raises(RuntimeError):
            gmres.GmresBatch(200, 3, 150)
    assert L.nmpc_hip_gmres_create(8, 4, 8, 0, None) == _capi.ERR_INVALID_ARGUMENT
    assert L.nmpc_hip_gmres_default_config(None) == _capi.ERR_INVALID_ARGUMENT
    for fn in (L.nmpc_hip_gmres_solve, L.nmpc_hip_gmres_synchronize):
        assert fn(None) == _capi.ERR_INVALID_ARGUMENT
    assert L.nmpc_hip_gmres_destroy(None) == _capi.OK


def test_cpp_mirror_and_example_compile_with_a_host_compiler_alone(tmp_path):
    """examples/gmres_batch.cpp against GmresBatch.hpp: g++, no HIP headers.  Run on one small size, it either meets the reference's
    bars (a device is there) or reports the library's no-device error; bad arguments end it with the usage line."""
    gmres.load()
    libdir = os.path.dirname(_capi.lib_path())
    exe = str(tmp_path / "gmres_batch")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT}/include", os.path.join(ROOT, "examples", "gmres_batch.cpp"),
           f"-L{libdir}", "-lnmpc_hip_ddp", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "4", "10", "50"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    last = r.stdout.splitlines()[-1]
    assert last == "ok gmres_wave_kernel" or last.startswith("runtime_error: no HIP device available"), last
    for bad in (["0"], ["4", "513"], ["4", "ten"]):
        r = subprocess.run([exe] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage" in r.stderr


# ---- the checker -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 50, 100, 500])
def test_checker_meets_the_reference_bars(checker, n):
    """TestGmres.cpp:98-142 on ten accepted systems per size, in the reference's (sequential) sum order."""
    A, b = gc.systems(n, 10)
    assert max(np.linalg.cond(a) for a in A) <= gc.COND_MAX
    legs = [(1000, True, True, 1e-10), (1000, True, False, 1e-10), (20, True, True, 1e2)] + ([(1000, False, True, 1e-10)] if n <= 100 else [])
    for k_max, tri, reorth, bar in legs:
        r = checker.solve(A, b, k_max=k_max, make_triangular=tri, apply_reorth=reorth)
        err = np.mean([np.linalg.norm(A[s] @ r.x[s] - b[s]) for s in range(10)])
        print("n %d k_max %d triangular %d reorth %d: mean |Ax - b| %.3e" % (n, k_max, tri, reorth, err))
        assert err < bar, (n, k_max, tri, reorth, err)
        assert (r.iters <= min(k_max, n)).all() and set(r.status.tolist()) <= {1, 2}


def numpy_gmres(A, b, x, k_max, eps, apply_reorth):
    """Gmres.h:67-192, triangular variant, statement by statement in NumPy (np.dot's own sum order)."""
    n = len(b)
    k_max = min(k_max, n)
    r = b - A @ x
    rho = np.linalg.norm(r)
    basis = [r / rho if rho > 0 else r]
    g = np.zeros(k_max + 1)
    g[0] = rho
    b_norm = np.linalg.norm(b)
    H = np.zeros((k_max + 1, k_max))
    err, cs, sn, k, fired = [rho], [], [], 0, 0
    while rho > eps * b_norm and k < k_max:
        k += 1
        Avk = A @ basis[-1]
        nb = Avk.copy()
        for j in range(k):
            H[j, k - 1] = nb @ basis[j]
            nb = nb - H[j, k - 1] * basis[j]
        nbn = np.linalg.norm(nb)
        H[k, k - 1] = nbn
        if apply_reorth:
            an = np.linalg.norm(Avk)
            if an + 1e-3 * nbn == an:
                fired += 1
                for j in range(k):
                    h = nb @ basis[j]
                    H[j, k - 1] += h
                    nb = nb - h * basis[j]
        z = np.linalg.norm(nb)
        basis.append(nb / z if z > 0 else nb)
        for i in range(k - 1):
            h0, h1 = H[i, k - 1], H[i + 1, k - 1]
            H[i, k - 1] = cs[i] * h0 - sn[i] * h1
            H[i + 1, k - 1] = sn[i] * h0 + cs[i] * h1
        nu = np.sqrt(H[k - 1, k - 1] ** 2 + H[k, k - 1] ** 2)
        c, s = H[k - 1, k - 1] / nu, -H[k, k - 1] / nu
        cs.append(c)
        sn.append(s)
        H[k - 1, k - 1] = c * H[k - 1, k - 1] - s * H[k, k - 1]
        H[k, k - 1] = 0
        g0, g1 = g[k - 1], g[k]
        g[k - 1], g[k] = c * g0 - s * g1, s * g0 + c * g1
        rho = abs(g[k])
        err.append(rho)
    y = np.linalg.solve(np.triu(H[:k, :k]), g[:k]) if k else np.zeros(0)
    for i in range(k):
        x = x + y[i] * basis[i]
    return x, k, fired, np.array(err), H, g


@pytest.mark.parametrize("n,B", [(10, 10), (65, 5), (100, 10)])
@pytest.mark.parametrize("order", gc.ORDERS)
def test_triangular_checker_agrees_with_a_numpy_restatement(checker, n, B, order):
    """Both sum orders of the checker against NumPy's own: same iteration counts, and x, err_list_, g_, H_ within a reordered sum's
    freedom on these systems (cond <= 1e4, n <= 100: 1e-9 relative is three orders above what is measured, 1e-12)."""
    A, b = gc.systems(n, B)
    for k_max, reorth in ((1000, True), (1000, False), (7, True)):
        r = checker.solve(A, b, k_max=k_max, apply_reorth=reorth, order=order)
        for s in range(B):
            x, k, fired, err, H, g = numpy_gmres(A[s], b[s], np.zeros(n), k_max, 1e-10, reorth)
            assert k == r.iters[s]
            worst = max(gc.rel_diff(r.x[s], x), gc.rel_diff(r.err[s][: k + 1], err), gc.rel_diff(r.g[s], g), gc.rel_diff(r.H[s], H))
            assert worst < 1e-9, (n, s, k_max, reorth, worst)
            assert np.isnan(r.err[s][k + 1:]).all()
    # a non-zero initial guess, and a second solve from the first's x (restart)
    x0 = np.random.default_rng(n).uniform(-1, 1, (B, n))
    r1 = checker.solve(A, b, x0=x0, k_max=5, order=order)
    r2 = checker.solve(A, b, x0=r1.x, k_max=5, order=order)
    for s in range(B):
        x, *_ = numpy_gmres(A[s], b[s], x0[s], 5, 1e-10, True)
        assert gc.rel_diff(r1.x[s], x) < 1e-9
        x, *_ = numpy_gmres(A[s], b[s], x, 5, 1e-10, True)
        assert gc.rel_diff(r2.x[s], x) < 1e-9


@pytest.mark.parametrize("n,B", [(1, 3), (2, 1), (10, 10), (65, 5), (100, 10)])
def test_householder_checker_agrees_with_lstsq(checker, n, B):
    """The Householder variant's y_k is the least-squares solution of the final (k + 1) x k problem H y = g (Gmres.h:172), its H_ the
    raw Hessenberg matrix (the triangular variant's before the rotations) and its rho the residual norm of that problem."""
    A, b = gc.systems(n, B)
    for k_max in (1000, 6):
        for order in gc.ORDERS:
            r = checker.solve(A, b, k_max=k_max, make_triangular=False, order=order)
            for s in range(B):
                k = int(r.iters[s])
                assert k == min(k_max, n)
                H, g = r.H[s][: k + 1, :k], r.g[s][: k + 1]
                y = np.linalg.lstsq(H, g, rcond=None)[0]
                scale = 1 + np.abs(y).max()
                assert np.abs(r.y[s][:k] - y).max() < 1e-9 * np.linalg.cond(H) * scale, (n, s, k_max)
                assert abs(r.err[s][k] - np.linalg.norm(g - H @ r.y[s][:k])) < 1e-12 * (1 + abs(r.err[s][0]))
                assert np.array_equal(g[1:], np.zeros(k)) and np.allclose(np.tril(H, -2), 0)
                V = r.basis[s][: k + 1]
                assert np.abs(A[s] @ V[:k].T - V.T @ H).max() < 1e-12 * n  # the Arnoldi relation A V_k = V_{k+1} H
    full = checker.solve(A, b, k_max=1000, make_triangular=False)
    tri = checker.solve(A, b, k_max=1000, make_triangular=True)
    assert gc.rel_diff(full.x, tri.x) < 1e-9  # both variants solve the same systems


# ---- decision stability of the GPU cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B,sub", gc.CASES, ids=lambda v: str(v))
def test_gpu_cases_decide_alike_in_both_sum_orders(checker, n, B, sub):
    """Every case of tests/test_gpu_gmres.py in both sum orders of the checker: ITERS and STATUS agree on every system, the REORTH
    count on at least 90 % of them; the reference's residual bar holds in both; the case's tolerance is printed."""
    A, b = gc.systems(n, B)
    seq, wave = gc.case_results(checker, n, B, sub)
    assert np.array_equal(seq.iters, wave.iters) and np.array_equal(seq.status, wave.status)
    stable = gc.decision_stable(seq, wave)
    assert stable.mean() >= 0.9, (n, B, sub, seq.reorth.tolist(), wave.reorth.tolist())
    want = gmres.STATUS_K_MAX if sub == "tri_k20" else gmres.STATUS_CONVERGED
    assert (seq.status == want).all()
    for r in (seq, wave):
        err = np.mean([np.linalg.norm(A[s] @ r.x[s] - b[s]) for s in range(B)])
        assert err < gc.residual_bar(sub), (n, B, sub, err)
    tol = gc.tolerance(seq, wave, (n, B, sub))
    assert all(np.isfinite(v) and v < 1e-7 for v in tol.values()), tol


@pytest.mark.parametrize("n", [10, 65, 130])
def test_low_rank_early_exit_on_the_checker(checker, n):
    """A = I + U V' of rank 3 converges at k = 4 with status 1 in both sum orders; the re-orthogonalisation fires in iteration 4 or
    not at all (there the new vector is rounding noise, and at n = 10 the two orders decide differently on two of three systems:
    tests/test_gpu_gmres.py holds the device to the wave order's decision, and to the sequential one where both agree)."""
    A, b = gc.low_rank_systems(n)
    seq, wave = (checker.solve(A, b, k_max=1000, order=o) for o in gc.ORDERS)
    assert (seq.iters == 4).all() and (wave.iters == 4).all() and (seq.status == 1).all() and (wave.status == 1).all()
    assert not seq.fired_at[:, :4].any() and not wave.fired_at[:, :4].any()
    assert np.array_equal(seq.fired_at.sum(axis=1), seq.reorth) and np.array_equal(wave.fired_at.sum(axis=1), wave.reorth)
    assert np.isnan(seq.err[:, 5:]).all() and np.isfinite(seq.err[:, :5]).all()
