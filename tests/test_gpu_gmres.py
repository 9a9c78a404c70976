"""Batched GMRES solver on the device (gmres_wave_kernel through nmpc_amd.gmres.GmresBatch) against the CPU checker
(tests/cpp/gmres_checker.cpp) in both of its sum orders:

  * "sequential" (the reference's order): ITERS and STATUS equal, REORTH equal on the systems whose decision is the same in both
    orders, X, ERR_LIST, G and the leading ITERS columns of H within gmres_checker.tolerance() of the case (10 x the measured
    difference between the two orders, floor 1e-13, relative to 1 + |value|; printed);
  * "wave" (the kernel's order): ITERS, STATUS and REORTH equal on every system, X and ERR_LIST byte for byte.

The cases, their systems and the checker's results live in tests/gmres_checker.py and are shared with tests/test_gmres_host_cpu.py,
which checks on the CPU that every case decides alike in both orders."""
import ctypes as C

import numpy as np
import pytest

import gmres_checker as gc
from nmpc_amd import _capi, gmres

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return gc.shared_checker(tmp_path_factory.mktemp("gmres_checker"))


def fields(s: gmres.GmresBatch) -> gc.Result:
    r = gc.Result()
    r.x, r.iters, r.reorth, r.status, r.err, r.g, r.H = s.x(), s.iters(), s.reorth(), s.status(), s.err_list_, s.g_, s.H_
    return r


def device_solve(A, b, x0=None, k_max=1000, make_triangular=True, apply_reorth=True, eps=1e-10, keep_basis=False, solver=None):
    B, n = b.shape
    s = solver or gmres.GmresBatch(n, B, k_max_capacity=k_max)
    s.make_triangular_, s.apply_reorth_, s.keep_basis = make_triangular, apply_reorth, keep_basis
    s.solve(A, b, x0, k_max=k_max, eps=eps)
    return s, fields(s)


def same_bits(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def assert_matches_checker(dev, seq, wave, tol, label):
    B = len(seq.iters)
    # the kernel's own order: every decision, and the bits of X and ERR_LIST
    assert np.array_equal(dev.iters, wave.iters) and np.array_equal(dev.status, wave.status) and np.array_equal(dev.reorth, wave.reorth), label
    byte_equal = same_bits(dev.x, wave.x) and same_bits(dev.err, wave.err)
    print("%s: byte-equal to the wave-order checker: %s (X %.3e, ERR_LIST %.3e)" % (label, byte_equal, gc.rel_diff(dev.x, wave.x),
                                                                                gc.rel_diff(dev.err, wave.err)))
    # the reference's order
    assert np.array_equal(dev.iters, seq.iters) and np.array_equal(dev.status, seq.status), label
    stable = gc.decision_stable(seq, wave)
    assert np.array_equal(dev.reorth[stable], seq.reorth[stable]), label
    got = {"X": gc.rel_diff(dev.x, seq.x), "ERR_LIST": gc.rel_diff(dev.err, seq.err), "G": gc.rel_diff(dev.g, seq.g),
           "H": max(gc.rel_diff(gc.leading_H(dev, s), gc.leading_H(seq, s)) for s in range(B))}
    print("%s: against the sequential checker: %s" % (label, ", ".join("%s %.3e" % kv for kv in got.items())))
    for q, v in got.items():
        assert v <= tol[q], (label, q, v, tol[q])
    assert byte_equal, label


@pytest.mark.parametrize("n,B,sub", gc.CASES, ids=lambda v: str(v))
def test_case_against_both_checker_orders(checker, n, B, sub):
    A, b = gc.systems(n, B)
    seq, wave = gc.case_results(checker, n, B, sub)
    tol = gc.tolerance(seq, wave, (n, B, sub))
    s, dev = device_solve(A, b, **gc.subcase_config(n, sub))
    assert s.kernelName() == "gmres_wave_kernel" and s.lastMs() > 0
    err = np.mean([np.linalg.norm(A[i] @ dev.x[i] - b[i]) for i in range(B)])
    print("%s: mean |Ax - b| %.3e, kernel %.3f ms" % ((n, B, sub), err, s.lastMs()))
    assert err < gc.residual_bar(sub)
    assert (dev.status == (gmres.STATUS_K_MAX if sub == "tri_k20" else gmres.STATUS_CONVERGED)).all()
    for i in range(B):
        assert np.isnan(dev.err[i][dev.iters[i] + 1:]).all() and np.isfinite(dev.err[i][: dev.iters[i] + 1]).all()
    assert_matches_checker(dev, seq, wave, tol, (n, B, sub))


# ---- early exits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 65, 130])
def test_low_rank_system_ends_at_k_4(checker, n):
    A, b = gc.low_rank_systems(n)
    B = len(b)
    seq, wave = (checker.solve(A, b, k_max=1000, order=o) for o in gc.ORDERS)
    assert (seq.iters == 4).all()  # (tests/test_gmres_host_cpu.py: confirmed on the checker)
    s, dev = device_solve(A, b)
    assert np.array_equal(dev.iters, seq.iters) and (dev.status == gmres.STATUS_CONVERGED).all()
    assert np.isnan(dev.err[:, 5:]).all() and np.isfinite(dev.err[:, :5]).all()
    assert same_bits(dev.x, wave.x) and same_bits(dev.err, wave.err)
    assert gc.rel_diff(dev.x, seq.x) <= gc.tolerance(seq, wave, ("low rank", n))["X"]
    # the iteration in which the re-orthogonalisation fires: REORTH of the same solve cut at k_max = 1 .. 4 counts it in
    counts = np.array([device_solve(A, b, k_max=k, solver=s)[1].reorth for k in range(1, 5)]).T  # [B][4]
    fired_at = np.diff(np.concatenate([np.zeros((B, 1), np.int32), counts], axis=1), axis=1)
    assert np.array_equal(fired_at, wave.fired_at[:, 1:5])
    agree = (seq.fired_at == wave.fired_at).all(axis=1)
    assert np.array_equal(fired_at[agree], seq.fired_at[agree][:, 1:5])


def test_identity_takes_one_iteration():
    n, B = 65, 3
    b = np.random.default_rng(3).uniform(-1, 1, (B, n))
    s, dev = device_solve(np.tile(np.eye(n), (B, 1, 1)), b)
    assert (dev.iters == 1).all() and (dev.reorth == 1).all() and (dev.status == gmres.STATUS_CONVERGED).all()
    # x = (|b| / h) * (b / |b|) with h = <v, v> of n rounded terms, |h - 1| <= n eps / 2, plus a handful of single roundings
    assert np.abs(dev.x - b).max() <= (n + 8) * np.finfo(float).eps


def test_initial_guess_that_solves_and_zero_right_hand_side():
    A, b = gc.systems(10, 10)
    x0 = np.linalg.solve(A, b[..., None])[..., 0]
    s, dev = device_solve(A, b, x0=x0)
    assert (dev.iters == 0).all() and same_bits(dev.x, x0) and (dev.status == gmres.STATUS_CONVERGED).all()
    assert np.isfinite(dev.err[:, 0]).all() and np.isnan(dev.err[:, 1:]).all() and (dev.reorth == 0).all()
    s, dev = device_solve(A, np.zeros_like(b), solver=s)
    assert (dev.iters == 0).all() and not dev.x.any() and (dev.err[:, 0] == 0).all() and (dev.status == gmres.STATUS_CONVERGED).all()


def test_a_singular_system_reports_non_finite_and_leaves_its_neighbours_alone():
    A, b = gc.systems(65, 5)
    _, clean = device_solve(A, b)
    A2, b2 = np.insert(A, 2, 0.0, axis=0), np.insert(b, 2, 1.0, axis=0)  # A = 0, b = ones in the middle of the batch
    _, dev = device_solve(A2, b2)
    assert dev.status[2] == gmres.STATUS_NON_FINITE and dev.iters[2] == 1 and np.isnan(dev.x[2]).all()
    keep = [0, 1, 3, 4, 5]
    for name in ("x", "err", "g", "H", "iters", "reorth", "status"):
        assert same_bits(getattr(dev, name)[keep], getattr(clean, name)), name


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
def test_device_arrays_with_a_transposed_image_give_the_host_paths_bits():
    import torch
    A, b = gc.systems(65, 5)
    x0 = np.random.default_rng(5).uniform(-1, 1, b.shape)
    _, host = device_solve(A, b, x0=x0, k_max=30)
    s = gmres.GmresBatch(65, 5, k_max_capacity=30)
    dA = torch.tensor(np.ascontiguousarray(A.transpose(0, 2, 1)), device="cuda")
    db, dx0 = torch.tensor(np.array(b), device="cuda"), torch.tensor(x0, device="cuda")
    s.set_system_device(dA, db, dx0, a_col_major=True)
    s.solve_device(k_max=30, stream=torch.cuda.current_stream())
    s.synchronize()
    dev = fields(s)
    for name in ("x", "err", "g", "H", "iters", "reorth", "status"):
        assert same_bits(getattr(dev, name), getattr(host, name)), name
    out = torch.zeros(5, 65, dtype=torch.float64, device="cuda")
    s.get_device(gmres.FIELD_X, out)
    assert same_bits(out.cpu().numpy(), host.x)
    # row-major device arrays go through the ingest kernel, as host arrays do; the host path with a_col_major takes the image as it is
    s.set_system_device(torch.tensor(np.array(A), device="cuda"), db, dx0)
    s.solve_device(k_max=30)
    s.synchronize()
    assert same_bits(s.x(), host.x)
    s.set_system(A.transpose(0, 2, 1), b, x0, a_col_major=True)
    s.solve_device(k_max=30)
    s.synchronize()
    assert same_bits(s.x(), host.x)


def test_second_solve_restarts_from_the_first(checker):
    A, b = gc.systems(100, 10)
    s, first = device_solve(A, b, k_max=20)
    x2 = s.solve(k_max=20)  # no new system: from the previous x
    second = fields(s)
    chk = {}
    for o in gc.ORDERS:
        r1 = checker.solve(A, b, k_max=20, order=o)
        chk[o] = (r1, checker.solve(A, b, x0=r1.x, k_max=20, order=o))
    assert same_bits(first.x, chk["wave"][0].x) and same_bits(x2, chk["wave"][1].x) and same_bits(second.err, chk["wave"][1].err)
    tol = gc.tolerance(chk["sequential"][1], chk["wave"][1], "restart")
    assert gc.rel_diff(x2, chk["sequential"][1].x) <= tol["X"] and gc.rel_diff(second.err, chk["sequential"][1].err) <= tol["ERR_LIST"]
    assert (second.err[:, 0] < first.err[:, 0]).all() and (second.status == gmres.STATUS_K_MAX).all()


def test_kept_basis_is_orthonormal(checker):
    """n = 100, re-orthogonalisation on, k_max = 60: the Gram matrix of the ITERS + 1 = 61 kept vectors is within 1e-10 of the identity.
    (With k_max = n the last of the n + 1 vectors is normalised rounding noise: 101 vectors of R^100 cannot be orthonormal.)"""
    A, b = gc.systems(100, 10)
    s, dev = device_solve(A, b, k_max=60, keep_basis=True)
    V = s.basis_
    assert V.shape == (10, 61, 100) and (dev.iters == 60).all()
    for i in range(10):
        assert np.abs(V[i] @ V[i].T - np.eye(61)).max() < 1e-10
    wave = checker.solve(A, b, k_max=60, order="wave")
    assert same_bits(V, wave.basis)
    s.keep_basis = False
    s.solve(k_max=60)
    with pytest.raises(ValueError):
        s.basis_


def test_one_handle_for_a_smaller_k_max_and_the_other_variant():
    A, b = gc.systems(63, 5)
    s, big = device_solve(A, b, k_max=63)
    for cfg in (dict(k_max=20), dict(k_max=40, make_triangular=False), dict(k_max=63, apply_reorth=False), dict(k_max=63)):
        _, reused = device_solve(A, b, solver=s, **cfg)
        _, fresh = device_solve(A, b, **cfg)
        for name in ("x", "err", "g", "H", "iters", "reorth", "status"):
            assert same_bits(getattr(reused, name), getattr(fresh, name)), (cfg, name)
    assert same_bits(reused.x, big.x)


def test_argument_checks_on_a_handle():
    from test_gmres_host_cpu import handle_argument_checks
    L = gmres.load()
    h = C.c_void_p()
    assert L.nmpc_hip_gmres_create(200, 3, 150, 0, C.byref(h)) == _capi.OK
    handle_argument_checks(L, h)
    assert L.nmpc_hip_gmres_destroy(h) == _capi.OK
    s = gmres.GmresBatch(200, 3, k_max_capacity=150)
    s.make_triangular_ = False
    A, b = gc.systems(200, 3)
    with pytest.raises(ValueError):
        s.solve(A, b, k_max=150)  # Householder above its bound
    with pytest.raises(ValueError):
        s.solve(A[:2], b[:2])
