"""The batched BoxQP solver (include/nmpc_hip_boxqp.h, nmpc_amd.boxqp.BoxQPBatch) on both of its kernels, against
oracle.ddp_numpy.boxqp (NumPy / SciPy) and oracle.boxqp_solve (the C++ oracle, which also counts factorisations).

  known answers   the five QPs of TestBoxQP.cpp:35-98 on lane and wave at n = 2, from zero (initial_x = NULL), from x_gt and from a
                  start outside the box: ||x - x_gt|| < 1e-6 (TestBoxQP.cpp:29); retval, iteration count, factorization_num and free
                  set equal oracle.boxqp_solve's.
  random cases    tests/boxqp_cases.py, 70 per size (one full wavefront plus six lanes on the lane kernel, seventy workgroups on the
                  wave kernel): lane at n in {1, 2, 3, 8, 16}, wave at n in {2, 16, 17, 33, 63, 64} (2: almost every lane idle; 16 / 17:
                  the lane kernel's limit and one past it; 17, 33, 63: odd n, rows only 8-byte aligned, idle lanes in the ballot and
                  the sums; 33: more than half a wave; 64: no idle lane, the full mask, 64 KB of LDS).  x inside the box, KKT as
                  check_kkt of tests/test_gpu_boxqp_known_answers.py, |x - x_oracle| <= 1e-9 (1 + max |x_oracle|), retval, ITER and
                  FREE_MASK equal on all 70 (tests/test_boxqp_host_cpu.py shows that no decision of the set is within rounding of its
                  threshold), OBJ the objective of the returned x, FACTOR's L L' = H[free, free].
  scaled twins    (H, g) * 2**30: x, KKT and FREE_MASK as above; retval 6 exactly where the oracle's is 6 and otherwise in {4, 5}.  The
                  4-versus-5 split and ITER are not compared: the reference itself flips them under a 1e-13 perturbation there.
  exits           max_iter = 1 (retval 1, the oracle's x after one iteration), H = -I and an H whose free block alone is indefinite
                  (retval -1, x the clamped start).
  trace           trace_capacity = 8: iter, factorization_num and clamped mask of every completed iteration equal a NumPy replay.
  plumbing        B = 1, 64, 65: solve_device on torch tensors, a reused handle, a repeated solve, get on the device — bit for bit.

A step-length exit (retval 2) has no constructed case: BoxQP.h:304-308 leaves only the inner loop, so a later exit overwrites the
code and no solve returns it.  retval -2 (search direction not a descent direction) has none either: with a positive definite free
block the Newton direction descends, and an indefinite one ends with -1 first.

Tolerances.  x and KKT: the bars of tests/test_gpu_boxqp_known_answers.py, two orders above the 9e-12 sensitivity of x to a 1e-13
perturbation of the data.  OBJ: |OBJ - f(x)| <= 1e-12 (|x.g| + 1/2 |x|'|H||x|): a sum of n + n^2 <= 4160 products carries at most
~4160 eps = 5e-13 of the sum of their magnitudes, whatever the order.  FACTOR: |L L' - H_ff| <= 1e-12 max |H_ff|: the backward error
of a Cholesky factorisation is of order n eps |L||L'| <= 64 * 1.1e-16 * n max |H_ff|."""
import numpy as np
import pytest

import boxqp_cases as bc
import oracle
from oracle import ddp_numpy as dn
from test_gpu_boxqp_known_answers import check_kkt

pytestmark = pytest.mark.gpu

LANE_SIZES = (1, 2, 3, 8, 16)
WAVE_SIZES = (2, 16, 17, 33, 63, 64)
KERNEL_SIZES = [("lane", n) for n in LANE_SIZES] + [("wave", n) for n in WAVE_SIZES]
FIELDS = ("x", "retval_", "iter", "factorization_num", "free_mask", "obj", "factor")


def make(n, B, kernel, **cfg):
    from nmpc_amd import boxqp
    qp = boxqp.BoxQPBatch(n, B)
    qp.setKernel(kernel)
    assert qp.kernelName() == "boxqp_%s_kernel" % kernel
    for k, v in cfg.items():
        setattr(qp.config(), k, v)
    return qp


def results(qp):
    out = {}
    for f in FIELDS:
        v = getattr(qp, f)
        out[f] = v() if callable(v) else v
    return out


def assert_same_bits(a, b):
    for f in FIELDS:
        assert a[f].tobytes() == b[f].tobytes(), f


def check_common(qp, cs, o, x):
    """Box, KKT, x against the oracle, FREE_MASK, OBJ and FACTOR for the solve just done on the cases cs."""
    B, n = cs.g.shape
    mask, obj, fac, ret = qp.free_mask(), qp.obj(), qp.factor(), qp.retval_
    assert np.array_equal(mask, o.free_mask), np.flatnonzero(mask != o.free_mask)
    for b in range(B):
        m = int(mask[b])
        check_kkt(x[b], cs.H[b], cs.g[b], cs.lower[b], cs.upper[b], m, n, False)
        assert np.abs(x[b] - o.x[b]).max() <= 1e-9 * (1 + np.abs(o.x[b]).max()), (b, np.abs(x[b] - o.x[b]).max())
        f = x[b] @ cs.g[b] + 0.5 * (x[b] @ (cs.H[b] @ x[b]))
        scale = np.abs(x[b]) @ np.abs(cs.g[b]) + 0.5 * (np.abs(x[b]) @ (np.abs(cs.H[b]) @ np.abs(x[b])))
        assert abs(obj[b] - f) <= 1e-12 * scale, (b, obj[b], f)
        free = [j for j in range(n) if m >> j & 1]
        nf = len(free)
        L = fac[b][:nf, :nf]
        rest = fac[b].copy()
        rest[:nf, :nf] = 0
        assert not rest.any() and not np.triu(L, 1).any(), b  # zeros outside the packed lower triangle
        if nf and ret[b] != -1:
            Hf = cs.H[b][np.ix_(free, free)]
            assert np.abs(L @ L.T - Hf).max() <= 1e-12 * np.abs(Hf).max(), (b, np.abs(L @ L.T - Hf).max())


# ---- known answers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["zero", "x_gt", "outside"])
@pytest.mark.parametrize("kernel", ["lane", "wave"])
def test_reference_known_answers(kernel, start):
    g, lo, up, x_gt = (np.array([q[i] for q in bc.QP_CASES]) for i in range(4))
    B = len(bc.QP_CASES)
    H = np.tile(bc.H_QP, (B, 1, 1))
    x0 = {"zero": None, "x_gt": x_gt, "outside": np.where(np.arange(2 * B).reshape(B, 2) % 3 == 0, lo - 3.0, up + 3.0)}[start]
    qp = make(2, B, kernel)
    x = qp.solve(H, g, lo, up, x0)
    assert (np.linalg.norm(x - x_gt, axis=1) < 1e-6).all(), x
    for b in range(B):
        want = oracle.boxqp_solve(bc.H_QP, g[b], lo[b], up[b], np.zeros(2) if x0 is None else x0[b])
        got = (qp.retval(b), int(qp.iter()[b]), int(qp.factorization_num()[b]), qp.freeIdxs(b))
        assert got == (want.retval, want.iter, want.factorization_num, [int(j) for j in want.free_idxs]), (b, got, want)
        assert qp.retstr(b) == {4: "Improvement smaller than tolerance", 5: "Gradient norm smaller than tolerance",
                                6: "All dimensions are clamped"}[want.retval]


# ---- random cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,n", KERNEL_SIZES)
def test_random_cases_against_the_oracle(kernel, n):
    cs, o = bc.cases(n), bc.oracle(n)
    qp = make(n, bc.COUNT, kernel)
    x = qp.solve(cs.H, cs.g, cs.lower, cs.upper, cs.x0)
    print("max |x - x_oracle| / (1 + max |x_oracle|):", (np.abs(x - o.x).max(axis=1) / (1 + np.abs(o.x).max(axis=1))).max())
    assert np.array_equal(qp.retval_, o.retval), np.flatnonzero(qp.retval_ != o.retval)
    assert np.array_equal(qp.iter(), o.iters), np.flatnonzero(qp.iter() != o.iters)
    check_common(qp, cs, o, x)
    # the C++ oracle counts factorisations too: the first ten cases (two of every kind)
    for b in range(10):
        want = oracle.boxqp_solve(cs.H[b], cs.g[b], cs.lower[b], cs.upper[b], cs.x0[b])
        assert (int(qp.factorization_num()[b]), qp.freeIdxs(b)) == (want.factorization_num, [int(j) for j in want.free_idxs]), b


@pytest.mark.parametrize("kernel,n", KERNEL_SIZES)
def test_scaled_twins(kernel, n):
    cs, o = bc.cases(n).scaled(), bc.oracle(n, scaled=True)
    qp = make(n, bc.COUNT, kernel)
    x = qp.solve(cs.H, cs.g, cs.lower, cs.upper, cs.x0)
    ret = qp.retval_
    print("retval 4 / 5 / 6:", [(ret == r).sum() for r in (4, 5, 6)], "oracle:", [(o.retval == r).sum() for r in (4, 5, 6)])
    assert np.array_equal(ret == 6, o.retval == 6) and np.isin(ret, (4, 5, 6)).all(), ret
    check_common(qp, cs, o, x)


# ---- exits -----------------------------------------------------------------------------------------------------------------
EXIT_KERNEL_SIZES = [("lane", 3), ("wave", 3), ("wave", 17)]


@pytest.mark.parametrize("kernel,n", EXIT_KERNEL_SIZES)
def test_max_iter_one(kernel, n):
    cs = bc.cases(n)
    o = bc.solve_oracle(cs, max_iter=1)
    assert (o.retval == 1).any()
    qp = make(n, bc.COUNT, kernel, max_iter=1)
    x = qp.solve(cs.H, cs.g, cs.lower, cs.upper, cs.x0)
    assert np.array_equal(qp.retval_, o.retval) and np.array_equal(qp.iter(), o.iters) and (qp.iter() == 1).all()
    assert np.array_equal(qp.free_mask(), o.free_mask)
    assert (np.abs(x - o.x).max(axis=1) <= 1e-9 * (1 + np.abs(o.x).max(axis=1))).all()


@pytest.mark.parametrize("kernel,n", EXIT_KERNEL_SIZES)
def test_not_positive_definite(kernel, n):
    """H = -I, and an H whose free block alone is indefinite: entry 0 starts on its lower limit with the gradient pointing out of the
    box, so it is clamped, and the block of the others has a positive first pivot and a negative second one."""
    rng = np.random.default_rng(n)
    B = 6
    lo, up = -rng.uniform(0.5, 1.5, (B, n)), rng.uniform(0.5, 1.5, (B, n))
    x0 = rng.normal(size=(B, n)) * 1.5
    x0[:, n - 1] = 0.0  # at least one entry strictly inside the box: not all clamped
    g = np.zeros((B, n))
    H = np.tile(-np.eye(n), (B, 1, 1))
    for b in range(B // 2, B):  # the indefinite free block
        H[b] = np.eye(n)
        H[b][1, 1], H[b][2, 2] = 2.0, 1.0
        H[b][1, 2] = H[b][2, 1] = 3.0  # 2 * 1 - 9 < 0: the second pivot of the free block is negative
        g[b][0] = 50.0
        x0[b][0] = lo[b][0] - 1.0
        x0[b][1:] = 0.5 * (lo[b][1:] + up[b][1:])  # strictly inside: free whatever the gradient
    start = np.maximum(np.minimum(x0, up), lo)
    qp = make(n, B, kernel)
    x = qp.solve(H, g, lo, up, x0)
    for b in range(B):
        want = dn.boxqp(H[b], g[b], lo[b], up[b], x0=x0[b])
        assert want.retval == -1 and qp.retval(b) == -1 and qp.retstr(b) == "Hessian is not positive definite"
        assert np.array_equal(x[b], start[b]) and np.array_equal(x[b], want.x)
        assert int(qp.iter()[b]) == want.iters == 1 and int(qp.factorization_num()[b]) == 0
        assert qp.freeIdxs(b) == [int(j) for j in want.free_idxs]
        if b >= B // 2:
            assert qp.freeIdxs(b) == list(range(1, n))


# ---- trace -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,n", [("lane", 8), ("wave", 17), ("wave", 64)])
def test_trace(kernel, n):
    cs, o = bc.cases(n), bc.oracle(n)
    cap = 8
    qp = make(n, bc.COUNT, kernel, trace_capacity=cap)
    x = qp.solve(cs.H, cs.g, cs.lower, cs.upper, cs.x0)
    with_trace = results(qp)
    tr = qp.trace()
    assert tr.shape == (bc.COUNT, cap)
    completed = 0
    for b in range(bc.COUNT):
        rows, ret, it = bc.replay(cs.H[b], cs.g[b], cs.lower[b], cs.upper[b], cs.x0[b])
        assert (ret, it) == (o.retval[b], o.iters[b]) == (qp.retval(b), int(qp.iter()[b]))
        assert tr[b][0]["iter"] == 0 and tr[b][0]["factorization_num"] == 0 and tr[b][0]["clamped_mask"] == 0  # the initial entry
        for r_iter, r_nfac, r_mask, _ in rows:
            if r_iter < cap:
                got = tr[b][r_iter]
                assert (got["iter"], got["factorization_num"], int(got["clamped_mask"])) == (r_iter, r_nfac, r_mask), (b, r_iter, got)
                completed += 1
        if it < cap:  # the entry of the iteration that left the loop: iter only; nothing beyond it
            assert tr[b][it]["iter"] == it and tr[b][it]["clamped_mask"] == 0 and tr[b][it]["obj"] == 0
            assert not tr[b][it + 1:].view(np.uint64).any()
        if b < 3:  # the mirror's list form
            assert [e["iter"] for e in qp.traceDataList(b)] == list(range(min(cap, it + 1)))
    assert completed > bc.COUNT
    # capacity 0: no trace, the same results
    qp0 = make(n, bc.COUNT, kernel, trace_capacity=0)
    x_0 = qp0.solve(cs.H, cs.g, cs.lower, cs.upper, cs.x0)
    assert qp0.trace().shape == (bc.COUNT, 0) and np.array_equal(x, x_0)
    assert_same_bits(with_trace, results(qp0))


# ---- plumbing --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64, 65])
@pytest.mark.parametrize("kernel,n", [("lane", 8), ("wave", 17)])
def test_plumbing(kernel, n, B):
    import torch
    from nmpc_amd import boxqp
    cs = bc.cases(n)
    first = [np.ascontiguousarray(a[:B]) for a in (cs.H, cs.g, cs.lower, cs.upper, cs.x0)]
    other = [np.ascontiguousarray(a[::-1][:B]) for a in (cs.H, cs.g, cs.lower, cs.upper, cs.x0)]
    qp = make(n, B, kernel)
    qp.solve(*first)
    r_first = results(qp)
    o = bc.oracle(n)
    assert np.array_equal(r_first["retval_"], o.retval[:B]) and np.array_equal(r_first["free_mask"], o.free_mask[:B])
    # the same solve again: the same bits
    qp.solve(*first)
    assert_same_bits(r_first, results(qp))
    # other data on the same handle: the bits of a fresh handle
    qp.solve(*other)
    r_other = results(qp)
    fresh = make(n, B, kernel)
    fresh.solve(*other)
    assert_same_bits(r_other, results(fresh))
    assert not np.array_equal(r_other["x"], r_first["x"]) or B == 1
    # solve_device on torch tensors: the bits of solve; on the solver's own stream and on a torch stream
    dev = [torch.tensor(a, dtype=torch.float64, device="cuda") for a in first]
    for stream in (None, torch.cuda.Stream()):
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        torch.cuda.synchronize()
        qp.solve_device(*dev, stream=stream)
        qp.synchronize()
        assert_same_bits(r_first, results(qp))
        assert qp.lastSolveMs() > 0
    # get on the device
    xd = torch.zeros((B, n), dtype=torch.float64, device="cuda")
    qp.get_device(boxqp.FIELD_X, xd)
    assert np.array_equal(xd.cpu().numpy(), r_first["x"])
    with pytest.raises(ValueError):
        qp.get_device(boxqp.FIELD_X, torch.zeros(B * n + 1, dtype=torch.float64, device="cuda"))
    # initial_x = None is a start from zero
    qp.solve_device(*dev[:4])
    qp.synchronize()
    fresh.solve(*first[:4], np.zeros((B, n)))
    assert_same_bits(results(qp), results(fresh))


def test_kernel_choice_round_trip():
    from nmpc_amd import boxqp
    for n, B in ((1, 1), (2, 65536), (3, 65535), (4, 65536), (8, 256), (16, 1024), (17, 4), (64, 2)):
        qp = boxqp.BoxQPBatch(n, B)
        auto = qp.kernelName()
        # the rule of nmpc_hip_boxqp.h: a pure function of (var_dim, batch)
        lane = n <= boxqp.AUTO_LANE_MAX_DIM and B >= boxqp.AUTO_LANE_MIN_BATCH
        assert auto == ("boxqp_lane_kernel" if lane else "boxqp_wave_kernel"), (n, B, auto)
        qp.setKernel("wave")
        assert qp.kernelName() == "boxqp_wave_kernel"
        if n <= boxqp.LANE_MAX_DIM:
            qp.setKernel("lane")
            assert qp.kernelName() == "boxqp_lane_kernel"
        else:
            with pytest.raises(ValueError):
                qp.setKernel("lane")
            assert qp.kernelName() == "boxqp_wave_kernel"
        qp.setKernel(None)
        assert qp.kernelName() == auto
        with pytest.raises(ValueError):
            qp.setKernel("tile")
    # the automatic choice is a function of (var_dim, batch) alone
    assert boxqp.BoxQPBatch(8, 256).kernelName() == boxqp.BoxQPBatch(8, 256).kernelName()
    with pytest.raises(RuntimeError):
        boxqp.BoxQPBatch(3, 2).x()  # no solve yet
