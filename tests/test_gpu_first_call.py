"""The first call on a fresh handle goes through the paths that allocate device memory and copy into it at once: GMRES's staging
copy of a row-major host A (and the x and b that create allocated), BoxQP's staging copies of solve()'s host arrays.  Its results are
those of the same call made again on the same handle, bit for bit.

tests/test_gpu_boxqp_batch.py::test_plumbing makes the same first / second comparison for BoxQP at other shapes (lane n = 8 and wave
n = 17, B = 1, 64, 65); tests/test_gpu_gmres.py compares a host solve with a device one, on two handles, but repeats neither."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(fields: dict) -> dict:
    return {k: (v.shape, v.dtype.str, v.tobytes()) for k, v in fields.items()}


def test_gmres_first_set_system_and_solve_on_a_fresh_handle():
    import torch
    from nmpc_amd import gmres
    n, B = 10, 3
    rng = np.random.default_rng(20)
    A = rng.uniform(-1, 1, (B, n, n)) + n * np.eye(n)  # row-major, from the host: staged and transposed on the device
    b = rng.uniform(-1, 1, (B, n))
    x0 = rng.uniform(-1, 1, (B, n))

    def fields(s):
        return _bits(dict(x=s.x(), iters=s.iters(), reorth=s.reorth(), status=s.status(), err_list=s.err_list_, g=s.g_, H=s.H_))

    s = gmres.GmresBatch(n, B)
    s.set_system(A, b, x0)
    s.solve()
    first = fields(s)
    s.set_system(A, b, x0)
    s.solve()
    assert fields(s) == first
    assert (s.status() == gmres.STATUS_CONVERGED).all()  # (the comparison is not one of failures)

    other = gmres.GmresBatch(n, B)  # a second fresh handle, given the transposed image as device arrays: read in place
    dev = [torch.tensor(np.ascontiguousarray(a), device="cuda") for a in (A.transpose(0, 2, 1), b, x0)]
    other.set_system_device(*dev, a_col_major=True)
    other.solve()
    assert fields(other) == first


@pytest.mark.parametrize("kernel", ["lane", "wave"])
def test_boxqp_first_host_solve_on_a_fresh_handle(kernel):
    from nmpc_amd import boxqp
    n, B = 8, 3
    rng = np.random.default_rng(21)
    M = rng.uniform(-1, 1, (B, n, n))
    H = M @ M.transpose(0, 2, 1) + np.eye(n)
    g = rng.uniform(-2, 2, (B, n))
    lower, upper = -rng.uniform(0.1, 1, (B, n)), rng.uniform(0.1, 1, (B, n))
    initial_x = rng.uniform(-1, 1, (B, n))  # non-zero, some of it outside the box

    def fields(qp):
        return _bits(dict(x=qp.x(), retval=qp.retval_, iter=qp.iter(), factorization_num=qp.factorization_num(),
                          free_mask=qp.free_mask(), obj=qp.obj(), factor=qp.factor()))

    qp = boxqp.BoxQPBatch(n, B)
    qp.setKernel(kernel)
    assert qp.kernelName() == "boxqp_%s_kernel" % kernel
    qp.solve(H, g, lower, upper, initial_x)
    first = fields(qp)
    qp.solve(H, g, lower, upper, initial_x)
    assert fields(qp) == first
    assert (qp.retval_ >= 0).all() and qp.free_mask().any()
