"""The heterogeneous queue's interface, without a GPU: the library exports nmpc_hip_ddp_solve_stream_ex, the C header declares it and
its inputs struct, and DDPSolverBatch.solveStream takes the queue's problem objects and limits (tests/test_gpu_stream_mixed.py runs
them on the device)."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_the_heterogeneous_stream_entry_point():
    from nmpc_amd import _capi
    L = _capi.load()
    assert "nmpc_hip_ddp_solve_stream_ex" in _capi.EXPORTS
    assert getattr(L, "nmpc_hip_ddp_solve_stream_ex") is not None
    assert getattr(L, "nmpc_hip_ddp_solve_stream") is not None  # (the shared-object entry point keeps its name)
    names = [f[0] for f in _capi.StreamInputs._fields_]
    assert names == ["t0", "x0", "u_init", "params", "bytes_per_instance", "lower", "upper"]


def test_the_library_holds_the_own_problem_resumable_instantiations():
    """<Problem, constrained, own problem, fan-out, resumable> of the quad kernel and <Problem, constrained, own problem, resumable> of the
    two-wave kernel, for constrained in {false, true}: what a heterogeneous queue and the ragged schedule of a handle with per-instance
    problem objects launch (the kernels' host-side handles in the library's symbol table)."""
    import subprocess

    from nmpc_amd import build as hip_build
    names = subprocess.run(["nm", "-C", hip_build.build()], check=True, capture_output=True, text=True).stdout
    cartpole = "nmpc_amd::DDPProblemCartPoleT<double>"
    for con in ("false", "true"):
        assert f"nmpc_amd::hip::ddp_solve_quad_kernel<{cartpole}, {con}, true, true, true>(" in names
        assert f"nmpc_amd::hip::ddp_solve_tpi2w_kernel<{cartpole}, {con}, true, true>(" in names


def test_the_header_declares_the_call_and_its_inputs():
    text = open(os.path.join(ROOT, "include", "nmpc_hip_ddp.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    flat = " ".join(code.split())
    assert ("int nmpc_hip_ddp_solve_stream_ex(nmpc_hip_ddp_handle h, int n_instances, const nmpc_hip_ddp_stream_inputs * in, int span);"
            in flat)
    m = re.search(r"typedef struct nmpc_hip_ddp_stream_inputs \{(.*?)\} nmpc_hip_ddp_stream_inputs;", flat)
    assert m, "struct nmpc_hip_ddp_stream_inputs"
    members = [" ".join(d.split()) for d in m.group(1).split(";") if d.strip()]
    assert members == ["const double * t0", "const double * x0", "const double * u_init", "const void * params",
                       "size_t bytes_per_instance", "const double * lower", "const double * upper"]
    # the old entry point keeps its signature, and streamed solves are no longer tied to one problem object
    assert "int nmpc_hip_ddp_solve_stream(nmpc_hip_ddp_handle h, int n_instances, const double * t0, const double * x0, const double * u_init, int span);" in flat
    assert "shared problem object and limits" not in " ".join(text.split())


def test_solve_stream_takes_problems_and_input_limits():
    import nmpc_amd
    sig = inspect.signature(nmpc_amd.DDPSolverBatch.solveStream)
    assert list(sig.parameters)[:5] == ["self", "current_t", "current_x", "initial_u_list", "span"]
    assert sig.parameters["problems"].default is None and sig.parameters["input_limits"].default is None
    assert sig.parameters["span"].default == 0
