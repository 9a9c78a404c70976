"""Static guard on the code object of the FMPC problem types with time-varying dimensions (fmpc_models_dynamic.o; no GPU needed:
llvm-objdump).  Their kernels keep every small array in registers — a register array indexed at run time would show up as scratch_
instructions — and they run the lane Riccati kernel only: the matrix-core, fused and tail kernels are fixed-dimension (N <= 4, M = 1)."""
import os
import re
import shutil
import subprocess

import pytest

from nmpc_amd import build as hip_build

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump not in this image")
    hip_build.build()
    out = {}
    work = str(tmp_path_factory.mktemp("fmpc_models_dynamic"))
    local = os.path.join(work, "x.o")
    shutil.copy(os.path.join(hip_build.OBJ_DIR, "fmpc_models_dynamic.o"), local)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=work, check=True, capture_output=True)
    for co in [f for f in os.listdir(work) if "gfx950" in f]:
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "-C", os.path.join(work, co)], check=True, capture_output=True,
                              text=True).stdout
        name = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
            if m:
                name = m.group(1).replace("nmpc_amd::hip::", "").replace("nmpc_amd::", "").replace("void ", "")
                out[name] = []
            elif name is not None:
                parts = line.split()
                if len(parts) >= 2 and not parts[0].endswith(":"):
                    out[name].append(parts[0])
    return out


def test_vertical_kernels_exist_and_issue_no_scratch_instructions(kernels):
    want = ("fmpc_dims_kernel<FmpcProblemVerticalMotion>", "fmpc_init_complementary_dims_kernel<FmpcProblemVerticalMotion>",
            "fmpc_coeff_dims_kernel<FmpcProblemVerticalMotion>", "fmpc_delta_dims_kernel<FmpcProblemVerticalMotion>",
            "fmpc_line_search_dims_kernel<FmpcProblemVerticalMotion>", "fmpc_plant_dims_kernel<FmpcProblemVerticalMotion>",
            "fmpc_riccati_kernel<2, 2>")
    for w in want:
        hits = [k for k in kernels if k.startswith(w)]
        assert hits, (w, sorted(kernels))
    for name, ins in kernels.items():
        assert len(ins) > 10, name
        assert sum(1 for i in ins if i.startswith("scratch_")) == 0, name


def test_no_fixed_dimension_only_kernel_is_instantiated_for_vertical(kernels):
    for name in kernels:
        for kind in ("fmpc_riccati_quad_kernel", "fmpc_riccati_fused_kernel", "fmpc_tail_kernel"):
            assert not name.startswith(kind), name
        # nor the fixed-dimension variants of the per-problem kernels
        for kind in ("fmpc_coeff_kernel<", "fmpc_delta_kernel<", "fmpc_line_search_kernel<", "fmpc_plant_kernel<",
                     "fmpc_init_complementary_kernel<"):
            assert not name.startswith(kind), name
