"""Static guard on the C/GMRES code objects (no GPU needed: llvm-objdump on the library's objects).  The kernels keep one instance
per lane with every run-time-indexed array in HBM (include/nmpc_amd/hip/cgmres_kernels.hpp): a spill or a register array indexed at
run time would show up as scratch_ instructions."""
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
    for src in ("cgmres_capi.o", "cgmres_models.o"):
        work = str(tmp_path_factory.mktemp(src[:-2]))
        local = os.path.join(work, "x.o")
        shutil.copy(os.path.join(hip_build.OBJ_DIR, src), local)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=work, check=True, capture_output=True)
        for co in [f for f in os.listdir(work) if "gfx950" in f]:
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "-C", os.path.join(work, co)], check=True, capture_output=True,
                                  text=True).stdout
            name = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
                if m:
                    name = re.sub(r"\(.*", "", m.group(1)).replace("nmpc_amd::hip::cgmres::", "").replace("nmpc_amd::", "")
                    name = name.replace("void ", "")
                    out[name] = []
                elif name is not None:
                    parts = line.split()
                    if len(parts) >= 2 and not parts[0].endswith(":"):
                        out[name].append(parts[0])
    return out


def test_cgmres_kernels_issue_no_scratch_instructions(kernels):
    cg = {k: v for k, v in kernels.items() if k.startswith("cgmres_") and "fill" not in k}
    kinds = ("cgmres_setup_kernel<", "cgmres_run_kernel<", "cgmres_control_input_kernel<", "cgmres_model_eval_kernel<")
    for kind in kinds:
        assert sum(1 for k in cg if k.startswith(kind)) == 3, (kind, sorted(cg))
    assert any(k.startswith("cgmres_gmres_dense_kernel") for k in cg)
    for name, ins in cg.items():
        assert len(ins) > 10, name
        assert sum(1 for i in ins if i.startswith("scratch_")) == 0, name
