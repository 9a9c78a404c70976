"""Static guard on the code object of the C/GMRES wave kernels (no GPU needed: llvm-objdump on cgmres_wave_models.o, as
tests/test_cgmres_isa.py does for the lane kernels): three instantiations of each kernel, no scratch, the lists in LDS."""
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
    work = str(tmp_path_factory.mktemp("cgmres_wave_models"))
    local = os.path.join(work, "x.o")
    shutil.copy(os.path.join(hip_build.OBJ_DIR, "cgmres_wave_models.o"), local)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=work, check=True, capture_output=True)
    for co in [f for f in os.listdir(work) if "gfx950" in f]:
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "-C", os.path.join(work, co)], check=True, capture_output=True,
                              text=True).stdout
        name = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
            if m:
                name = re.sub(r"\(.*", "", m.group(1)).replace("nmpc_amd::hip::cgmres::", "").replace("nmpc_amd::", "").replace("void ", "")
                out[name] = []
            elif name is not None:
                parts = line.split()
                if len(parts) >= 2 and not parts[0].endswith(":"):
                    out[name].append(parts[0])
    return out


def test_three_instantiations_without_scratch_and_with_lds(kernels):
    for kind in ("cgmres_wave_run_kernel<", "cgmres_wave_control_input_kernel<"):
        mine = {k: v for k, v in kernels.items() if k.startswith(kind)}
        assert len(mine) == 3, (kind, sorted(kernels))
        for name, ins in mine.items():
            assert len(ins) > 100, name
            assert sum(1 for i in ins if i.startswith("scratch_")) == 0, name
            assert sum(1 for i in ins if i.startswith("ds_")) > 0, name
            # the lists are in LDS: no generic-address access that could hide one in HBM
            assert sum(1 for i in ins if i.startswith("flat_")) == 0, name


def test_the_lane_kernels_are_not_in_this_object(kernels):
    """tests/test_cgmres_isa.py counts the lane kernels per object; this translation unit adds none of them anywhere."""
    assert not any(k.startswith(("cgmres_run_kernel<", "cgmres_control_input_kernel<", "cgmres_setup_kernel<")) for k in kernels)
