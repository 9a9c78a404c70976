"""Static guard on the batched FMPC step code object (no GPU needed): fmpc_step_capi.o is compiled for gfx950 and fmpc_step_wave_kernel
keeps everything that is indexed at run time in LDS or HBM (include/nmpc_amd/hip/fmpc_step_kernels.hpp), so its private segment
(scratch) is empty and no vector register is spilled.  Reads the code object's metadata only (the AMDGPU notes); DESIGN.md 2.12 quotes
the register figures printed here."""
import os
import re
import shutil
import subprocess

import pytest

from nmpc_amd import build as hip_build

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{kernel name: {metadata key: value}} of the gfx950 code object in fmpc_step_capi.o."""
    for tool in ("llvm-objdump", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(tool + " not in this image")
    hip_build.build()
    work = str(tmp_path_factory.mktemp("fmpc_step_capi"))
    local = os.path.join(work, "x.o")
    shutil.copy(os.path.join(hip_build.OBJ_DIR, "fmpc_step_capi.o"), local)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=work, check=True, capture_output=True)
    objects = [f for f in os.listdir(work) if "gfx950" in f]
    assert len(objects) == 1, os.listdir(work)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(work, objects[0])], check=True, capture_output=True,
                           text=True).stdout
    assert "amdgcn-amd-amdhsa--gfx950" in notes
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        block = ".agpr_count:" + block
        meta = {k: v.strip() for k, v in re.findall(r"\.(\w+):\s+(\S+)", block)}
        out[re.sub(r"\.kd$", "", meta["symbol"]).strip("'")] = meta
    return out


def test_fmpc_step_wave_kernel_uses_no_scratch(kernels):
    names = [k for k in kernels if "fmpc_step_wave_kernel" in k]
    assert len(names) == 1, sorted(kernels)
    meta = kernels[names[0]]
    print("fmpc_step_wave_kernel: vgpr %s, agpr %s, sgpr %s (%s moved to VGPR lanes), static LDS %s B, scratch %s B, wavefront %s, "
          "max workgroup %s" % (meta["vgpr_count"], meta["agpr_count"], meta["sgpr_count"], meta.get("sgpr_spill_count", "?"),
                                meta["group_segment_fixed_size"], meta["private_segment_fixed_size"], meta["wavefront_size"],
                                meta["max_flat_workgroup_size"]))
    assert int(meta["private_segment_fixed_size"]) == 0
    assert meta.get("uses_dynamic_stack", "false") == "false"
    assert int(meta["vgpr_spill_count"]) == 0
    assert int(meta["wavefront_size"]) == 64 and int(meta["max_flat_workgroup_size"]) == 64
    assert int(meta["group_segment_fixed_size"]) == 0  # all of its LDS is the dynamic request of the launch
