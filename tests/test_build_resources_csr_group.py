"""The pseudobulk kernels must not use private memory, and two blocks of the fill must fit a CU's 160 KiB of LDS.  hipcc cross-compiles
without a GPU: this reads the compiler's own resource remarks for every kernel of the production build of vtx_csr_group.hip.  Scratch, the
dynamic stack and the LDS of a block are asserted; the register table is printed (DESIGN.md §4.11 records it)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {"csr_group_check_kernel", "csr_group_count_kernel", "csr_group_fill_kernel"}
LDS_LIMIT = 80 * 1024


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_csr_group_kernels_have_no_scratch_and_two_blocks_fit_a_cu():
    src = os.path.join(ROOT, "vartrix_amd", "csrc", "vtx_csr_group.hip")
    with tempfile.TemporaryDirectory() as td:
        p = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-result", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(td, "c.o"), src],
                           capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", p.stderr)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        mine = [k for k in KERNELS if k in name]
        if not mine:
            continue                                       # hipcub's scan kernels: not this project's
        sgprs = int(re.search(r"SGPRs: (\d+)", b).group(1))
        vgprs = int(re.search(r"VGPRs: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        dyn = re.search(r"Dynamic Stack: (\w+)", b).group(1)
        print(mine[0], "SGPRs", sgprs, "VGPRs", vgprs, "scratch", scratch, "LDS", lds, "occupancy", occ)
        assert scratch == 0 and dyn == "False", (name, scratch, dyn)
        assert lds <= LDS_LIMIT, (name, lds)
        seen[mine[0]] = lds
    assert set(seen) == KERNELS, KERNELS - set(seen)
    assert seen["csr_group_fill_kernel"] > 0               # the tile is LDS, not registers or global memory
