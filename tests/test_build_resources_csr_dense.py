"""The CSR x integer-table kernel must not use private memory or LDS: a lane's state is its 64-bit sum, and the entries and table words of
one trip of the unrolled walk are registers indexed by literals.  hipcc cross-compiles without a GPU: this reads the compiler's own
resource remarks for the three instantiations of csr_dense_kernel in the production build of vtx_csr_dense.hip, told apart by the
template arguments in the mangled name.  Scratch, the dynamic stack, LDS and the VGPRs are asserted — the VGPR bound is the figure of the
form that is kept (DESIGN.md §4.14 records the table): an assertion against register growth, not a target."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# csr_dense_kernel<ALT, REF>: Lb1ELb1E, Lb1ELb0E, Lb0ELb1E in the mangled name
KERNELS = {"csr_dense_kernel<true, true>": "Lb1ELb1E", "csr_dense_kernel<true, false>": "Lb1ELb0E", "csr_dense_kernel<false, true>": "Lb0ELb1E"}
MAX_VGPRS = {"csr_dense_kernel<true, true>": 74, "csr_dense_kernel<true, false>": 52, "csr_dense_kernel<false, true>": 52}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_csr_dense_kernels_have_no_scratch_no_dynamic_stack_and_no_lds():
    src = os.path.join(ROOT, "vartrix_amd", "csrc", "vtx_csr_dense.hip")
    with tempfile.TemporaryDirectory() as td:
        p = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-result", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(td, "c.o"), src],
                           capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", p.stderr)[1:]
    seen = set()
    for b in blocks:
        name = b.split()[0]
        mine = [k for k, part in KERNELS.items() if "csr_dense_kernel" in name and part in name]
        if not mine:
            continue
        sgprs = int(re.search(r"SGPRs: (\d+)", b).group(1))
        vgprs = int(re.search(r"VGPRs: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        dyn = re.search(r"Dynamic Stack: (\w+)", b).group(1)
        print(mine[0], "SGPRs", sgprs, "VGPRs", vgprs, "scratch", scratch, "LDS", lds, "occupancy", occ)
        assert len(mine) == 1 and mine[0] not in seen, (name, mine)
        assert scratch == 0 and dyn == "False" and lds == 0, (name, scratch, dyn, lds)
        assert vgprs <= MAX_VGPRS[mine[0]], (name, vgprs)
        seen.add(mine[0])
    assert seen == set(KERNELS), set(KERNELS) - seen
