"""The donor and doublet tally kernels must not use private memory: the twelve / eighteen numbers of a lane are registers, selected by
predicated additions.  hipcc cross-compiles without a GPU: this reads the compiler's own resource remarks for every kernel of the
production build of vtx_csr_geno.hip — the two check kernels and the two instantiations of csr_tally_kernel, told apart by the policy in
the mangled name.  Scratch, the dynamic stack, LDS and the tallies' VGPRs are asserted; the register table is printed (DESIGN.md §4.13
records it)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {"csr_geno_check_kernel": ("csr_geno_check_kernel",), "csr_geno_pair_check_kernel": ("csr_geno_pair_check_kernel",),
           "csr_tally_kernel<DonorHyp>": ("csr_tally_kernel", "DonorHyp"), "csr_tally_kernel<PairHyp>": ("csr_tally_kernel", "PairHyp")}
MAX_VGPRS = {"csr_tally_kernel<DonorHyp>": 70, "csr_tally_kernel<PairHyp>": 85}      # the hand-written kernels' that the template replaced


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_csr_geno_kernels_have_no_scratch_no_dynamic_stack_and_no_lds():
    src = os.path.join(ROOT, "vartrix_amd", "csrc", "vtx_csr_geno.hip")
    with tempfile.TemporaryDirectory() as td:
        p = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-result", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(td, "c.o"), src],
                           capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", p.stderr)[1:]
    seen = set()
    for b in blocks:
        name = b.split()[0]
        mine = [k for k, parts in KERNELS.items() if all(part in name for part in parts)]
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
        assert scratch == 0 and dyn == "False" and lds == 0, (name, scratch, dyn, lds)      # the tally is registers: no tile, no LDS atomics
        assert vgprs <= MAX_VGPRS.get(mine[0], vgprs), (name, vgprs)
        seen.add(mine[0])
    assert seen == set(KERNELS), set(KERNELS) - seen
