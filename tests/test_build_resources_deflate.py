"""Resource figures of the gzip path's kernels (vtx_deflate.hip), from the compiler's own remarks on the production source; hipcc
cross-compiles without a GPU.

mtx_deflate_kernel is one wavefront per workgroup, and what bounds its residency is LDS: the 16 KiB hash table, 4 KiB of CRC tables
and about 5 KiB of code tables, 25 KiB in all.  At most 26 KiB is asserted: six workgroups then fit a CU's 160 KiB (the issue's floor
is two: 80 KiB), i.e. at most two wavefronts on a SIMD — so a VGPR count up to 256 costs no residency.  The bound asserted is tighter,
192 VGPRs and no AGPRs: the encoder keeps a step's 64-bit token bits, its hash, candidate and match length per lane and needs 160
today, and a step towards 256 would mean that per-lane tables have moved into registers or spill lanes.  Occupancy as the
compiler reports it must be at least 2.  No scratch and no dynamic stack: every table the encoder indexes at run time lies in LDS.
mtx_gz_compact_kernel is a copy: no LDS, at most 64 VGPRs, full occupancy (8)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_deflate_kernels_resources():
    src = os.path.join(ROOT, "vartrix_amd", "csrc", "vtx_deflate.hip")
    with tempfile.TemporaryDirectory() as td:
        p = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-result", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(td, "d.o"), src],
                           capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    seen = set()
    for b in re.split(r"remark: Function Name: ", p.stderr)[1:]:
        name = b.split()[0]
        m = re.search(r"(mtx_deflate_kernel|mtx_gz_compact_kernel)", name)
        if not m:
            continue
        vgprs = int(re.search(r"\bVGPRs: (\d+)", b).group(1))
        agprs = int(re.search(r"AGPRs: (\d+)", b).group(1))
        vspill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        dyn = re.search(r"Dynamic Stack: (\w+)", b).group(1)
        print(name, "VGPRs", vgprs, "scratch", scratch, "occupancy", occ, "LDS", lds)
        assert scratch == 0 and dyn == "False" and lds <= 80 * 1024, (name, scratch, dyn, lds)
        if m.group(1) == "mtx_deflate_kernel":
            assert lds <= 26 * 1024 and vgprs <= 192 and agprs == 0 and vspill == 0 and occ >= 2, (name, vgprs, agprs, vspill, occ, lds)
        else:
            assert lds == 0 and vgprs <= 64 and occ >= 8, (name, vgprs, occ, lds)
        seen.add(m.group(1))
    assert seen == {"mtx_deflate_kernel", "mtx_gz_compact_kernel"}, seen
