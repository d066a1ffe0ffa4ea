"""The Matrix-Market text kernels must not use private memory: the f64 formatter (vtx_f64_text.h) holds its digits in registers and
writes them straight to the output — a digit buffer indexed at run time would land in scratch.  hipcc cross-compiles without a GPU: this
reads the compiler's own resource remarks for both instantiations (integral values / real values) of mtx_len_kernel and mtx_text_kernel
in the production build of vtx_ingest.hip."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_mtx_kernels_have_no_scratch():
    src = os.path.join(ROOT, "vartrix_amd", "csrc", "vtx_ingest.hip")
    with tempfile.TemporaryDirectory() as td:
        p = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-result", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(td, "i.o"), src],
                           capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", p.stderr)[1:]
    seen = set()
    for b in blocks:
        name = b.split()[0]
        m = re.search(r"mtx_(len|text)_kernelILb([01])E", name)
        if not m:
            continue
        vgprs = int(re.search(r"VGPRs: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        dyn = re.search(r"Dynamic Stack: (\w+)", b).group(1)
        print(name, "VGPRs", vgprs, "scratch", scratch, "occupancy", occ)
        assert scratch == 0 and dyn == "False" and vgprs <= 64 and occ >= 8, (name, vgprs, scratch, occ)
        seen.add(m.groups())
    assert seen == {("len", "0"), ("len", "1"), ("text", "0"), ("text", "1")}, seen
