// byteops_host.cpp — HOST build of the byte compare and the base codes of vartrix_amd/csrc/vtx_fast_core.h (eq8, kw_code8, kw_code): the
// portable path behind the header's device-only dot-product path.  tests/test_gpu_byteops.py compiles this file itself, runs the same
// vectors through it and through the device (libvtx_dev.so: vtxk_dev_byteops) and compares both with the definition.  Same output
// layout as the device export.  TEST INFRASTRUCTURE ONLY.
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../vartrix_amd/csrc/vtx_fast_core.h"

extern "C" void fastcore_byteops(const uint64_t* a, const uint64_t* b, uint32_t n, uint32_t* out) {
    for (uint32_t i = 0; i < n; ++i) {
        out[i] = vtxf::eq8(a[i], b[i]);
        out[n + i] = vtxf::kw_code8(a[i]);
        out[2 * n + i] = vtxf::kw_code((uint32_t)a[i], (uint32_t)(a[i] >> 32) & 0xffffu);
    }
}
