// maskops_host.cpp — HOST build of the mask and bit helpers of vartrix_amd/csrc/vtx_fast_core.h that band_diag_kernel is built from
// (m_range, ones_below, closure_count, t3_hits, harmless_item4, m_bit, closure_scan): the portable path.  tests/test_gpu_maskops.py compiles this file itself, runs the same
// vectors through it and through the device (libvtx_dev.so: vtxk_dev_maskops, ops 0 - 5 and 7) and compares both with the definitions.  Same
// layouts as the device export.  TEST INFRASTRUCTURE ONLY.
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../vartrix_amd/csrc/vtx_fast_core.h"

static_assert(vtxf::NW == 4, "the layouts below carry four words per mask");

struct HostMatchList {
    const uint32_t* p;
    static constexpr int XS = 8;
    static constexpr uint32_t YM = 0xffu;
    uint32_t s(int k) const { return p[k]; }
};

extern "C" int fastcore_maskops(uint32_t op, const void* in, uint32_t n, void* out) {
    for (uint32_t i = 0; i < n; ++i) {
        if (op == 0) {
            const int lo = ((const int32_t*)in)[2 * i], hi = ((const int32_t*)in)[2 * i + 1];
            const vtxf::M192 a = vtxf::m_range<3>(lo, hi), b = vtxf::m_range<4>(lo, hi);
            for (int k = 0; k < 4; ++k) {
                ((uint64_t*)out)[8 * (size_t)i + k] = a.w[k];
                ((uint64_t*)out)[8 * (size_t)i + 4 + k] = b.w[k];
            }
        } else if (op == 1) {
            ((uint64_t*)out)[i] = vtxf::ones_below(((const int32_t*)in)[i]);
        } else if (op == 2) {
            uint32_t lo = 0, hi = 0;
            vtxf::closure_count(((const uint32_t*)in)[i], lo, hi);
            ((uint32_t*)out)[2 * i] = lo; ((uint32_t*)out)[2 * i + 1] = hi;
        } else if (op == 3) {
            ((uint32_t*)out)[i] = vtxf::t3_hits(((const uint64_t*)in)[2 * i], (uint32_t)((const uint64_t*)in)[2 * i + 1]);
        } else if (op == 4) {
            const int32_t* p = (const int32_t*)in + 8 * (size_t)i;
            const uint32_t pw4[4] = {(uint32_t)p[0], (uint32_t)p[1], (uint32_t)p[2], (uint32_t)p[3]};
            struct { const uint32_t* w; uint32_t at(int k) const { return w[k]; } } pl{pw4};
            int r = 0;
            while (r < 4 && pw4[r] != 0u) ++r;
            ((uint32_t*)out)[2 * i] = vtxf::harmless_item4(pw4, p[4], p[5], p[6], p[7]);
            ((uint32_t*)out)[2 * i + 1] = vtxf::harmless_item(pl, r, p[4], p[5], p[6], p[7]);
        } else if (op == 5) {
            const uint64_t* p = (const uint64_t*)in + 5 * (size_t)i;
            vtxf::M192 a;
            for (int k = 0; k < vtxf::NW; ++k) a.w[k] = p[k];
            ((uint32_t*)out)[i] = vtxf::m_bit(a, (int)p[4]) ? 1u : 0u;
        } else if (op == 7) {
            const uint32_t* p = (const uint32_t*)in + 48 * (size_t)i;
            ((int32_t*)out)[i] = vtxf::closure_scan((int)p[1], (int)p[0], HostMatchList{p + 6}, (uint64_t)p[2] | ((uint64_t)p[3] << 32), (int)p[4], (int)p[5]);
        } else {
            return 1;
        }
    }
    return 0;
}
