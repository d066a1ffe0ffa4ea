// The kernel of vartrix_amd/csrc/vtx_csr_dense.hip with the lanes as loops and the exchange between lanes as array reads, over
// vtx_csr_dense_core.h (the lane's walk itself is the header's dense_walk: the device runs the same function): what harness.cpp (a
// shared object for ctypes) and main.cpp (a stand-alone program, also built under sanitizers) both run.  Host code only.
#ifndef CSRDENSE_LANES_H
#define CSRDENSE_LANES_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../vartrix_amd/csrc/vtx_csr_dense_core.h"

namespace csrdense {

constexpr uint32_t WAVE = vtxr::GENO_WAVE;

// what the kernel takes (vtx_dense_in of vtx_device.h, which a host build cannot include)
struct SumIn {
    const uint64_t* indptr; uint32_t n_major; const uint32_t* indices; const uint32_t *alt, *ref; const int32_t *w_alt, *w_ref; uint32_t n_cols;
};

// csr_dense_kernel<ALT, REF>.  stores (n_major * n_cols bytes, may be NULL) counts the lanes that store each output element.
template <bool ALT, bool REF> inline void sum_rows(const SumIn& in, int64_t* out, uint8_t* stores) {
    for (uint64_t r = 0; r < in.n_major; ++r) {
        const uint64_t begin = in.indptr[r], end = in.indptr[r + 1];
        for (uint32_t base = 0; base < in.n_cols; base += WAVE) {
            const uint32_t Dp = vtxr::pass_lanes(in.n_cols, base), stride = vtxr::sub_groups(Dp);
            uint64_t acc[WAVE];
            memset(acc, 0xA5, sizeof acc);                        // registers hold what the last pass left
            for (uint32_t lane = 0; lane < WAVE; ++lane) {
                const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
                acc[lane] = vtxr::dense_walk<ALT, REF>(in, begin, end, me.sub, stride, vtxr::lane_live(base, me.d, in.n_cols), base + me.d);
            }
            for (uint32_t s = vtxr::fold_first(Dp); vtxr::fold_more(s); s = vtxr::fold_next(s)) {
                uint64_t o[WAVE];
                for (uint32_t lane = 0; lane < WAVE; ++lane) o[lane] = acc[lane ^ s];      // __shfl_xor: what the other lane held BEFORE the step
                for (uint32_t lane = 0; lane < WAVE; ++lane) acc[lane] += o[lane];
            }
            for (uint32_t lane = 0; lane < WAVE; ++lane) {
                const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
                if (me.sub != 0 || !vtxr::lane_live(base, me.d, in.n_cols)) continue;
                const uint64_t q = vtxr::dense_out_index(r, in.n_cols, base + me.d);
                if (stores && stores[q] < 255) ++stores[q];
                out[q] = (int64_t)acc[lane];
            }
        }
    }
}

// vtxr_dense_sum: which tables are there picks the instantiation
inline void sum(const SumIn& in, int64_t* out, uint8_t* stores) {
    if (in.w_alt && in.w_ref) sum_rows<true, true>(in, out, stores);
    else if (in.w_alt) sum_rows<true, false>(in, out, stores);
    else sum_rows<false, true>(in, out, stores);
}

}  // namespace csrdense
#endif
