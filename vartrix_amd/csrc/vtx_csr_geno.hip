// vtx_csr_geno.hip — every cell's reads tallied against the genotypes of pooled donors: a CSR (rows = cells, minor = variants) and a
// table of one genotype byte per (variant, donor) into, per (cell, donor) pair, the alt and ref reads and the informative entries by
// the donor's genotype class.  (A file of its own beside vtx_csr_group.hip, whose donor label this step produces; the CSR check is
// vtx_csr.hip's through vtxr_check.)
//
// What it replaces: nothing in the reference, which writes the matrix and stops (src/main.rs:381-389).  Its users score cells against
// donors with the matrices (the demuxlet / vireo / souporcell step).  The per-lane rules are vtx_csr_geno_core.h's; the kernels are
// loads, those functions, and stores.
//
//   genotypes   csr_geno_check_kernel   lanes over the bytes of geno[n_minor * n_donors]: a byte that is neither 0, 1, 2 nor
//                                       VTX_GENO_NONE lowers the 64-bit word first_bad to its flat index (integer minimum: the lowest
//                                       offender, whatever the order of the lanes)
//   tally       csr_geno_tally_kernel   one wavefront per row, four rows per block.  Per pass of up to 64 donors the wavefront is 64 / Dp
//                                       sub-groups of Dp lanes (Dp: the power of two that holds the pass's donors): a sub-group's lanes
//                                       load the same entry (indices, alt, ref) and Dp consecutive genotype bytes, each lane adds the
//                                       entry to the twelve registers of its donor; after the row the sub-groups are folded by
//                                       __shfl_xor over the distances Dp .. 32 and sub-group 0 stores
//
// n_donors > 64: the wavefront repeats its row once per 64 donors (at most GENO_MAX_PASSES times: vtx_csr_geno_max).  Every loop is
// bounded by n_donors and by the offsets of the checked CSR.  No scratch, no LDS, no atomics in the tally, no zeroing pass: every output
// element, of rows without entries too, is stored exactly once by one lane.  Integer additions only, so the output is a function of the
// input alone.  The waves of a block never wait for one another.
#include <hip/hip_runtime.h>

#include "vtx_csr_geno_core.h"
#include "vtx_device.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kRows = kBlock / vtxr::GENO_WAVE;         // rows (wavefronts) per block
constexpr uint32_t kCheckBlocks = 1u << 20;                  // the check's grid at most: its lanes stride over longer tables

inline dim3 grid_rows(uint32_t n_major) { return dim3((uint32_t)(((uint64_t)n_major + kRows - 1) / kRows)); }

// lanes over n_bytes = n_minor * n_donors bytes
__global__ __launch_bounds__(kBlock) void csr_geno_check_kernel(const uint8_t* __restrict__ geno, uint64_t n_bytes,
                                                                unsigned long long* __restrict__ first_bad) {
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_bytes; i += step)
        if (vtxr::geno_bad(geno[i])) atomicMin(first_bad, (unsigned long long)i);
}

__device__ __forceinline__ vtxr::GenoTally tally_from(const vtxr::GenoTally& t, uint32_t s) {      // the tally of lane ^ s
    vtxr::GenoTally o;
#pragma unroll
    for (uint32_t g = 0; g < vtxr::GENO_CLASSES; ++g) {
        o.sum_alt[g] = __shfl_xor((unsigned long long)t.sum_alt[g], (int)s, (int)vtxr::GENO_WAVE);
        o.sum_ref[g] = __shfl_xor((unsigned long long)t.sum_ref[g], (int)s, (int)vtxr::GENO_WAVE);
        o.n_obs[g] = __shfl_xor(t.n_obs[g], (int)s, (int)vtxr::GENO_WAVE);
    }
    return o;
}

// n_major wavefronts
__global__ __launch_bounds__(kBlock) void csr_geno_tally_kernel(vtx_geno_in in, vtx_geno_tally out) {
    const uint32_t lane = threadIdx.x % vtxr::GENO_WAVE, wave = threadIdx.x / vtxr::GENO_WAVE;
    const uint64_t r = (uint64_t)blockIdx.x * kRows + wave;
    if (r >= in.n_major) return;                              // the whole wavefront
    const uint64_t begin = in.indptr[r], end = in.indptr[r + 1];
    for (uint32_t base = 0; base < in.n_donors; base += vtxr::GENO_WAVE) {
        const uint32_t Dp = vtxr::pass_lanes(in.n_donors, base), stride = vtxr::sub_groups(Dp);
        const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
        const bool live = vtxr::lane_live(base, me.d, in.n_donors);
        vtxr::GenoTally t = vtxr::tally_zero();
        for (uint64_t k = begin + me.sub; k < end; k += stride) {
            const uint32_t v = in.indices[k], a = in.alt[k], f = in.ref[k];
            if (live) vtxr::tally_add(t, vtxr::geno_class(in.geno[vtxr::geno_index(v, in.n_donors, base, me.d)]), a, f);
        }
        for (uint32_t s = vtxr::fold_first(Dp); vtxr::fold_more(s); s = vtxr::fold_next(s)) {      // every lane takes every step
            const vtxr::GenoTally o = tally_from(t, s);
            vtxr::tally_merge(t, o);
        }
        if (me.sub == 0 && live) {
            const uint64_t q = vtxr::tally_index(r, in.n_donors, base + me.d, 0);
#pragma unroll
            for (uint32_t g = 0; g < vtxr::GENO_CLASSES; ++g) {
                if (out.sum_alt) out.sum_alt[q + g] = t.sum_alt[g];
                if (out.sum_ref) out.sum_ref[q + g] = t.sum_ref[g];
                if (out.n_obs) out.n_obs[q + g] = t.n_obs[g];
            }
        }
    }
}

}  // namespace

extern "C" {

hipError_t vtxr_geno_check(const uint8_t* geno, uint64_t n_bytes, uint64_t* first_bad, hipStream_t s) {
    if (!n_bytes) return hipSuccess;
    const uint64_t blocks = (n_bytes + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(csr_geno_check_kernel, dim3((uint32_t)(blocks < kCheckBlocks ? blocks : kCheckBlocks)), dim3(kBlock), 0, s, geno, n_bytes,
                       (unsigned long long*)first_bad);
    return hipGetLastError();
}

hipError_t vtxr_geno_tally(const vtx_geno_in& in, const vtx_geno_tally* out, hipStream_t s) {
    if (!in.n_major) return hipSuccess;
    hipLaunchKernelGGL(csr_geno_tally_kernel, grid_rows(in.n_major), dim3(kBlock), 0, s, in, *out);
    return hipGetLastError();
}

}
