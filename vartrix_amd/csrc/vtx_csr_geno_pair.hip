// vtx_csr_geno_pair.hip — every cell's reads tallied against PAIRS of pooled donors: a CSR (rows = cells, minor = variants), the table of
// one genotype byte per (variant, donor) that vtx_csr_geno.hip reads, and a list of donor pairs into, per (cell, pair), the alt and ref
// reads and the informative entries by the pair's dosage class (g_a + g_b in 0 .. 4; 5: either donor without a call).  The two-donor
// hypotheses beside vtx_csr_geno.hip's one-donor ones; the CSR check is vtx_csr.hip's through vtxr_check, the table's is vtxr_geno_check.
//
// What it replaces: nothing in the reference, which writes the matrix and stops (src/main.rs:381-389).  The per-lane rules are
// vtx_csr_geno_pair_core.h's (and, for the lane map and the fold distances, vtx_csr_geno_core.h's); the kernels are loads, those
// functions, and stores.
//
//   pairs   csr_geno_pair_check_kernel   lanes over the pairs: a pair with a donor >= n_donors lowers the 64-bit word first_bad to its index
//                                        (integer minimum: the lowest offender, whatever the order of the lanes)
//   tally   csr_geno_pair_tally_kernel   one wavefront per row, four rows per block.  Per pass of up to 64 pairs the wavefront is 64 / Dp
//                                        sub-groups of Dp lanes (Dp: the power of two that holds the pass's pairs): a live lane loads its
//                                        (a, b) once, a sub-group's lanes load the same entry (indices, alt, ref) and each live lane the two
//                                        bytes of its donors, and adds the entry to the eighteen registers of its pair; after the row the
//                                        sub-groups are folded by __shfl_xor over the distances Dp .. 32 and sub-group 0 stores
//
// n_pairs > 64: the wavefront repeats its row once per 64 pairs (at most PAIR_MAX_PASSES times: vtx_csr_geno_pair_max).  Every loop is
// bounded by n_pairs and by the offsets of the checked CSR.  No scratch, no LDS, no atomics in the tally, no zeroing pass: every output
// element, of rows without entries and of pairs of uncalled donors too, is stored exactly once by one lane.  Integer additions only, so
// the output is a function of the input alone.  The waves of a block never wait for one another.
#include <hip/hip_runtime.h>

#include "vtx_csr_geno_pair_core.h"
#include "vtx_device.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kRows = kBlock / vtxr::GENO_WAVE;         // rows (wavefronts) per block

inline dim3 grid_rows(uint32_t n_major) { return dim3((uint32_t)(((uint64_t)n_major + kRows - 1) / kRows)); }

// lanes over n_pairs pairs (n_pairs <= PAIR_MAX: the grid covers them)
__global__ __launch_bounds__(kBlock) void csr_geno_pair_check_kernel(const uint32_t* __restrict__ pairs, uint32_t n_pairs, uint32_t n_donors,
                                                                     unsigned long long* __restrict__ first_bad) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pairs) return;
    if (vtxr::pair_bad(pairs[2 * p], pairs[2 * p + 1], n_donors)) atomicMin(first_bad, (unsigned long long)p);
}

__device__ __forceinline__ vtxr::PairTally tally_from(const vtxr::PairTally& t, uint32_t s) {      // the tally of lane ^ s
    vtxr::PairTally o;
#pragma unroll
    for (uint32_t c = 0; c < vtxr::PAIR_CLASSES; ++c) {
        o.sum_alt[c] = __shfl_xor((unsigned long long)t.sum_alt[c], (int)s, (int)vtxr::GENO_WAVE);
        o.sum_ref[c] = __shfl_xor((unsigned long long)t.sum_ref[c], (int)s, (int)vtxr::GENO_WAVE);
        o.n_obs[c] = __shfl_xor(t.n_obs[c], (int)s, (int)vtxr::GENO_WAVE);
    }
    return o;
}

// n_major wavefronts
__global__ __launch_bounds__(kBlock) void csr_geno_pair_tally_kernel(vtx_geno_pair_in in, vtx_geno_pair_tally out) {
    const uint32_t lane = threadIdx.x % vtxr::GENO_WAVE, wave = threadIdx.x / vtxr::GENO_WAVE;
    const uint64_t r = (uint64_t)blockIdx.x * kRows + wave;
    if (r >= in.n_major) return;                              // the whole wavefront
    const uint64_t begin = in.indptr[r], end = in.indptr[r + 1];
    for (uint32_t base = 0; base < in.n_pairs; base += vtxr::GENO_WAVE) {
        const uint32_t Dp = vtxr::pass_lanes(in.n_pairs, base), stride = vtxr::sub_groups(Dp);
        const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
        const bool live = vtxr::lane_live(base, me.d, in.n_pairs);
        uint32_t da = 0, db = 0;                              // a dead lane loads neither its pair nor a byte
        if (live) { da = in.pairs[2 * (base + me.d)]; db = in.pairs[2 * (base + me.d) + 1]; }
        vtxr::PairTally t = vtxr::pair_tally_zero();
        for (uint64_t k = begin + me.sub; k < end; k += stride) {
            const uint32_t v = in.indices[k], a = in.alt[k], f = in.ref[k];
            if (live)
                vtxr::pair_tally_add(t, vtxr::pair_class(in.geno[vtxr::pair_geno_index(v, in.n_donors, da)], in.geno[vtxr::pair_geno_index(v, in.n_donors, db)]), a, f);
        }
        for (uint32_t s = vtxr::fold_first(Dp); vtxr::fold_more(s); s = vtxr::fold_next(s)) {      // every lane takes every step
            const vtxr::PairTally o = tally_from(t, s);
            vtxr::pair_tally_merge(t, o);
        }
        if (me.sub == 0 && live) {
            const uint64_t q = vtxr::pair_tally_index(r, in.n_pairs, base + me.d, 0);
#pragma unroll
            for (uint32_t c = 0; c < vtxr::PAIR_CLASSES; ++c) {
                if (out.sum_alt) out.sum_alt[q + c] = t.sum_alt[c];
                if (out.sum_ref) out.sum_ref[q + c] = t.sum_ref[c];
                if (out.n_obs) out.n_obs[q + c] = t.n_obs[c];
            }
        }
    }
}

}  // namespace

extern "C" {

hipError_t vtxr_geno_pair_check(const uint32_t* pairs, uint32_t n_pairs, uint32_t n_donors, uint64_t* first_bad, hipStream_t s) {
    if (!n_pairs) return hipSuccess;
    hipLaunchKernelGGL(csr_geno_pair_check_kernel, dim3((n_pairs + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pairs, n_pairs, n_donors,
                       (unsigned long long*)first_bad);
    return hipGetLastError();
}

hipError_t vtxr_geno_pair_tally(const vtx_geno_pair_in& in, const vtx_geno_pair_tally* out, hipStream_t s) {
    if (!in.n_major) return hipSuccess;
    hipLaunchKernelGGL(csr_geno_pair_tally_kernel, grid_rows(in.n_major), dim3(kBlock), 0, s, in, *out);
    return hipGetLastError();
}

}
