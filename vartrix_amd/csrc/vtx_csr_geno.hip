// vtx_csr_geno.hip — every cell's reads tallied against the genotypes of pooled donors, one donor or a pair of donors at a time: a CSR
// (rows = cells, minor = variants), a table of one genotype byte per (variant, donor) and, for pairs, a list of donor pairs into, per
// (cell, hypothesis), the alt and ref reads and the informative entries by the hypothesis' class at the entry's variant — the donor's
// genotype class (4), or the pair's dosage class (g_a + g_b in 0 .. 4; 5: either donor without a call).  The donor label this step
// produces is what vtx_csr_group.hip takes; the CSR check is vtx_csr.hip's through vtxr_check.
//
// What it replaces: nothing in the reference, which writes the matrix and stops (src/main.rs:381-389).  Its users score cells against
// donors with the matrices (the demuxlet / vireo / souporcell step).  The per-lane rules are vtx_csr_geno_core.h's and, for a pair,
// vtx_csr_geno_pair_core.h's; the kernels are loads, those functions, and stores.
//
//   genotypes   csr_geno_check_kernel        lanes over the bytes of geno[n_minor * n_donors]: a byte that is neither 0, 1, 2 nor
//                                            VTX_GENO_NONE lowers the 64-bit word first_bad to its flat index (integer minimum: the
//                                            lowest offender, whatever the order of the lanes)
//   pairs       csr_geno_pair_check_kernel   lanes over the pairs: a pair with a donor >= n_donors lowers first_bad to its index
//   tally       csr_tally_kernel<H>          H = vtxr::DonorHyp or vtxr::PairHyp: the class count, the hypothesis count, what a live lane
//                                            loads per pass (nothing; its pair) and the class of an entry (one genotype byte; two).  One
//                                            wavefront per row, four rows per block.  Per pass of up to 64 hypotheses the wavefront is
//                                            64 / Dp sub-groups of Dp lanes (Dp: the power of two that holds the pass's hypotheses): a
//                                            sub-group's lanes load the same entry (indices, alt, ref), each live lane the byte(s) of its
//                                            hypothesis, and adds the entry to its 3 x CLASSES registers; after the row the sub-groups
//                                            are folded by __shfl_xor over the distances Dp .. 32 and sub-group 0 stores
//
// More than 64 hypotheses: the wavefront repeats its row once per 64 (at most GENO_MAX_PASSES / PAIR_MAX_PASSES times: vtx_csr_geno_max,
// vtx_csr_geno_pair_max).  Every loop is bounded by the hypothesis count and by the offsets of the checked CSR; a dead lane loads neither
// its pair nor a genotype byte.  No scratch, no LDS, no atomics in the tally, no zeroing pass: every output element, of rows without
// entries and of pairs of uncalled donors too, is stored exactly once by one lane.  Integer additions only, so the output is a function
// of the input alone.  The waves of a block never wait for one another.
#include <hip/hip_runtime.h>

#include "vtx_csr_geno_pair_core.h"
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

// lanes over n_pairs pairs (n_pairs <= PAIR_MAX: the grid covers them)
__global__ __launch_bounds__(kBlock) void csr_geno_pair_check_kernel(const uint32_t* __restrict__ pairs, uint32_t n_pairs, uint32_t n_donors,
                                                                     unsigned long long* __restrict__ first_bad) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_pairs) return;
    if (vtxr::pair_bad(pairs[2 * p], pairs[2 * p + 1], n_donors)) atomicMin(first_bad, (unsigned long long)p);
}

template <uint32_t N> __device__ __forceinline__ vtxr::ClassTally<N> tally_from(const vtxr::ClassTally<N>& t, uint32_t s) {      // the tally of lane ^ s
    vtxr::ClassTally<N> o;
#pragma unroll
    for (uint32_t g = 0; g < N; ++g) {
        o.sum_alt[g] = __shfl_xor((unsigned long long)t.sum_alt[g], (int)s, (int)vtxr::GENO_WAVE);
        o.sum_ref[g] = __shfl_xor((unsigned long long)t.sum_ref[g], (int)s, (int)vtxr::GENO_WAVE);
        o.n_obs[g] = __shfl_xor(t.n_obs[g], (int)s, (int)vtxr::GENO_WAVE);
    }
    return o;
}

// n_major wavefronts.  H: the hypotheses (vtxr::DonorHyp, vtxr::PairHyp); In / Out: the call's structs (vtx_device.h, include/vtx.h)
template <class H, class In, class Out> __global__ __launch_bounds__(kBlock) void csr_tally_kernel(In in, Out out) {
    constexpr uint32_t N = H::CLASSES;
    const uint32_t lane = threadIdx.x % vtxr::GENO_WAVE, wave = threadIdx.x / vtxr::GENO_WAVE;
    const uint64_t r = (uint64_t)blockIdx.x * kRows + wave;
    if (r >= in.n_major) return;                              // the whole wavefront
    const uint64_t begin = in.indptr[r], end = in.indptr[r + 1];
    const uint32_t n_hyp = H::count(in);
    for (uint32_t base = 0; base < n_hyp; base += vtxr::GENO_WAVE) {
        const uint32_t Dp = vtxr::pass_lanes(n_hyp, base), stride = vtxr::sub_groups(Dp);
        const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
        const bool live = vtxr::lane_live(base, me.d, n_hyp);
        typename H::Lane mine{};                              // a dead lane loads neither its pair nor a byte
        if (live) mine = H::load(in, base + me.d);
        vtxr::ClassTally<N> t = vtxr::tally_zero<N>();
        for (uint64_t k = begin + me.sub; k < end; k += stride) {
            const uint32_t v = in.indices[k], a = in.alt[k], f = in.ref[k];
            if (live) vtxr::tally_add(t, H::cls(in, mine, v, base + me.d), a, f);
        }
        for (uint32_t s = vtxr::fold_first(Dp); vtxr::fold_more(s); s = vtxr::fold_next(s)) {      // every lane takes every step
            const vtxr::ClassTally<N> o = tally_from(t, s);
            vtxr::tally_merge(t, o);
        }
        if (me.sub == 0 && live) {
            const uint64_t q = vtxr::tally_index<N>(r, n_hyp, base + me.d, 0);
#pragma unroll
            for (uint32_t g = 0; g < N; ++g) {
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
    hipLaunchKernelGGL((csr_tally_kernel<vtxr::DonorHyp, vtx_geno_in, vtx_geno_tally>), grid_rows(in.n_major), dim3(kBlock), 0, s, in, *out);
    return hipGetLastError();
}

hipError_t vtxr_geno_pair_check(const uint32_t* pairs, uint32_t n_pairs, uint32_t n_donors, uint64_t* first_bad, hipStream_t s) {
    if (!n_pairs) return hipSuccess;
    hipLaunchKernelGGL(csr_geno_pair_check_kernel, dim3((n_pairs + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pairs, n_pairs, n_donors,
                       (unsigned long long*)first_bad);
    return hipGetLastError();
}

hipError_t vtxr_geno_pair_tally(const vtx_geno_pair_in& in, const vtx_geno_pair_tally* out, hipStream_t s) {
    if (!in.n_major) return hipSuccess;
    hipLaunchKernelGGL((csr_tally_kernel<vtxr::PairHyp, vtx_geno_pair_in, vtx_geno_pair_tally>), grid_rows(in.n_major), dim3(kBlock), 0, s, in, *out);
    return hipGetLastError();
}

}
