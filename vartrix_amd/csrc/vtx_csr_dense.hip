// vtx_csr_dense.hip — a CSR times integer tables: per (row, column) the alt counts of the row's entries times the column's weight at
// the entry's variant in one table, plus the ref counts times the weight in another, summed modulo 2^64.  On a cells x variants CSR
// with tables of fixed-point log-probabilities it is every cell's log-likelihood under every cluster (the E-step of api.cluster_donors);
// on the variants x cells CSR with the cells' quantised responsibilities as the table it is every cluster's weighted alt or ref reads
// per variant (the M-step).  The CSR check is vtx_csr.hip's through vtxr_check; any int32 is a weight, so the tables have no check.
//
// What it replaces: nothing in the reference, which writes the matrix and stops (src/main.rs:381-389).  The per-lane rules are
// vtx_csr_dense_core.h's, the lane map and the fold vtx_csr_geno_core.h's; the kernel is those functions, the exchange and a store.
//
//   sum   csr_dense_kernel<ALT, REF>   which tables are there is the instantiation, never a test per entry.  One wavefront per row,
//                                      four rows per block.  Per pass of up to 64 columns the wavefront is 64 / Dp sub-groups of Dp
//                                      lanes (Dp: the power of two that holds the pass's columns): a sub-group's lanes load the same
//                                      entries, each live lane its own one or two table words per entry, DENSE_UNROLL entries per
//                                      trip; after the row the sub-groups are folded by __shfl_xor over the distances Dp .. 32 and
//                                      sub-group 0 stores
//
// More than 64 columns: the wavefront repeats its row once per 64 (at most DENSE_MAX_PASSES times: vtx_csr_dense_max).  Every loop is
// bounded by the column count and by the offsets of the checked CSR; a dead lane loads no table word.  No scratch, no LDS, no atomics,
// no zeroing pass: every output element, of rows without entries too, is stored exactly once by one lane.  Integer arithmetic only,
// wrapping: the output is a function of the input alone.  The waves of a block never wait for one another.
#include <hip/hip_runtime.h>

#include "vtx_csr_dense_core.h"
#include "vtx_device.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kRows = kBlock / vtxr::GENO_WAVE;         // rows (wavefronts) per block

// n_major wavefronts
template <bool ALT, bool REF> __global__ __launch_bounds__(kBlock) void csr_dense_kernel(vtx_dense_in in, int64_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x % vtxr::GENO_WAVE, wave = threadIdx.x / vtxr::GENO_WAVE;
    const uint64_t r = (uint64_t)blockIdx.x * kRows + wave;
    if (r >= in.n_major) return;                              // the whole wavefront
    const uint64_t begin = in.indptr[r], end = in.indptr[r + 1];
    for (uint32_t base = 0; base < in.n_cols; base += vtxr::GENO_WAVE) {
        const uint32_t Dp = vtxr::pass_lanes(in.n_cols, base), stride = vtxr::sub_groups(Dp);
        const vtxr::GenoLane me = vtxr::lane_map(lane, Dp);
        const bool live = vtxr::lane_live(base, me.d, in.n_cols);
        uint64_t acc = vtxr::dense_walk<ALT, REF>(in, begin, end, me.sub, stride, live, base + me.d);
        for (uint32_t s = vtxr::fold_first(Dp); vtxr::fold_more(s); s = vtxr::fold_next(s))      // every lane takes every step
            acc += __shfl_xor((unsigned long long)acc, (int)s, (int)vtxr::GENO_WAVE);
        if (me.sub == 0 && live) out[vtxr::dense_out_index(r, in.n_cols, base + me.d)] = (int64_t)acc;
    }
}

}  // namespace

extern "C" {

hipError_t vtxr_dense_sum(const vtx_dense_in& in, int64_t* out, hipStream_t s) {
    if (!in.n_major) return hipSuccess;
    const dim3 grid((uint32_t)(((uint64_t)in.n_major + kRows - 1) / kRows)), block(kBlock);
    if (in.w_alt && in.w_ref) hipLaunchKernelGGL((csr_dense_kernel<true, true>), grid, block, 0, s, in, out);
    else if (in.w_alt) hipLaunchKernelGGL((csr_dense_kernel<true, false>), grid, block, 0, s, in, out);
    else hipLaunchKernelGGL((csr_dense_kernel<false, true>), grid, block, 0, s, in, out);
    return hipGetLastError();
}

}
