// vtx_csr_group.hip — pseudobulk on the device: a CSR summed per group of columns.  (A file of its own beside vtx_csr_ops.hip, whose
// row statistics it computes per (row, group) pair; the CSR check is vtx_csr.hip's through vtxr_check.)
//
// What it replaces: nothing in the reference, which writes the matrix and stops (src/main.rs:381-389).  Its users take a label per cell
// (cluster, donor, clone, sample) and fold variants x cells into variants x groups.  The per-lane rules are vtx_csr_group_core.h's; the
// kernels are loads, those functions, and stores.
//
//   labels   csr_group_check_kernel   one lane per column: a label that is neither < n_groups nor VTX_GROUP_NONE lowers the word
//                                     first_bad to its column (integer minimum: the lowest offending column, whatever the order)
//   count    csr_group_count_kernel   one wavefront per row, four rows per block; the wavefront's tile is a BITMAP of GROUP_WINDOW bits
//                                     in LDS (only which groups occur matters here): lanes walk the row with stride 64, load
//                                     group[indices[k]] and set the bit; the popcount of the tile is the row's number of entries.
//                                     An exclusive sum (hipcub, in place) turns the counts into pos[], pos[n_major] = nnz_out
//   fill     csr_group_fill_kernel    the same walk over a tile of GROUP_WINDOW x seven accumulators (40 bytes a group, 40 KiB a block):
//                                     LDS atomic additions, u32 and u64; then the tile is swept 64 bins at a time and the non-empty
//                                     bins go to pos[r] + rank, rank from a ballot and a popcount prefix carried over the steps and
//                                     the windows
//
// n_groups > GROUP_WINDOW: the wavefront repeats its row once per window of GROUP_WINDOW groups, in ascending order (at most
// GROUP_MAX_WINDOWS times: vtx_csr_group_max).  Every loop is bounded by n_groups and by the offsets of the checked CSR.  No scratch, no
// global atomics in the count and the fill, no zeroing pass over global memory; integer additions only, so the output is a function of
// the input alone.  The waves of a block never wait for one another: there is no block barrier, each wave orders its own LDS traffic.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "vtx_csr_group_core.h"
#include "vtx_device.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kRows = kBlock / vtxr::GROUP_WAVE;        // rows (wavefronts) per block

inline dim3 grid_for(uint64_t lanes) { return dim3((uint32_t)((lanes + kBlock - 1) / kBlock)); }
inline dim3 grid_rows(uint32_t n_major) { return dim3((uint32_t)(((uint64_t)n_major + 1 + kRows - 1) / kRows)); }      // row n_major: the last offset

// The lanes of ONE wavefront have written LDS that other lanes of the same wavefront read next: its LDS instructions complete in the
// order they were issued, so all that is needed is that the compiler keeps that order.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// n_minor lanes
__global__ __launch_bounds__(kBlock) void csr_group_check_kernel(const uint32_t* __restrict__ group, uint32_t n_minor, uint32_t n_groups,
                                                                 uint32_t* __restrict__ first_bad) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_minor) return;
    if (vtxr::label_bad(group[j], n_groups)) atomicMin(first_bad, (uint32_t)j);
}

// (n_major + 1) wavefronts: counts[r] = the groups that occur in row r; counts[n_major] = 0 (the exclusive sum puts nnz_out there)
__global__ __launch_bounds__(kBlock) void csr_group_count_kernel(vtx_group_in in, uint32_t* __restrict__ counts) {
    __shared__ vtxr::GroupBits tiles[kRows];
    const uint32_t lane = threadIdx.x % vtxr::GROUP_WAVE, wave = threadIdx.x / vtxr::GROUP_WAVE;
    const uint64_t r = (uint64_t)blockIdx.x * kRows + wave;
    if (r > in.n_major) return;                               // the whole wavefront
    uint32_t n = 0;
    const uint64_t begin = r < in.n_major ? in.indptr[r] : 0ull, end = r < in.n_major ? in.indptr[r + 1] : 0ull;
    vtxr::GroupBits& t = tiles[wave];
    if (begin != end) {
        for (uint32_t base = 0; base < in.n_groups; base += vtxr::GROUP_WINDOW) {
            const uint32_t bins = vtxr::window_bins(in.n_groups, base);
            if (lane < vtxr::GROUP_WINDOW / 32) vtxr::bits_zero(t, lane);
            wave_sync();
            for (uint64_t k = begin + lane; k < end; k += vtxr::GROUP_WAVE) {
                uint32_t b;
                if (vtxr::window_slot(in.group[in.indices[k]], base, bins, &b)) vtxr::bits_set(t, b);
            }
            wave_sync();
            n += vtxr::bits_count(t);
            wave_sync();
        }
    }
    if (lane == 0) counts[r] = n;
}

// (n_major + 1) wavefronts over pos[] = the exclusive sum of the counts: wavefront r writes indptr_out[r] and the entries of row r
__global__ __launch_bounds__(kBlock) void csr_group_fill_kernel(vtx_group_in in, const uint32_t* __restrict__ pos, uint64_t* __restrict__ indptr_out,
                                                                uint32_t* __restrict__ indices_out, vtx_csr_stats out) {
    __shared__ vtxr::GroupTile tiles[kRows];
    const uint32_t lane = threadIdx.x % vtxr::GROUP_WAVE, wave = threadIdx.x / vtxr::GROUP_WAVE;
    const uint64_t r = (uint64_t)blockIdx.x * kRows + wave;
    if (r > in.n_major) return;                               // the whole wavefront
    const uint32_t first = pos[r];
    if (lane == 0) indptr_out[r] = first;
    if (r == in.n_major) return;
    const uint64_t begin = in.indptr[r], end = in.indptr[r + 1];
    if (begin == end) return;
    vtxr::GroupTile& t = tiles[wave];
    uint32_t rank = 0;                                        // entries of this row already stored: the same on every lane
    for (uint32_t base = 0; base < in.n_groups; base += vtxr::GROUP_WINDOW) {
        const uint32_t bins = vtxr::window_bins(in.n_groups, base);
        for (uint32_t b = lane; b < bins; b += vtxr::GROUP_WAVE) vtxr::tile_zero(t, b);
        wave_sync();
        for (uint64_t k = begin + lane; k < end; k += vtxr::GROUP_WAVE) {
            uint32_t b;
            if (vtxr::window_slot(in.group[in.indices[k]], base, bins, &b)) vtxr::tile_add(t, b, in.alt[k], in.ref[k], in.unk[k]);
        }
        wave_sync();
        for (uint32_t b0 = 0; b0 < bins; b0 += vtxr::GROUP_WAVE) {      // every lane takes every step: the ballot is the whole wavefront's
            const uint32_t b = b0 + lane;
            const bool full = b < bins && t.n_entries[b] != 0u;
            const uint64_t ballot = __ballot(full);
            if (full) {
                const uint64_t q = (uint64_t)first + rank + vtxr::step_rank(ballot, lane);      // < pos[r + 1]: the count saw the same bins
                const vtxr::RowStats s = vtxr::tile_read(t, b);
                if (indices_out) indices_out[q] = base + b;
                if (out.n_entries) out.n_entries[q] = s.n_entries;
                if (out.n_alt) out.n_alt[q] = s.n_alt;
                if (out.n_ref) out.n_ref[q] = s.n_ref;
                if (out.n_both) out.n_both[q] = s.n_both;
                if (out.sum_alt) out.sum_alt[q] = s.sum_alt;
                if (out.sum_ref) out.sum_ref[q] = s.sum_ref;
                if (out.sum_unk) out.sum_unk[q] = s.sum_unk;
            }
            rank += vtxr::popcount64(ballot);
        }
        wave_sync();
    }
}

}  // namespace

extern "C" {

hipError_t vtxr_group_check(const uint32_t* group, uint32_t n_minor, uint32_t n_groups, uint32_t* first_bad, hipStream_t s) {
    if (!n_minor) return hipSuccess;
    hipLaunchKernelGGL(csr_group_check_kernel, grid_for(n_minor), dim3(kBlock), 0, s, group, n_minor, n_groups, first_bad);
    return hipGetLastError();
}

hipError_t vtxr_group_count(const vtx_group_in& in, uint32_t* pos, void* temp, size_t temp_bytes, hipStream_t s) {
    hipLaunchKernelGGL(csr_group_count_kernel, grid_rows(in.n_major), dim3(kBlock), 0, s, in, pos);
    if (hipError_t e = hipGetLastError()) return e;
    return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, pos, (size_t)in.n_major + 1, s);
}

hipError_t vtxr_group_fill(const vtx_group_in& in, const uint32_t* pos, uint64_t* indptr_out, uint32_t* indices_out, const vtx_csr_stats* out,
                           hipStream_t s) {
    hipLaunchKernelGGL(csr_group_fill_kernel, grid_rows(in.n_major), dim3(kBlock), 0, s, in, pos, indptr_out, indices_out, *out);
    return hipGetLastError();
}

}
