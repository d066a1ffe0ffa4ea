// vtx_csr_ops.hip — summarise and filter a CSR on the device: the seven statistics of every row, and the stable selection of rows and
// columns by byte masks.  (A file of its own beside vtx_csr.hip, whose check kernel it uses through vtxr_check.)
//
// What it replaces: nothing in the reference, which writes the matrix and stops (src/main.rs:381-389).  The consumers of that file
// count per variant the cells with alt / ref support and drop the variants too few cells inform before anything else; with the CSR
// already on the card (vtx_device_csr, vtx_csr_transpose) both steps run there.  The per-lane rules are vtx_csr_ops_core.h's; the
// kernels are loads, those functions, and stores.
//
//   statistics   csr_row_stats_kernel<G>   G lanes per row (G from vtxr::group_lanes: mean row length / 8), 64 / G rows per wavefront;
//                                          the group walks its row with stride G (coalesced), accumulates in registers and folds with
//                                          lane shuffles inside the wavefront; one lane stores.  No atomics, no zeroing, no LDS.
//   selection    csr_mask_flags_kernel     1 / 0 per column and per row of the masks, n + 1 words each (the last one 0); an exclusive
//                                          sum (hipcub, in place) turns them into minor_map / major_map — the new numbers, and the
//                                          kept count in the last word
//                csr_keep_flags_kernel     one lane per entry: its row (binary search in indptr) and column kept?  nnz + 1 words, scanned
//                                          in place into pos[]
//                csr_select_offsets_kernel one lane per row (+ 1): indptr_out[major_map[r]] = pos[indptr[r]] for the kept rows and the end
//                csr_select_ids_kernel     optional: the source row / column of every kept one
//                csr_select_place_kernel   one lane per entry, no per-row loop: a kept entry (pos[k + 1] != pos[k]) goes to pos[k] with
//                                          its new column number and its payload words, bit for bit
//
// Integer work only; nothing here depends on the order in which lanes run.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "vtx_csr_ops_core.h"
#include "vtx_device.h"

namespace {

constexpr uint32_t kBlock = 256;

__device__ __forceinline__ uint64_t lane_id() { return (uint64_t)blockIdx.x * kBlock + threadIdx.x; }
inline dim3 grid_for(uint64_t lanes) { return dim3((uint32_t)((lanes + kBlock - 1) / kBlock)); }

// n_major * G lanes.  Every lane of a wavefront reaches the shuffles: a group past the last row walks an empty range.
template <uint32_t G>
__global__ __launch_bounds__(kBlock) void csr_row_stats_kernel(const uint64_t* __restrict__ indptr, uint32_t n_major,
                                                               const uint32_t* __restrict__ alt, const uint32_t* __restrict__ ref,
                                                               const uint32_t* __restrict__ unk, vtx_csr_stats out) {
    const uint64_t lane = lane_id();
    const uint64_t r = lane / G;
    const uint32_t j = (uint32_t)(lane % G);
    const bool live = r < n_major;
    const uint64_t begin = live ? indptr[r] : 0ull, end = live ? indptr[r + 1] : 0ull;
    vtxr::RowStats s = vtxr::stats_walk(alt, ref, unk, begin, end, j, G);
#pragma unroll
    for (uint32_t d = G / 2; d; d /= 2) {                     // d < G: the partner lies in the same group, the same wavefront
        vtxr::RowStats o;
        o.n_entries = __shfl_xor(s.n_entries, d); o.n_alt = __shfl_xor(s.n_alt, d); o.n_ref = __shfl_xor(s.n_ref, d);
        o.n_both = __shfl_xor(s.n_both, d);
        o.sum_alt = __shfl_xor((unsigned long long)s.sum_alt, d); o.sum_ref = __shfl_xor((unsigned long long)s.sum_ref, d);
        o.sum_unk = __shfl_xor((unsigned long long)s.sum_unk, d);
        vtxr::stats_merge(s, o);
    }
    if (!live || j) return;
    if (out.n_entries) out.n_entries[r] = s.n_entries;
    if (out.n_alt) out.n_alt[r] = s.n_alt;
    if (out.n_ref) out.n_ref[r] = s.n_ref;
    if (out.n_both) out.n_both[r] = s.n_both;
    if (out.sum_alt) out.sum_alt[r] = s.sum_alt;
    if (out.sum_ref) out.sum_ref[r] = s.sum_ref;
    if (out.sum_unk) out.sum_unk[r] = s.sum_unk;
}

// n + 1 lanes: flag[i] = mask keeps i (the last word: 0, so that its exclusive sum is the kept count)
__global__ __launch_bounds__(kBlock) void csr_mask_flags_kernel(const uint8_t* __restrict__ mask, uint32_t n, uint32_t* __restrict__ flag) {
    const uint64_t i = lane_id();
    if (i > n) return;
    flag[i] = i < n ? vtxr::mask_keeps(mask, i) : 0u;
}

// nnz + 1 lanes over a VALIDATED CSR: flag[k] = the keep predicate of entry k (the last word: 0)
__global__ __launch_bounds__(kBlock) void csr_keep_flags_kernel(const uint64_t* __restrict__ indptr, uint32_t n_major, const uint32_t* __restrict__ indices,
                                                                uint64_t nnz, const uint8_t* __restrict__ keep_major,
                                                                const uint8_t* __restrict__ keep_minor, uint32_t* __restrict__ flag) {
    const uint64_t k = lane_id();
    if (k > nnz) return;
    flag[k] = k < nnz ? vtxr::keep_entry(keep_major, keep_minor, keep_major ? vtxr::row_of(indptr, n_major, k) : 0u, indices[k]) : 0u;
}

// n_major + 1 lanes: the offsets of the selected matrix, each written once (vtx_csr_ops_core.h)
__global__ __launch_bounds__(kBlock) void csr_select_offsets_kernel(const uint64_t* __restrict__ indptr, uint32_t n_major,
                                                                    const uint8_t* __restrict__ keep_major, const uint32_t* __restrict__ major_map,
                                                                    const uint32_t* __restrict__ pos, uint64_t* __restrict__ indptr_out) {
    const uint64_t r = lane_id();
    if (r > n_major) return;
    if (vtxr::select_offset_lane(r, n_major, keep_major)) indptr_out[major_map[r]] = pos[indptr[r]];
}

// n lanes: ids[map[i]] = i for every kept i
__global__ __launch_bounds__(kBlock) void csr_select_ids_kernel(const uint8_t* __restrict__ mask, uint32_t n, const uint32_t* __restrict__ map,
                                                                uint32_t* __restrict__ ids) {
    const uint64_t i = lane_id();
    if (i >= n) return;
    if (vtxr::mask_keeps(mask, i)) ids[map[i]] = (uint32_t)i;
}

constexpr uint32_t kMaxPayload = 8;      // payload arrays per launch of csr_select_place_kernel
struct Payloads {
    const void* in[kMaxPayload];
    void* out[kMaxPayload];
    uint32_t wide[kMaxPayload];          // 1: 8-byte elements, 0: 4-byte
    uint32_t n;
};

__global__ __launch_bounds__(kBlock) void csr_select_place_kernel(const uint32_t* __restrict__ indices, uint64_t nnz, const uint32_t* __restrict__ pos,
                                                                  const uint32_t* __restrict__ minor_map, uint32_t* __restrict__ indices_out, Payloads pl) {
    const uint64_t k = lane_id();
    if (k >= nnz) return;
    const uint32_t q = pos[k];
    if (pos[k + 1] == q) return;                              // not kept: the scan did not count it
    if (indices_out) indices_out[q] = minor_map[indices[k]];
    for (uint32_t a = 0; a < pl.n; ++a) {                    // wavefront-uniform: the pointers come from the kernel's arguments
        if (pl.wide[a]) ((uint64_t*)pl.out[a])[q] = ((const uint64_t*)pl.in[a])[k];
        else ((uint32_t*)pl.out[a])[q] = ((const uint32_t*)pl.in[a])[k];
    }
}

template <uint32_t G>
hipError_t launch_row_stats(const uint64_t* indptr, uint32_t n_major, const uint32_t* alt, const uint32_t* ref, const uint32_t* unk,
                            const vtx_csr_stats& out, hipStream_t s) {
    hipLaunchKernelGGL(csr_row_stats_kernel<G>, grid_for((uint64_t)n_major * G), dim3(kBlock), 0, s, indptr, n_major, alt, ref, unk, out);
    return hipGetLastError();
}

}  // namespace

extern "C" {

// G: a power of two, 1 .. 64 (vtxr::group_lanes)
hipError_t vtxr_row_stats(const uint64_t* indptr, uint32_t n_major, const uint32_t* alt, const uint32_t* ref, const uint32_t* unk,
                          const vtx_csr_stats* out, uint32_t G, hipStream_t s) {
    if (!n_major) return hipSuccess;
    switch (G) {
    case 1: return launch_row_stats<1>(indptr, n_major, alt, ref, unk, *out, s);
    case 2: return launch_row_stats<2>(indptr, n_major, alt, ref, unk, *out, s);
    case 4: return launch_row_stats<4>(indptr, n_major, alt, ref, unk, *out, s);
    case 8: return launch_row_stats<8>(indptr, n_major, alt, ref, unk, *out, s);
    case 16: return launch_row_stats<16>(indptr, n_major, alt, ref, unk, *out, s);
    case 32: return launch_row_stats<32>(indptr, n_major, alt, ref, unk, *out, s);
    case 64: return launch_row_stats<64>(indptr, n_major, alt, ref, unk, *out, s);
    default: return hipErrorInvalidValue;
    }
}

// the work space of one in-place exclusive sum over n 32-bit words
size_t vtxr_scan_temp_bytes(uint64_t n) {
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (uint32_t*)nullptr, (size_t)std::max<uint64_t>(n, 1));
    return bytes;
}

// map[0 .. n]: the number of kept ones below i; map[n] = how many are kept
hipError_t vtxr_mask_map(const uint8_t* mask, uint32_t n, uint32_t* map, void* temp, size_t temp_bytes, hipStream_t s) {
    hipLaunchKernelGGL(csr_mask_flags_kernel, grid_for((uint64_t)n + 1), dim3(kBlock), 0, s, mask, n, map);
    if (hipError_t e = hipGetLastError()) return e;
    return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, map, (size_t)n + 1, s);
}

// pos[0 .. nnz]: the number of kept entries below k; pos[nnz] = nnz_out.  The CSR has passed vtxr_check.
hipError_t vtxr_keep_positions(const uint64_t* indptr, uint32_t n_major, const uint32_t* indices, uint64_t nnz, const uint8_t* keep_major,
                               const uint8_t* keep_minor, uint32_t* pos, void* temp, size_t temp_bytes, hipStream_t s) {
    hipLaunchKernelGGL(csr_keep_flags_kernel, grid_for(nnz + 1), dim3(kBlock), 0, s, indptr, n_major, indices, nnz, keep_major, keep_minor, pos);
    if (hipError_t e = hipGetLastError()) return e;
    return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, pos, (size_t)nnz + 1, s);
}

hipError_t vtxr_select_offsets(const uint64_t* indptr, uint32_t n_major, const uint8_t* keep_major, const uint32_t* major_map, const uint32_t* pos,
                               uint64_t* indptr_out, hipStream_t s) {
    hipLaunchKernelGGL(csr_select_offsets_kernel, grid_for((uint64_t)n_major + 1), dim3(kBlock), 0, s, indptr, n_major, keep_major, major_map, pos,
                       indptr_out);
    return hipGetLastError();
}

hipError_t vtxr_select_ids(const uint8_t* mask, uint32_t n, const uint32_t* map, uint32_t* ids, hipStream_t s) {
    if (!n || !ids) return hipSuccess;
    hipLaunchKernelGGL(csr_select_ids_kernel, grid_for(n), dim3(kBlock), 0, s, mask, n, map, ids);
    return hipGetLastError();
}

hipError_t vtxr_select_place(const uint32_t* indices, uint64_t nnz, const uint32_t* pos, const uint32_t* minor_map, uint32_t* indices_out,
                             const void* const* in, void* const* out, const uint32_t* elem_bytes, uint32_t n_payload, hipStream_t s) {
    if (!nnz) return hipSuccess;
    uint32_t done = 0;
    do {                                                      // the first launch also writes indices_out
        Payloads pl{};
        pl.n = std::min(kMaxPayload, n_payload - done);
        for (uint32_t a = 0; a < pl.n; ++a) { pl.in[a] = in[done + a]; pl.out[a] = out[done + a]; pl.wide[a] = elem_bytes[done + a] == 8; }
        hipLaunchKernelGGL(csr_select_place_kernel, grid_for(nnz), dim3(kBlock), 0, s, indices, nnz, pos, minor_map, done ? nullptr : indices_out, pl);
        if (hipError_t e = hipGetLastError()) return e;
        done += pl.n;
    } while (done < n_payload);
    return hipSuccess;
}

}
