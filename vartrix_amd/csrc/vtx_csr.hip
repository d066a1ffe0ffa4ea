// vtx_csr.hip — the matrices as CSR on the device: row offsets of the run's triplets, and the stable transpose of any CSR.
//
// What it replaces: nothing in the reference — its only output is sprs::io::write_matrix_market (src/main.rs:381-389), variants x
// cells.  A user of scanpy / AnnData, scipy or torch parses that text back, converts the triplets to CSR and transposes them (AnnData's
// X is cells x variants).  The triplets are already on the card in the merge loop's order (src/main.rs:320-348), so:
//
//   variant-major   only the offsets are new: csr_offsets_kernel, one lane per boundary of the sorted `row` array (vtx_csr_core.h);
//                   a stretch of more than 256 rows without entries is left to csr_fill_kernel, one lane per row of the window.
//   cell-major      a STABLE sort of the entries by column:
//     check    csr_check_kernel     the caller's indptr / indices, before anything is written through them (flag word, integer OR)
//     keys     csr_iota_kernel      positions 0 .. nnz - 1
//     sort     hipcub LSD radix sort of (column -> position) over the bits a column needs: stable, so perm = argsort(indices, stable)
//     offsets  csr_offsets_kernel   on the sorted columns: indptr_t
//     place    csr_place_kernel     per output entry k: p = perm[k]; indices_t[k] = the row that holds p (binary search in indptr, an
//                                   L2-resident array); every payload array out[k] = in[p] as 4- or 8-byte words, bit for bit
//
// No float is ever computed here, no float atomic exists; the one integer atomic (OR into the flag word) cannot depend on its order.
// All of it is HBM-bound index work: the place kernel reads perm coalesced, gathers the payloads (random 4 / 8-byte reads — the cost of
// a transpose) and writes everything coalesced.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "vtx_csr_core.h"
#include "vtx_device.h"

namespace {

constexpr uint32_t kBlock = 256;

__device__ __forceinline__ uint64_t lane_id() { return (uint64_t)blockIdx.x * kBlock + threadIdx.x; }
inline dim3 grid_for(uint64_t lanes) { return dim3((uint32_t)((lanes + kBlock - 1) / kBlock)); }

// vtx_device_csr: every triplet's row inside the window?
__global__ __launch_bounds__(kBlock) void csr_window_kernel(const uint32_t* __restrict__ row, uint64_t n, uint32_t begin, uint32_t end,
                                                            uint32_t* __restrict__ flag) {
    const uint64_t k = lane_id();
    if (k >= n) return;
    const uint32_t bad = vtxr::row_bad(row[k], begin, end);
    if (bad) atomicOr(flag, bad);
}

// n + 1 lanes over the boundaries of key[0 .. n) (sorted, inside [begin, end)): indptr[r - begin] for r in [begin, end]
__global__ __launch_bounds__(kBlock) void csr_offsets_kernel(const uint32_t* __restrict__ key, uint64_t n, uint32_t begin, uint32_t end,
                                                             uint64_t* __restrict__ indptr) {
    const uint64_t k = lane_id();
    if (k > n) return;
    const uint32_t prev = k ? key[k - 1] : 0u, cur = k < n ? key[k] : 0u;
    uint64_t lo, hi;
    vtxr::offset_rows(k, n, prev, cur, begin, end, &lo, &hi);
    if (vtxr::long_gap(lo, hi)) return;                       // csr_fill_kernel writes it: one lane per row, not one lane for all
    for (uint64_t r = lo; r <= hi; ++r) indptr[r - begin] = k;
}

// end - begin + 1 lanes, one per row of the window: the offsets of the LONG intervals, which csr_offsets_kernel leaves out
__global__ __launch_bounds__(kBlock) void csr_fill_kernel(const uint32_t* __restrict__ key, uint64_t n, uint32_t begin, uint32_t end,
                                                          uint64_t* __restrict__ indptr) {
    const uint64_t r = (uint64_t)begin + lane_id();
    if (r > end) return;
    const uint64_t k = vtxr::lower_bound(key, n, r);
    const uint32_t prev = k ? key[k - 1] : 0u, cur = k < n ? key[k] : 0u;
    uint64_t lo, hi;
    vtxr::offset_rows(k, n, prev, cur, begin, end, &lo, &hi);
    if (vtxr::long_gap(lo, hi)) indptr[r - begin] = k;
}

// max(n_major + 1, nnz) lanes: the caller's CSR, read only
__global__ __launch_bounds__(kBlock) void csr_check_kernel(const uint64_t* __restrict__ indptr, uint32_t n_major, uint64_t nnz,
                                                           const uint32_t* __restrict__ indices, uint32_t n_minor, uint32_t* __restrict__ flag) {
    const uint64_t i = lane_id();
    uint32_t bad = 0;
    if (i <= n_major) bad |= vtxr::indptr_bad(i, n_major, nnz, indptr[i], i < n_major ? indptr[i + 1] : 0ull);
    if (i < nnz) bad |= vtxr::index_bad(indices[i], n_minor);
    if (bad) atomicOr(flag, bad);
}

__global__ __launch_bounds__(kBlock) void csr_iota_kernel(uint32_t* __restrict__ p, uint64_t n) {
    const uint64_t k = lane_id();
    if (k < n) p[k] = (uint32_t)k;
}

constexpr uint32_t kMaxPayload = 8;      // payload arrays per launch of csr_place_kernel
struct Payloads {
    const void* in[kMaxPayload];
    void* out[kMaxPayload];
    uint32_t wide[kMaxPayload];          // 1: 8-byte elements, 0: 4-byte
    uint32_t n;
};

__global__ __launch_bounds__(kBlock) void csr_place_kernel(const uint64_t* __restrict__ indptr, uint32_t n_major, const uint32_t* __restrict__ perm,
                                                           uint64_t n, uint32_t* __restrict__ indices_t, Payloads pl) {
    const uint64_t k = lane_id();
    if (k >= n) return;
    const uint32_t p = perm[k];
    if (indices_t) indices_t[k] = vtxr::row_of(indptr, n_major, p);
    for (uint32_t a = 0; a < pl.n; ++a) {                    // wavefront-uniform: the pointers come from the kernel's arguments
        if (pl.wide[a]) ((uint64_t*)pl.out[a])[k] = ((const uint64_t*)pl.in[a])[p];
        else ((uint32_t*)pl.out[a])[k] = ((const uint32_t*)pl.in[a])[p];
    }
}

}  // namespace

extern "C" {

hipError_t vtxr_window_check(const uint32_t* row, uint64_t n, uint32_t begin, uint32_t end, uint32_t* flag, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(csr_window_kernel, grid_for(n), dim3(kBlock), 0, s, row, n, begin, end, flag);
    return hipGetLastError();
}

hipError_t vtxr_offsets(const uint32_t* key, uint64_t n, uint32_t begin, uint32_t end, uint64_t* indptr, hipStream_t s) {
    hipLaunchKernelGGL(csr_offsets_kernel, grid_for(n + 1), dim3(kBlock), 0, s, key, n, begin, end, indptr);
    if (hipError_t e = hipGetLastError()) return e;
    const uint64_t rows = (uint64_t)end - begin + 1;
    if (rows <= vtxr::GAP_LANE_ROWS) return hipSuccess;       // no interval of such a window can be a long one
    hipLaunchKernelGGL(csr_fill_kernel, grid_for(rows), dim3(kBlock), 0, s, key, n, begin, end, indptr);
    return hipGetLastError();
}

hipError_t vtxr_check(const uint64_t* indptr, uint32_t n_major, uint64_t nnz, const uint32_t* indices, uint32_t n_minor, uint32_t* flag,
                      hipStream_t s) {
    hipLaunchKernelGGL(csr_check_kernel, grid_for(std::max<uint64_t>((uint64_t)n_major + 1, nnz)), dim3(kBlock), 0, s, indptr, n_major, nnz,
                       indices, n_minor, flag);
    return hipGetLastError();
}

// the work space of vtxr_sort_positions for the same n and the same bit range
size_t vtxr_sort_temp_bytes(uint64_t n, int end_bit) {
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             std::max<uint64_t>(n, 1), 0, end_bit);
    return bytes;
}

// stable: perm = the positions 0 .. n - 1 ordered by key, equal keys in position order; key_sorted = the keys in that order
hipError_t vtxr_sort_positions(const uint32_t* key, uint32_t* key_sorted, uint32_t* iota, uint32_t* perm, uint64_t n, int end_bit, void* temp,
                               size_t temp_bytes, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(csr_iota_kernel, grid_for(n), dim3(kBlock), 0, s, iota, n);
    if (hipError_t e = hipGetLastError()) return e;
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, key, key_sorted, (const uint32_t*)iota, perm, n, 0, end_bit, s);
}

hipError_t vtxr_place(const uint64_t* indptr, uint32_t n_major, const uint32_t* perm, uint64_t n, uint32_t* indices_t, const void* const* in,
                      void* const* out, const uint32_t* elem_bytes, uint32_t n_payload, hipStream_t s) {
    if (!n) return hipSuccess;
    uint32_t done = 0;
    do {                                                      // the first launch also writes indices_t
        Payloads pl{};
        pl.n = std::min(kMaxPayload, n_payload - done);
        for (uint32_t a = 0; a < pl.n; ++a) { pl.in[a] = in[done + a]; pl.out[a] = out[done + a]; pl.wide[a] = elem_bytes[done + a] == 8; }
        hipLaunchKernelGGL(csr_place_kernel, grid_for(n), dim3(kBlock), 0, s, indptr, n_major, perm, n, done ? nullptr : indices_t, pl);
        if (hipError_t e = hipGetLastError()) return e;
        done += pl.n;
    } while (done < n_payload);
    return hipSuccess;
}

}
