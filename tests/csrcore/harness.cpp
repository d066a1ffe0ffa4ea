// Host build of vartrix_amd/csrc/vtx_csr_core.h for tests/test_csr_core.py: the functions one lane of the CSR kernels (vtx_csr.hip)
// runs alone, with the lanes as a loop.  No device code, no sanitizer: a shared object ctypes loads.
#include <stdint.h>

#include "../../vartrix_amd/csrc/vtx_csr_core.h"

extern "C" {

// csr_offsets_kernel (n + 1 lanes over key[0 .. n)), then csr_fill_kernel (one lane per row) for the long intervals.  indptr has end - begin + 1 slots; writes[slot] counts the stores into it.
// Returns the number of stores that would have fallen outside the slots (must be 0; they are not done).
uint64_t csr_offsets(const uint32_t* key, uint64_t n, uint32_t begin, uint32_t end, uint64_t* indptr, uint8_t* writes) {
    uint64_t outside = 0;
    const uint64_t slots = (uint64_t)end - begin + 1;
    for (uint64_t k = 0; k <= n; ++k) {
        uint64_t lo, hi;
        vtxr::offset_rows(k, n, k ? key[k - 1] : 0u, k < n ? key[k] : 0u, begin, end, &lo, &hi);
        if (vtxr::long_gap(lo, hi)) continue;                 // left to the per-row lanes below
        for (uint64_t r = lo; r <= hi; ++r) {
            if (r < begin || r - begin >= slots) { ++outside; continue; }
            indptr[r - begin] = k;
            if (writes[r - begin] < 255) ++writes[r - begin];
        }
    }
    if (slots <= vtxr::GAP_LANE_ROWS) return outside;         // as the launcher: no interval of such a window is a long one
    for (uint64_t r = begin; r <= end; ++r) {                 // csr_fill_kernel: one lane per row of the window
        const uint64_t k = vtxr::lower_bound(key, n, r);
        uint64_t lo, hi;
        vtxr::offset_rows(k, n, k ? key[k - 1] : 0u, k < n ? key[k] : 0u, begin, end, &lo, &hi);
        if (!vtxr::long_gap(lo, hi)) continue;
        indptr[r - begin] = k;
        if (writes[r - begin] < 255) ++writes[r - begin];
    }
    return outside;
}

// csr_check_kernel: the OR of the lanes' bits
uint32_t csr_check(const uint64_t* indptr, uint32_t n_major, uint64_t nnz, const uint32_t* indices, uint32_t n_minor) {
    uint32_t bad = 0;
    for (uint64_t i = 0; i <= n_major; ++i) bad |= vtxr::indptr_bad(i, n_major, nnz, indptr[i], i < n_major ? indptr[i + 1] : 0ull);
    for (uint64_t i = 0; i < nnz; ++i) bad |= vtxr::index_bad(indices[i], n_minor);
    return bad;
}

// csr_window_kernel
uint32_t csr_window(const uint32_t* row, uint64_t n, uint32_t begin, uint32_t end) {
    uint32_t bad = 0;
    for (uint64_t k = 0; k < n; ++k) bad |= vtxr::row_bad(row[k], begin, end);
    return bad;
}

// csr_place_kernel's row expansion: out[k] = the row that holds entry p[k]
void csr_rows(const uint64_t* indptr, uint32_t n_major, const uint32_t* p, uint64_t n, uint32_t* out) {
    for (uint64_t k = 0; k < n; ++k) out[k] = vtxr::row_of(indptr, n_major, p[k]);
}

}
