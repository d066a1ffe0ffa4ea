// Host build of vartrix_amd/csrc/vtx_csr_core.h as a stand-alone program for tests/test_csr_core.py: what the lanes TOUCH.
//   csr_host IN OUT   IN: u32 n_cases, then per case { u32 begin, u32 end, u32 n, n x u32 key }.
//                     OUT per case: (end - begin + 1) x u64 indptr, then n x u32 row (row_of every entry over that indptr, + begin;
//                     0xffffffff each when a key lies outside the window: the offsets are still written inside their slots).
// Every array is an allocation of exactly the size the device gives it, filled with a pattern first: under the sanitizer build
// (`make csr_host_san`) a store or load outside it is an error, and a slot the rule does not write keeps the pattern and fails the
// comparison in the test.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../vartrix_amd/csrc/vtx_csr_core.h"

namespace {
bool read_file(const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(f);
    return true;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: csr_host IN OUT\n"); return 2; }
    std::vector<uint8_t> in;
    if (!read_file(argv[1], in) || in.size() < 4) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* f = fopen(argv[2], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    uint32_t n_cases;
    memcpy(&n_cases, in.data(), 4);
    size_t p = 4;
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint32_t h[3];
        if (p + 12 > in.size()) { fprintf(stderr, "truncated case %u\n", c); return 2; }
        memcpy(h, in.data() + p, 12);
        p += 12;
        const uint32_t begin = h[0], end = h[1], n = h[2];
        if (begin > end || p + 4ull * n > in.size()) { fprintf(stderr, "bad case %u\n", c); return 2; }
        uint32_t* key = (uint32_t*)malloc(4ull * n + (n ? 0 : 1));
        if (n) memcpy(key, in.data() + p, 4ull * n);
        p += 4ull * n;
        const uint64_t slots = (uint64_t)end - begin + 1;
        uint64_t* indptr = (uint64_t*)malloc(8 * slots);
        uint32_t* row = (uint32_t*)malloc(4ull * n + (n ? 0 : 1));
        if (!key || !indptr || !row) { fprintf(stderr, "out of memory\n"); return 2; }
        memset(indptr, 0xA5, 8 * slots);
        for (uint64_t k = 0; k <= n; ++k) {                                      // csr_offsets_kernel's lanes
            uint64_t lo, hi;
            vtxr::offset_rows(k, n, k ? key[k - 1] : 0u, k < n ? key[k] : 0u, begin, end, &lo, &hi);
            if (vtxr::long_gap(lo, hi)) continue;
            for (uint64_t r = lo; r <= hi; ++r) indptr[r - begin] = k;
        }
        for (uint64_t r = begin; slots > vtxr::GAP_LANE_ROWS && r <= end; ++r) {   // csr_fill_kernel's lanes: the long intervals
            const uint64_t k = vtxr::lower_bound(key, n, r);
            uint64_t lo, hi;
            vtxr::offset_rows(k, n, k ? key[k - 1] : 0u, k < n ? key[k] : 0u, begin, end, &lo, &hi);
            if (vtxr::long_gap(lo, hi)) indptr[r - begin] = k;
        }
        uint32_t outside = 0;                                                    // csr_window_kernel: such a window is refused, its offsets never used
        for (uint32_t k = 0; k < n; ++k) outside |= vtxr::row_bad(key[k], begin, end);
        for (uint32_t k = 0; k < n; ++k) row[k] = outside ? 0xffffffffu : begin + vtxr::row_of(indptr, end - begin, k);      // csr_place_kernel's row expansion
        if (fwrite(indptr, 8, slots, f) != slots || fwrite(row, 4, n, f) != n) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        free(key); free(indptr); free(row);
    }
    if (fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    return 0;
}
