// Host build of vartrix_amd/csrc/vtx_csr_ops_core.h as a stand-alone program for tests/test_csr_ops_core.py: what the lanes TOUCH.
//   csr_ops_host IN OUT
//   IN:  u32 n_cases, then per case { u32 n_major, n_minor, nnz, has_keep_major, has_keep_minor; (n_major + 1) x u64 indptr;
//        nnz x u32 each of indices, alt, ref, unk; n_major x u8 keep_major if has_keep_major; n_minor x u8 keep_minor if has_keep_minor }.
//   OUT per case: for G = 1, 2, 4 .. 64: n_major x u32 each of n_entries, n_alt, n_ref, n_both, then n_major x u64 each of sum_alt,
//        sum_ref, sum_unk; then the selection: 3 x u32 sizes, (n_major_out + 1) x u64 indptr_out, nnz_out x u32 indices_out,
//        n_major_out x u32 major_ids, n_minor_out x u32 minor_ids, nnz_out x u32 (the alt payload), nnz_out x u64 (payload: 2^40 + source position).
// Every array is an allocation of exactly the size the device gives it, filled with a pattern first: under the sanitizer build
// (`make csr_ops_host_san`) a store or load outside it is an error, and a slot the rules do not write keeps the pattern and fails the
// comparison in the test.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lanes.h"

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

// exactly `bytes` bytes (one when 0, so that the pointer is a real allocation), every byte 0xA5
template <typename T> T* pattern(size_t count) {
    const size_t bytes = count * sizeof(T);
    T* p = (T*)malloc(bytes ? bytes : 1);
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, 0xA5, bytes ? bytes : 1);
    return p;
}

template <typename T> T* take(const std::vector<uint8_t>& in, size_t& p, size_t count) {
    if (p + count * sizeof(T) > in.size()) { fprintf(stderr, "truncated input\n"); exit(2); }
    T* a = pattern<T>(count);
    if (count) memcpy(a, in.data() + p, count * sizeof(T));
    p += count * sizeof(T);
    return a;
}

template <typename T> void put(FILE* f, const T* a, size_t count) {
    if (fwrite(a, sizeof(T), count, f) != count) { fprintf(stderr, "cannot write the output\n"); exit(2); }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: csr_ops_host IN OUT\n"); return 2; }
    std::vector<uint8_t> in;
    if (!read_file(argv[1], in) || in.size() < 4) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* f = fopen(argv[2], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    uint32_t n_cases;
    memcpy(&n_cases, in.data(), 4);
    size_t p = 4;
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint32_t* h = take<uint32_t>(in, p, 5);
        const uint32_t n_major = h[0], n_minor = h[1], nnz = h[2], has_major = h[3], has_minor = h[4];
        free(h);
        uint64_t* indptr = take<uint64_t>(in, p, (size_t)n_major + 1);
        uint32_t *indices = take<uint32_t>(in, p, nnz), *alt = take<uint32_t>(in, p, nnz), *ref = take<uint32_t>(in, p, nnz),
                 *unk = take<uint32_t>(in, p, nnz);
        uint8_t* keep_major = has_major ? take<uint8_t>(in, p, n_major) : nullptr;
        uint8_t* keep_minor = has_minor ? take<uint8_t>(in, p, n_minor) : nullptr;
        uint32_t bad = 0;                                                        // csr_check_kernel: a refused CSR never reaches the lanes below
        for (uint64_t i = 0; i <= n_major; ++i) bad |= vtxr::indptr_bad(i, n_major, nnz, indptr[i], i < n_major ? indptr[i + 1] : 0ull);
        for (uint64_t i = 0; i < nnz; ++i) bad |= vtxr::index_bad(indices[i], n_minor);
        if (bad) { fprintf(stderr, "case %u: not a CSR (%u)\n", c, bad); return 2; }
        for (uint32_t G = 1; G <= vtxr::MAX_GROUP; G *= 2) {
            uint32_t* cnt[4];
            uint64_t* sum[3];
            for (auto& a : cnt) a = pattern<uint32_t>(n_major);
            for (auto& a : sum) a = pattern<uint64_t>(n_major);
            csrops::row_stats(indptr, n_major, alt, ref, unk, G, csrops::StatsOut{cnt[0], cnt[1], cnt[2], cnt[3], sum[0], sum[1], sum[2]});
            for (auto& a : cnt) { put(f, a, n_major); free(a); }
            for (auto& a : sum) { put(f, a, n_major); free(a); }
        }
        csrops::Maps m;
        uint32_t sizes[3];
        csrops::scans(indptr, n_major, n_minor, indices, nnz, keep_major, keep_minor, m, sizes);
        uint64_t* wide = pattern<uint64_t>(nnz);
        for (uint32_t k = 0; k < nnz; ++k) wide[k] = (1ull << 40) + k;
        uint64_t* indptr_out = pattern<uint64_t>((size_t)sizes[0] + 1);
        uint32_t *indices_out = pattern<uint32_t>(sizes[2]), *major_ids = pattern<uint32_t>(sizes[0]), *minor_ids = pattern<uint32_t>(sizes[1]),
                 *alt_out = pattern<uint32_t>(sizes[2]);
        uint64_t* wide_out = pattern<uint64_t>(sizes[2]);
        csrops::place(indptr, n_major, n_minor, indices, nnz, keep_major, keep_minor, m, indptr_out, nullptr, indices_out, major_ids, minor_ids, alt,
                      alt_out, wide, wide_out);
        put(f, sizes, 3); put(f, indptr_out, (size_t)sizes[0] + 1); put(f, indices_out, sizes[2]); put(f, major_ids, sizes[0]);
        put(f, minor_ids, sizes[1]); put(f, alt_out, sizes[2]); put(f, wide_out, sizes[2]);
        free(indptr); free(indices); free(alt); free(ref); free(unk); free(keep_major); free(keep_minor); free(wide); free(indptr_out);
        free(indices_out); free(major_ids); free(minor_ids); free(alt_out); free(wide_out);
    }
    if (fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    return 0;
}
