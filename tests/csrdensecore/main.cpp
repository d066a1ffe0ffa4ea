// Host build of vartrix_amd/csrc/vtx_csr_dense_core.h as a stand-alone program for tests/test_csr_dense_core.py: what the lanes TOUCH.
//   csr_dense_host IN OUT
//   IN:  u32 n_cases, then per case { u32 n_major, n_minor, nnz, n_cols, has_alt, has_ref; (n_major + 1) x u64 indptr; nnz x u32 each of
//        indices, alt, ref; then n_minor * n_cols x i32 w_alt if has_alt, and as many w_ref if has_ref }.
//   OUT per case: n_major * n_cols x i64.
// Every array is an allocation of exactly the size the device gives it — a table exactly n_minor * n_cols words, an absent one no
// allocation at all (NULL) — filled with a pattern first: under the sanitizer build (`make csr_dense_host_san`) a store or load outside
// it, such as a dead lane's read past a table or a trip of the walk that runs over the end of the row's last entry, is an error, and an
// element the rules do not write keeps the pattern and fails the comparison in the test.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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
    if (argc != 3) { fprintf(stderr, "usage: csr_dense_host IN OUT\n"); return 2; }
    std::vector<uint8_t> in;
    if (!read_file(argv[1], in) || in.size() < 4) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* f = fopen(argv[2], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    uint32_t n_cases;
    memcpy(&n_cases, in.data(), 4);
    size_t p = 4;
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint32_t* h = take<uint32_t>(in, p, 6);
        const uint32_t n_major = h[0], n_minor = h[1], nnz = h[2], n_cols = h[3], has_alt = h[4], has_ref = h[5];
        free(h);
        uint64_t* indptr = take<uint64_t>(in, p, (size_t)n_major + 1);
        uint32_t *indices = take<uint32_t>(in, p, nnz), *alt = take<uint32_t>(in, p, nnz), *ref = take<uint32_t>(in, p, nnz);
        const size_t n_words = (size_t)n_minor * n_cols;
        int32_t* w_alt = has_alt ? take<int32_t>(in, p, n_words) : nullptr;
        int32_t* w_ref = has_ref ? take<int32_t>(in, p, n_words) : nullptr;
        uint32_t bad = 0;                                                        // csr_check_kernel: a refused CSR never reaches the lanes below
        for (uint64_t i = 0; i <= n_major; ++i) bad |= vtxr::indptr_bad(i, n_major, nnz, indptr[i], i < n_major ? indptr[i + 1] : 0ull);
        for (uint64_t i = 0; i < nnz; ++i) bad |= vtxr::index_bad(indices[i], n_minor);
        if (bad || !n_cols || n_cols > vtxr::DENSE_MAX || (n_minor && !has_alt && !has_ref)) {
            fprintf(stderr, "case %u: not an input the call takes (%u)\n", c, bad);
            return 2;
        }
        const size_t n = (size_t)n_major * n_cols;
        int64_t* out = pattern<int64_t>(n);
        csrdense::sum(csrdense::SumIn{indptr, n_major, indices, alt, ref, w_alt, w_ref, n_cols}, out, nullptr);
        put(f, out, n);
        free(out); free(indptr); free(indices); free(alt); free(ref); free(w_alt); free(w_ref);
    }
    if (fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    return 0;
}
