// Host build of vartrix_amd/csrc/vtx_prep_core.h as a stand-alone program for tests/test_prep_core.py: what the preparation TOUCHES.
//   prep_host IN OUT
// IN:  u32 n, then n cases of { u32 n_loci, n_records, tag_bytes, read_bytes, max_read_len, nibbles, n_barcodes, bc_bytes, use_umi,
//      weak_rounds; n_loci vtx_locus; n_records vtx_raw_record; tag_bytes bytes; (n_barcodes + 1) u64 offsets; bc_bytes bytes }.
// OUT: per case { i32 status, u32 kept, u32 rounds, u32 pad, u64 not_cell_bc, u64 non_umi } and, when status is 0, kept vtx_record,
//      n_loci u32 rec_begin, n_loci u32 rec_count.
// Every array of a case lives in a heap allocation of EXACTLY its size (a tag that lies flush against the arena's end has the
// allocation's end behind its last byte): under the sanitizer build (`make prep_host_san`) a read past a tag is a report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "prep_host.h"

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
template <class T> T* exact(const std::vector<uint8_t>& in, size_t& p, size_t count) {      // count elements copied out of the file
    const size_t bytes = count * sizeof(T);
    if (p + bytes > in.size()) return nullptr;
    T* m = (T*)malloc(bytes ? bytes : 1);
    if (m && bytes) memcpy(m, in.data() + p, bytes);
    p += bytes;
    return m;
}
template <class T> void put(std::vector<uint8_t>& out, const T* v, size_t count) {
    const uint8_t* b = (const uint8_t*)v;
    out.insert(out.end(), b, b + count * sizeof(T));
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: prep_host IN OUT\n"); return 2; }
    std::vector<uint8_t> in, out;
    if (!read_file(argv[1], in) || in.size() < 4) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint32_t n;
    memcpy(&n, in.data(), 4);
    size_t p = 4;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t h[10];
        if (p + sizeof h > in.size()) { fprintf(stderr, "truncated case %u\n", i); return 2; }
        memcpy(h, in.data() + p, sizeof h);
        p += sizeof h;
        const uint32_t nl = h[0], nr = h[1], tag_bytes = h[2], read_bytes = h[3], nb = h[6], bc_bytes = h[7];
        vtx_locus* loci = exact<vtx_locus>(in, p, nl);
        vtx_raw_record* raw = exact<vtx_raw_record>(in, p, nr);
        uint8_t* tags = exact<uint8_t>(in, p, tag_bytes);
        uint64_t* off = exact<uint64_t>(in, p, (size_t)nb + 1);
        uint8_t* bcs = exact<uint8_t>(in, p, bc_bytes);
        if (!loci || !raw || !tags || !off || !bcs) { fprintf(stderr, "truncated case %u\n", i); return 2; }
        // what vtx_submit_raw and vtx_set_barcodes check on the host
        uint32_t next = 0;
        bool ok = off[nb] == bc_bytes;
        for (uint32_t l = 0; l < nl && ok; ++l) { ok = loci[l].rec_begin == next && (uint64_t)next + loci[l].rec_count <= nr; next += loci[l].rec_count; }
        for (uint32_t j = 0; j < nb && ok; ++j) ok = off[j] <= off[j + 1];
        if (!ok || next != nr) { fprintf(stderr, "bad case %u\n", i); return 2; }
        prep_host::In pin{loci, nl, raw, nr, tags, tag_bytes, read_bytes, h[4], (int)h[5], bcs, off, nb, (int)h[8], h[9]};
        const prep_host::Out o = prep_host::run(pin);
        const int32_t status = o.status;
        const uint32_t head[3] = {o.kept, o.rounds, 0};
        const uint64_t cnt[2] = {o.not_cell_bc, o.non_umi};
        put(out, &status, 1); put(out, head, 3); put(out, cnt, 2);
        if (!status) { put(out, o.records.data(), o.kept); put(out, o.rec_begin.data(), nl); put(out, o.rec_count.data(), nl); }
        free(loci); free(raw); free(tags); free(off); free(bcs);
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    return 0;
}
