// Host build of vartrix_amd/csrc/vtx_deflate_core.h for tests/test_deflate_core.py and tests/test_gpu_mtx_gz.py: the functions
// mtx_deflate_kernel is compiled from, the 64 lanes of the wavefront as a loop, as a stand-alone program.
//   deflate_host IN OUT          IN: records of { u32 n, n bytes }.  OUT: per record { u32 m, m bytes }: the record cut into chunks of
//                                65 280 bytes, one BGZF member per chunk (a record of 0 bytes: one empty member), then the EOF block.
//   deflate_host --file IN OUT   IN: one input, the whole file.  OUT: its BGZF file (what vtx_write_mtx_gz writes from one slab).
// The CRC comes from vtx_crc32_core.h's host wavefront, as the kernel takes it from the device one.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../vartrix_amd/csrc/vtx_crc32_core.h"
#include "../../vartrix_amd/csrc/vtx_deflate_core.h"

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

// one input -> members + EOF block, appended to out; false when a member's size is not what its BSIZE says or exceeds n + 31
bool encode(const uint8_t* data, size_t n, std::vector<uint8_t>& out) {
    static std::vector<uint32_t> tab;
    if (tab.empty()) { tab.resize(vtxc::TABLE_WORDS(4)); for (uint32_t i = 0; i < tab.size(); ++i) tab[i] = vtxc::table_entry<4>(i); }
    VTXD_LDS_DECL(static)
    std::vector<uint32_t> chunk(vtxd::CHUNK / 4 + 4), slot(vtxd::SLOT / 4), tok(vtxd::CHUNK);       // exact sizes: the sanitizer build sees an overrun
    size_t off = 0;
    do {
        const uint32_t m = (uint32_t)(n - off < vtxd::CHUNK ? n - off : vtxd::CHUNK);
        std::vector<uint8_t> in(data + off, data + off + m);                                        // exactly m bytes: reads behind the chunk show
        std::vector<uint32_t> aligned((m + 3) / 4 + 1);
        if (m) memcpy(aligned.data(), in.data(), m);
        const uint32_t crc = vtxc::block_crc_host<4>((const uint8_t*)aligned.data(), 0, m, tab.data());
        memset(slot.data(), 0xA5, vtxd::SLOT);
        const uint32_t size = vtxd::encode_member(in.data(), m, crc, (uint8_t*)slot.data(), tok.data(), lds);
        const uint8_t* s = (const uint8_t*)slot.data();
        if (size > m + 31 || size < 28 || (uint32_t)(s[16] | (s[17] << 8)) + 1 != size) { fprintf(stderr, "member of %u bytes for a chunk of %u: BSIZE %u\n", size, m, (s[16] | (s[17] << 8)) + 1); return false; }
        out.insert(out.end(), s, s + size);
        off += m;
    } while (off < n);
    out.insert(out.end(), vtxd::EOF_BLOCK, vtxd::EOF_BLOCK + 28);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const bool whole = argc == 4 && !strcmp(argv[1], "--file");
    if (!(argc == 3 || whole)) { fprintf(stderr, "usage: deflate_host [--file] IN OUT\n"); return 2; }
    std::vector<uint8_t> in, out;
    if (!read_file(argv[argc - 2], in)) { fprintf(stderr, "cannot read %s\n", argv[argc - 2]); return 2; }
    if (whole) {
        if (!encode(in.data(), in.size(), out)) return 1;
    } else {
        size_t p = 0;
        while (p + 4 <= in.size()) {
            uint32_t n;
            memcpy(&n, in.data() + p, 4);
            p += 4;
            if (p + n > in.size()) { fprintf(stderr, "truncated record\n"); return 2; }
            std::vector<uint8_t> one;
            if (!encode(in.data() + p, n, one)) return 1;
            const uint32_t m = (uint32_t)one.size();
            out.insert(out.end(), (const uint8_t*)&m, (const uint8_t*)&m + 4);
            out.insert(out.end(), one.begin(), one.end());
            p += n;
        }
    }
    FILE* f = fopen(argv[argc - 1], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[argc - 1]); return 2; }
    return 0;
}
