// Host build of vartrix_amd/csrc/vtx_crc32_core.h as a stand-alone program for tests/test_crc32_core.py: what the wavefront TOUCHES.
//   crc32_host IN OUT   IN: u32 n, then n cases of { u32 W, u32 s, u32 len, u32 total, u32 fill, len bytes }.  OUT: u32 crc per case.
// Every case gets the inflated buffer as the device has it: a 16-byte aligned allocation of exactly total + 64 bytes filled with
// the case's fill byte, the block at [s, s + len) — s below W: its head read starts at the buffer's base; s + len == total: it is the
// last block.  Under the sanitizer build (`make crc32_host_san`) the red zones start where the device's allocation begins and ends.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../vartrix_amd/csrc/vtx_crc32_core.h"

namespace {
template <int W> const uint32_t* tables() {
    static std::vector<uint32_t> t;
    if (t.empty()) { t.resize(vtxc::TABLE_WORDS(W)); for (uint32_t i = 0; i < t.size(); ++i) t[i] = vtxc::table_entry<W>(i); }
    return t.data();
}
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
    if (argc != 3) { fprintf(stderr, "usage: crc32_host IN OUT\n"); return 2; }
    std::vector<uint8_t> in;
    std::vector<uint32_t> res;
    if (!read_file(argv[1], in) || in.size() < 4) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint32_t n;
    memcpy(&n, in.data(), 4);
    size_t p = 4;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t h[5];
        if (p + 20 > in.size()) { fprintf(stderr, "truncated case %u\n", i); return 2; }
        memcpy(h, in.data() + p, 20);
        p += 20;
        const uint32_t W = h[0], s = h[1], len = h[2], total = h[3], fill = h[4] & 0xffu;
        if (p + len > in.size() || (uint64_t)s + len > total || !(W == 4 || W == 8 || W == 16)) { fprintf(stderr, "bad case %u\n", i); return 2; }
        void* mem = nullptr;
        if (posix_memalign(&mem, 16, (size_t)total + 64) != 0) { fprintf(stderr, "out of memory\n"); return 2; }
        uint8_t* buf = (uint8_t*)mem;
        memset(buf, (int)fill, (size_t)total + 64);
        if (len) memcpy(buf + s, in.data() + p, len);
        p += len;
        const uint64_t e = (uint64_t)s + len;
        res.push_back(W == 4 ? vtxc::block_crc_host<4>(buf, s, e, tables<4>()) : W == 8 ? vtxc::block_crc_host<8>(buf, s, e, tables<8>())
                                                                                        : vtxc::block_crc_host<16>(buf, s, e, tables<16>()));
        free(buf);
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(res.data(), 4, res.size(), f) != res.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    return 0;
}
