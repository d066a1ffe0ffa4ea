// Host build of vartrix_amd/csrc/vtx_inflate_core.h as a stand-alone program for tests/test_inflate_bounds.py: what the decoder TOUCHES.
//   inflate_host IN OUT   IN: u32 n, then n cases of { u32 in_len, u32 out_len, u32 fill, in_len bytes }.
//                         OUT: per case { u32 status, u32 trips, u32 pad_ok, u32 m, m bytes }: m = out_len when the block was accepted,
//                         else 0; pad_ok = 1: the OUT_PAD bytes behind the output still hold what they were filled with.
// Every case gets allocations of exactly the sizes the device gives the LAST block of an upload: in_len + IN_PAD bytes for the payload,
// out_len + OUT_PAD for the output, the slack filled with the case's fill byte — under the sanitizer build (`make inflate_host_san`)
// the red zone starts where the device's allocation would end.  The scratch is exactly vtxi::BYTES / HI_WORDS / CNT_WORDS.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../vartrix_amd/csrc/vtx_inflate_core.h"

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
void put32(std::vector<uint8_t>& out, uint32_t v) { out.insert(out.end(), (const uint8_t*)&v, (const uint8_t*)&v + 4); }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: inflate_host IN OUT\n"); return 2; }
    std::vector<uint8_t> in, res;
    if (!read_file(argv[1], in) || in.size() < 4) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint32_t n;
    memcpy(&n, in.data(), 4);
    size_t p = 4;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t h[3];
        if (p + 12 > in.size()) { fprintf(stderr, "truncated case %u\n", i); return 2; }
        memcpy(h, in.data() + p, 12);
        p += 12;
        const uint32_t in_len = h[0], out_len = h[1], fill = h[2] & 0xffu;
        if (p + in_len > in.size()) { fprintf(stderr, "truncated case %u\n", i); return 2; }
        uint8_t* payload = (uint8_t*)malloc((size_t)in_len + vtxi::IN_PAD);
        uint8_t* out = (uint8_t*)malloc((size_t)out_len + vtxi::OUT_PAD);
        uint8_t* sb = (uint8_t*)malloc(vtxi::BYTES);
        uint32_t* sh = (uint32_t*)malloc(vtxi::HI_WORDS * sizeof(uint32_t));
        uint16_t* scn = (uint16_t*)malloc(vtxi::CNT_WORDS * sizeof(uint16_t));
        if (!payload || !out || !sb || !sh || !scn) { fprintf(stderr, "out of memory\n"); return 2; }
        if (in_len) memcpy(payload, in.data() + p, in_len);
        memset(payload + in_len, (int)fill, vtxi::IN_PAD);
        memset(out, (int)fill, (size_t)out_len + vtxi::OUT_PAD);
        memset(sb, 0xde, vtxi::BYTES);
        memset(sh, 0xde, vtxi::HI_WORDS * sizeof(uint32_t));
        memset(scn, 0xde, vtxi::CNT_WORDS * sizeof(uint16_t));
        p += in_len;
        const vtxi::Scratch sc{sb, sh, scn, 1};
        uint32_t trips = 0;
        const uint32_t st = vtxi::inflate_block(payload, in_len, out, out_len, sc, &trips);
        uint32_t pad_ok = 1;
        for (uint32_t k = 0; k < vtxi::OUT_PAD; ++k) pad_ok &= out[out_len + k] == fill ? 1u : 0u;
        const uint32_t m = st == vtxi::ST_OK ? out_len : 0u;
        put32(res, st); put32(res, trips); put32(res, pad_ok); put32(res, m);
        res.insert(res.end(), out, out + m);
        free(payload); free(out); free(sb); free(sh); free(scn);
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(res.data(), 1, res.size(), f) != res.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    return 0;
}
