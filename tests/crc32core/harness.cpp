// Host build of vartrix_amd/csrc/vtx_crc32_core.h for tests/test_crc32_core.py: the functions bgzf_crc32_kernel is compiled from, the
// 64 lanes of the wavefront as a loop.  The block lies at a chosen misalignment inside a 16-byte aligned buffer whose other bytes
// are 0xA5 (the head mask and the read range [start & ~(W - 1), end) are part of what is tested).
#include <stdint.h>
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
}  // namespace

extern "C" {
uint32_t vtxt_mulmod(uint32_t a, uint32_t b) { return vtxc::mulmod(a, b); }
uint32_t vtxt_mulx(uint32_t a) { return vtxc::mulx(a); }
uint32_t vtxt_divx(uint32_t a) { return vtxc::divx(a); }
uint32_t vtxt_xpow8(uint64_t n) { return vtxc::xpow8(n); }
uint32_t vtxt_combine(uint32_t a, uint32_t b, uint64_t len_b) { return vtxc::combine(a, b, len_b); }
// the CRC of bytes[0 .. n) as the wavefront computes it with slicing width W, the block starting `misalign` bytes behind a 16-byte
// boundary (any value: 16 k + m moves it by whole pieces too); 0xFFFFFFFF + 1 is never returned, -1 = bad W / out of memory
int64_t vtxt_block_crc(int W, const uint8_t* bytes, uint64_t n, uint32_t misalign) {
    const size_t cap = ((size_t)misalign + n + 64 + 15) & ~(size_t)15;
    uint8_t* buf = (uint8_t*)aligned_alloc(16, cap);
    if (!buf) return -1;
    memset(buf, 0xA5, cap);
    if (n) memcpy(buf + misalign, bytes, n);
    int64_t r = -1;
    if (W == 4) r = vtxc::block_crc_host<4>(buf, misalign, misalign + n, tables<4>());
    else if (W == 8) r = vtxc::block_crc_host<8>(buf, misalign, misalign + n, tables<8>());
    else if (W == 16) r = vtxc::block_crc_host<16>(buf, misalign, misalign + n, tables<16>());
    free(buf);
    return r;
}
// the cut of a block: a0, head, n_pieces, rows, pad, tail_begin
int vtxt_cut(int W, uint64_t s, uint64_t e, uint64_t* out) {
    vtxc::Cut c;
    if (W == 4) c = vtxc::cut_block<4>(s, e); else if (W == 8) c = vtxc::cut_block<8>(s, e); else if (W == 16) c = vtxc::cut_block<16>(s, e); else return -1;
    out[0] = c.a0; out[1] = c.head; out[2] = c.n_pieces; out[3] = c.rows; out[4] = c.pad; out[5] = c.tail_begin;
    return 0;
}
}
