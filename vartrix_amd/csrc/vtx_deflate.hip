// vtx_deflate.hip — the Matrix-Market text of vtx_write_mtx_gz, deflated on the device: what leaves the card is the .gz file.
//
// The reference writes plain text (sprs::io::write_matrix_market, src/main.rs:381-389); every reader of a 10x matrix directory takes
// matrix.mtx.gz.  The text is formatted into a device buffer by mtx_text_kernel (vtx_ingest.hip); here it is cut into chunks of
// vtxd::CHUNK bytes and
//   mtx_deflate_kernel     one wavefront (= one workgroup) per chunk, grid-stride: the chunk's CRC-32 (vtx_crc32_core.h), then one
//                          complete BGZF member into the chunk's slot of vtxd::SLOT bytes (vtx_deflate_core.h: LZ77 against a hash
//                          table in LDS, Huffman codes built in LDS, bits packed through an LDS window); the tokens between the two
//                          passes lie in the workgroup's own stretch of a work buffer in HBM
//   (inclusive scan of the member sizes)
//   mtx_gz_compact_kernel  one workgroup per chunk: the member from its slot to its final offset, dword stores
// LDS per workgroup: 16 KiB hash table + 4 KiB CRC tables + 5 KiB of code tables: six workgroups per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "vtx_device.h"
#include "vtx_ingest.h"
#include "vtx_crc32_core.h"
#include "vtx_deflate_core.h"

namespace {

// text: 4-byte aligned, `total` bytes.  Chunk ch = text[ch * CHUNK, min(total, (ch + 1) * CHUNK)).  slots: n_chunks * SLOT bytes.
// tok: gridDim.x * CHUNK words.  sizes[ch] = the member's size (<= chunk length + 31 <= SLOT).
__global__ __launch_bounds__(64) void mtx_deflate_kernel(const uint8_t* __restrict__ text, uint64_t total, uint32_t n_chunks,
                                                         uint8_t* __restrict__ slots, uint32_t* __restrict__ sizes, uint32_t* __restrict__ tok) {
    __shared__ uint32_t s_tab[vtxc::TABLE_WORDS(4)];
    VTXD_LDS_DECL(__shared__)
    for (uint32_t i = threadIdx.x; i < (uint32_t)vtxc::TABLE_WORDS(4); i += 64) s_tab[i] = vtxc::table_entry<4>(i);
    __syncthreads();
    const uint32_t lane = threadIdx.x;
    for (uint32_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const uint64_t s = (uint64_t)ch * vtxd::CHUNK, e = std::min<uint64_t>(total, s + vtxd::CHUNK);
        const vtxc::Cut c = vtxc::cut_block<4>(s, e);
        uint32_t v = vtxc::lane_pieces<4>(text, c, lane, s_tab);
        for (int k = 0; k < 6; ++k) {
            const uint32_t partner = __shfl_xor(v, 1 << k);
            if (lane & (1u << k)) v = vtxc::lane_join<4>(partner, v, k);
        }
        const uint32_t crc = vtxc::finish_block<4>(__shfl(v, 63), text, c, s, e);
        const uint32_t size = vtxd::encode_member(text + s, (uint32_t)(e - s), crc, slots + (uint64_t)ch * vtxd::SLOT,
                                                  tok + (uint64_t)blockIdx.x * vtxd::CHUNK, lds);
        if (lane == 0) sizes[ch] = size;
        __syncthreads();
    }
}

// end: the inclusive scan of sizes.  Member ch goes from its slot to out + end[ch] - sizes[ch]: bytes up to the first 4-byte boundary
// of the destination, dwords (the source is read unaligned), the last bytes.
__global__ __launch_bounds__(256) void mtx_gz_compact_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes,
                                                             const uint32_t* __restrict__ end, uint8_t* __restrict__ out) {
    const uint32_t ch = blockIdx.x, sz = std::min(sizes[ch], vtxd::SLOT);
    const uint8_t* src = slots + (uint64_t)ch * vtxd::SLOT;
    uint8_t* dst = out + (end[ch] - sizes[ch]);
    const uint32_t head = std::min<uint32_t>(sz, (uint32_t)((0u - (uintptr_t)dst) & 3u)), words = (sz - head) >> 2, tail = head + 4 * words;
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < words; i += 256) *(uint32_t*)(dst + head + 4 * i) = vtxd::ld32(src + head + 4 * i);
    if (threadIdx.x < sz - tail) dst[tail + threadIdx.x] = src[tail + threadIdx.x];
}

}  // namespace

extern "C" {

uint32_t vtxg_deflate_grid(uint32_t n_chunks) { return std::min<uint32_t>(n_chunks, 256u * 6u); }

hipError_t vtxg_mtx_deflate(const uint8_t* text, uint64_t total, uint32_t n_chunks, uint8_t* slots, uint32_t* sizes, uint32_t* tok, hipStream_t s) {
    if (!n_chunks) return hipSuccess;
    if (((uintptr_t)text | (uintptr_t)slots) & 3u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mtx_deflate_kernel, dim3(vtxg_deflate_grid(n_chunks)), dim3(64), 0, s, text, total, n_chunks, slots, sizes, tok);
    return hipGetLastError();
}

hipError_t vtxg_mtx_gz_compact(const uint8_t* slots, const uint32_t* sizes, const uint32_t* end, uint32_t n_chunks, uint8_t* out, hipStream_t s) {
    if (!n_chunks) return hipSuccess;
    hipLaunchKernelGGL(mtx_gz_compact_kernel, dim3(n_chunks), dim3(256), 0, s, slots, sizes, end, out);
    return hipGetLastError();
}

}  // extern "C"
