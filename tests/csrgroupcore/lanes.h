// The kernels of vartrix_amd/csrc/vtx_csr_group.hip with the lanes as loops and the tile as an array, over vtx_csr_group_core.h: what
// harness.cpp (a shared object for ctypes) and main.cpp (a stand-alone program, also built under sanitizers) both run.  Host code only.
#ifndef CSRGROUP_LANES_H
#define CSRGROUP_LANES_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../vartrix_amd/csrc/vtx_csr_group_core.h"

namespace csrgroup {

constexpr uint32_t WAVE = vtxr::GROUP_WAVE;

struct StatsOut {          // nnz_out elements each; a NULL array is not written
    uint32_t *n_entries, *n_alt, *n_ref, *n_both;
    uint64_t *sum_alt, *sum_ref, *sum_unk;
};

// csr_group_check_kernel: the integer minimum over the lanes
inline uint32_t first_bad(const uint32_t* group, uint32_t n_minor, uint32_t n_groups) {
    uint32_t first = 0xFFFFFFFFu;
    for (uint32_t j = 0; j < n_minor; ++j)
        if (vtxr::label_bad(group[j], n_groups) && j < first) first = j;
    return first;
}

// csr_group_count_kernel (one wavefront per row, the tile a bitmap) and the exclusive sum: pos[0 .. n_major]
inline void count(const uint64_t* indptr, uint32_t n_major, const uint32_t* indices, const uint32_t* group, uint32_t n_groups,
                  std::vector<uint32_t>& pos) {
    pos.assign((size_t)n_major + 1, 0u);
    for (uint32_t r = 0; r < n_major; ++r) {
        const uint64_t begin = indptr[r], end = indptr[r + 1];
        vtxr::GroupBits t;
        memset(&t, 0xA5, sizeof t);                           // LDS holds what the last wavefront left
        uint32_t n = 0;
        if (begin == end) continue;
        for (uint32_t base = 0; base < n_groups; base += vtxr::GROUP_WINDOW) {
            const uint32_t bins = vtxr::window_bins(n_groups, base);
            for (uint32_t lane = 0; lane < WAVE; ++lane)
                if (lane < vtxr::GROUP_WINDOW / 32) vtxr::bits_zero(t, lane);
            for (uint32_t lane = 0; lane < WAVE; ++lane)
                for (uint64_t k = begin + lane; k < end; k += WAVE) {
                    uint32_t b;
                    if (vtxr::window_slot(group[indices[k]], base, bins, &b)) vtxr::bits_set(t, b);
                }
            n += vtxr::bits_count(t);
        }
        pos[r] = n;
    }
    uint32_t run = 0;
    for (auto& x : pos) { const uint32_t f = x; x = run; run += f; }
}

// csr_group_fill_kernel.  stores (nnz_out bytes, may be NULL) counts the lanes that store into each output slot.
inline void fill(const uint64_t* indptr, uint32_t n_major, const uint32_t* indices, const uint32_t* alt, const uint32_t* ref, const uint32_t* unk,
                 const uint32_t* group, uint32_t n_groups, const std::vector<uint32_t>& pos, uint64_t* indptr_out, uint32_t* indices_out,
                 const StatsOut& out, uint8_t* stores) {
    for (uint64_t r = 0; r <= n_major; ++r) {
        const uint32_t first = pos[r];
        indptr_out[r] = first;
        if (r == n_major) break;
        const uint64_t begin = indptr[r], end = indptr[r + 1];
        if (begin == end) continue;
        vtxr::GroupTile t;
        memset(&t, 0xA5, sizeof t);                           // LDS holds what the last wavefront left
        uint32_t rank = 0;
        for (uint32_t base = 0; base < n_groups; base += vtxr::GROUP_WINDOW) {
            const uint32_t bins = vtxr::window_bins(n_groups, base);
            for (uint32_t lane = 0; lane < WAVE; ++lane)
                for (uint32_t b = lane; b < bins; b += WAVE) vtxr::tile_zero(t, b);
            for (uint32_t lane = 0; lane < WAVE; ++lane)
                for (uint64_t k = begin + lane; k < end; k += WAVE) {
                    uint32_t b;
                    if (vtxr::window_slot(group[indices[k]], base, bins, &b)) vtxr::tile_add(t, b, alt[k], ref[k], unk[k]);
                }
            for (uint32_t b0 = 0; b0 < bins; b0 += WAVE) {
                uint64_t ballot = 0;
                for (uint32_t lane = 0; lane < WAVE; ++lane)
                    if (b0 + lane < bins && t.n_entries[b0 + lane] != 0u) ballot |= 1ull << lane;
                for (uint32_t lane = 0; lane < WAVE; ++lane) {
                    if (!(ballot >> lane & 1ull)) continue;
                    const uint32_t b = b0 + lane;
                    const uint64_t q = (uint64_t)first + rank + vtxr::step_rank(ballot, lane);
                    const vtxr::RowStats s = vtxr::tile_read(t, b);
                    if (stores && stores[q] < 255) ++stores[q];
                    if (indices_out) indices_out[q] = base + b;
                    if (out.n_entries) out.n_entries[q] = s.n_entries;
                    if (out.n_alt) out.n_alt[q] = s.n_alt;
                    if (out.n_ref) out.n_ref[q] = s.n_ref;
                    if (out.n_both) out.n_both[q] = s.n_both;
                    if (out.sum_alt) out.sum_alt[q] = s.sum_alt;
                    if (out.sum_ref) out.sum_ref[q] = s.sum_ref;
                    if (out.sum_unk) out.sum_unk[q] = s.sum_unk;
                }
                rank += vtxr::popcount64(ballot);
            }
        }
    }
}

}  // namespace csrgroup
#endif
