// The kernels of vartrix_amd/csrc/vtx_csr_ops.hip with the lanes as loops, over vtx_csr_ops_core.h: what harness.cpp (a shared object
// for ctypes) and main.cpp (a stand-alone program, also built under sanitizers) both run.  Host code only.
#ifndef CSROPS_LANES_H
#define CSROPS_LANES_H
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../vartrix_amd/csrc/vtx_csr_ops_core.h"

namespace csrops {

struct StatsOut {          // n_major elements each; a NULL array is not written
    uint32_t *n_entries, *n_alt, *n_ref, *n_both;
    uint64_t *sum_alt, *sum_ref, *sum_unk;
};

// csr_row_stats_kernel<G>: wavefronts of 64 lanes, G lanes per row; the shuffles are reads of the partner lane's registers
inline void row_stats(const uint64_t* indptr, uint32_t n_major, const uint32_t* alt, const uint32_t* ref, const uint32_t* unk, uint32_t G,
                      const StatsOut& out) {
    const uint64_t lanes = (uint64_t)n_major * G;
    for (uint64_t w = 0; w * 64 < lanes; ++w) {
        vtxr::RowStats s[64], o[64];
        for (uint32_t l = 0; l < 64; ++l) {
            const uint64_t lane = w * 64 + l, r = lane / G;
            const bool live = r < n_major;
            s[l] = vtxr::stats_walk(alt, ref, unk, live ? indptr[r] : 0, live ? indptr[r + 1] : 0, (uint32_t)(lane % G), G);
        }
        for (uint32_t d = G / 2; d; d /= 2) {
            for (uint32_t l = 0; l < 64; ++l) o[l] = s[l ^ d];
            for (uint32_t l = 0; l < 64; ++l) vtxr::stats_merge(s[l], o[l]);
        }
        for (uint32_t l = 0; l < 64; ++l) {
            const uint64_t lane = w * 64 + l, r = lane / G;
            if (r >= n_major || lane % G) continue;
            if (out.n_entries) out.n_entries[r] = s[l].n_entries;
            if (out.n_alt) out.n_alt[r] = s[l].n_alt;
            if (out.n_ref) out.n_ref[r] = s[l].n_ref;
            if (out.n_both) out.n_both[r] = s[l].n_both;
            if (out.sum_alt) out.sum_alt[r] = s[l].sum_alt;
            if (out.sum_ref) out.sum_ref[r] = s[l].sum_ref;
            if (out.sum_unk) out.sum_unk[r] = s[l].sum_unk;
        }
    }
}

inline void exclusive_sum(std::vector<uint32_t>& v) {
    uint32_t run = 0;
    for (auto& x : v) { const uint32_t f = x; x = run; run += f; }
}

struct Maps { std::vector<uint32_t> major_map, minor_map, pos; };

// csr_mask_flags_kernel (twice) and csr_keep_flags_kernel, each followed by its exclusive sum: the plan
inline void scans(const uint64_t* indptr, uint32_t n_major, uint32_t n_minor, const uint32_t* indices, uint64_t nnz, const uint8_t* keep_major,
                  const uint8_t* keep_minor, Maps& m, uint32_t sizes[3]) {
    m.major_map.assign((size_t)n_major + 1, 0u); m.minor_map.assign((size_t)n_minor + 1, 0u); m.pos.assign(nnz + 1, 0u);
    for (uint64_t i = 0; i < n_major; ++i) m.major_map[i] = vtxr::mask_keeps(keep_major, i);
    for (uint64_t i = 0; i < n_minor; ++i) m.minor_map[i] = vtxr::mask_keeps(keep_minor, i);
    for (uint64_t k = 0; k < nnz; ++k)
        m.pos[k] = vtxr::keep_entry(keep_major, keep_minor, keep_major ? vtxr::row_of(indptr, n_major, k) : 0u, indices[k]);
    exclusive_sum(m.major_map); exclusive_sum(m.minor_map); exclusive_sum(m.pos);
    sizes[0] = m.major_map[n_major]; sizes[1] = m.minor_map[n_minor]; sizes[2] = m.pos[nnz];
}

// csr_select_offsets_kernel, csr_select_ids_kernel (twice), csr_select_place_kernel with one 4-byte and one 8-byte payload.
// writes[slot] (n_major_out + 1 bytes, may be NULL) counts the stores into indptr_out.
inline void place(const uint64_t* indptr, uint32_t n_major, uint32_t n_minor, const uint32_t* indices, uint64_t nnz, const uint8_t* keep_major,
                  const uint8_t* keep_minor, const Maps& m, uint64_t* indptr_out, uint8_t* writes, uint32_t* indices_out, uint32_t* major_ids,
                  uint32_t* minor_ids, const uint32_t* pay32_in, uint32_t* pay32_out, const uint64_t* pay64_in, uint64_t* pay64_out) {
    for (uint64_t r = 0; r <= n_major; ++r) {
        if (!vtxr::select_offset_lane(r, n_major, keep_major)) continue;
        indptr_out[m.major_map[r]] = m.pos[indptr[r]];
        if (writes && writes[m.major_map[r]] < 255) ++writes[m.major_map[r]];
    }
    for (uint64_t i = 0; major_ids && i < n_major; ++i) if (vtxr::mask_keeps(keep_major, i)) major_ids[m.major_map[i]] = (uint32_t)i;
    for (uint64_t i = 0; minor_ids && i < n_minor; ++i) if (vtxr::mask_keeps(keep_minor, i)) minor_ids[m.minor_map[i]] = (uint32_t)i;
    for (uint64_t k = 0; k < nnz; ++k) {
        const uint32_t q = m.pos[k];
        if (m.pos[k + 1] == q) continue;
        if (indices_out) indices_out[q] = m.minor_map[indices[k]];
        if (pay32_out) pay32_out[q] = pay32_in[k];
        if (pay64_out) pay64_out[q] = pay64_in[k];
    }
}

}  // namespace csrops
#endif
