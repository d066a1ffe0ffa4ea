// Host build of vartrix_amd/csrc/vtx_ingest_plan_core.h for tests/test_ingest_plan_core.py: the checks and the rewrite vtx_submit_bam /
// vtx_submit_bam_segments run on a caller's plan, in the API's order but for the loci's haplotypes (check_loci_haps stays in vtx_api.hip,
// between the two calls below).  No device code, no sanitizer: a shared object ctypes loads.
#include <string.h>

#include "../../vartrix_amd/csrc/vtx_ingest_plan_core.h"

namespace {
struct Result {
    int status = VTX_OK;
    char why[512] = {0};
    uint32_t ni = 0, nref = 0;
    vtxp::Layout L;
};
}  // namespace

extern "C" {

// sg == NULL: the contiguous plan g; else the segmented plan sg (g is ignored: the base is sg->base)
void* ipc_plan(const vtx_bam_ingest* g, const vtx_bam_segments* sg) {
    if (sg) g = &sg->base;
    Result* r = new Result;
    r->ni = g->n_intervals; r->nref = g->n_ref;
    r->status = vtxp::check_arrays(*g, r->why, sizeof r->why);
    if (r->status == VTX_OK) r->status = vtxp::layout(*g, sg, r->L, r->why, sizeof r->why);
    return r;
}
int ipc_status(const void* h) { return ((const Result*)h)->status; }
const char* ipc_why(const void* h) { return ((const Result*)h)->why; }
void ipc_free(void* h) { delete (Result*)h; }

// out[10]: the element counts of blocks, segs, seed_seg, pieces, iv; then lo, hi, utotal, comp_bytes, end_upos
void ipc_figures(const void* h, uint64_t* out) {
    const vtxp::Layout& L = ((const Result*)h)->L;
    const uint64_t f[10] = {L.blocks.size(), L.segs.size(), L.seed_seg.size(), L.pieces.size(), L.iv.size(), L.lo, L.hi, L.utotal, L.comp_bytes, L.end_upos};
    memcpy(out, f, sizeof f);
}

// which: 0 blocks (vtxg_block), 1 segs (vtxg_segment), 2 seed_seg (u32), 3 pieces (3 x u64), 4 the packed interval array (u32); and its
// five sub-arrays THROUGH THE ACCESSORS the device side uses: 5 start, 6 end (i32), 7 locus, 8 tid_begin (u32), 9 tid_span (i32)
const void* ipc_array(void* h, int which) {
    Result* r = (Result*)h;
    const vtxp::IntervalArrays a = r->L.intervals(r->ni, r->nref);
    switch (which) {
    case 0: return r->L.blocks.data();
    case 1: return r->L.segs.data();
    case 2: return r->L.seed_seg.data();
    case 3: return r->L.pieces.data();
    case 4: return r->L.iv.data();
    case 5: return a.start();
    case 6: return a.end();
    case 7: return a.locus();
    case 8: return a.tid_begin();
    case 9: return a.tid_span();
    }
    return nullptr;
}

// the layouts the device's kernels and the tests' dtypes are written against
void ipc_sizes(uint32_t* out) { out[0] = sizeof(vtxg_block); out[1] = sizeof(vtxg_segment); out[2] = sizeof(vtxp::Piece); }

}
