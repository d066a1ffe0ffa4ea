// Host build of vartrix_amd/csrc/vtx_ingest_plan_core.h as a stand-alone program for tests/test_ingest_plan_core.py: what the checks TOUCH.
//   ingest_plan_host IN OUT
//   IN:  u32 n_cases, then per case { u32 has_segments, n_blocks, n_ref, n_seeds, n_intervals, n_loci, n_segments, null_mask, 0;
//        u64 file_bytes, end_upos, hap_bytes; n_blocks x vtx_bgzf_block; n_seeds x u64; n_intervals x vtx_bam_interval; (n_ref + 1) x u32
//        tid_begin; n_ref x i32 tid_max_span; n_segments x vtx_bam_segment }.  null_mask: the pointers handed over as NULL whatever the
//        counts say — bit 0 file, 1 blocks, 2 seeds, 3 intervals, 4 tid_begin, 5 tid_max_span, 6 loci, 7 hap_arena, 8 segments.
//   OUT per case: i32 status; on a reject u32 length + the message; else 10 x u64 (the element counts of blocks, segs, seed_seg, pieces, iv;
//        lo, hi, utotal, comp_bytes, end_upos) and those five arrays.
// Every array the checks may read is an allocation of exactly the stated size: under the sanitizer build (`make ingest_plan_host_san`) a
// check that follows an index of the plan before it has bounded it — the rejects of the test's table point one past their arrays — is an
// error.  The file and the hap arena are one byte each: the core hands them on, it never reads them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../vartrix_amd/csrc/vtx_ingest_plan_core.h"

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

// exactly count * sizeof(T) bytes (one when 0, so that the pointer is a real allocation) from the input
template <typename T> T* take(const std::vector<uint8_t>& in, size_t& p, size_t count) {
    const size_t bytes = count * sizeof(T);
    if (p + bytes > in.size()) { fprintf(stderr, "truncated input\n"); exit(2); }
    T* a = (T*)malloc(bytes ? bytes : 1);
    if (!a) { fprintf(stderr, "out of memory\n"); exit(2); }
    if (bytes) memcpy(a, in.data() + p, bytes);
    p += bytes;
    return a;
}

template <typename T> void put(FILE* f, const T* a, size_t count) {
    if (count && fwrite(a, sizeof(T), count, f) != count) { fprintf(stderr, "cannot write the output\n"); exit(2); }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: ingest_plan_host IN OUT\n"); return 2; }
    std::vector<uint8_t> in;
    if (!read_file(argv[1], in) || in.size() < 4) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE* f = fopen(argv[2], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    uint32_t n_cases;
    memcpy(&n_cases, in.data(), 4);
    size_t p = 4;
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint32_t* h = take<uint32_t>(in, p, 9);
        uint64_t* q = take<uint64_t>(in, p, 3);
        const uint32_t has_sg = h[0], nb = h[1], nref = h[2], ns = h[3], ni = h[4], nl = h[5], nseg = h[6], nulls = h[7];
        vtx_bgzf_block* blocks = take<vtx_bgzf_block>(in, p, nb);
        uint64_t* seeds = take<uint64_t>(in, p, ns);
        vtx_bam_interval* intervals = take<vtx_bam_interval>(in, p, ni);
        uint32_t* tid_begin = take<uint32_t>(in, p, (size_t)nref + 1);
        int32_t* tid_max_span = take<int32_t>(in, p, nref);
        vtx_bam_segment* segments = take<vtx_bam_segment>(in, p, nseg);
        vtx_locus* loci = (vtx_locus*)calloc(nl ? nl : 1, sizeof(vtx_locus));
        uint8_t *file = (uint8_t*)malloc(1), *hap = (uint8_t*)malloc(1);
        auto unless = [&](int bit, auto* ptr) { return (nulls >> bit) & 1 ? (decltype(ptr))nullptr : ptr; };
        vtx_bam_segments sg;
        memset(&sg, 0, sizeof sg);
        vtx_bam_ingest& g = sg.base;
        g.file = unless(0, file); g.file_bytes = q[0]; g.blocks = unless(1, blocks); g.n_blocks = nb; g.n_ref = nref;
        g.seeds = unless(2, seeds); g.n_seeds = ns; g.n_intervals = ni; g.end_upos = q[1]; g.intervals = unless(3, intervals);
        g.tid_begin = unless(4, tid_begin); g.tid_max_span = unless(5, tid_max_span); g.loci = unless(6, loci); g.n_loci = nl;
        g.hap_arena = unless(7, hap); g.hap_bytes = q[2];
        sg.segments = unless(8, segments); sg.n_segments = nseg;

        vtxp::Layout L;
        char why[512] = {0};
        int32_t status = vtxp::check_arrays(g, why, sizeof why);
        if (status == VTX_OK) status = vtxp::layout(g, has_sg ? &sg : nullptr, L, why, sizeof why);
        put(f, &status, 1);
        if (status != VTX_OK) {
            const uint32_t len = (uint32_t)strlen(why);
            put(f, &len, 1); put(f, why, len);
        } else {
            const uint64_t fig[10] = {L.blocks.size(), L.segs.size(), L.seed_seg.size(), L.pieces.size(), L.iv.size(), L.lo, L.hi, L.utotal, L.comp_bytes, L.end_upos};
            put(f, fig, 10); put(f, L.blocks.data(), L.blocks.size()); put(f, L.segs.data(), L.segs.size()); put(f, L.seed_seg.data(), L.seed_seg.size());
            put(f, L.pieces.data(), L.pieces.size()); put(f, L.iv.data(), L.iv.size());
        }
        free(h); free(q); free(blocks); free(seeds); free(intervals); free(tid_begin); free(tid_max_span); free(segments); free(loci); free(file); free(hap);
    }
    if (fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    return 0;
}
