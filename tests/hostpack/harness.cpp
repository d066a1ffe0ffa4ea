// Stand-alone host program for tests/test_host_pack_pinned.py: one call of the packer through its public interface, built with
// AddressSanitizer + UBSan and with ThreadSanitizer (tests/hostpack/Makefile).
//   host_pack_*san VCF BAM FASTA BARCODES cooked|raw|plan THREADS      (use_umi on, nibbles, every other option at its default)
// stdout gets the bytes the test's digest is taken over (pack_stream / plan_stream there): per batch loci, records, hap_arena,
// read_arena (raw: and tag_arena) — or the plan's arrays without compressed offsets and sizes — then "metrics" and the nine counts,
// n_variants, the barcodes and the variant names, a line each.  Exit 1 with the packer's message when the call fails.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../include/vtx_host.h"

namespace {
void put(const void* p, size_t n) { if (n) fwrite(p, 1, n, stdout); }

void put_tail(const vtxh_pack* P) {
    vtxh_metrics m;
    vtxh_get_metrics(P, &m);
    const uint64_t nine[9] = {m.num_reads, m.num_low_mapq, m.num_non_primary, m.num_duplicates, m.num_not_cell_bc,
                              m.num_not_useful, m.num_non_umi, m.num_invalid_recs, m.num_multiallelic_recs};
    put("metrics", 7);
    put(nine, sizeof nine);
    const uint32_t nv = vtxh_num_variants(P), nb = vtxh_num_barcodes(P);
    put(&nv, 4);
    for (uint32_t j = 0; j < nb; ++j) { const std::string s = std::string(vtxh_barcode(P, j)) + "\n"; put(s.data(), s.size()); }
    for (uint32_t i = 0; i < nv; ++i) { const std::string s = std::string(vtxh_variant_name(P, i)) + "\n"; put(s.data(), s.size()); }
}

void put_plan(const vtxh_pack* P) {
    const uint32_t kind = (uint32_t)vtxh_plan_kind(P);
    vtx_bam_segments sg;
    vtx_bam_ingest one;
    const int rc = kind == VTXH_PLAN_SEGMENTED ? vtxh_get_ingest_segments(P, &sg) : vtxh_get_ingest(P, &one);
    const vtx_bam_ingest& g = kind == VTXH_PLAN_SEGMENTED ? sg.base : one;
    put(&kind, 4);
    const std::string reason = std::string(rc == 0 ? "" : vtxh_last_error()) + "\n";
    put(reason.data(), reason.size());
    if (rc != 0) return;
    for (uint32_t b = 0; b < g.n_blocks; ++b) put(&g.blocks[b].isize, 4);
    put(g.seeds, 8 * (size_t)g.n_seeds);
    put(&g.end_upos, 8);
    if (kind == VTXH_PLAN_SEGMENTED) {
        put(sg.segments, sizeof(vtx_bam_segment) * (size_t)sg.n_segments);
        put(&sg.contiguous_blocks, 4);
        put(&sg.contiguous_inflated, 8);
    }
    put(g.intervals, sizeof(vtx_bam_interval) * (size_t)g.n_intervals);
    put(g.tid_begin, 4 * ((size_t)g.n_ref + 1));
    put(g.tid_max_span, 4 * (size_t)g.n_ref);
    put(g.loci, sizeof(vtx_locus) * (size_t)g.n_loci);
    put(g.hap_arena, (size_t)g.hap_bytes);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 7) { fprintf(stderr, "usage: %s VCF BAM FASTA BARCODES cooked|raw|plan THREADS\n", argv[0]); return 2; }
    const std::string mode = argv[5];
    vtxh_args a;
    memset(&a, 0, sizeof a);
    a.vcf = argv[1]; a.bam = argv[2]; a.fasta = argv[3]; a.cell_barcodes = argv[4];
    a.padding = 100; a.use_umi = 1; a.bam_tag = "CB"; a.valid_chars = "ATGCatgc"; a.threads = atoi(argv[6]);
    a.read_format = VTX_READS_NIBBLES;
    vtxh_pack* P = nullptr;
    int rc;
    if (mode == "plan") rc = vtxh_plan_ingest(&a, 0, 0xffffffffu, &P);
    else if (mode == "raw") rc = vtxh_pack_files_raw(&a, &P);
    else if (mode == "cooked") rc = vtxh_pack_files(&a, &P);
    else { fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
    if (rc != 0) { fprintf(stderr, "%d: %s\n", rc, vtxh_last_error()); return 1; }
    if (mode == "plan") put_plan(P);
    const size_t rdiv = vtxh_read_format(P) == VTX_READS_NIBBLES ? 2 : 1;
    for (uint32_t i = 0; mode != "plan" && i < vtxh_num_batches(P); ++i) {
        if (mode == "raw") {
            vtx_raw_batch b;
            vtxh_get_raw_batch_at(P, i, &b);
            put(b.loci, sizeof(vtx_locus) * (size_t)b.n_loci);
            put(b.records, sizeof(vtx_raw_record) * (size_t)b.n_records);
            put(b.hap_arena, (size_t)b.hap_bytes);
            put(b.read_arena, (size_t)b.read_bytes / rdiv);
            put(b.tag_arena, (size_t)b.tag_bytes);
        } else {
            vtx_batch b;
            vtxh_get_batch_at(P, i, &b);
            put(b.loci, sizeof(vtx_locus) * (size_t)b.n_loci);
            put(b.records, sizeof(vtx_record) * (size_t)b.n_records);
            put(b.hap_arena, (size_t)b.hap_bytes);
            put(b.read_arena, (size_t)b.read_bytes / rdiv);
        }
    }
    put_tail(P);
    vtxh_free(P);
    vtxh_trim();
    return fflush(stdout) == 0 ? 0 : 1;
}
