// Host build of vartrix_amd/csrc/vtx_scan_core.h as a stand-alone program for tests/test_scan_core.py: what the record logic TOUCHES.
//   scan_host IN OUT   IN: u32 n, then n cases of { u32 kind, u32 bytes, payload }.  OUT: per case { u32 m, m bytes }.
//     kind 0  view_record    payload { u32 pre, u32 fill, record }                      -> 12 x i64 (as vtxs_t_view of scan_host.cpp)
//     kind 1  aux_string     payload { u32 pre, u32 fill, u32 tag, aux block }          -> u32 offset, u32 len
//     kind 2  scan_pairs     payload { u32 pre, u32 fill, u32 filter[5], u32 n_ref, u32 ni, i32 start[ni], i32 end[ni],
//                                      u32 tid_begin[n_ref + 1], i32 tid_span[n_ref], record }
//                                                                                       -> i32 n, u32 verdict[11], n x { u32 k, u32 outcome }
//     kind 3  chain walk     payload { u64 p, u64 stop, data }                          -> u32 records, u32 bad, u64 p at the end
// Kinds 0-2: the record (or aux block) is the LAST thing of an inflated buffer of exactly pre + size + 64 bytes (d_bam_data's slack),
// the other bytes filled with `fill`; the interval tables are exactly their sizes.  Kind 3: the walk of bam_chain_kernel /
// bam_chain_seg_kernel over a buffer of exactly `limit` bytes: nothing at or beyond limit may be read.  Under the sanitizer build
// (`make scan_host_san`) the red zone starts where each allocation ends.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../vartrix_amd/csrc/vtx_scan_core.h"

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
template <class T> void put(std::vector<uint8_t>& out, const T& v) { out.insert(out.end(), (const uint8_t*)&v, (const uint8_t*)&v + sizeof v); }
template <class T> T* exact(const uint8_t* src, size_t n) {          // a malloc of exactly n elements
    T* p = (T*)malloc(n * sizeof(T));
    if (!p && n) { fprintf(stderr, "out of memory\n"); exit(2); }
    if (n) memcpy(p, src, n * sizeof(T));
    return p;
}
// the bytes as the last thing of a buffer of pre + n + 64
uint8_t* place_last(const uint8_t* src, size_t n, uint32_t pre, uint32_t fill) {
    uint8_t* buf = (uint8_t*)malloc((size_t)pre + n + 64);
    if (!buf) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(buf, (int)(fill & 0xffu), (size_t)pre + n + 64);
    if (n) memcpy(buf + pre, src, n);
    return buf;
}

bool run_case(uint32_t kind, const uint8_t* q, size_t len, std::vector<uint8_t>& out) {
    uint32_t h[2];
    if (kind <= 2) { if (len < 8) return false; memcpy(h, q, 8); q += 8; len -= 8; }
    if (kind == 0) {
        uint8_t* buf = place_last(q, len, h[0], h[1]);
        const vtxs::RecView v = vtxs::view_record(buf, h[0]);
        const int64_t r[12] = {v.bs, v.tid, v.pos, v.endpos, v.mapq, v.flag, v.n_cig, v.l_seq, v.cig - v.r, v.sq - v.r, v.aux - v.r, v.malformed ? 1 : 0};
        put(out, r);
        free(buf);
    } else if (kind == 1) {
        if (len < 4) return false;
        uint32_t tag;
        memcpy(&tag, q, 4);
        uint8_t* buf = place_last(q + 4, len - 4, h[0], h[1]);
        uint32_t ln = 0;
        const uint32_t o = vtxs::aux_string(buf + h[0], (uint32_t)(len - 4), tag, &ln);
        put(out, o); put(out, ln);
        free(buf);
    } else if (kind == 2) {
        if (len < 28) return false;
        uint32_t f[7];
        memcpy(f, q, 28);
        q += 28; len -= 28;
        const uint32_t n_ref = f[5], ni = f[6];
        const size_t tables = 8 * (size_t)ni + 4 * ((size_t)n_ref + 1) + 4 * (size_t)n_ref;
        if (len < tables) return false;
        int32_t* st = exact<int32_t>(q, ni);
        int32_t* en = exact<int32_t>(q + 4 * (size_t)ni, ni);
        uint32_t* tb = exact<uint32_t>(q + 8 * (size_t)ni, (size_t)n_ref + 1);
        int32_t* sp = exact<int32_t>(q + 8 * (size_t)ni + 4 * ((size_t)n_ref + 1), n_ref);
        uint8_t* buf = place_last(q + tables, len - tables, h[0], h[1]);
        const vtxs::RecView v = vtxs::view_record(buf, h[0]);
        int32_t n = -1;
        vtxs::Verdict V;
        std::vector<uint32_t> pairs;
        if (!v.malformed) {
            const vtxs::Filter flt{f[0], f[1], f[2], f[3], f[4]};
            vtxs::scan_pairs<true>(v, flt, st, en, tb, sp, V, [&](uint32_t k, uint32_t outcome, uint32_t) { pairs.push_back(k); pairs.push_back(outcome); });
            n = (int32_t)(pairs.size() / 2);
        }
        const uint32_t vd[11] = {V.hits, V.reads, V.low_mapq, V.non_primary, V.duplicate, V.not_useful, V.no_barcode, V.bc_rel, V.umi_rel, V.bc_len, V.umi_len};
        put(out, n); put(out, vd);
        for (uint32_t x : pairs) put(out, x);
        free(buf); free(st); free(en); free(tb); free(sp);
    } else if (kind == 3) {
        if (len < 16) return false;
        uint64_t p, stop;
        memcpy(&p, q, 8); memcpy(&stop, q + 8, 8);
        const uint64_t limit = len - 16;
        uint8_t* data = exact<uint8_t>(q + 16, limit);
        uint32_t k = 0;
        bool bad = false;
        while (p < stop) {                       // (the loop of the two kernels)
            if (!vtxs::chain_step(data, p, limit)) { bad = true; break; }
            ++k;
        }
        const uint32_t b = bad || p != stop ? 1u : 0u;
        put(out, k); put(out, b); put(out, p);
        free(data);
    } else return false;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: scan_host IN OUT\n"); return 2; }
    std::vector<uint8_t> in, res;
    if (!read_file(argv[1], in) || in.size() < 4) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint32_t n;
    memcpy(&n, in.data(), 4);
    size_t p = 4;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t h[2];
        if (p + 8 > in.size()) { fprintf(stderr, "truncated case %u\n", i); return 2; }
        memcpy(h, in.data() + p, 8);
        p += 8;
        if (p + h[1] > in.size()) { fprintf(stderr, "truncated case %u\n", i); return 2; }
        std::vector<uint8_t> one;
        if (!run_case(h[0], in.data() + p, h[1], one)) { fprintf(stderr, "bad case %u\n", i); return 2; }
        p += h[1];
        put(res, (uint32_t)one.size());
        res.insert(res.end(), one.begin(), one.end());
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(res.data(), 1, res.size(), f) != res.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    return 0;
}
