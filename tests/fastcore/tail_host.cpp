// tail_host.cpp — HOST check and census of band_diag_kernel's deferral to band_tail_kernel (vtx_fast_core.h: closure_first, tail_pack,
// tail_unpack, back_rest).  TEST / MEASUREMENT INFRASTRUCTURE: tests/test_tail_record.py and tools/tail_census.py compile it themselves.
//   g++ -O2 -std=c++17 -fPIC -shared -o libtail_host.so tests/fastcore/tail_host.cpp
#include "fastcore_host.cpp"

namespace {
// what the routing of a task reads once its last phase is over (vtx_band.hip: diag_route)
struct Outcome {
    int32_t sc; uint32_t why, aux, pack; int cert; vtxf::M192 far;
    bool operator==(const Outcome& o) const {
        bool f = true;
        for (int k = 0; k < vtxf::NW; ++k) f = f && far.w[k] == o.far.w[k];
        return f && sc == o.sc && why == o.why && aux == o.aux && pack == o.pack && cert == o.cert;
    }
};
template <class LN> Outcome outcome(const vtxf::Front& fr, int ns, const LN& ln, int32_t sc, uint32_t why, uint32_t aux) {
    return Outcome{sc, why, aux, vtxf::band_pack(fr), fr.cert, vtxf::far_rows(fr.d, ns, ln)};
}
constexpr int N_T = 6;
const int kThresholds[N_T] = {8, 12, 16, 20, 24, 28};

// one wavefront's 64 consecutive tasks: per lane (-1: not in the last phase) its costs
struct WaveAcc {
    int scans_all = 0, scans_kept = 0, pairs_all = 0, pairs_kept = 0, work_all = 0, work_kept = 0, any_deferred = 0;
    int ns2_all = 0, ns2_kept[N_T] = {0, 0, 0, 0, 0, 0};
};
}  // namespace

extern "C" {
// Every task of the batch (task order: 2 * record + haplotype, band_diag_kernel's lanes) through the front, the probes, the sort and the
// harmless tests as band_diag_kernel runs them; a task that reaches the closure goes BOTH ways: uninterrupted back_rest, and the deferral
// (closure_first; when >= 0: tail_pack into a record, tail_unpack into a poisoned lane, back_rest again as band_tail_kernel runs it).
// out (uint64[64]):  0 tasks  1 tasks in the closure  2 deferred  3 outcomes that differ  4 deferred tasks with aux != 0xffffffff
//   5 wavefronts  6 / 7 sum over the wavefronts of the largest closure scan count (all lanes / without the deferred ones)
//   8 / 9 the same for (r + ng)^2, the piece pairs of one fixpoint pass  10 wavefronts with a deferred lane
//   11 / 12 the same for scans x ns (match visits of the closure)  13 tasks with ns > SMAX  14 tasks that failed the harmless tests
//   16 + i  tasks in the sort with ns > kThresholds[i]  23 sum over wavefronts of the largest ns^2 (the sort's insertion steps, all lanes)
//   24 + i  the same without the lanes with ns > kThresholds[i]  30 tasks in the sort
int vtxt_tail_census(const vtx_batch* b, int wide, uint64_t* out) {
    using namespace vtxf;
    const uint32_t n_heads = 1024;
    uint32_t max_hap = 8;
    for (uint32_t l = 0; l < b->n_loci; ++l) max_hap = std::max(max_hap, std::max(b->loci[l].ref_len, b->loci[l].alt_len));
    const bool narrow = max_hap <= 255 && !wide;
    const uint32_t stride = tab_stride(max_hap, n_heads);
    std::vector<uint8_t> gt((size_t)2 * stride + 64);
    std::vector<uint8_t> readbuf;
    uint32_t lane[LANE_WORDS], lane_b[LANE_WORDS], lane_c[LANE_WORDS], generic[GM], gen_b[GM], gen_c[GM];
    uint32_t rec[TAIL_WORDS];
    memset(out, 0, 64 * sizeof(uint64_t));
    WaveAcc wa;
    uint64_t task = 0;
    auto close_wave = [&]() {
        out[5]++;
        out[6] += (uint64_t)wa.scans_all; out[7] += (uint64_t)wa.scans_kept;
        out[8] += (uint64_t)wa.pairs_all; out[9] += (uint64_t)wa.pairs_kept;
        out[10] += (uint64_t)wa.any_deferred;
        out[11] += (uint64_t)wa.work_all; out[12] += (uint64_t)wa.work_kept;
        out[23] += (uint64_t)wa.ns2_all;
        for (int i = 0; i < N_T; ++i) out[24 + i] += (uint64_t)wa.ns2_kept[i];
        wa = WaveAcc();
    };
    auto one = [&](auto ln, auto ln_b, auto ln_c, const uint8_t* x, int m, const Tab& tb, int n) {
        const bool tw = narrow && tab_has_twins(tb);
        const Front fr = front(x, m, tb, n, ln, tw);
        if (fr.why != W_OK || whole_read(fr, m)) return;
        const int ns = probe_rows(x, tb, fr, ln, tw ? twin_matches(tb, fr, m, ln) : 0);
        if (ns > decltype(ln)::SMAX) { out[13]++; return; }
        out[30]++;
        wa.ns2_all = std::max(wa.ns2_all, ns * ns);
        for (int i = 0; i < N_T; ++i) {
            if (ns > kThresholds[i]) out[16 + i]++;
            else wa.ns2_kept[i] = std::max(wa.ns2_kept[i], ns * ns);
        }
        back_sort(ns, ln);
        if (!back_harmless(fr, ns, ln)) { out[14]++; return; }
        out[1]++;
        memcpy(lane_b, lane, sizeof lane);
        // uninterrupted
        for (int i = 0; i < GM; ++i) generic[i] = 0xffffffffu;
        uint32_t why_a = W_OK, aux_a = 0;
        const int32_t sc_a = back_rest(fr, ns, ln, Lane{generic, 1}, &why_a, 0, nullptr, &aux_a);
        const Outcome oa = outcome(fr, ns, ln, sc_a, why_a, aux_a);
        int ng = 0;
        while (ng < GM && generic[ng] != 0xffffffffu) ++ng;
        // deferred or not, as band_diag_kernel decides
        const int first = closure_first(fr, ns, ln_b);
        Outcome ob;
        if (first >= 0) {
            out[2]++;
            for (int i = 0; i < TAIL_WORDS; ++i) rec[i] = 0xdeadbeefu;
            tail_pack(rec, 1, (uint32_t)task, fr, ns, ln_b);
            memset(lane_c, 0xa5, sizeof lane_c);
            memset(gen_c, 0x5a, sizeof gen_c);
            Front fc;
            int nc = -1;
            uint32_t pack = 0, why_b = W_OK, aux_b = 0;
            const uint32_t t = tail_unpack(rec, 1, fc, nc, ln_c, &pack);
            const int32_t sc_b = back_rest(fc, nc, ln_c, Lane{gen_c, 1}, &why_b, 0, nullptr, &aux_b);
            ob = outcome(fc, nc, ln_c, sc_b, why_b, aux_b);
            if (t != (uint32_t)task || nc != ns || pack != oa.pack) out[3]++;
            if (aux_b != 0xffffffffu) out[4]++;
        } else {
            uint32_t why_b = W_OK, aux_b = 0;
            for (int i = 0; i < GM; ++i) gen_b[i] = 0x5a5a5a5au;
            const int32_t sc_b = back_rest(fr, ns, ln_b, Lane{gen_b, 1}, &why_b, 0, nullptr, &aux_b, first);
            ob = outcome(fr, ns, ln_b, sc_b, why_b, aux_b);
        }
        if (!(oa == ob)) out[3]++;
        // costs: closure scans (ng + 1), pairs of one fixpoint pass ((r + ng)^2; ng = 0: the main-only bound, r^2 in registers)
        const int scans = ng + 1, pairs = (fr.r + ng) * (fr.r + ng), work = scans * ns;
        wa.scans_all = std::max(wa.scans_all, scans); wa.pairs_all = std::max(wa.pairs_all, pairs); wa.work_all = std::max(wa.work_all, work);
        if (first >= 0) wa.any_deferred = 1;
        else { wa.scans_kept = std::max(wa.scans_kept, scans); wa.pairs_kept = std::max(wa.pairs_kept, pairs); wa.work_kept = std::max(wa.work_kept, work); }
    };
    for (uint32_t l = 0; l < b->n_loci; ++l) {
        const vtx_locus& L = b->loci[l];
        build_table(gt.data(), b->hap_arena + L.ref_off, L.ref_len, max_hap, n_heads);
        build_table(gt.data() + stride, b->hap_arena + L.alt_off, L.alt_len, max_hap, n_heads);
        for (uint32_t r = L.rec_begin; r < L.rec_begin + L.rec_count; ++r) {
            const vtx_record& R = b->records[r];
            readbuf.assign(R.read_len + 16, 0);
            memcpy(readbuf.data(), b->read_arena + R.read_off, R.read_len);
            for (int h = 0; h < 2; ++h, ++task) {
                if (task % 64 == 0 && task) close_wave();
                out[0]++;
                Tab tb;
                tb.gt = gt.data(); tb.ent = (uint32_t)h * stride; tb.head = tb.ent + max_hap * 8;
                tb.bytes = tb.ent + tab_bytes_off(max_hap, n_heads); tb.uq = tb.ent + tab_uq_off(max_hap, n_heads);
                tb.pb = tb.ent + tab_pb_off(max_hap, n_heads); tb.hmask = n_heads - 1;
                const int m = (int)R.read_len, n = (int)(h ? L.alt_len : L.ref_len);
                if (m < K || n < K || m > 64 * NW) continue;
                if (narrow)
                    one(LaneS<uint16_t>{lane + S_WORDS, 1, (uint16_t*)lane, 1}, LaneS<uint16_t>{lane_b + S_WORDS, 1, (uint16_t*)lane_b, 1},
                        LaneS<uint16_t>{lane_c + S_WORDS, 1, (uint16_t*)lane_c, 1}, readbuf.data(), m, tb, n);
                else
                    one(LaneS<uint32_t>{lane + S_WORDS, 1, lane, 1}, LaneS<uint32_t>{lane_b + S_WORDS, 1, lane_b, 1},
                        LaneS<uint32_t>{lane_c + S_WORDS, 1, lane_c, 1}, readbuf.data(), m, tb, n);
            }
        }
    }
    if (task % 64) close_wave();
    return 0;
}
}  // extern "C"
