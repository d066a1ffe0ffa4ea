// recheck_host.cpp — HOST mirror of band_diag_kernel's first stage WITH the recheck of the tasks that fail its harmless test
// (vtx_fast_core.h: tail_pack, tail_unpack, LaneSR, recheck_rest; vtx_band.hip: band_tail_kernel's recheck mode).
// TEST / MEASUREMENT INFRASTRUCTURE: tests/test_recheck_core.py, tests/test_gpu_recheck.py and tools/recheck_census.py compile it themselves.
//   g++ -O2 -std=c++17 -fPIC -shared -o librecheck_host.so tests/fastcore/recheck_host.cpp
#include "fastcore_host.cpp"

extern "C" {
// route[t], bit by bit — what became of task t = 2 * record + haplotype:
enum : uint8_t {
    RK_LOOSE_FAILED = 1,     // band_diag_kernel's harmless test (one running maximum) failed: the task left a recheck record
    RK_CLEARED = 2,          // the tight test on the record's list (packed, unpacked into a poisoned lane) cleared it
    RK_CLEARED_DIRECT = 4,   // back_harmless<TIGHT> run directly on the lane's own list cleared it (must equal RK_CLEARED)
    RK_DECIDED = 8,          // cert == ub: score[t] is final (a bound of the FULL score)
    RK_BAND = 16,            // the task keeps its certificate and a one-diagonal band: pack[t] = vtxf::band_pack, score[t] = the certificate ...
    RK_CORRIDOR = 32,        // ... and band_corridor_kernel's bound decided it: score[t] is the BANDED score
};
// Every task of the batch as band_diag_kernel, band_tail_kernel's recheck mode and band_corridor_kernel treat it (two-byte match entries:
// every haplotype <= 255 bases, else -1).  why[t]: W_OK for a decided task, the reason otherwise (W_NOT_HARMLESS: not cleared either).
// recheck == 0: without the recheck (a task that fails the first test leaves with W_NOT_HARMLESS), for the census.
int vtxt_recheck_batch(const vtx_batch* b, int recheck, int32_t* score, uint32_t* why, uint8_t* route, uint32_t* pack) {
    using namespace vtxf;
    const uint32_t n_heads = 1024;
    uint32_t max_hap = 8;
    for (uint32_t l = 0; l < b->n_loci; ++l) max_hap = std::max(max_hap, std::max(b->loci[l].ref_len, b->loci[l].alt_len));
    if (max_hap > 255) return -1;
    const uint32_t stride = tab_stride(max_hap, n_heads);
    std::vector<uint8_t> gt((size_t)2 * stride + 64);
    std::vector<uint8_t> readbuf;
    typedef LaneS<uint16_t> L1;
    typedef LaneSR<uint16_t> LR;
    uint32_t lane[LANE_WORDS], lane_c[LANE_WORDS], lane_d[LANE_WORDS], generic[GM], rec[TAIL_WORDS];
    uint8_t ub_c[LR::SMAX], ub_d[LR::SMAX];
    for (uint32_t l = 0; l < b->n_loci; ++l) {
        const vtx_locus& L = b->loci[l];
        build_table(gt.data(), b->hap_arena + L.ref_off, L.ref_len, max_hap, n_heads);
        build_table(gt.data() + stride, b->hap_arena + L.alt_off, L.alt_len, max_hap, n_heads);
        for (uint32_t r = L.rec_begin; r < L.rec_begin + L.rec_count; ++r) {
            const vtx_record& R = b->records[r];
            readbuf.assign(R.read_len + 16, 0);
            memcpy(readbuf.data(), b->read_arena + R.read_off, R.read_len);
            const uint8_t* x = readbuf.data();
            const int m = (int)R.read_len;
            Tab tbs[2];
            int ns2[2], dd[2] = {0, 0};
            bool live[2], have_d[2];
            for (int h = 0; h < 2; ++h) {
                Tab& tb = tbs[h];
                tb.gt = gt.data(); tb.ent = (uint32_t)h * stride; tb.head = tb.ent + max_hap * 8;
                tb.bytes = tb.ent + tab_bytes_off(max_hap, n_heads); tb.uq = tb.ent + tab_uq_off(max_hap, n_heads);
                tb.pb = tb.ent + tab_pb_off(max_hap, n_heads); tb.hmask = n_heads - 1;
                ns2[h] = (int)(h ? L.alt_len : L.ref_len);
                live[h] = m >= K && ns2[h] >= K && m <= MAX_READ;
                have_d[h] = !live[h];
            }
            // The main diagonal as band_diag_kernel's lanes find it (not vtxf::front's search, one lane on its own): the two lanes of a
            // record look ONE sample row up per round, each in its own table, and try both candidates; the first that passes verify_diag
            // is the lane's diagonal, and its mask must hold 20 matching bases.
            for (int round = 0; round < N_SAMPLES / 2; ++round) {
                int cand[2];
                for (int h = 0; h < 2; ++h) cand[h] = have_d[h] ? NO_DIAG : cand_diag(x, sample_row(2 * round + h, m), tbs[h]);
                for (int h = 0; h < 2; ++h)
                    for (int u = 0; u < 2; ++u) {
                        const int dc = u ? cand[h ^ 1] : cand[h];
                        if (have_d[h] || dc == NO_DIAG || dc < -(m - K) || dc > ns2[h] - K) continue;
                        if (verify_diag(x, m, tbs[h], ns2[h], dc)) { dd[h] = dc; have_d[h] = true; }
                    }
            }
            for (int h = 0; h < 2; ++h) {
                const size_t t = 2 * (size_t)r + h;
                const Tab& tb = tbs[h];
                const int n = ns2[h];
                score[t] = -1; why[t] = W_OK; route[t] = 0; pack[t] = 0;
                if (!live[h]) { why[t] = W_SHAPE; continue; }
                const L1 ln{lane + S_WORDS, 1, (uint16_t*)lane, 1};
                const bool tw = tab_has_twins(tb);
                M192 M = m_zero();
                if (have_d[h]) M = diag_mask(read_words(x, m), x, m, tb, n, dd[h]);
                if (!have_d[h] || m_pop(M) < 20) { why[t] = W_NO_DIAG; continue; }
                const Front fr = front_rest(x, m, tb, n, ln, dd[h], M, tw);
                if (fr.why != W_OK) { why[t] = fr.why; continue; }
                if (whole_read(fr, m)) { score[t] = m; route[t] = RK_DECIDED; continue; }
                const int ns = probe_rows(x, tb, fr, ln, tw ? twin_matches(tb, fr, m, ln) : 0);
                if (ns > L1::SMAX) { why[t] = W_MATCHES; continue; }
                back_sort(ns, ln);
                int32_t sc = -1;
                uint32_t wy = W_OK;
                Front fe = fr;                       // the front and the list the last phase ran on (the record's, for a rechecked task)
                int ne = ns;
                const uint32_t* le = lane;
                if (back_harmless(fr, ns, ln)) {
                    sc = back_rest(fr, ns, ln, Lane{generic, 1}, &wy, 0, nullptr, nullptr);
                } else {
                    route[t] |= RK_LOOSE_FAILED;
                    if (!recheck) { why[t] = W_NOT_HARMLESS; continue; }
                    // the tight test directly, on a copy of the lane
                    memcpy(lane_d, lane, sizeof lane);
                    memset(ub_d, 0xa5, sizeof ub_d);
                    if (back_harmless(fr, ns, LR{lane_d + S_WORDS, 1, (uint16_t*)lane_d, 1, ub_d, 1})) route[t] |= RK_CLEARED_DIRECT;
                    // ... and the way the two kernels do it: the record, a poisoned lane, recheck_rest
                    for (int i = 0; i < TAIL_WORDS; ++i) rec[i] = 0xdeadbeefu;
                    tail_pack(rec, 1, (uint32_t)t, fr, ns, ln);
                    memset(lane_c, 0xa5, sizeof lane_c);
                    memset(ub_c, 0x5a, sizeof ub_c);
                    const LR lc{lane_c + S_WORDS, 1, (uint16_t*)lane_c, 1, ub_c, 1};
                    uint32_t pk = 0, aux = 0;
                    bool cleared = false;
                    if (tail_unpack(rec, 1, fe, ne, lc, &pk) != (uint32_t)t || ne != ns || pk != band_pack(fr)) return -2;
                    sc = recheck_rest(fe, ne, lc, Lane{generic, 1}, &wy, &aux, &cleared);
                    le = lane_c;
                    if (cleared) route[t] |= RK_CLEARED;
                    else { why[t] = W_NOT_HARMLESS; continue; }
                }
                if (sc >= 0) { score[t] = sc; route[t] |= RK_DECIDED; continue; }
                // harmless matches only, bounds apart or the generic set full: the certificate, the one-diagonal band, the corridor bound
                why[t] = wy;
                route[t] |= RK_BAND;
                pack[t] = band_pack(fe);
                score[t] = fe.cert;
                const L1 lf{const_cast<uint32_t*>(le) + S_WORDS, 1, (uint16_t*)const_cast<uint32_t*>(le), 1};
                const int cs = corridor_bound(x, m, tb.gt + tb.bytes, n, fe.d, fe.ca, fe.cb, far_rows(fe.d, ne, lf));
                if (cs >= 0) { score[t] = cs; route[t] |= RK_CORRIDOR; why[t] = W_OK; }
            }
        }
    }
    return 0;
}
}  // extern "C"
