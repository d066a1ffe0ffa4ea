// Stand-alone host program for tests/test_mtx_parts_host.py: vtxh_mtx_part on the pieces of one triplet list, vtx_mtx_join's
// implementation (vartrix_amd/csrc/vtx_mtx_join.h) on the parts, and vtxh_write_mtx / vtxh_write_mtx_gz on the whole — built with
// AddressSanitizer and UBSan (tests/mtxparts/Makefile).
//   mtx_parts_san IN OUTDIR     IN: u32 n_rows, u32 n_cols, u64 nnz, u32 n_cuts, u64 cuts[n_cuts] (ascending, 0 first, nnz last),
//                               u32 row[nnz], u32 col[nnz], f64 value[nnz].
//   OUTDIR gets whole.mtx, whole.mtx.gz (the writers), joined.mtx, joined.mtx.gz (parts + join).  Exit 1 when the joined plain file is
//   not the whole one byte for byte, when a part's counts are off, or when an error case does not answer as vtx.h says.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/vtx_host.h"
#include "../../vartrix_amd/csrc/vtx_mtx_join.h"

namespace {
typedef struct vtx_mtx_part Part;

bool slurp(const std::string& path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(f);
    return true;
}

bool exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); return 1; } } while (0)
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: mtx_parts_san IN OUTDIR\n"); return 2; }
    std::vector<uint8_t> in;
    if (!slurp(argv[1], in) || in.size() < 20) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint32_t n_rows, n_cols, n_cuts;
    uint64_t nnz;
    size_t p = 0;
    memcpy(&n_rows, &in[p], 4); p += 4;
    memcpy(&n_cols, &in[p], 4); p += 4;
    memcpy(&nnz, &in[p], 8); p += 8;
    memcpy(&n_cuts, &in[p], 4); p += 4;
    if (n_cuts < 1 || in.size() != p + 8ull * n_cuts + 16ull * nnz) { fprintf(stderr, "bad input size\n"); return 2; }
    std::vector<uint64_t> cuts(n_cuts);
    std::vector<uint32_t> row(nnz), col(nnz);
    std::vector<double> val(nnz);
    memcpy(cuts.data(), &in[p], 8ull * n_cuts); p += 8ull * n_cuts;
    if (nnz) { memcpy(row.data(), &in[p], 4 * nnz); p += 4 * nnz; memcpy(col.data(), &in[p], 4 * nnz); p += 4 * nnz; memcpy(val.data(), &in[p], 8 * nnz); }
    const std::string dir = argv[2];
    const std::string whole = dir + "/whole.mtx", whole_gz = dir + "/whole.mtx.gz";
    CHECK(vtxh_write_mtx(whole.c_str(), n_rows, n_cols, nnz, row.data(), col.data(), val.data()) == 0, "vtxh_write_mtx: %s", vtxh_last_error());
    CHECK(vtxh_write_mtx_gz(whole_gz.c_str(), n_rows, n_cols, nnz, row.data(), col.data(), val.data()) == 0, "vtxh_write_mtx_gz: %s", vtxh_last_error());
    char why[512];
    std::vector<uint8_t> want, got;
    CHECK(slurp(whole, want), "cannot read %s", whole.c_str());
    for (int gz = 0; gz < 2; ++gz) {
        std::vector<Part> parts(n_cuts - 1);
        uint64_t lines = 0, text = 0;
        for (uint32_t i = 0; i + 1 < n_cuts; ++i) {
            const uint64_t a = cuts[i], n = cuts[i + 1] - cuts[i];
            CHECK(cuts[i + 1] >= cuts[i] && cuts[i + 1] <= nnz, "bad cuts");
            // (exact-size copies: a read behind a piece's arrays is the sanitizer's to see)
            std::vector<uint32_t> r(row.begin() + a, row.begin() + a + n), c(col.begin() + a, col.begin() + a + n);
            std::vector<double> v(val.begin() + a, val.begin() + a + n);
            CHECK(vtxh_mtx_part(n, r.data(), c.data(), v.data(), gz, &parts[i]) == 0, "vtxh_mtx_part: %s", vtxh_last_error());
            double s = 0;
            for (double x : v) s += x;
            CHECK(parts[i].nnz == n && parts[i].gz == (uint32_t)gz && (gz || parts[i].n_bytes == parts[i].text_bytes), "part %u: counts", i);
            CHECK((std::isnan(s) && std::isnan(parts[i].sum)) || s == parts[i].sum, "part %u: sum", i);
            CHECK(n || (parts[i].n_bytes == 0 && parts[i].bytes == nullptr), "part %u: an empty part has bytes", i);
            lines += parts[i].nnz; text += parts[i].text_bytes;
        }
        const std::string out = dir + (gz ? "/joined.mtx.gz" : "/joined.mtx");
        uint64_t tb = 0;
        CHECK(vtxj::join(out.c_str(), n_rows, n_cols, gz, parts.data(), (uint32_t)parts.size(), &tb, why, sizeof why) == 0, "join: %s", why);
        CHECK(lines == nnz && tb == want.size() && text + (tb - text) == want.size(), "text_bytes %llu, the whole file has %zu", (unsigned long long)tb, want.size());
        if (!gz) {
            got.clear();
            CHECK(slurp(out, got) && got == want, "the joined file differs from vtxh_write_mtx's");
        }
        // the error cases: a part of the other kind; a path that cannot be written
        if (!parts.empty()) {
            const std::string bad = dir + "/mismatch.out";
            CHECK(vtxj::join(bad.c_str(), n_rows, n_cols, !gz, parts.data(), (uint32_t)parts.size(), nullptr, why, sizeof why) == VTX_E_INVAL && !exists(bad), "mismatch accepted");
        }
        const std::string nodir = dir + "/no_such_dir/m.out";
        CHECK(vtxj::join(nodir.c_str(), n_rows, n_cols, gz, parts.data(), (uint32_t)parts.size(), nullptr, why, sizeof why) != 0 && !exists(nodir), "unwritable path accepted");
        for (Part& q : parts) vtxh_mtx_part_free(&q);
        for (Part& q : parts) vtxh_mtx_part_free(&q);      // a zeroed struct: nothing to do
    }
    return 0;
}
