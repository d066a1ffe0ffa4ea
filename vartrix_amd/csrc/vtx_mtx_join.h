// vtx_mtx_join.h — vtx_mtx_join of include/vtx.h: the parts of a Matrix-Market file (vtx_mtx_part, vtxh_mtx_part) behind its header.
// Host code only, no device and no context: vtx_api.hip wraps it, and tests/mtxparts/ compiles it into a stand-alone program.
#ifndef VTX_MTX_JOIN_H
#define VTX_MTX_JOIN_H

#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../include/vtx.h"

namespace vtxj {

// sprs::io::write_matrix_market's three header lines (src/main.rs:381-389); returns their length
inline int header(char* head, size_t cap, uint32_t n_rows, uint32_t n_cols, uint64_t nnz) {
    return snprintf(head, cap, "%%%%MatrixMarket matrix coordinate real general\n%% written by sprs\n%u %u %llu\n", n_rows, n_cols, (unsigned long long)nnz);
}

// gzip's CRC-32, bit by bit: the header lines are under 160 bytes
inline uint32_t crc32_small(const uint8_t* p, size_t n) {
    uint32_t crc = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        crc ^= p[i];
        for (int b = 0; b < 8; ++b) crc = (crc >> 1) ^ (0xedb88320u & (0u - (crc & 1u)));
    }
    return ~crc;
}

// 0, or a negative vtx_status with the message in why; on an error nothing is left at path
inline int join(const char* path, uint32_t n_rows, uint32_t n_cols, int gz, const struct vtx_mtx_part* parts, uint32_t n_parts, uint64_t* text_bytes,
                char* why, size_t why_cap) {
    if (!path || (n_parts && !parts)) { snprintf(why, why_cap, "vtx_mtx_join: bad argument"); return VTX_E_INVAL; }
    uint64_t nnz = 0, text_total = 0;
    for (uint32_t i = 0; i < n_parts; ++i) {
        if ((parts[i].gz != 0) != (gz != 0)) {
            snprintf(why, why_cap, "vtx_mtx_join: part %u is %s, the file is to be %s", i, parts[i].gz ? "BGZF members" : "text", gz ? "gzip" : "text");
            return VTX_E_INVAL;
        }
        if (parts[i].n_bytes && !parts[i].bytes) {
            snprintf(why, why_cap, "vtx_mtx_join: part %u has %llu bytes and no buffer", i, (unsigned long long)parts[i].n_bytes);
            return VTX_E_INVAL;
        }
        nnz += parts[i].nnz; text_total += parts[i].text_bytes;
    }
    uint8_t head[18 + 5 + 160 + 8];                       // gz: the header lines as one member with a stored block (n + 31 bytes)
    const int hl = header((char*)head + (gz ? 23 : 0), 160, n_rows, n_cols, nnz);
    size_t head_bytes = (size_t)hl;
    if (gz) {
        static const uint8_t kHead[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};
        head_bytes = (size_t)hl + 31;
        const uint32_t crc = crc32_small(head + 23, (size_t)hl), isize = (uint32_t)hl;
        const uint16_t bsize1 = (uint16_t)(head_bytes - 1), len = (uint16_t)hl, nlen = (uint16_t)~len;
        memcpy(head, kHead, 16);
        memcpy(head + 16, &bsize1, 2);
        head[18] = 0x01;                                  // BFINAL, BTYPE 00: stored
        memcpy(head + 19, &len, 2);
        memcpy(head + 21, &nlen, 2);
        memcpy(head + 23 + hl, &crc, 4);
        memcpy(head + 27 + hl, &isize, 4);
    }
    static const uint8_t kEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) { snprintf(why, why_cap, "cannot open %s for writing", path); return VTX_E_INVAL; }
    // every byte's place in the file is known beforehand (n_bytes): the head, then slices of the parts of at most kSlice bytes, then the
    // end-of-file member.  A large file is written by several threads, each pwrite()ing slices at their offsets — the copy into the
    // page cache is most of the time of a file of several hundred MB (the host formatter writes the same way).
    struct Job { const uint8_t* p; uint64_t n, off; };
    const uint64_t kSlice = 8u << 20;
    std::vector<Job> jobs;
    jobs.push_back(Job{head, head_bytes, 0});
    uint64_t off = head_bytes;
    for (uint32_t i = 0; i < n_parts; ++i) {
        for (uint64_t o = 0; o < parts[i].n_bytes; o += kSlice) jobs.push_back(Job{parts[i].bytes + o, parts[i].n_bytes - o < kSlice ? parts[i].n_bytes - o : kSlice, off + o});
        off += parts[i].n_bytes;
    }
    if (gz) jobs.push_back(Job{kEof, sizeof kEof, off});
    std::atomic<size_t> next{0};
    std::atomic<bool> bad{false};
    auto worker = [&] {
        for (size_t j; (j = next.fetch_add(1)) < jobs.size() && !bad.load();) {
            const uint8_t* p = jobs[j].p;
            uint64_t n = jobs[j].n, o = jobs[j].off;
            while (n) {
                const ssize_t k = pwrite(fd, p, (size_t)n, (off_t)o);
                if (k <= 0) { bad = true; break; }
                p += k; n -= (uint64_t)k; o += (uint64_t)k;
            }
        }
    };
    const size_t n_threads = off < (16u << 20) ? 1 : (jobs.size() < 8 ? jobs.size() : 8);
    std::vector<std::thread> th;
    for (size_t t = 1; t < n_threads; ++t) th.emplace_back(worker);
    worker();
    for (auto& t : th) t.join();
    bool ok = !bad.load();
    ok = (close(fd) == 0) && ok;
    if (!ok) { unlink(path); snprintf(why, why_cap, "error writing %s", path); return VTX_E_INVAL; }
    if (text_bytes) *text_bytes = (uint64_t)hl + text_total;
    return VTX_OK;
}

}  // namespace vtxj
#endif
