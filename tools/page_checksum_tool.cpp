// page_checksum_tool — GPU-backed, contract-compatible replacement for the
// reference CLI (tools/page_checksum_tool.cpp:47-123).
//
//   page_checksum_tool <file_path> <offset_bytes> [page_size_bytes]
//       Reference contract: numbers parsed like std::stoull(s, &idx, 0) with the
//       whole string consumed (decimal, 0x hex, leading-0 octal); page size 0
//       rejected; default page size 4096 (KvOptions::data_page_size,
//       include/kv_options.h:184); [offset, offset+P) must lie inside the file.
//       Prints "Checksum OK|FAILED for page at offset <dec>", then
//       "Page bytes (offset:value)" and a hex dump (16 bytes per row,
//       "%06x: " + "%02x " each).  Exit 0 = OK, 2 = FAILED, 1 = usage / IO error.
//
// Added modes (not in the reference):
//   page_checksum_tool --scan  <file_path> [page_size]   validate every page
//   page_checksum_tool --stamp <file_path> [page_size]   SetChecksum on every page
//   page_checksum_tool --gen   <file_path> <n_pages> [page_size] [seed]
//       write n synthetic pages (splitmix64 words, see include/eloqstore_pcs.h)
//       and stamp them.
//   page_checksum_tool --scrub <file_path> [page_size]   classify every page: ok,
//       corrupted or blank (all zero: the never-written tail of a fallocated
//       data file), count the ok pages by PageType and list up to 64
//       corrupted offsets.  Exit 2 if any page is corrupted; blank pages do
//       not fail a scrub (--scan counts them as corrupted).
//   page_checksum_tool --extents <file_path> [page_size]   --scrub's counts, then
//       where the classes lie: the written extent (pages [0, W), W = 1 + the
//       last non-blank page) and the blank tail behind it, the holes (blank
//       runs below W) and up to 64 corrupted extents as offset and length.
//       Exit 2 if any page is corrupted, else 3 if there is a hole, else 0.
//       An append-mode data file is written in page order, so only there does
//       a hole (exit 3) mean a lost or trimmed write.
//   page_checksum_tool --scrub-files <page_size> <file>...   scrub many data
//       files in one pass: the files are packed back to back into the pinned
//       chunks, each chunk is one pcs_pages_scrub_files_host call, and every
//       file gets a report of its own (counts, written extent, holes).  One
//       line per file that has a corrupted page or a hole, then the totals.
//       Exit 2 if any file has a corrupted page, else 3 if any has a hole,
//       else 0.  A file with no whole page is skipped with a warning.
//   page_checksum_tool --check-manifest <file>...   walk and verify every record
//       of manifest files (the reference's tools/manifest_check_tool.cpp, whose
//       one-file contract is kept): all files of the invocation go through one
//       pcs_manifest_scan_host call at page_align 4096.  One file: that tool's
//       output ("Log #i at offset ...", record size, root, ttl_root,
//       payload_bytes, checksum: OK|FAILED, payload_hex for failed records,
//       "Parsed N logs from <path>") and exit codes: 0, 2 on any checksum
//       failure, 1 with its messages for a truncated header or payload or for
//       no records; padding cut by the end of the file is no error, as there.
//       Several files: one line per file (records, corrupt, verdict,
//       valid_prefix_bytes); exit 2 if any manifest is broken or has a bad
//       snapshot, else 3 if any has a torn tail, else 1 if any is empty or
//       unreadable, else 0.
//   page_checksum_tool --live <manifest> <page_size> <pages_per_file_shift> <data_file>...
//       is any page the tree still points to damaged?  The manifest is replayed
//       (pcs_manifest_replay_host); when it cannot be (not replayable or
//       malformed) one line says why, exit 2.  A data file's id comes from its
//       base name data_<file_id>_<term> (a name that does not parse: exit 1);
//       each file is scrubbed (pcs_pages_scrub_host) and its class bytes go to
//       pcs_scrub_live_host with fp_first = file_id << shift.  One line per
//       file with live ok/blank/corrupt and dead ok/blank/corrupt, one line per
//       damaged live page (page id, file page id, class), then root, ttl_root,
//       max_fp_id, the mapped pages and how many of them lie in files not
//       given.  Exit 2 if any live page is corrupt, else 3 if any is blank,
//       else 0; dead damage never fails the run.
//   page_checksum_tool --tree <manifest> <page_size> <pages_per_file_shift> <data_file>...
//       does the index tree that hangs off the replayed roots hold together?
//       The manifest is replayed as for --live (the same refusal line, exit 2).
//       The given files are loaded into ONE window that spans their file ids,
//       [min_id << shift, (max_id + 1) << shift); pages of files not given (and
//       pages past the end of a short file) get class byte 3 and are reported
//       ABSENT when the tree points to them.  A span that does not fit in
//       device memory: a message, exit 1.  The files are scrubbed, the tree
//       check runs on root and ttl_root (pcs_tree_check_host), and the tool
//       prints one line per tree, one line per problem (page id, parent, depth,
//       bit names) and a last line with the unreached mapped pages by type.
//       Exit 2 when a reached page is corrupt, malformed, of the wrong type,
//       unmapped or has a child beyond the table; else 3 when a reached page is
//       blank; else 0.  ABSENT (nothing was checked) and BAD_LINK (no store
//       written by the reference was at hand to confirm that every committed
//       state keeps the sibling links) are printed and never change the status.
//   page_checksum_tool --leaves <manifest> <page_size> <pages_per_file_shift> <data_file>...
//       can every value be read back?  Everything --tree does and prints
//       (pcs_leaf_check_host runs the tree check first), then every data page
//       the tree reached in good health is decoded and the overflow chain of
//       every large value walked: two summary lines (data pages and entries;
//       overflow pages, pointers and leaked pages) and one line per problem
//       (page id, owner, the owner's entry offset, bit names).  Exit 2 when a
//       row is unmapped, corrupt, of the wrong type, malformed or has a bad
//       pointer, or when a chain points into the tree, has pointers in a page
//       that is not the last of its group or was cut at the group cap, or when
//       --tree would exit 2; else 3 when a chain page is blank; else as --tree.
//       ABSENT, SHARED and leaked overflow pages are printed and never change
//       the status: no store written by the reference was at hand to confirm
//       that every committed state is free of them.
//   --scan/--stamp print a summary line with the GiB/s of the call; exit codes
//   as above (--scan: 2 if any page is corrupted).
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "eloqstore/page_checksum.h"
#include "eloqstore_pcs.h"
#include "extent_merge.h"
#include "file_merge.h"
#include "leaf_check.h"
#include "manifest_replay.h"
#include "manifest_scan.h"
#include "scrub_merge.h"
#include "tree_check.h"

namespace {

bool parse_u64(const char* s, uint64_t& out) {
    try {
        size_t idx = 0;
        const std::string str(s);
        const unsigned long long v = std::stoull(str, &idx, 0);
        if (idx != str.size()) return false;
        out = v;
        return true;
    } catch (...) {
        return false;
    }
}

void usage(const char* prog) {
    std::fprintf(stderr,
                 "Usage: %s <file_path> <offset_bytes> [page_size_bytes]\n"
                 "Offset and page size accept decimal or 0x-prefixed hex values.\n"
                 "       %s --scan|--stamp <file_path> [page_size_bytes]\n"
                 "       %s --scrub <file_path> [page_size_bytes]\n"
                 "       %s --extents <file_path> [page_size_bytes]\n"
                 "           exit 2: corrupted pages; exit 3: a blank page below the last written one\n"
                 "           (a lost write only for append-mode files, which are written in page order)\n"
                 "       %s --scrub-files <page_size_bytes> <file>...\n"
                 "       %s --gen <file_path> <n_pages> [page_size_bytes] [seed]\n"
                 "       %s --check-manifest <manifest_file>...\n"
                 "           one file: the manifest_check_tool report (exit 2: a checksum failed);\n"
                 "           several: a line per file (exit 2: broken or bad snapshot, 3: torn tail, 1: empty)\n"
                 "       %s --live <manifest_file> <page_size_bytes> <pages_per_file_shift> <data_file>...\n"
                 "           exit 2: a mapped page is corrupt or the manifest cannot be replayed; exit 3: a mapped\n"
                 "           page is blank; damage in pages the manifest no longer maps never fails the run\n"
                 "       %s --tree <manifest_file> <page_size_bytes> <pages_per_file_shift> <data_file>...\n"
                 "           walks the index tree from root and ttl_root; exit 2: a reached page is corrupt,\n"
                 "           malformed, of the wrong type, unmapped or points beyond the table; exit 3: a reached\n"
                 "           page is blank.  absent pages (files not given) and bad-link (sibling links: not\n"
                 "           confirmed against a store written by the reference) are printed, never fail the run\n"
                 "       %s --leaves <manifest_file> <page_size_bytes> <pages_per_file_shift> <data_file>...\n"
                 "           --tree, then every reached data page is decoded and every overflow chain walked;\n"
                 "           exit 2: a data page is malformed, a chain page is unmapped, corrupt, of the wrong type or\n"
                 "           malformed, a pointer leaves the table or enters the tree, a page that is not the last of\n"
                 "           its group has pointers, or a chain exceeds 4096 groups; exit 3: a chain page is blank;\n"
                 "           else as --tree.  absent, shared and leaked overflow pages are printed, never fail the run\n",
                 prog, prog, prog, prog, prog, prog, prog, prog, prog, prog);
}

constexpr uint64_t kDefaultPageSize = 4096;  // KvOptions{}.data_page_size

int single_page(const char* path, const char* off_s, const char* size_s) {
    uint64_t offset = 0, P = kDefaultPageSize;
    if (!parse_u64(off_s, offset)) {
        std::fprintf(stderr, "Invalid offset: %s\n", off_s);
        return 1;
    }
    if (size_s && (!parse_u64(size_s, P) || P == 0)) {
        std::fprintf(stderr, "Invalid page size: %s\n", size_s);
        return 1;
    }
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "Failed to open %s: %s\n", path, std::strerror(errno));
        return 1;
    }
    std::fseek(f, 0, SEEK_END);
    const uint64_t fsize = (uint64_t)std::ftell(f);
    if (offset + P > fsize) {
        std::fprintf(stderr, "Requested range [%llu, %llu) exceeds file size %llu\n", (unsigned long long)offset,
                     (unsigned long long)(offset + P), (unsigned long long)fsize);
        std::fclose(f);
        return 1;
    }
    std::vector<char> page(P);
    std::fseek(f, (long)offset, SEEK_SET);
    const size_t got = std::fread(page.data(), 1, P, f);
    std::fclose(f);
    if (got != P) {
        std::fprintf(stderr, "Unable to read %llu bytes at offset %llu\n", (unsigned long long)P,
                     (unsigned long long)offset);
        return 1;
    }
    const bool ok = eloqstore::ValidateChecksum(std::string_view(page.data(), P));
    std::printf("%s for page at offset %llu\n", ok ? "Checksum OK" : "Checksum FAILED", (unsigned long long)offset);
    std::printf("Page bytes (offset:value)\n");
    for (uint64_t i = 0; i < P; i += 16) {
        std::printf("%06llx: ", (unsigned long long)i);
        for (uint64_t j = 0; j < 16 && i + j < P; ++j) std::printf("%02x ", (unsigned)(uint8_t)page[i + j]);
        std::printf("\n");
    }
    return ok ? 0 : 2;
}

// Whole-file scrub / stamp: the file is read with pread into two pinned
// 64 MiB buffers and each chunk goes to the GPU as an asynchronous batch
// (pcs_batch_*); a contiguous pinned run is DMA'd in place, so the host does
// no gather copy.  Reading chunk k+1 overlaps checking chunk k.
struct Fd {
    int fd = -1;
    ~Fd() {
        if (fd >= 0) close(fd);
    }
};

bool pread_full(int fd, char* buf, uint64_t len, uint64_t off) {
    while (len) {
        const ssize_t r = pread(fd, buf, len, (off_t)off);
        if (r <= 0) return false;
        buf += r;
        len -= (uint64_t)r;
        off += (uint64_t)r;
    }
    return true;
}

bool pwrite_full(int fd, const char* buf, uint64_t len, uint64_t off) {
    while (len) {
        const ssize_t r = pwrite(fd, buf, len, (off_t)off);
        if (r <= 0) return false;
        buf += r;
        len -= (uint64_t)r;
        off += (uint64_t)r;
    }
    return true;
}

// pread of one chunk split over a few threads: a single thread's copy out of
// the page cache (~6 GiB/s) would otherwise bound the scrub.
// PCS_SCAN_THREADS / PCS_SCAN_PIECE_MIB / PCS_SCAN_CHUNK_MIB override the
// reader threads (16, at most the host's), the read piece (4 MiB) and the
// chunk per batch (64 MiB); tools/lab/scan_lab.sh sweeps them: 16 x 4 MiB
// against 8 x 8 MiB: 19.2-19.8 vs 13.5-14.9 GiB/s on a 1 GiB file, 25-31 vs
// 27.5 on 4 GiB; 128 MiB chunks slower (profiles/r02/scan_lab.txt).
uint64_t env_u64(const char* name, uint64_t dflt) {
    const char* v = std::getenv(name);
    uint64_t x;
    return v && parse_u64(v, x) && x > 0 ? x : dflt;
}

bool pread_parallel(int fd, char* buf, uint64_t len, uint64_t off) {
    static const uint64_t kThreads =
        env_u64("PCS_SCAN_THREADS", std::min<uint64_t>(16, std::max(1u, std::thread::hardware_concurrency())));
    static const uint64_t kPiece = env_u64("PCS_SCAN_PIECE_MIB", 4) << 20;
    const unsigned T = (unsigned)std::min<uint64_t>(kThreads, (len + kPiece - 1) / kPiece);
    if (T <= 1) return pread_full(fd, buf, len, off);
    std::vector<std::thread> th;
    std::vector<char> ok(T, 1);
    for (unsigned k = 0; k < T; ++k) {
        const uint64_t b = len * k / T, e = len * (k + 1) / T;
        th.emplace_back([&, k, b, e] { ok[k] = pread_full(fd, buf + b, e - b, off + b); });
    }
    for (auto& x : th) x.join();
    return std::all_of(ok.begin(), ok.end(), [](char c) { return c != 0; });
}

int bulk(bool stamp, const char* path, const char* size_s) {
    uint64_t P = kDefaultPageSize;
    if (size_s && (!parse_u64(size_s, P) || P < 8)) {
        std::fprintf(stderr, "Invalid page size: %s\n", size_s);
        return 1;
    }
    Fd f;
    f.fd = open(path, stamp ? O_RDWR : O_RDONLY);
    struct stat st;
    if (f.fd < 0 || fstat(f.fd, &st) != 0) {
        std::fprintf(stderr, "Failed to open %s: %s\n", path, std::strerror(errno));
        return 1;
    }
    const uint64_t n = (uint64_t)st.st_size / P;
    if (n == 0) {
        std::fprintf(stderr, "File %s holds no whole page of %llu bytes\n", path, (unsigned long long)P);
        return 1;
    }
    const uint64_t chunk = std::max<uint64_t>(1, (env_u64("PCS_SCAN_CHUNK_MIB", 64) << 20) / P);
    void* buf[2] = {nullptr, nullptr};
    pcs_batch* batch[2] = {nullptr, nullptr};
    int rc = 0;
    for (int k = 0; k < 2 && !rc; ++k) {
        rc = pcs_host_alloc_pinned(chunk * P, &buf[k]);
        if (!rc) rc = pcs_batch_create(&batch[k]);
    }
    if (rc) {
        std::fprintf(stderr, "GPU setup failed (%d): %s\n", rc, pcs_last_error());
        return 1;
    }
    std::vector<const void*> ptrs[2];
    std::vector<uint8_t> ok(chunk);
    uint64_t first[2] = {0, 0}, count[2] = {0, 0}, bad = 0, first_bad = n;
    bool busy[2] = {false, false};
    auto collect = [&](int k) -> bool {
        if (!busy[k]) return true;
        busy[k] = false;
        if (pcs_batch_wait(batch[k])) return false;
        if (stamp) return pwrite_full(f.fd, static_cast<char*>(buf[k]), count[k] * P, first[k] * P);
        uint64_t fb = UINT64_MAX;
        if (pcs_batch_result(batch[k], ok.data(), nullptr, &fb)) return false;
        for (uint64_t i = 0; i < count[k]; ++i) bad += ok[i] == 0;
        if (fb != UINT64_MAX) first_bad = std::min(first_bad, first[k] + fb);
        return true;
    };
    {
        // warm the GPU path (code-object load, first launch) before the clock
        // starts: ~30 ms that would otherwise land on the first chunk of a
        // scrub (a long-running service pays it once)
        std::memset(buf[0], 0, (size_t)P);
        const void* one = buf[0];
        if (pcs_batch_submit(batch[0], stamp ? PCS_BATCH_DIGEST : PCS_BATCH_VALIDATE, &one, P, 1,
                             PCS_XXH3_64) == PCS_OK)
            (void)pcs_batch_wait(batch[0]);
    }
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t k = 0;
    for (uint64_t p0 = 0; p0 < n; p0 += chunk, ++k) {
        const int s = (int)(k & 1);
        if (!collect(s)) {
            rc = 1;
            break;
        }
        const uint64_t cnt = std::min(chunk, n - p0);
        char* b = static_cast<char*>(buf[s]);
        if (!pread_parallel(f.fd, b, cnt * P, p0 * P)) {
            std::fprintf(stderr, "read failed at offset %llu: %s\n", (unsigned long long)(p0 * P), std::strerror(errno));
            rc = 1;
            break;
        }
        ptrs[s].resize(cnt);
        for (uint64_t i = 0; i < cnt; ++i) ptrs[s][i] = b + i * P;
        if (pcs_batch_submit(batch[s], stamp ? PCS_BATCH_STAMP : PCS_BATCH_VALIDATE, ptrs[s].data(), P, cnt,
                             PCS_XXH3_64)) {
            rc = 1;
            break;
        }
        first[s] = p0;
        count[s] = cnt;
        busy[s] = true;
    }
    for (int s = 0; s < 2; ++s)
        if (!collect(s)) rc = 1;
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int s = 0; s < 2; ++s) {
        pcs_batch_destroy(batch[s]);
        pcs_host_free_pinned(buf[s]);
    }
    if (rc) {
        std::fprintf(stderr, "%s failed: %s\n", stamp ? "stamp" : "scan", pcs_last_error());
        return 1;
    }
    const double gib = (double)(n * P) / (1024.0 * 1024.0 * 1024.0);
    if (stamp) {
        std::printf("Stamped %llu pages of %llu bytes in %.3f s (%.2f GiB/s incl. file I/O)\n", (unsigned long long)n,
                    (unsigned long long)P, secs, gib / secs);
        return 0;
    }
    std::printf("Scanned %llu pages of %llu bytes: %llu corrupted", (unsigned long long)n, (unsigned long long)P,
                (unsigned long long)bad);
    if (bad) std::printf(", first at offset %llu", (unsigned long long)(first_bad * P));
    std::printf(" (%.3f s, %.2f GiB/s incl. file I/O)\n", secs, gib / secs);
    return bad ? 2 : 0;
}

// Blank-aware scrub: --scan's pinned double-buffered read loop with
// pcs_pages_scrub_host per chunk.  The call is synchronous, so the overlap
// comes from reading chunk k+1 on a helper thread while this thread scrubs
// chunk k.  Never-written (all-zero) pages are counted, not failed; the first
// kScrubLines corrupted pages are listed by offset.
constexpr uint64_t kScrubLines = 64;
// --extents: the same loop with pcs_pages_scrub_extents_host per file chunk
// (no per-page array comes back) and the file chunks merged by ScrubMerge and
// ExtentMerge.  The corrupted extents printed are those among the first
// kExtentRuns runs of the file.
constexpr uint64_t kExtentRuns = 1024;

int scrub(const char* path, const char* size_s, bool extents = false) {
    uint64_t P = kDefaultPageSize;
    if (size_s && (!parse_u64(size_s, P) || P < 249 || P > 0xFFFFFFFFull)) {
        std::fprintf(stderr, "Invalid page size: %s (scrub needs 249 <= page size < 2^32)\n", size_s);
        return 1;
    }
    Fd f;
    f.fd = open(path, O_RDONLY);
    struct stat st;
    if (f.fd < 0 || fstat(f.fd, &st) != 0) {
        std::fprintf(stderr, "Failed to open %s: %s\n", path, std::strerror(errno));
        return 1;
    }
    const uint64_t n = (uint64_t)st.st_size / P;  // a trailing partial page is ignored
    if (n == 0) {
        std::fprintf(stderr, "File %s holds no whole page of %llu bytes\n", path, (unsigned long long)P);
        return 1;
    }
    const uint64_t chunk = std::max<uint64_t>(1, (env_u64("PCS_SCAN_CHUNK_MIB", 64) << 20) / P);
    void* buf[2] = {nullptr, nullptr};
    int rc = 0;
    for (int k = 0; k < 2 && !rc; ++k) rc = pcs_host_alloc_pinned(chunk * P, &buf[k]);
    if (rc) {
        std::fprintf(stderr, "GPU setup failed (%d): %s\n", rc, pcs_last_error());
        for (void* b : buf) pcs_host_free_pinned(b);
        return 1;
    }
    std::vector<const void*> ptrs(std::min(chunk, n));
    std::vector<uint8_t> cls(ptrs.size());
    pcs_scrub_summary total{}, part{};
    total.first_corrupt = UINT64_MAX;
    uint64_t listed[kScrubLines];
    // --extents only
    pcs_scrub_summary ex_total;
    pcs_extent_summary ext_total, ext_part{};
    std::vector<pcs_extent> runs(extents ? kExtentRuns : 0), part_runs;
    pcs::ScrubMerge scrub_merge(&ex_total, listed, kScrubLines);
    pcs::ExtentMerge extent_merge(&ext_total, runs.data(), runs.size());
    uint64_t part_listed[kScrubLines];
    {
        // warm the GPU path before the clock starts, as --scan does
        std::memset(buf[0], 0, (size_t)P);
        const void* one = buf[0];
        (void)pcs_pages_scrub_host(&one, P, 1, cls.data(), nullptr, &part, nullptr, 0);
    }
    const auto t0 = std::chrono::steady_clock::now();
    auto read_chunk = [&](uint64_t p0, int s) {
        return pread_parallel(f.fd, static_cast<char*>(buf[s]), std::min(chunk, n - p0) * P, p0 * P);
    };
    bool read_ok = read_chunk(0, 0);
    uint64_t k = 0;
    for (uint64_t p0 = 0; p0 < n && !rc; p0 += chunk, ++k) {
        const int s = (int)(k & 1);
        if (!read_ok) {
            std::fprintf(stderr, "read failed at offset %llu: %s\n", (unsigned long long)(p0 * P), std::strerror(errno));
            rc = 1;
            break;
        }
        const uint64_t cnt = std::min(chunk, n - p0);
        bool next_ok = true;
        std::thread reader;
        if (p0 + chunk < n) reader = std::thread([&, p0, s] { next_ok = read_chunk(p0 + chunk, s ^ 1); });
        const char* b = static_cast<const char*>(buf[s]);
        for (uint64_t i = 0; i < cnt; ++i) ptrs[i] = b + i * P;
        const uint64_t room = kScrubLines - total.n_listed;
        if (extents) {
            part_runs.resize(pcs::ExtentMerge::chunk_cap(runs.size(), cnt));
            if (pcs_pages_scrub_extents_host(ptrs.data(), P, cnt, nullptr, nullptr, &part, part_listed, kScrubLines,
                                             &ext_part, part_runs.data(), part_runs.size())) {
                rc = 1;
            } else {
                scrub_merge.add(part, part_listed, p0);
                extent_merge.add(ext_part, part_runs.data(), p0);
            }
        } else if (pcs_pages_scrub_host(ptrs.data(), P, cnt, cls.data(), nullptr, &part, room ? listed + total.n_listed : nullptr,
                                 room)) {
            rc = 1;
        } else {
            total.n_pages += part.n_pages;
            total.n_ok += part.n_ok;
            total.n_corrupt += part.n_corrupt;
            total.n_blank += part.n_blank;
            for (int t = 0; t < 6; ++t) total.ok_by_type[t] += part.ok_by_type[t];
            for (uint64_t i = 0; i < part.n_listed; ++i) listed[total.n_listed + i] += p0;
            total.n_listed += part.n_listed;
        }
        if (reader.joinable()) reader.join();
        read_ok = next_ok;
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (void* b : buf) pcs_host_free_pinned(b);
    if (rc) {
        std::fprintf(stderr, "scrub failed: %s\n", pcs_last_error());
        return 1;
    }
    if (extents) total = ex_total;
    const double gib = (double)(n * P) / (1024.0 * 1024.0 * 1024.0);
    std::printf("Scrubbed %llu pages of %llu bytes: %llu ok, %llu corrupted, %llu blank (%.3f s, %.2f GiB/s incl. file I/O)\n",
                (unsigned long long)n, (unsigned long long)P, (unsigned long long)total.n_ok,
                (unsigned long long)total.n_corrupt, (unsigned long long)total.n_blank, secs, gib / secs);
    std::printf("ok by type: nonleaf_index=%llu leaf_index=%llu data=%llu overflow=%llu deleted=%llu other=%llu\n",
                (unsigned long long)total.ok_by_type[0], (unsigned long long)total.ok_by_type[1],
                (unsigned long long)total.ok_by_type[2], (unsigned long long)total.ok_by_type[3],
                (unsigned long long)total.ok_by_type[4], (unsigned long long)total.ok_by_type[5]);
    if (extents) {
        const pcs_extent_summary& e = ext_total;
        std::printf("written extent: pages [0, %llu) of %llu, blank tail: %llu pages\n",
                    (unsigned long long)e.written_pages, (unsigned long long)e.n_pages,
                    (unsigned long long)(e.n_pages - e.written_pages));
        if (e.n_holes)
            std::printf("holes: %llu (%llu pages), first at offset %llu\n", (unsigned long long)e.n_holes,
                        (unsigned long long)e.n_hole_pages, (unsigned long long)(e.first_hole * P));
        else
            std::printf("holes: none\n");
        uint64_t lines = 0, shown = 0;
        for (uint64_t i = 0; i < e.n_listed && lines < kScrubLines; ++i) {
            if (runs[i].cls != PCS_PAGE_CORRUPT) continue;
            std::printf("corrupted extent at offset %llu: %llu pages\n", (unsigned long long)(runs[i].first_page * P),
                        (unsigned long long)runs[i].n_pages);
            ++lines;
            shown += runs[i].n_pages;
        }
        if (total.n_corrupt > shown)
            std::printf("... and %llu more corrupted pages\n", (unsigned long long)(total.n_corrupt - shown));
        return total.n_corrupt ? 2 : e.n_holes ? 3 : 0;
    }
    for (uint64_t i = 0; i < total.n_listed; ++i)
        std::printf("corrupted page at offset %llu\n", (unsigned long long)(listed[i] * P));
    if (total.n_corrupt > kScrubLines)
        std::printf("... and %llu more corrupted pages\n", (unsigned long long)(total.n_corrupt - kScrubLines));
    return total.n_corrupt ? 2 : 0;
}

// --scrub-files: many data files in one pass.  The files that hold at least
// one whole page form one batch, back to back in argument order; the batch
// flows through the two pinned chunks as in scrub() (chunk k + 1 is read on a
// helper thread while chunk k is scrubbed), so a chunk holds whole files and
// parts of files, and a file larger than what is left of a chunk continues in
// the next one.  Each chunk is one pcs_pages_scrub_files_host call over the
// chunk-local boundaries of its parts; a file's parts are folded by FileMerge.
int scrub_files(const char* size_s, int n_paths, char** paths) {
    uint64_t P = 0;
    if (!parse_u64(size_s, P) || P < 249 || P > 0xFFFFFFFFull) {
        std::fprintf(stderr, "Invalid page size: %s (scrub needs 249 <= page size < 2^32)\n", size_s);
        return 1;
    }
    struct DataFile {
        const char* path;
        uint64_t first;  // the file's first page in the batch
    };
    std::vector<DataFile> files;
    std::vector<Fd> fds(n_paths);
    std::vector<int> fd_of;
    std::vector<uint64_t> first{0};  // batch boundaries of the files scrubbed
    uint64_t skipped = 0;
    for (int i = 0; i < n_paths; ++i) {
        fds[i].fd = open(paths[i], O_RDONLY);
        struct stat st;
        if (fds[i].fd < 0 || fstat(fds[i].fd, &st) != 0) {
            std::fprintf(stderr, "Failed to open %s: %s\n", paths[i], std::strerror(errno));
            return 1;
        }
        const uint64_t n = (uint64_t)st.st_size / P;  // a trailing partial page is ignored
        if (n == 0) {
            std::fprintf(stderr, "File %s holds no whole page of %llu bytes: skipped\n", paths[i], (unsigned long long)P);
            ++skipped;
            continue;
        }
        files.push_back(DataFile{paths[i], first.back()});
        fd_of.push_back(fds[i].fd);
        first.push_back(first.back() + n);
    }
    const uint64_t n = first.back(), n_files = files.size();
    std::vector<pcs_file_report> reports(n_files);
    for (uint64_t f = 0; f < n_files; ++f) reports[f] = pcs::FileMerge::empty(0);
    const uint64_t chunk = std::max<uint64_t>(1, (env_u64("PCS_SCAN_CHUNK_MIB", 64) << 20) / P);
    double secs = 0;
    if (n) {
        void* buf[2] = {nullptr, nullptr};
        int rc = 0;
        for (int k = 0; k < 2 && !rc; ++k) rc = pcs_host_alloc_pinned(std::min(chunk, n) * P, &buf[k]);
        if (rc) {
            std::fprintf(stderr, "GPU setup failed (%d): %s\n", rc, pcs_last_error());
            for (void* b : buf) pcs_host_free_pinned(b);
            return 1;
        }
        std::vector<const void*> ptrs(std::min(chunk, n));
        {
            // warm the GPU path before the clock starts, as --scan does
            std::memset(buf[0], 0, (size_t)P);
            const void* one = buf[0];
            uint8_t c = 0;
            pcs_scrub_summary warm{};
            (void)pcs_pages_scrub_host(&one, P, 1, &c, nullptr, &warm, nullptr, 0);
        }
        const auto t0 = std::chrono::steady_clock::now();
        // the files that reach into batch pages [p0, p0 + cnt): [lo, hi)
        auto span_of = [&](uint64_t p0, uint64_t cnt, uint64_t& lo, uint64_t& hi) {
            lo = (uint64_t)(std::upper_bound(first.begin(), first.end(), p0) - first.begin()) - 1;
            hi = (uint64_t)(std::lower_bound(first.begin(), first.end(), p0 + cnt) - first.begin());
        };
        uint64_t failed_at = 0;
        auto read_chunk = [&](uint64_t p0, int s) {
            const uint64_t cnt = std::min(chunk, n - p0);
            uint64_t lo, hi;
            span_of(p0, cnt, lo, hi);
            for (uint64_t f = lo; f < hi; ++f) {
                const uint64_t a = std::max(first[f], p0), b = std::min(first[f + 1], p0 + cnt);
                if (!pread_parallel(fd_of[f], static_cast<char*>(buf[s]) + (a - p0) * P, (b - a) * P, (a - first[f]) * P)) {
                    failed_at = f;
                    return false;
                }
            }
            return true;
        };
        std::vector<uint64_t> bounds;
        std::vector<pcs_file_report> parts;
        pcs_files_summary part_sum;
        bool read_ok = read_chunk(0, 0);
        uint64_t k = 0;
        for (uint64_t p0 = 0; p0 < n && !rc; p0 += chunk, ++k) {
            const int s = (int)(k & 1);
            if (!read_ok) {
                std::fprintf(stderr, "read failed in %s: %s\n", files[failed_at].path, std::strerror(errno));
                rc = 1;
                break;
            }
            const uint64_t cnt = std::min(chunk, n - p0);
            bool next_ok = true;
            std::thread reader;
            if (p0 + chunk < n) reader = std::thread([&, p0, s] { next_ok = read_chunk(p0 + chunk, s ^ 1); });
            const char* b = static_cast<const char*>(buf[s]);
            for (uint64_t i = 0; i < cnt; ++i) ptrs[i] = b + i * P;
            uint64_t lo, hi;
            span_of(p0, cnt, lo, hi);
            bounds.clear();
            for (uint64_t f = lo; f < hi; ++f) bounds.push_back(std::max(first[f], p0) - p0);
            bounds.push_back(cnt);
            parts.resize(hi - lo);
            if (pcs_pages_scrub_files_host(ptrs.data(), P, cnt, bounds.data(), hi - lo, parts.data(), &part_sum, nullptr, 0)) {
                rc = 1;
            } else {
                for (uint64_t f = lo; f < hi; ++f) pcs::FileMerge::add(reports[f], parts[f - lo]);
            }
            if (reader.joinable()) reader.join();
            read_ok = next_ok;
        }
        secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (void* b : buf) pcs_host_free_pinned(b);
        if (rc) {
            std::fprintf(stderr, "scrub failed: %s\n", pcs_last_error());
            return 1;
        }
    }
    pcs_files_summary total;
    pcs::files_summarize(reports.data(), n_files, &total, nullptr, 0);
    for (uint64_t f = 0; f < n_files; ++f) {
        const pcs_file_report& r = reports[f];
        if (!r.n_corrupt && !r.n_holes) continue;
        std::printf("%s: %llu pages, written [0, %llu), %llu ok, %llu corrupted, %llu blank, %llu holes (%llu pages), ",
                    files[f].path, (unsigned long long)r.n_pages, (unsigned long long)r.written_pages,
                    (unsigned long long)r.n_ok, (unsigned long long)r.n_corrupt, (unsigned long long)r.n_blank,
                    (unsigned long long)r.n_holes, (unsigned long long)r.n_hole_pages);
        if (r.n_corrupt)
            std::printf("first corrupted page at offset %llu\n", (unsigned long long)(r.first_corrupt * P));
        else
            std::printf("first hole at offset %llu\n", (unsigned long long)(r.first_hole * P));
    }
    const double gib = (double)(n * P) / (1024.0 * 1024.0 * 1024.0);
    std::printf("Scrubbed %llu files, %llu pages of %llu bytes: %llu clean, %llu corrupted, %llu with holes, %llu unwritten",
                (unsigned long long)n_files, (unsigned long long)n, (unsigned long long)P,
                (unsigned long long)(n_files - total.n_bad_files - total.n_unwritten_files),
                (unsigned long long)total.n_corrupt_files, (unsigned long long)total.n_hole_files,
                (unsigned long long)total.n_unwritten_files);
    if (skipped) std::printf(", %llu skipped", (unsigned long long)skipped);
    std::printf(" (%.3f s, %.2f GiB/s incl. file I/O)\n", secs, secs > 0 ? gib / secs : 0.0);
    return total.n_corrupt_files ? 2 : total.n_hole_files ? 3 : 0;
}

int gen(const char* path, const char* n_s, const char* size_s, const char* seed_s) {
    uint64_t n = 0, P = kDefaultPageSize, seed = 0x5EED0001;
    if (!parse_u64(n_s, n) || n == 0 || (size_s && (!parse_u64(size_s, P) || P < 8 || P % 8)) ||
        (seed_s && !parse_u64(seed_s, seed))) {
        std::fprintf(stderr, "Invalid --gen arguments\n");
        return 1;
    }
    FILE* f = std::fopen(path, "wb");
    if (!f) {
        std::fprintf(stderr, "Failed to open %s: %s\n", path, std::strerror(errno));
        return 1;
    }
    std::vector<uint64_t> page(P / 8);
    for (uint64_t p = 0; p < n; ++p) {
        for (uint64_t w = 0; w < P / 8; ++w) {
            uint64_t z = (seed ^ p) + (w + 1) * 0x9E3779B97F4A7C15ull;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            page[w] = z ^ (z >> 31);
        }
        if (std::fwrite(page.data(), 1, P, f) != P) {
            std::fprintf(stderr, "write failed: %s\n", std::strerror(errno));
            std::fclose(f);
            return 1;
        }
    }
    std::fclose(f);
    return bulk(true, path, size_s);  // stamp the pages just written
}

}  // namespace

// --check-manifest: every file is read whole into memory and all of them go
// through one pcs_manifest_scan_host call; an unreadable file is reported and
// left out of the call.
int check_manifests(int n_paths, char** paths) {
    constexpr uint32_t kPageAlign = 4096;  // page_align, include/storage/page.h
    std::vector<std::vector<char>> data;
    std::vector<const char*> names;
    bool unreadable = false;
    for (int i = 0; i < n_paths; ++i) {
        FILE* f = std::fopen(paths[i], "rb");
        if (!f) {
            std::fprintf(stderr, "Failed to open %s: %s\n", paths[i], std::strerror(errno));
            if (n_paths == 1) return 1;
            unreadable = true;
            continue;
        }
        std::vector<char> bytes;
        char chunk[1 << 16];
        size_t got;
        while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) bytes.insert(bytes.end(), chunk, chunk + got);
        std::fclose(f);
        data.push_back(std::move(bytes));
        names.push_back(paths[i]);
    }
    const uint64_t n = data.size();
    std::vector<const void*> ptrs(n);
    std::vector<uint64_t> sizes(n);
    uint64_t cap = 0;  // a record per 4 KiB slot at most
    for (uint64_t i = 0; i < n; ++i) {
        ptrs[i] = data[i].data();
        sizes[i] = data[i].size();
        cap += sizes[i] / kPageAlign + 1;
    }
    std::vector<pcs_manifest_report> reports(n);
    std::vector<pcs_manifest_record> records(n_paths == 1 ? cap : 0);
    pcs_manifest_summary sum{};
    if (const int rc = pcs_manifest_scan_host(ptrs.data(), sizes.data(), n, kPageAlign, reports.data(), &sum,
                                              records.data(), records.size())) {
        std::fprintf(stderr, "Manifest scan failed (%d): %s\n", rc, pcs_last_error());
        return 1;
    }
    if (n_paths == 1) {
        const pcs::ManifestToolText t = pcs::manifest_tool_text(
            names[0], reinterpret_cast<const uint8_t*>(data[0].data()), reports[0], records.data());
        std::fputs(t.out.c_str(), stdout);
        std::fputs(t.err.c_str(), stderr);
        return t.exit_code;
    }
    for (uint64_t i = 0; i < n; ++i) std::fputs(pcs::manifest_tool_line(names[i], reports[i]).c_str(), stdout);
    return pcs::manifest_tool_exit(reports.data(), n, unreadable);
}

static bool read_whole(const char* path, std::vector<char>& bytes) {
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "Failed to open %s: %s\n", path, std::strerror(errno));
        return false;
    }
    char chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) bytes.insert(bytes.end(), chunk, chunk + got);
    std::fclose(f);
    return true;
}

// The table, root and ttl_root a manifest describes: 0, or the exit code after
// the message (1) or the one line that says why it cannot be replayed (2).
int replay_manifest(const char* manifest, pcs_replay_report& rep, std::vector<uint64_t>& table) {
    constexpr uint32_t kPageAlign = 4096;
    std::vector<char> image;
    if (!read_whole(manifest, image)) return 1;
    const void* ptr = image.data();
    const uint64_t size = image.size();
    pcs_replay_summary sum{};
    // the rows are not known before the replay: ask without a table first
    if (const int rc = pcs_manifest_replay_host(&ptr, &size, 1, kPageAlign, nullptr, &rep, &sum, nullptr, 0)) {
        std::fprintf(stderr, "Manifest replay failed (%d): %s\n", rc, pcs_last_error());
        return 1;
    }
    table.assign(rep.status == PCS_REPLAY_TABLE_CAP ? rep.table_size : 0, 0);
    if (!table.empty()) {
        if (const int rc = pcs_manifest_replay_host(&ptr, &size, 1, kPageAlign, nullptr, &rep, &sum, table.data(),
                                                    table.size())) {
            std::fprintf(stderr, "Manifest replay failed (%d): %s\n", rc, pcs_last_error());
            return 1;
        }
    }
    const std::string refusal = pcs::live_tool_refusal(manifest, rep);
    if (!refusal.empty()) {
        std::fputs(refusal.c_str(), stdout);
        return 2;
    }
    return 0;
}

// parses the data file names of --live and --tree: false after the message
bool data_file_ids(int n_files, char** files, std::vector<uint64_t>& ids) {
    ids.assign(n_files, 0);
    for (int f = 0; f < n_files; ++f) {
        uint64_t term = 0;
        if (!pcs::live_parse_data_file(files[f], ids[f], term)) {
            std::fprintf(stderr, "Not a data file name (data_<file_id>_<term>): %s\n", files[f]);
            return false;
        }
        for (int g = 0; g < f; ++g) {
            if (ids[g] == ids[f]) {  // its mapped pages would be counted twice
                std::fprintf(stderr, "File id %llu is given twice: %s\n", (unsigned long long)ids[f], files[f]);
                return false;
            }
        }
    }
    return true;
}

// --live: replay the manifest, scrub every data file, and ask of each file's
// class bytes which pages the replayed table still points to.
int live(const char* manifest, const char* size_s, const char* shift_s, int n_files, char** files) {
    uint64_t page_size = 0, shift = 0;
    if (!parse_u64(size_s, page_size) || page_size == 0 || !parse_u64(shift_s, shift) || shift > 40) {
        std::fprintf(stderr, "Invalid page size or pages_per_file_shift\n");
        return 1;
    }
    std::vector<uint64_t> ids;
    if (!data_file_ids(n_files, files, ids)) return 1;
    pcs_replay_report rep{};
    std::vector<uint64_t> table;
    if (const int rc = replay_manifest(manifest, rep, table)) return rc;
    std::vector<pcs_live_summary> sums;
    uint64_t mapped_in_files = 0;
    for (int f = 0; f < n_files; ++f) {
        std::vector<char> bytes;
        if (!read_whole(files[f], bytes)) return 1;
        const uint64_t n_pages = bytes.size() / page_size;
        if (n_pages > (1ull << shift)) {
            std::fprintf(stderr, "%s holds more than 1 << %llu pages\n", files[f], (unsigned long long)shift);
            return 1;
        }
        std::vector<const void*> pages(n_pages);
        for (uint64_t p = 0; p < n_pages; ++p) pages[p] = bytes.data() + p * page_size;
        std::vector<uint8_t> cls(n_pages);
        pcs_scrub_summary ssum{};
        if (const int rc = pcs_pages_scrub_host(pages.data(), page_size, n_pages, cls.data(), nullptr, &ssum, nullptr, 0)) {
            std::fprintf(stderr, "Scrub of %s failed (%d): %s\n", files[f], rc, pcs_last_error());
            return 1;
        }
        const uint64_t fp_first = ids[f] << shift;
        pcs_live_summary ls{};
        std::vector<pcs_live_page> damaged(n_pages);
        if (const int rc = pcs_scrub_live_host(cls.data(), n_pages, fp_first, table.data(), table.size(), nullptr, &ls,
                                               damaged.data(), damaged.size())) {
            std::fprintf(stderr, "Scrub live of %s failed (%d): %s\n", files[f], rc, pcs_last_error());
            return 1;
        }
        std::fputs(pcs::live_tool_file_line(files[f], ids[f], ls).c_str(), stdout);
        for (uint64_t k = 0; k < ls.n_listed; ++k) std::fputs(pcs::live_tool_page_line(fp_first, damaged[k]).c_str(), stdout);
        mapped_in_files += ls.n_mapped_in_window;
        sums.push_back(ls);
    }
    std::fputs(pcs::live_tool_footer(rep, mapped_in_files).c_str(), stdout);
    return pcs::live_tool_exit(sums.data(), sums.size());
}

// --tree: replay the manifest, load the given data files into one window,
// scrub them and walk the index tree from root and ttl_root.  --leaves: the
// same, and then the data pages are decoded and the overflow chains walked.
int tree(bool with_leaves, const char* manifest, const char* size_s, const char* shift_s, int n_files, char** files) {
    uint64_t page_size = 0, shift = 0;
    if (!parse_u64(size_s, page_size) || page_size == 0 || !parse_u64(shift_s, shift) || shift > 40) {
        std::fprintf(stderr, "Invalid page size or pages_per_file_shift\n");
        return 1;
    }
    std::vector<uint64_t> ids;
    if (!data_file_ids(n_files, files, ids)) return 1;
    pcs_replay_report rep{};
    std::vector<uint64_t> table;
    if (const int rc = replay_manifest(manifest, rep, table)) return rc;
    const uint64_t lo = *std::min_element(ids.begin(), ids.end()), hi = *std::max_element(ids.begin(), ids.end());
    const uint64_t per_file = 1ull << shift, fp_first = lo << shift;
    const char* too_large = "The span of the given files does not fit in device memory\n";
    if ((hi - lo + 1) > (1ull << 40) / per_file / page_size) {
        std::fputs(too_large, stderr);
        return 1;
    }
    const uint64_t n_pages = (hi - lo + 1) * per_file;
    std::vector<char> window;
    std::vector<uint8_t> cls;
    try {
        window.assign(n_pages * page_size, 0);
        cls.assign(n_pages, PCS_TREE_CLASS_ABSENT);
    } catch (const std::bad_alloc&) {
        std::fputs(too_large, stderr);
        return 1;
    }
    for (int f = 0; f < n_files; ++f) {
        std::vector<char> bytes;
        if (!read_whole(files[f], bytes)) return 1;
        const uint64_t n = bytes.size() / page_size;
        if (n > per_file) {
            std::fprintf(stderr, "%s holds more than 1 << %llu pages\n", files[f], (unsigned long long)shift);
            return 1;
        }
        const uint64_t first = (ids[f] - lo) * per_file;
        std::memcpy(window.data() + first * page_size, bytes.data(), n * page_size);
        std::vector<const void*> pages(n);
        for (uint64_t p = 0; p < n; ++p) pages[p] = window.data() + (first + p) * page_size;
        pcs_scrub_summary ssum{};
        if (const int rc = pcs_pages_scrub_host(pages.data(), page_size, n, cls.data() + first, nullptr, &ssum, nullptr, 0)) {
            std::fprintf(stderr, "Scrub of %s failed (%d): %s\n", files[f], rc, pcs_last_error());
            return 1;
        }
    }
    const uint64_t roots[2] = {rep.root, rep.ttl_root};
    std::vector<pcs_tree_node> nodes(table.size());
    std::vector<pcs_tree_problem> problems(table.size());
    pcs_tree_summary sum{};
    std::vector<pcs_leaf_node> leaves(with_leaves ? table.size() : 0);
    std::vector<pcs_leaf_problem> leaf_problems(with_leaves ? table.size() : 0);
    pcs_leaf_summary lsum{};
    int rc;
    if (with_leaves) {
        rc = pcs_leaf_check_host(window.data(), page_size, n_pages, fp_first, cls.data(), table.data(), table.size(),
                                 roots, 2, nodes.data(), &sum, leaves.data(), &lsum, leaf_problems.data(),
                                 leaf_problems.size());
        // the tree's problems are its reached nodes with any bit set, ascending
        sum.n_listed = 0;
        for (size_t p = 0; rc == PCS_OK && p < nodes.size(); ++p)
            if (nodes[p].parent != UINT32_MAX && nodes[p].bits)
                problems[sum.n_listed++] = pcs_tree_problem{(uint32_t)p, nodes[p].parent, nodes[p].bits, nodes[p].depth};
    } else {
        rc = pcs_tree_check_host(window.data(), page_size, n_pages, fp_first, cls.data(), table.data(), table.size(),
                                 roots, 2, nodes.data(), &sum, problems.data(), problems.size());
    }
    if (rc == PCS_ERR_NOMEM) {
        std::fputs(too_large, stderr);
        return 1;
    }
    if (rc) {
        std::fprintf(stderr, "%s check failed (%d): %s\n", with_leaves ? "Leaf" : "Tree", rc, pcs_last_error());
        return 1;
    }
    static const char* const tree_name[2] = {"root", "ttl_root"};
    for (int t = 0; t < 2; ++t) {
        if (roots[t] >= UINT32_MAX) {
            std::printf("tree %s none\n", tree_name[t]);
            continue;
        }
        uint64_t reached = 0, by_type[3] = {}, bad = 0, depth = 0;
        for (const pcs_tree_node& n : nodes) {
            if (n.parent == UINT32_MAX || n.tree != t) continue;
            ++reached;
            depth = std::max<uint64_t>(depth, n.depth);
            if (n.bits) ++bad;
            else if (n.type < 3) ++by_type[n.type];
        }
        std::printf("tree %s %llu reached %llu nonleaf %llu leaf_index %llu data %llu problems %llu max_depth %llu\n",
                    tree_name[t], (unsigned long long)roots[t], (unsigned long long)reached,
                    (unsigned long long)by_type[0], (unsigned long long)by_type[1], (unsigned long long)by_type[2],
                    (unsigned long long)bad, (unsigned long long)depth);
    }
    for (uint64_t k = 0; k < sum.n_listed; ++k) {
        char names[96];
        pcs::tree_bit_names(problems[k].bits, names);
        std::printf("  problem: page_id %u parent %u depth %u %s\n", problems[k].page_id, problems[k].parent,
                    problems[k].depth, names);
    }
    std::printf("unreached mapped %llu nonleaf %llu leaf_index %llu data %llu overflow %llu deleted %llu other %llu "
                "unread %llu\n",
                (unsigned long long)sum.n_unreached_mapped, (unsigned long long)sum.unreached_by_type[0],
                (unsigned long long)sum.unreached_by_type[1], (unsigned long long)sum.unreached_by_type[2],
                (unsigned long long)sum.unreached_by_type[3], (unsigned long long)sum.unreached_by_type[4],
                (unsigned long long)sum.unreached_by_type[5], (unsigned long long)sum.n_unreached_unread);
    if (!with_leaves) return pcs::tree_tool_exit(sum);
    using ull = unsigned long long;
    std::printf("leaves data_pages %llu ok %llu entries %llu overflow_values %llu expiring %llu compressed %llu "
                "inline_bytes %llu\n",
                (ull)lsum.n_data_pages, (ull)lsum.n_data_ok, (ull)lsum.n_entries, (ull)lsum.n_overflow_values,
                (ull)lsum.n_expiring, (ull)lsum.n_compressed, (ull)lsum.inline_value_bytes);
    std::printf("overflow pages %llu ok %llu value_bytes %llu refs %llu extra %llu out_of_range %llu to_tree %llu "
                "misplaced %llu capped %llu max_groups %llu leaked %llu\n",
                (ull)lsum.n_overflow_pages, (ull)lsum.n_overflow_ok, (ull)lsum.overflow_value_bytes, (ull)lsum.n_refs,
                (ull)lsum.n_extra_refs, (ull)lsum.n_out_of_range_refs, (ull)lsum.n_refs_to_tree,
                (ull)lsum.n_misplaced_pointers, (ull)lsum.n_chain_capped, (ull)lsum.max_groups,
                (ull)lsum.n_leaked_overflow);
    for (uint64_t k = 0; k < lsum.n_listed; ++k) {
        char names[112];
        pcs::leaf_bit_names(leaf_problems[k].bits, names);
        std::printf("  leaf problem: page_id %u owner %u entry %u %s\n", leaf_problems[k].page_id, leaf_problems[k].owner,
                    leaf_problems[k].owner_entry, names);
    }
    return pcs::leaf_tool_exit(lsum, pcs::tree_tool_exit(sum));
}

int main(int argc, char** argv) {
    if (argc >= 2 && (!std::strcmp(argv[1], "--tree") || !std::strcmp(argv[1], "--leaves"))) {
        if (argc < 6) {
            usage(argv[0]);
            return 1;
        }
        return tree(argv[1][2] == 'l', argv[2], argv[3], argv[4], argc - 5, argv + 5);
    }
    if (argc >= 2 && !std::strcmp(argv[1], "--live")) {
        if (argc < 6) {
            usage(argv[0]);
            return 1;
        }
        return live(argv[2], argv[3], argv[4], argc - 5, argv + 5);
    }
    if (argc >= 2 && !std::strcmp(argv[1], "--check-manifest")) {
        if (argc < 3) {
            usage(argv[0]);
            return 1;
        }
        return check_manifests(argc - 2, argv + 2);
    }
    if (argc >= 2 && (!std::strcmp(argv[1], "--scan") || !std::strcmp(argv[1], "--stamp"))) {
        if (argc < 3 || argc > 4) {
            usage(argv[0]);
            return 1;
        }
        return bulk(argv[1][2] == 's' && argv[1][3] == 't', argv[2], argc == 4 ? argv[3] : nullptr);
    }
    if (argc >= 2 && (!std::strcmp(argv[1], "--scrub") || !std::strcmp(argv[1], "--extents"))) {
        if (argc < 3 || argc > 4) {
            usage(argv[0]);
            return 1;
        }
        return scrub(argv[2], argc == 4 ? argv[3] : nullptr, argv[1][2] == 'e');
    }
    if (argc >= 2 && !std::strcmp(argv[1], "--scrub-files")) {
        if (argc < 4) {
            usage(argv[0]);
            return 1;
        }
        return scrub_files(argv[2], argc - 3, argv + 3);
    }
    if (argc >= 2 && !std::strcmp(argv[1], "--gen")) {
        if (argc < 4 || argc > 6) {
            usage(argv[0]);
            return 1;
        }
        return gen(argv[2], argv[3], argc > 4 ? argv[4] : nullptr, argc > 5 ? argv[5] : nullptr);
    }
    if (argc < 3 || argc > 4) {
        usage(argv[0]);
        return 1;
    }
    return single_page(argv[1], argv[2], argc == 4 ? argv[3] : nullptr);
}
