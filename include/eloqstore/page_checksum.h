// page_checksum.h — C++ drop-in for EloqStore's page checksum call surface,
// backed by the MI355X kernels behind include/eloqstore_pcs.h.
//
// Reference surface (namespace eloqstore, include/storage/page.h:25-26):
//     void SetChecksum(std::string_view blob);      // src/storage/page.cpp:18-23
//     bool ValidateChecksum(std::string_view blob);  // src/storage/page.cpp:25-31
// This header only re-declares those two functions (an identical
// redeclaration is legal next to page.h) and defines nothing page.h defines:
// the header constants (checksum_bytes = 8, page_type_offset, page.h:11-12)
// stay page.h's, so both headers can be included in one translation unit
// (tests/test_integration_compile.py compiles INTEGRATION.md's call-site
// snippets against the reference's own page.h).
// Same names, namespace and argument meaning: blob is one whole page,
// blob.size() >= 8 is assumed exactly as in the reference (a shorter blob
// never validates and SetChecksum leaves it untouched); SetChecksum writes the
// little-endian digest into blob[0, 8) through const_cast, as page.cpp does.
// The two single-page functions are defined ONLY in the opt-in
// libeloqstore_pcs_dropin.so (for a store that deletes page.cpp's bodies);
// the batch library libeloqstore_pcs.so does not export them, so a store that
// keeps page.cpp's CPU definitions (the recommended integration,
// INTEGRATION.md §2.4) resolves them to page.cpp in any link or DSO order.
// They terminate the process on a GPU failure (the reference's functions
// cannot fail, and a silent `false` would be reported by callers as
// KvError::Corrupted).
//
// Batched forms for the natural batch points of the callers
// (IouringMgr::ReadPages, async_io_manager.cpp:353-366; FlushBatchPages,
// write_task.cpp:155-167) — scattered pool pages of one page size — in two
// flavours: the Try* forms return a status (PCS_OK or a negative pcs_status,
// message in LastChecksumError()) so a call site can fall back to the
// reference's per-page loop on a GPU failure, and
// the plain forms terminate with the message instead.
#pragma once

#include <cstddef>
#include <cstdint>
#include <span>
#include <string_view>
#include <vector>

struct pcs_batch;  // include/eloqstore_pcs.h (global namespace, C ABI)

namespace eloqstore {

void SetChecksum(std::string_view blob);
bool ValidateChecksum(std::string_view blob);

// Hash variant for the batched forms (the reference path is always XXH3).
enum class PageHash : int { XXH3_64 = 0, XXH64 = 1 };

// Batch-size policy for the call sites.  A GPU batch pays
// a fixed launch + completion cost before any byte is hashed (~14 µs for one
// page) while the reference's CPU loop pays per page (~0.6 µs per cache-cold
// 4 KiB page), so small batches stay on the reference's own per-page
// ValidateChecksum / SetChecksum (page.cpp:18-31): the 6-page scan prefetch
// (types.h:31, scan_task.cpp:215), short overflow reads (task.cpp:136), the
// tail of a write batch.  Defaults are the measured latency crossovers of one
// call against one core running the reference loop over the same scattered
// 4 KiB pool pages (integration_snippets --crossover, every repetition timing
// the columns in a fresh random order, with a control column that must agree
// within 3 %; DESIGN.md §5, profiles/r05/crossover_r05e.txt):
//   registered pool (RegisterPagePool, zero-copy): GPU faster from 32 pages
//   to validate (32 pages = 128 KiB) and from 32-48 pages to stamp (three
//   boxes: 32, 48, 48; the write gate is 48 pages = 192 KiB);
//   unregistered pages (gathered into staging):    GPU faster from 192-256 pages.
inline constexpr size_t kGpuChecksumMinBatchBytes = size_t(128) << 10;
inline constexpr size_t kGpuStampMinBatchBytes = size_t(192) << 10;  // FlushBatchPages
inline constexpr size_t kGpuChecksumMinBatchBytesStaged = size_t(1) << 20;
inline bool GpuChecksumPays(size_t n_pages, size_t page_size, size_t min_bytes = kGpuChecksumMinBatchBytes) {
    return n_pages * page_size >= min_bytes;
}

// Manifest records (ManifestBuilder::CalcChecksum, root_meta.cpp:150-174):
// the host-memory ManifestChecksum copies the record over PCIe and runs three
// launches (~54 µs at 64 KiB), so only records from this size on (snapshots,
// large mapping logs) are faster on the GPU; smaller ones keep the reference
// loop.  Measured crossover, same harness: 6 MiB (259 vs 239 µs; 64 MiB:
// 2.8 ms on one core, 1.44 ms on the GPU).
inline constexpr size_t kGpuManifestMinBytes = size_t(6) << 20;

// Non-aborting forms.  Return PCS_OK (0) or a negative pcs_status
// (include/eloqstore_pcs.h) with the message in LastChecksumError(); on
// PCS_OK, *first_bad (if given) is the first corrupted index or pages.size().
// A failed call has written nothing a caller may trust: the read path falls
// back to page.cpp's ValidateChecksum loop, as the reference would run it
// (async_io_manager.cpp:353-366), and the write path to SetChecksum.
int TryValidateChecksums(std::span<const char* const> pages, size_t page_size, uint8_t* ok_out, size_t* first_bad,
                         PageHash hash = PageHash::XXH3_64, bool skip_verify = false);
int TrySetChecksums(std::span<char* const> pages, size_t page_size, PageHash hash = PageHash::XXH3_64);
const char* LastChecksumError();  // the calling thread's last failure (pcs_last_error)

// Validates every page; ok_out[i] = 1 if page i's stored digest matches.
// Returns the index of the first corrupted page, or pages.size() if all match
// (the reference loop stops at the first failure, async_io_manager.cpp:357-363;
// the batch checks all and reports the first).  skip_verify mirrors
// KvOptions::skip_verify_checksum (kv_options.h:41): nothing is hashed and every
// page is reported valid (PCS_FLAG_SKIP_VERIFY; needs no GPU).
size_t ValidateChecksums(std::span<const char* const> pages, size_t page_size, uint8_t* ok_out,
                         PageHash hash = PageHash::XXH3_64, bool skip_verify = false);

// Stamps every page in place (batched SetChecksum).
void SetChecksums(std::span<char* const> pages, size_t page_size, PageHash hash = PageHash::XXH3_64);

// Digests without touching the pages.
void PageDigests(std::span<const char* const> pages, size_t page_size, uint64_t* digests_out,
                 PageHash hash = PageHash::XXH3_64);

// Scrub (pcs_pages_scrub_host): classifies every page as ok (stored digest
// matches), blank (every byte zero: the never-written tail of a fallocated
// data file) or corrupt, counts the ok pages by PageType (page byte 8) and
// lists the corrupt ones.  XXH3 pages of at least 249 bytes only.
struct ScrubReport {
    uint64_t n_pages = 0, n_ok = 0, n_corrupt = 0, n_blank = 0;
    // ok pages by type: NonLeafIndex, LeafIndex, Data, Overflow, Deleted (255), any other byte
    uint64_t ok_by_type[6] = {};
    uint64_t first_corrupt = UINT64_MAX;  // UINT64_MAX when none
    std::vector<uint64_t> corrupt;        // the smallest corrupt page indices, ascending, at most max_listed
    std::vector<uint8_t> page_class;      // pcs_page_class of every page
    std::vector<uint8_t> page_type;       // byte 8 of every page
};
// PCS_OK or a negative pcs_status (message in LastChecksumError()); a failed
// call leaves the report unspecified.
int TryScrubPages(std::span<const char* const> pages, size_t page_size, ScrubReport& report,
                  size_t max_listed = 1024);
ScrubReport ScrubPages(std::span<const char* const> pages, size_t page_size, size_t max_listed = 1024);

// Scrub extents (pcs_pages_scrub_extents_host): the scrub above without the
// per-page arrays, plus where the classes lie: the maximal runs of equal class
// (the first max_runs of them, ascending, each with its full length), the
// written extent and the holes.  An append-mode data file is written in page
// order, so a blank page below written_pages (a hole) is a lost or trimmed
// write there; the blank pages from written_pages on are the never-written tail.
struct PageExtent {
    uint64_t first_page = 0, n_pages = 0;
    uint8_t page_class = 0;  // pcs_page_class
};
struct ExtentReport {
    uint64_t n_pages = 0, n_ok = 0, n_corrupt = 0, n_blank = 0;
    uint64_t ok_by_type[6] = {};       // as ScrubReport
    uint64_t first_corrupt = UINT64_MAX;
    std::vector<uint64_t> corrupt;     // the smallest corrupt page indices, ascending, at most max_listed
    uint64_t n_runs = 0;               // all runs, whatever max_runs
    uint64_t written_pages = 0;        // 1 + the last non-blank page; 0 when every page is blank
    uint64_t n_blank_runs = 0;         // the tail included
    uint64_t first_blank = UINT64_MAX;
    uint64_t n_holes = 0, n_hole_pages = 0;
    uint64_t first_hole = UINT64_MAX;
    std::vector<PageExtent> runs;      // the first min(n_runs, max_runs) runs
};
// PCS_OK or a negative pcs_status (message in LastChecksumError()); a failed
// call leaves the report unspecified.
int TryScrubExtents(std::span<const char* const> pages, size_t page_size, ExtentReport& report,
                    size_t max_runs = 1024, size_t max_listed = 1024);
ExtentReport ScrubExtents(std::span<const char* const> pages, size_t page_size, size_t max_runs = 1024,
                          size_t max_listed = 1024);

// Scrub files (pcs_pages_scrub_files_host): a batch that holds several data
// files, scrubbed in one call, one report per file.  File f is pages
// [file_first_page[f], file_first_page[f + 1]) of `pages`; the n_files + 1
// boundaries ascend (equal neighbours: an empty file) from 0 to pages.size().
// A file's counts are ScrubReport's and its written extent and holes
// ExtentReport's over the file's pages alone, with file-local page indices: a
// blank run never crosses a file boundary.  A file is bad when it has a
// corrupt page or a hole; bad_files lists the first max_listed of them.
struct FileReport {
    uint64_t first_page = 0, n_pages = 0;  // the file's range in the batch
    uint64_t n_ok = 0, n_corrupt = 0, n_blank = 0;
    uint64_t ok_by_type[6] = {};           // as ScrubReport
    uint64_t first_corrupt = UINT64_MAX;   // file-local
    uint64_t written_pages = 0;            // file-local: 1 + the last non-blank page
    uint64_t n_holes = 0, n_hole_pages = 0;
    uint64_t first_hole = UINT64_MAX;      // file-local
};
struct FilesReport {
    std::vector<FileReport> files;
    uint64_t n_pages = 0, n_ok = 0, n_corrupt = 0, n_blank = 0;  // pages, over all files
    uint64_t n_corrupt_files = 0, n_hole_files = 0, n_bad_files = 0, n_unwritten_files = 0;
    uint64_t first_bad_file = UINT64_MAX;
    std::vector<uint64_t> bad_files;       // the first min(n_bad_files, max_listed) bad files, ascending
};
// PCS_OK or a negative pcs_status (message in LastChecksumError()); a failed
// call leaves the report unspecified.
int TryScrubFiles(std::span<const char* const> pages, size_t page_size, std::span<const uint64_t> file_first_page,
                  FilesReport& report, size_t max_listed = 1024);
FilesReport ScrubFiles(std::span<const char* const> pages, size_t page_size,
                       std::span<const uint64_t> file_first_page, size_t max_listed = 1024);
// The store's usual case: files of pages_per_file pages each (> 0), the last
// one short when pages.size() is no multiple of it.
int TryScrubFiles(std::span<const char* const> pages, size_t page_size, uint64_t pages_per_file, FilesReport& report,
                  size_t max_listed = 1024);
FilesReport ScrubFiles(std::span<const char* const> pages, size_t page_size, uint64_t pages_per_file,
                       size_t max_listed = 1024);

// Manifest scan (pcs_manifest_scan_host): walks every record of many manifest
// images in one call and checks each against ManifestBuilder::CalcChecksum,
// following Replayer::ParseNextRecord (src/replayer.cpp:74-140).  Image i is
// images[i], a whole manifest file in host memory (any alignment); align is
// the record alignment (page_align).  A manifest's verdict maps to the
// replayer's outcome: kClean replays whole, kTornTail is cut back to
// valid_prefix_bytes, kBroken is KvError::Corrupted (replayer.cpp:60-63),
// kBadSnapshot fails the open (replayer.cpp:37-38), kEmpty has no record.
enum class ManifestVerdict : uint64_t { kClean = 0, kTornTail = 1, kBroken = 2, kBadSnapshot = 3, kEmpty = 4 };
enum class ManifestEnd : uint64_t { kClean = 0, kShortHeader = 1, kShortPayload = 2, kShortPadding = 3 };
struct ManifestRecord {
    uint64_t offset = 0;                // in its image
    uint64_t stored = 0, computed = 0;  // the record's checksum word / CalcChecksum of its content
    uint32_t payload_len = 0, root = 0, ttl_root = 0, ok = 0;
};
struct ManifestReport {
    uint64_t size = 0, n_records = 0, n_ok = 0, n_corrupt = 0;
    uint64_t first_corrupt = UINT64_MAX;  // record index in the image
    uint64_t n_ok_after_corrupt = 0;
    uint64_t valid_prefix_bytes = 0;      // offset of the first corrupt record, else where the walk stopped
    uint64_t end_offset = 0;
    ManifestEnd end_reason = ManifestEnd::kClean;
    ManifestVerdict verdict = ManifestVerdict::kEmpty;
    uint64_t first_record = 0;            // index of the image's record 0 in ManifestsReport::records
    uint64_t max_record_bytes = 0;
};
struct ManifestsReport {
    std::vector<ManifestReport> manifests;
    uint64_t n_records = 0, n_ok = 0, n_corrupt = 0;
    uint64_t n_by_verdict[5] = {};
    uint64_t first_bad_manifest = UINT64_MAX;  // first verdict other than kClean
    std::vector<ManifestRecord> records;       // the first min(n_records, max_records) records, images in order
};
// PCS_OK or a negative pcs_status (message in LastChecksumError()); a failed
// call leaves the report unspecified.
int TryScanManifests(std::span<const std::string_view> images, ManifestsReport& report, uint32_t align = 4096,
                     size_t max_records = 1 << 16);
ManifestsReport ScanManifests(std::span<const std::string_view> images, uint32_t align = 4096,
                              size_t max_records = 1 << 16);

// Manifest replay (pcs_manifest_replay_host): what Replayer::Replay computes
// (src/replayer.cpp:27-72, 142-228) for every image of a batch: the final
// logical-page to file-page table, root, ttl_root and max_fp_id.  Manifest i's
// rows are table[table_first .. table_first + table_size) when its status is
// kOk; a row nobody wrote is MappingSnapshot::InvalidValue (7); a row maps file
// page v >> 3 iff (v & 7) == 1.  max_rows caps the rows of the whole batch: a
// manifest whose rows do not fit is kTableCap and writes none.
enum class ReplayStatus : uint64_t { kOk = 0, kNotReplayable = 1, kMalformed = 2, kTableCap = 3 };
struct ManifestReplay {
    ReplayStatus status = ReplayStatus::kNotReplayable;
    uint64_t n_replayed = 0;
    uint64_t malformed_record = UINT64_MAX;  // lowest record that breaks a decode rule (kMalformed)
    uint64_t root = 0, ttl_root = 0, max_fp_id = 0, dict_bytes = 0;
    uint64_t snapshot_pages = 0, n_log_entries = 0;
    uint64_t table_size = 0, table_first = 0;
    uint64_t n_mapped = 0;
    uint64_t min_fp = UINT64_MAX, max_fp = UINT64_MAX;  // of the mapped file page ids
    uint64_t n_fp_beyond_max = 0;                       // mapped ids >= max_fp_id
    uint64_t n_term_pairs = 0;
};
struct ManifestsReplay {
    std::vector<ManifestReplay> manifests;
    uint64_t n_by_status[4] = {};
    uint64_t n_rows = 0, n_mapped = 0, n_log_entries = 0;
    uint64_t first_bad_manifest = UINT64_MAX;  // first status other than kOk
    std::vector<uint64_t> table;               // the n_rows_written rows of the kOk manifests, in order
    std::vector<ManifestReport> scans;         // the scan's report of every image
};
// The call holds 8 bytes per row of max_rows on the host and 12 on the device
// while it runs, whatever the manifests need: pass what the batch can hold.
int TryReplayManifests(std::span<const std::string_view> images, ManifestsReplay& report, uint32_t align = 4096,
                       size_t max_rows = 1 << 20);
ManifestsReplay ReplayManifests(std::span<const std::string_view> images, uint32_t align = 4096,
                                size_t max_rows = 1 << 20);

// Scrub live (pcs_scrub_live_host): classes is a scrub's class byte per file
// page fp_first .. fp_first + classes.size(), table a replayed mapping table.
// A page is live iff a table row maps it; owner[i] is the lowest such row
// (UINT32_MAX for a dead page).  damaged lists every live page whose class is
// not ok, ascending, at most max_listed of them; n_damaged is always full.
struct LivePage {
    uint64_t index = 0;            // in the window
    uint32_t page_id = 0, cls = 0; // its owner, its class byte
};
struct LiveReport {
    uint64_t n_pages = 0, table_size = 0, n_mapped = 0, n_mapped_in_window = 0, n_duplicate = 0;
    uint64_t live_ok = 0, live_blank = 0, live_corrupt = 0, dead_ok = 0, dead_blank = 0, dead_corrupt = 0;
    uint64_t n_damaged = 0;
    uint64_t first_damaged = UINT64_MAX, last_live = UINT64_MAX;
    std::vector<LivePage> damaged;
    std::vector<uint32_t> owner;
};
int TryScrubLive(std::span<const uint8_t> classes, uint64_t fp_first, std::span<const uint64_t> table,
                 LiveReport& report, size_t max_listed = 1024);
LiveReport ScrubLive(std::span<const uint8_t> classes, uint64_t fp_first, std::span<const uint64_t> table,
                     size_t max_listed = 1024);

// Tree check (pcs_tree_check_host): walks the index tree that hangs off every
// root of a replayed table, breadth-first, over the file pages fp_first ..
// fp_first + pages.size() / page_size held in ONE contiguous buffer (the whole
// window must fit in device memory).  classes are a scrub's class bytes for
// those pages; an empty span scrubs them on the device first.  A root >=
// UINT32_MAX is an empty tree.  nodes[p] describes table row p (parent
// UINT32_MAX: reached from no root); problems lists the reached pages with any
// bit set, ascending by page id, at most max_listed of them; n_problems is
// always full.  The bits are enum pcs_tree_bits of eloqstore_pcs.h.
struct TreeNode {
    uint32_t parent = UINT32_MAX;
    uint8_t depth = 0xFF, tree = 0xFF, type = 0xFF, bits = 0;
    uint32_t n_children = 0, n_bad_children = 0;
};
struct TreeProblem {
    uint32_t page_id = 0, parent = 0, bits = 0, depth = 0;
};
struct TreeReport {
    uint64_t n_pages = 0, table_size = 0, n_mapped = 0, n_reached = 0;
    uint64_t n_nonleaf = 0, n_leaf_index = 0, n_data = 0;
    uint64_t n_refs = 0, n_extra_refs = 0, n_out_of_range_refs = 0;
    uint64_t max_depth = UINT64_MAX, n_depth_capped = 0;
    uint64_t n_by_bit[8] = {};
    uint64_t n_problems = 0, first_problem = UINT64_MAX;
    uint64_t n_unreached_mapped = 0, unreached_by_type[6] = {}, n_unreached_unread = 0;
    uint64_t n_chain_heads = 0;
    std::vector<TreeProblem> problems;
    std::vector<TreeNode> nodes;
};
int TryCheckTree(std::span<const uint8_t> pages, size_t page_size, uint64_t fp_first,
                 std::span<const uint8_t> classes, std::span<const uint64_t> table, std::span<const uint64_t> roots,
                 TreeReport& report, size_t max_listed = 1024);
TreeReport CheckTree(std::span<const uint8_t> pages, size_t page_size, uint64_t fp_first,
                     std::span<const uint8_t> classes, std::span<const uint64_t> table,
                     std::span<const uint64_t> roots, size_t max_listed = 1024);

// Leaf check (pcs_leaf_check_host): the tree check as above, and then every data
// page it reached in good health is decoded entry by entry and the overflow
// chain of every large value is walked.  tree is the tree check's report (its
// problems list every reached page with a bit set, uncapped); leaves[p]
// describes table row p (owner UINT32_MAX: neither a checked data page nor an
// overflow page some value claimed); problems lists the checked or claimed
// rows with any bit set, ascending by page id, at most max_listed of them;
// n_problems is always full.  The bits are enum pcs_leaf_bits of eloqstore_pcs.h.
struct LeafNode {
    uint32_t owner = UINT32_MAX;
    uint16_t owner_entry = 0, bits = 0;
    uint32_t a = 0, b = 0;
};
struct LeafProblem {
    uint32_t page_id = 0, owner = 0, bits = 0, owner_entry = 0;
};
struct LeafReport {
    TreeReport tree;
    uint64_t n_pages = 0, table_size = 0, n_data_pages = 0, n_data_ok = 0;
    uint64_t n_entries = 0, n_overflow_values = 0, n_expiring = 0, n_compressed = 0;
    uint64_t inline_value_bytes = 0, overflow_value_bytes = 0;
    uint64_t n_refs = 0, n_out_of_range_refs = 0, n_extra_refs = 0, n_refs_to_tree = 0;
    uint64_t n_misplaced_pointers = 0, n_chain_capped = 0, max_groups = 0, n_overflow_pages = 0;
    uint64_t n_by_bit[9] = {};
    uint64_t n_problems = 0, first_problem = UINT64_MAX;
    uint64_t n_leaked_overflow = 0, n_overflow_ok = 0;
    std::vector<LeafProblem> problems;
    std::vector<LeafNode> leaves;
};
int TryCheckLeaves(std::span<const uint8_t> pages, size_t page_size, uint64_t fp_first,
                   std::span<const uint8_t> classes, std::span<const uint64_t> table, std::span<const uint64_t> roots,
                   LeafReport& report, size_t max_listed = 1024);
LeafReport CheckLeaves(std::span<const uint8_t> pages, size_t page_size, uint64_t fp_first,
                       std::span<const uint8_t> classes, std::span<const uint64_t> table,
                       std::span<const uint64_t> roots, size_t max_listed = 1024);

// Registers a page-pool chunk or io_uring buffer ring once (PagesPool::Extend,
// src/storage/page.cpp:95-120): batches whose pages all lie in registered
// memory are then hashed in place over PCIe in one launch, with no gather
// copy (pcs_host_register).  Unregister only when no batch over it is in flight.
void RegisterPagePool(void* base, size_t bytes);
void UnregisterPagePool(void* base);

// Pre-armed validate service (pcs_service_start, opt-in): while it is on,
// ValidateChecksums, SetChecksums and ChecksumBatch's validate and stamp
// batches of up to 256 registered pages are served through a resident kernel
// polling a request line, instead of a launch per batch, and the GPU pays
// from kGpuChecksumMinBatchBytesService on (4 KiB pool pages,
// integration_snippets --crossover, profiles/r05/crossover_r05e.txt: one page
// 7.8 µs to validate instead of 14.8 and 8.2 µs to stamp instead of 15.2;
// faster than the reference loop from 24 pages, both ways).  The kernel holds
// `workgroups` CUs (16 serves 128-256 pages 10-15 % faster than 4) and
// leaves after idle_us without a request or 2 * idle_us of life; the next
// request starts a new one.  `lines` request lines (1-8) let that many calls
// be served at once, each line by its own `workgroups` workgroups.  A call
// that finds every line owned, or that arrives while more than
// PCS_TUNE_SERVICE_MAX_CALLERS + lines - 1 eligible calls are in progress on
// the device (a decaying average; the knob is 2 by default), takes the launch
// path.  Start and stop act on the calling thread's current device; each
// device has its own service.
void StartChecksumService(int workgroups = 4, uint32_t idle_us = 1000, int lines = 1);
void StopChecksumService();
// Optional, once per shard thread at start-up (pcs_thread_prepare): creates
// the thread's stream and the pinned buffers a batch of up to 256 pages uses
// and runs one 1-page batch, so the thread's first ReadPages / FlushBatchPages
// batch does not pay for that (16-35 ms with eight threads starting at once).
void PrepareChecksumThread();
inline constexpr size_t kGpuChecksumMinBatchBytesService = size_t(96) << 10;

// Asynchronous batch for coroutine call sites: Submit, then Poll() from the
// shard work loop (shard.cpp:67-130) until it returns true.  Pages must stay
// valid until then; SubmitStamp writes the digests into them on completion.
// With the validate service on, an eligible batch is posted to it (no
// launch) and Poll() watches its verdict words.
class ChecksumBatch {
public:
    ChecksumBatch();  // never aborts: a failed creation is Status(), and every call reports it
    ~ChecksumBatch();
    ChecksumBatch(const ChecksumBatch&) = delete;
    ChecksumBatch& operator=(const ChecksumBatch&) = delete;

    // skip_verify mirrors KvOptions::skip_verify_checksum (kv_options.h:41):
    // the batch completes at submit with every page reported valid.
    void SubmitValidate(std::span<const char* const> pages, size_t page_size, PageHash hash = PageHash::XXH3_64,
                        bool skip_verify = false);
    void SubmitStamp(std::span<char* const> pages, size_t page_size, PageHash hash = PageHash::XXH3_64);
    bool Poll();  // true once complete; never blocks
    void Wait();
    // Non-aborting forms: PCS_OK / a negative pcs_status (TrySubmit*), and
    // 1 complete / 0 in flight / a negative pcs_status (TryPoll).
    int TrySubmitValidate(std::span<const char* const> pages, size_t page_size, PageHash hash = PageHash::XXH3_64,
                          bool skip_verify = false);
    int TrySubmitStamp(std::span<char* const> pages, size_t page_size, PageHash hash = PageHash::XXH3_64);
    int TryPoll();
    int Status() const { return status_; }  // PCS_OK, or why the batch could not be created
    // Validate mode, after completion: index of the first corrupted page, or
    // the batch size if every page matched.
    size_t FirstBad() const { return first_bad_; }
    const uint8_t* Verdicts() const { return ok_.data(); }
    // PCS_PATH_* bits of the last submission: which path served it (pcs_batch_path).
    int Path() const;

private:
    int Collect();
    ::pcs_batch* batch_ = nullptr;
    int status_ = 0;
    std::vector<uint8_t> ok_;
    size_t n_ = 0, first_bad_ = 0;
    bool validate_ = false, collected_ = false;
};

// ManifestBuilder::CalcChecksum / ValidateChecksum (src/storage/root_meta.cpp:138-174).
uint64_t ManifestChecksum(std::string_view content);
bool ValidateManifestRecord(std::string_view record);

}  // namespace eloqstore
