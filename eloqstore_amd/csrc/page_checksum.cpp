// page_checksum.cpp — the batched C++ forms of eloqstore's page checksum over
// the C ABI (include/eloqstore/page_checksum.h).  The single-page
// SetChecksum / ValidateChecksum live in page_checksum_dropin.cpp, a library
// of their own, so linking this one never interposes on page.cpp's.
#include "eloqstore/page_checksum.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "eloqstore_pcs.h"

namespace eloqstore {
namespace {

[[noreturn]] void die(const char* where, int rc) {
    std::fprintf(stderr, "eloqstore page checksum: %s failed (%d): %s\n", where, rc, pcs_last_error());
    std::abort();
}

}  // namespace

int TryValidateChecksums(std::span<const char* const> pages, size_t page_size, uint8_t* ok_out, size_t* first_bad,
                         PageHash hash, bool skip_verify) {
    uint64_t fb = UINT64_MAX;
    static_assert(sizeof(const char*) == sizeof(const void*));
    const int rc = pcs_pages_validate_host_ex(reinterpret_cast<const void* const*>(pages.data()), page_size,
                                              pages.size(), static_cast<int>(hash), ok_out, &fb,
                                              skip_verify ? PCS_FLAG_SKIP_VERIFY : PCS_FLAG_NONE);
    if (rc == PCS_OK && first_bad) *first_bad = fb == UINT64_MAX ? pages.size() : static_cast<size_t>(fb);
    return rc;
}

int TrySetChecksums(std::span<char* const> pages, size_t page_size, PageHash hash) {
    return pcs_pages_stamp_host(reinterpret_cast<void* const*>(pages.data()), page_size, pages.size(),
                                static_cast<int>(hash));
}

const char* LastChecksumError() { return pcs_last_error(); }

size_t ValidateChecksums(std::span<const char* const> pages, size_t page_size, uint8_t* ok_out, PageHash hash,
                         bool skip_verify) {
    size_t first_bad = pages.size();
    if (int rc = TryValidateChecksums(pages, page_size, ok_out, &first_bad, hash, skip_verify))
        die("ValidateChecksums", rc);
    return first_bad;
}

void SetChecksums(std::span<char* const> pages, size_t page_size, PageHash hash) {
    if (int rc = TrySetChecksums(pages, page_size, hash)) die("SetChecksums", rc);
}

void PageDigests(std::span<const char* const> pages, size_t page_size, uint64_t* digests_out, PageHash hash) {
    if (int rc = pcs_pages_digest_host(reinterpret_cast<const void* const*>(pages.data()), page_size, pages.size(),
                                       static_cast<int>(hash), digests_out))
        die("PageDigests", rc);
}

int TryScrubPages(std::span<const char* const> pages, size_t page_size, ScrubReport& report, size_t max_listed) {
    const size_t n = pages.size();
    report.page_class.assign(n, 0);
    report.page_type.assign(n, 0);
    report.corrupt.assign(std::min(max_listed, n), 0);
    pcs_scrub_summary sum{};
    const int rc = pcs_pages_scrub_host(reinterpret_cast<const void* const*>(pages.data()), page_size, n,
                                        report.page_class.data(), report.page_type.data(), &sum,
                                        report.corrupt.data(), report.corrupt.size());
    if (rc != PCS_OK) return rc;
    report.n_pages = sum.n_pages;
    report.n_ok = sum.n_ok;
    report.n_corrupt = sum.n_corrupt;
    report.n_blank = sum.n_blank;
    for (int k = 0; k < 6; ++k) report.ok_by_type[k] = sum.ok_by_type[k];
    report.first_corrupt = sum.first_corrupt;
    report.corrupt.resize(sum.n_listed);
    return PCS_OK;
}

ScrubReport ScrubPages(std::span<const char* const> pages, size_t page_size, size_t max_listed) {
    ScrubReport report;
    if (int rc = TryScrubPages(pages, page_size, report, max_listed)) die("ScrubPages", rc);
    return report;
}

int TryScrubExtents(std::span<const char* const> pages, size_t page_size, ExtentReport& report, size_t max_runs,
                    size_t max_listed) {
    const size_t n = pages.size();
    report.corrupt.assign(std::min(max_listed, n), 0);
    std::vector<pcs_extent> runs(std::min(max_runs, n));
    pcs_scrub_summary sum{};
    pcs_extent_summary ext{};
    const int rc = pcs_pages_scrub_extents_host(reinterpret_cast<const void* const*>(pages.data()), page_size, n,
                                                nullptr, nullptr, &sum, report.corrupt.data(), report.corrupt.size(),
                                                &ext, runs.data(), runs.size());
    if (rc != PCS_OK) return rc;
    report.n_pages = sum.n_pages;
    report.n_ok = sum.n_ok;
    report.n_corrupt = sum.n_corrupt;
    report.n_blank = sum.n_blank;
    for (int k = 0; k < 6; ++k) report.ok_by_type[k] = sum.ok_by_type[k];
    report.first_corrupt = sum.first_corrupt;
    report.corrupt.resize(sum.n_listed);
    report.n_runs = ext.n_runs;
    report.written_pages = ext.written_pages;
    report.n_blank_runs = ext.n_blank_runs;
    report.first_blank = ext.first_blank;
    report.n_holes = ext.n_holes;
    report.n_hole_pages = ext.n_hole_pages;
    report.first_hole = ext.first_hole;
    report.runs.resize(ext.n_listed);
    for (size_t i = 0; i < report.runs.size(); ++i)
        report.runs[i] = PageExtent{runs[i].first_page, runs[i].n_pages, static_cast<uint8_t>(runs[i].cls)};
    return PCS_OK;
}

ExtentReport ScrubExtents(std::span<const char* const> pages, size_t page_size, size_t max_runs, size_t max_listed) {
    ExtentReport report;
    if (int rc = TryScrubExtents(pages, page_size, report, max_runs, max_listed)) die("ScrubExtents", rc);
    return report;
}

int TryScrubFiles(std::span<const char* const> pages, size_t page_size, std::span<const uint64_t> file_first_page,
                  FilesReport& report, size_t max_listed) {
    static_assert(sizeof(FileReport) == sizeof(pcs_file_report), "FileReport mirrors pcs_file_report");
    if (file_first_page.empty()) return pcs_pages_scrub_files_host(nullptr, page_size, 0, nullptr, 0, nullptr, nullptr, nullptr, 0);
    const size_t n_files = file_first_page.size() - 1;
    std::vector<pcs_file_report> reports(n_files);
    report.bad_files.assign(std::min(max_listed, n_files), 0);
    pcs_files_summary sum{};
    const int rc = pcs_pages_scrub_files_host(reinterpret_cast<const void* const*>(pages.data()), page_size,
                                              pages.size(), file_first_page.data(), n_files, reports.data(), &sum,
                                              report.bad_files.data(), report.bad_files.size());
    if (rc != PCS_OK) return rc;
    report.files.resize(n_files);
    for (size_t f = 0; f < n_files; ++f) {
        const pcs_file_report& r = reports[f];
        FileReport& o = report.files[f];
        o.first_page = r.first_page;
        o.n_pages = r.n_pages;
        o.n_ok = r.n_ok;
        o.n_corrupt = r.n_corrupt;
        o.n_blank = r.n_blank;
        for (int k = 0; k < 6; ++k) o.ok_by_type[k] = r.ok_by_type[k];
        o.first_corrupt = r.first_corrupt;
        o.written_pages = r.written_pages;
        o.n_holes = r.n_holes;
        o.n_hole_pages = r.n_hole_pages;
        o.first_hole = r.first_hole;
    }
    report.n_pages = sum.n_pages;
    report.n_ok = sum.n_ok;
    report.n_corrupt = sum.n_corrupt;
    report.n_blank = sum.n_blank;
    report.n_corrupt_files = sum.n_corrupt_files;
    report.n_hole_files = sum.n_hole_files;
    report.n_bad_files = sum.n_bad_files;
    report.n_unwritten_files = sum.n_unwritten_files;
    report.first_bad_file = sum.first_bad_file;
    report.bad_files.resize(sum.n_listed);
    return PCS_OK;
}

FilesReport ScrubFiles(std::span<const char* const> pages, size_t page_size, std::span<const uint64_t> file_first_page,
                       size_t max_listed) {
    FilesReport report;
    if (int rc = TryScrubFiles(pages, page_size, file_first_page, report, max_listed)) die("ScrubFiles", rc);
    return report;
}

int TryScrubFiles(std::span<const char* const> pages, size_t page_size, uint64_t pages_per_file, FilesReport& report,
                  size_t max_listed) {
    std::vector<uint64_t> first;  // left empty for pages_per_file == 0: refused as a null boundary array
    if (pages_per_file) {
        const uint64_t n = pages.size(), n_files = n / pages_per_file + (n % pages_per_file ? 1 : 0);
        first.resize(n_files + 1);
        for (uint64_t f = 0; f < n_files; ++f) first[f] = f * pages_per_file;
        first[n_files] = n;
    }
    return TryScrubFiles(pages, page_size, std::span<const uint64_t>(first), report, max_listed);
}

FilesReport ScrubFiles(std::span<const char* const> pages, size_t page_size, uint64_t pages_per_file,
                       size_t max_listed) {
    FilesReport report;
    if (int rc = TryScrubFiles(pages, page_size, pages_per_file, report, max_listed)) die("ScrubFiles", rc);
    return report;
}

int TryScanManifests(std::span<const std::string_view> images, ManifestsReport& report, uint32_t align,
                     size_t max_records) {
    static_assert(sizeof(ManifestRecord) == sizeof(pcs_manifest_record), "ManifestRecord mirrors pcs_manifest_record");
    const size_t n = images.size();
    std::vector<const void*> ptrs(n);
    std::vector<uint64_t> sizes(n);
    for (size_t i = 0; i < n; ++i) {
        ptrs[i] = images[i].data();
        sizes[i] = images[i].size();
    }
    std::vector<pcs_manifest_report> reports(n);
    std::vector<pcs_manifest_record> records(max_records);
    pcs_manifest_summary sum{};
    const int rc = pcs_manifest_scan_host(ptrs.data(), sizes.data(), n, align, reports.data(), &sum, records.data(),
                                          max_records);
    if (rc != PCS_OK) return rc;
    report.manifests.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const pcs_manifest_report& r = reports[i];
        ManifestReport& o = report.manifests[i];
        o.size = r.size;
        o.n_records = r.n_records;
        o.n_ok = r.n_ok;
        o.n_corrupt = r.n_corrupt;
        o.first_corrupt = r.first_corrupt;
        o.n_ok_after_corrupt = r.n_ok_after_corrupt;
        o.valid_prefix_bytes = r.valid_prefix_bytes;
        o.end_offset = r.end_offset;
        o.end_reason = static_cast<ManifestEnd>(r.end_reason);
        o.verdict = static_cast<ManifestVerdict>(r.verdict);
        o.first_record = r.first_record;
        o.max_record_bytes = r.max_record_bytes;
    }
    report.n_records = sum.n_records;
    report.n_ok = sum.n_ok;
    report.n_corrupt = sum.n_corrupt;
    for (int k = 0; k < 5; ++k) report.n_by_verdict[k] = sum.n_by_verdict[k];
    report.first_bad_manifest = sum.first_bad_image;
    report.records.resize(sum.n_listed);
    for (size_t k = 0; k < sum.n_listed; ++k) {
        const pcs_manifest_record& r = records[k];
        report.records[k] = ManifestRecord{r.offset, r.stored, r.computed, r.payload_len, r.root, r.ttl_root, r.ok};
    }
    return PCS_OK;
}

ManifestsReport ScanManifests(std::span<const std::string_view> images, uint32_t align, size_t max_records) {
    ManifestsReport report;
    if (int rc = TryScanManifests(images, report, align, max_records)) die("ScanManifests", rc);
    return report;
}

static ManifestReport to_report(const pcs_manifest_report& r) {
    ManifestReport o;
    o.size = r.size;
    o.n_records = r.n_records;
    o.n_ok = r.n_ok;
    o.n_corrupt = r.n_corrupt;
    o.first_corrupt = r.first_corrupt;
    o.n_ok_after_corrupt = r.n_ok_after_corrupt;
    o.valid_prefix_bytes = r.valid_prefix_bytes;
    o.end_offset = r.end_offset;
    o.end_reason = static_cast<ManifestEnd>(r.end_reason);
    o.verdict = static_cast<ManifestVerdict>(r.verdict);
    o.first_record = r.first_record;
    o.max_record_bytes = r.max_record_bytes;
    return o;
}

int TryReplayManifests(std::span<const std::string_view> images, ManifestsReplay& report, uint32_t align,
                       size_t max_rows) {
    const size_t n = images.size();
    std::vector<const void*> ptrs(n);
    std::vector<uint64_t> sizes(n);
    for (size_t i = 0; i < n; ++i) {
        ptrs[i] = images[i].data();
        sizes[i] = images[i].size();
    }
    std::vector<pcs_manifest_report> scans(n);
    std::vector<pcs_replay_report> reports(n);
    pcs_replay_summary sum{};
    report.table.resize(max_rows);
    const int rc = pcs_manifest_replay_host(ptrs.data(), sizes.data(), n, align, scans.data(), reports.data(), &sum,
                                            report.table.data(), max_rows);
    if (rc != PCS_OK) return rc;
    report.manifests.resize(n);
    report.scans.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const pcs_replay_report& r = reports[i];
        ManifestReplay& o = report.manifests[i];
        o.status = static_cast<ReplayStatus>(r.status);
        o.n_replayed = r.n_replayed;
        o.malformed_record = r.malformed_record;
        o.root = r.root;
        o.ttl_root = r.ttl_root;
        o.max_fp_id = r.max_fp_id;
        o.dict_bytes = r.dict_bytes;
        o.snapshot_pages = r.snapshot_pages;
        o.n_log_entries = r.n_log_entries;
        o.table_size = r.table_size;
        o.table_first = r.table_first;
        o.n_mapped = r.n_mapped;
        o.min_fp = r.min_fp;
        o.max_fp = r.max_fp;
        o.n_fp_beyond_max = r.n_fp_beyond_max;
        o.n_term_pairs = r.n_term_pairs;
        report.scans[i] = to_report(scans[i]);
    }
    for (int k = 0; k < 4; ++k) report.n_by_status[k] = sum.n_by_status[k];
    report.n_rows = sum.n_rows;
    report.n_mapped = sum.n_mapped;
    report.n_log_entries = sum.n_log_entries;
    report.first_bad_manifest = sum.first_bad_image;
    report.table.resize(sum.n_rows_written);
    return PCS_OK;
}

ManifestsReplay ReplayManifests(std::span<const std::string_view> images, uint32_t align, size_t max_rows) {
    ManifestsReplay report;
    if (int rc = TryReplayManifests(images, report, align, max_rows)) die("ReplayManifests", rc);
    return report;
}

int TryScrubLive(std::span<const uint8_t> classes, uint64_t fp_first, std::span<const uint64_t> table,
                 LiveReport& report, size_t max_listed) {
    static_assert(sizeof(LivePage) == sizeof(pcs_live_page), "LivePage mirrors pcs_live_page");
    std::vector<pcs_live_page> listed(max_listed);
    pcs_live_summary sum{};
    report.owner.resize(classes.size());
    const int rc = pcs_scrub_live_host(classes.data(), classes.size(), fp_first, table.data(), table.size(),
                                       report.owner.data(), &sum, listed.data(), max_listed);
    if (rc != PCS_OK) return rc;
    report.n_pages = sum.n_pages;
    report.table_size = sum.table_size;
    report.n_mapped = sum.n_mapped;
    report.n_mapped_in_window = sum.n_mapped_in_window;
    report.n_duplicate = sum.n_duplicate;
    report.live_ok = sum.live_ok;
    report.live_blank = sum.live_blank;
    report.live_corrupt = sum.live_corrupt;
    report.dead_ok = sum.dead_ok;
    report.dead_blank = sum.dead_blank;
    report.dead_corrupt = sum.dead_corrupt;
    report.n_damaged = sum.n_damaged;
    report.first_damaged = sum.first_damaged;
    report.last_live = sum.last_live;
    report.damaged.resize(sum.n_listed);
    for (size_t k = 0; k < sum.n_listed; ++k) report.damaged[k] = LivePage{listed[k].index, listed[k].page_id, listed[k].cls};
    return PCS_OK;
}

LiveReport ScrubLive(std::span<const uint8_t> classes, uint64_t fp_first, std::span<const uint64_t> table,
                     size_t max_listed) {
    LiveReport report;
    if (int rc = TryScrubLive(classes, fp_first, table, report, max_listed)) die("ScrubLive", rc);
    return report;
}

static void fill_tree_report(const pcs_tree_summary& sum, TreeReport& report);

int TryCheckTree(std::span<const uint8_t> pages, size_t page_size, uint64_t fp_first,
                 std::span<const uint8_t> classes, std::span<const uint64_t> table, std::span<const uint64_t> roots,
                 TreeReport& report, size_t max_listed) {
    static_assert(sizeof(TreeNode) == sizeof(pcs_tree_node), "TreeNode mirrors pcs_tree_node");
    static_assert(sizeof(TreeProblem) == sizeof(pcs_tree_problem), "TreeProblem mirrors pcs_tree_problem");
    if (page_size == 0 || pages.size() % page_size) return PCS_ERR_INVALID;
    const uint64_t n_pages = pages.size() / page_size;
    if (!classes.empty() && classes.size() != n_pages) return PCS_ERR_INVALID;
    report.nodes.assign(table.size(), TreeNode{});
    report.problems.assign(max_listed, TreeProblem{});
    pcs_tree_summary sum{};
    const int rc = pcs_tree_check_host(pages.data(), page_size, n_pages, fp_first,
                                       classes.empty() ? nullptr : classes.data(), table.data(), table.size(),
                                       roots.data(), static_cast<uint32_t>(std::min<size_t>(roots.size(), UINT32_MAX)),
                                       reinterpret_cast<pcs_tree_node*>(report.nodes.data()), &sum,
                                       reinterpret_cast<pcs_tree_problem*>(report.problems.data()), max_listed);
    if (rc != PCS_OK) return rc;
    fill_tree_report(sum, report);
    report.problems.resize(sum.n_listed);
    return PCS_OK;
}

// the counters of a pcs_tree_summary into a TreeReport (problems and nodes are the caller's)
static void fill_tree_report(const pcs_tree_summary& sum, TreeReport& report) {
    report.n_pages = sum.n_pages;
    report.table_size = sum.table_size;
    report.n_mapped = sum.n_mapped;
    report.n_reached = sum.n_reached;
    report.n_nonleaf = sum.n_nonleaf;
    report.n_leaf_index = sum.n_leaf_index;
    report.n_data = sum.n_data;
    report.n_refs = sum.n_refs;
    report.n_extra_refs = sum.n_extra_refs;
    report.n_out_of_range_refs = sum.n_out_of_range_refs;
    report.max_depth = sum.max_depth;
    report.n_depth_capped = sum.n_depth_capped;
    for (int k = 0; k < 8; ++k) report.n_by_bit[k] = sum.n_by_bit[k];
    report.n_problems = sum.n_problems;
    report.first_problem = sum.first_problem;
    report.n_unreached_mapped = sum.n_unreached_mapped;
    for (int k = 0; k < 6; ++k) report.unreached_by_type[k] = sum.unreached_by_type[k];
    report.n_unreached_unread = sum.n_unreached_unread;
    report.n_chain_heads = sum.n_chain_heads;
}

TreeReport CheckTree(std::span<const uint8_t> pages, size_t page_size, uint64_t fp_first,
                     std::span<const uint8_t> classes, std::span<const uint64_t> table,
                     std::span<const uint64_t> roots, size_t max_listed) {
    TreeReport report;
    if (int rc = TryCheckTree(pages, page_size, fp_first, classes, table, roots, report, max_listed))
        die("CheckTree", rc);
    return report;
}

int TryCheckLeaves(std::span<const uint8_t> pages, size_t page_size, uint64_t fp_first,
                   std::span<const uint8_t> classes, std::span<const uint64_t> table, std::span<const uint64_t> roots,
                   LeafReport& report, size_t max_listed) {
    static_assert(sizeof(LeafNode) == sizeof(pcs_leaf_node), "LeafNode mirrors pcs_leaf_node");
    static_assert(sizeof(LeafProblem) == sizeof(pcs_leaf_problem), "LeafProblem mirrors pcs_leaf_problem");
    if (page_size == 0 || pages.size() % page_size) return PCS_ERR_INVALID;
    const uint64_t n_pages = pages.size() / page_size;
    if (!classes.empty() && classes.size() != n_pages) return PCS_ERR_INVALID;
    report.tree.nodes.assign(table.size(), TreeNode{});
    report.tree.problems.clear();
    report.leaves.assign(table.size(), LeafNode{});
    report.problems.assign(max_listed, LeafProblem{});
    pcs_tree_summary tsum{};
    pcs_leaf_summary sum{};
    const int rc = pcs_leaf_check_host(pages.data(), page_size, n_pages, fp_first,
                                       classes.empty() ? nullptr : classes.data(), table.data(), table.size(),
                                       roots.data(), static_cast<uint32_t>(std::min<size_t>(roots.size(), UINT32_MAX)),
                                       reinterpret_cast<pcs_tree_node*>(report.tree.nodes.data()), &tsum,
                                       reinterpret_cast<pcs_leaf_node*>(report.leaves.data()), &sum,
                                       reinterpret_cast<pcs_leaf_problem*>(report.problems.data()), max_listed);
    if (rc != PCS_OK) return rc;
    fill_tree_report(tsum, report.tree);
    // the tree's problems are its reached nodes with any bit set, ascending: all of them, from the nodes
    for (size_t p = 0; p < report.tree.nodes.size(); ++p) {
        const TreeNode& n = report.tree.nodes[p];
        if (n.parent != UINT32_MAX && n.bits)
            report.tree.problems.push_back(TreeProblem{static_cast<uint32_t>(p), n.parent, n.bits, n.depth});
    }
    report.n_pages = sum.n_pages;
    report.table_size = sum.table_size;
    report.n_data_pages = sum.n_data_pages;
    report.n_data_ok = sum.n_data_ok;
    report.n_entries = sum.n_entries;
    report.n_overflow_values = sum.n_overflow_values;
    report.n_expiring = sum.n_expiring;
    report.n_compressed = sum.n_compressed;
    report.inline_value_bytes = sum.inline_value_bytes;
    report.overflow_value_bytes = sum.overflow_value_bytes;
    report.n_refs = sum.n_refs;
    report.n_out_of_range_refs = sum.n_out_of_range_refs;
    report.n_extra_refs = sum.n_extra_refs;
    report.n_refs_to_tree = sum.n_refs_to_tree;
    report.n_misplaced_pointers = sum.n_misplaced_pointers;
    report.n_chain_capped = sum.n_chain_capped;
    report.max_groups = sum.max_groups;
    report.n_overflow_pages = sum.n_overflow_pages;
    for (int k = 0; k < 9; ++k) report.n_by_bit[k] = sum.n_by_bit[k];
    report.n_problems = sum.n_problems;
    report.first_problem = sum.first_problem;
    report.n_leaked_overflow = sum.n_leaked_overflow;
    report.n_overflow_ok = sum.n_overflow_ok;
    report.problems.resize(sum.n_listed);
    return PCS_OK;
}

LeafReport CheckLeaves(std::span<const uint8_t> pages, size_t page_size, uint64_t fp_first,
                       std::span<const uint8_t> classes, std::span<const uint64_t> table,
                       std::span<const uint64_t> roots, size_t max_listed) {
    LeafReport report;
    if (int rc = TryCheckLeaves(pages, page_size, fp_first, classes, table, roots, report, max_listed))
        die("CheckLeaves", rc);
    return report;
}

void RegisterPagePool(void* base, size_t bytes) {
    if (int rc = pcs_host_register(base, bytes)) die("RegisterPagePool", rc);
}

void UnregisterPagePool(void* base) {
    if (int rc = pcs_host_unregister(base)) die("UnregisterPagePool", rc);
}

void StartChecksumService(int workgroups, uint32_t idle_us, int lines) {
    if (int rc = pcs_service_start_ex(lines, workgroups, idle_us)) die("StartChecksumService", rc);
}

void StopChecksumService() {
    if (int rc = pcs_service_stop()) die("StopChecksumService", rc);
}

void PrepareChecksumThread() {
    if (int rc = pcs_thread_prepare()) die("PrepareChecksumThread", rc);
}

ChecksumBatch::ChecksumBatch() { status_ = pcs_batch_create(&batch_); }

ChecksumBatch::~ChecksumBatch() { pcs_batch_destroy(batch_); }

int ChecksumBatch::TrySubmitValidate(std::span<const char* const> pages, size_t page_size, PageHash hash,
                                     bool skip_verify) {
    if (status_) return status_;
    n_ = pages.size();
    validate_ = true;
    collected_ = false;
    ok_.assign(n_, 0);
    return pcs_batch_submit_ex(batch_, PCS_BATCH_VALIDATE, reinterpret_cast<const void* const*>(pages.data()),
                               page_size, n_, static_cast<int>(hash),
                               skip_verify ? PCS_FLAG_SKIP_VERIFY : PCS_FLAG_NONE);
}

int ChecksumBatch::TrySubmitStamp(std::span<char* const> pages, size_t page_size, PageHash hash) {
    if (status_) return status_;
    n_ = pages.size();
    validate_ = false;
    collected_ = false;
    return pcs_batch_submit(batch_, PCS_BATCH_STAMP, reinterpret_cast<const void* const*>(pages.data()), page_size,
                            n_, static_cast<int>(hash));
}

void ChecksumBatch::SubmitValidate(std::span<const char* const> pages, size_t page_size, PageHash hash,
                                   bool skip_verify) {
    if (int rc = TrySubmitValidate(pages, page_size, hash, skip_verify)) die("ChecksumBatch::SubmitValidate", rc);
}

void ChecksumBatch::SubmitStamp(std::span<char* const> pages, size_t page_size, PageHash hash) {
    if (int rc = TrySubmitStamp(pages, page_size, hash)) die("ChecksumBatch::SubmitStamp", rc);
}

int ChecksumBatch::Collect() {
    if (collected_) return PCS_OK;
    uint64_t fb = UINT64_MAX;
    if (int rc = pcs_batch_result(batch_, validate_ ? ok_.data() : nullptr, nullptr, &fb)) return rc;
    first_bad_ = fb == UINT64_MAX ? n_ : static_cast<size_t>(fb);
    collected_ = true;
    return PCS_OK;
}

int ChecksumBatch::Path() const { return batch_ ? pcs_batch_path(batch_) : 0; }

int ChecksumBatch::TryPoll() {
    if (status_) return status_;
    const int rc = pcs_batch_poll(batch_);
    if (rc == 1) {
        if (int c = Collect()) return c;
    }
    return rc;
}

bool ChecksumBatch::Poll() {
    const int rc = TryPoll();
    if (rc < 0) die("ChecksumBatch::Poll", rc);
    return rc == 1;
}

void ChecksumBatch::Wait() {
    if (status_) die("ChecksumBatch::Wait", status_);
    if (int rc = pcs_batch_wait(batch_)) die("ChecksumBatch::Wait", rc);
    if (int rc = Collect()) die("ChecksumBatch::Wait", rc);
}

uint64_t ManifestChecksum(std::string_view content) {
    uint64_t h = 0;
    if (int rc = pcs_manifest_checksum_host(content.data(), content.size(), &h)) die("ManifestChecksum", rc);
    return h;
}

bool ValidateManifestRecord(std::string_view record) {
    int valid = 0;
    if (int rc = pcs_manifest_validate_host(record.data(), record.size(), &valid)) die("ValidateManifestRecord", rc);
    return valid != 0;
}

}  // namespace eloqstore
