// manifest_replay.h — host-side logic of the manifest replay and the
// liveness-aware scrub (pcs_manifest_replay_host and pcs_scrub_live_host in
// pcs_capi.cpp, page_checksum_tool --live): the argument rules, the carry of
// table rows across the staging groups of a host batch, the summary of whole
// reports, the data-file name rule and the tool's text and exit code.  No HIP
// here: tests/cpp/manifest_replay_logic_test.cpp drives this header alone
// under ASAN + UBSan.
#pragma once

#include <errno.h>
#include <stdint.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "eloqstore_pcs.h"
#include "manifest_scan.h"

namespace pcs {

constexpr uint64_t kReplayInvalidValue = 7;  // MappingSnapshot::InvalidValue

// ---- argument rules: nullptr when the arguments are acceptable ---------------
inline const char* replay_dev_args(const void* d_base, uint64_t total_bytes, const void* d_off, const void* d_size,
                                   uint64_t n_images, uint32_t align, const void* d_scan_reports,
                                   const void* d_reports, const void* d_summary, const void* d_table,
                                   uint64_t table_cap) {
    if (!d_summary) return "d_summary is null";
    if (!manifest_align_ok(align)) return "align must be a power of two in [64, 65536]";
    if (total_bytes && !d_base) return "d_base is null";
    if (reinterpret_cast<uintptr_t>(d_base) % 8) return "d_base is not 8-byte aligned";
    if (n_images && (!d_off || !d_size)) return "d_img_off / d_img_size is null";
    if (n_images && !d_reports) return "d_reports is null";
    if (reinterpret_cast<uintptr_t>(d_scan_reports) % 8 || reinterpret_cast<uintptr_t>(d_reports) % 8 ||
        reinterpret_cast<uintptr_t>(d_summary) % 8 || reinterpret_cast<uintptr_t>(d_table) % 8)
        return "an output array is not 8-byte aligned";
    if (table_cap && !d_table) return "d_table is null with table_cap > 0";
    if (table_cap >= (1ull << 60)) return "table_cap is too large";
    if (total_bytes >= (1ull << 32)) return "total_bytes must stay below 2^32";
    if (!manifest_batch_fits(total_bytes, n_images, align))
        return "total_bytes / align + n_images + total_bytes / 2^20 must stay below 2^31";
    return nullptr;
}

inline const char* replay_host_args(const void* const* images, const uint64_t* sizes, uint64_t n_images,
                                    uint32_t align, const void* reports, const void* summary, const void* table,
                                    uint64_t table_cap) {
    if (!summary) return "summary is null";
    if (!manifest_align_ok(align)) return "align must be a power of two in [64, 65536]";
    if (n_images && (!images || !sizes)) return "images / sizes is null";
    if (n_images && !reports) return "reports is null";
    if (table_cap && !table) return "table is null with table_cap > 0";
    if (table_cap >= (1ull << 60)) return "table_cap is too large";
    if (n_images >= (1ull << 31)) return "too many images";
    for (uint64_t i = 0; i < n_images; ++i) {
        if (sizes[i] && !images[i]) return "an image of non-zero size is null";
        if (sizes[i] + align >= (1ull << 32) || !manifest_batch_fits(sizes[i] + align, 1, align))
            return "an image is too large";
    }
    return nullptr;
}

inline const char* live_args(const void* cls, uint64_t n_pages, uint64_t fp_first, const void* table,
                             uint64_t table_size, const void* summary, const void* damaged, uint64_t damaged_cap) {
    if (!summary) return "summary is null";
    if (n_pages && !cls) return "class bytes are null";
    if (table_size && !table) return "table is null";
    if (table_size > 0xFFFFFFFFull) return "table_size must be at most 2^32 - 1";
    if (damaged_cap && !damaged) return "damaged list is null with damaged_cap > 0";
    if (n_pages >= (1ull << 43)) return "too many pages";
    if (fp_first + n_pages < fp_first || fp_first + n_pages > (1ull << 61)) return "the window leaves the file page ids";
    return nullptr;
}

// ---- the carry across the staging groups of a host batch --------------------
// The device form counts table_first from table_base and tests it against the
// absolute table_cap, so a group that starts at the rows of the groups before
// it reports exactly what one call over the whole batch would.
struct ReplayCarry {
    uint64_t rows = 0;  // sum of table_size over the OK and TABLE_CAP images so far
    // the rows of a group's reports move the base of the next group
    void add(const pcs_replay_report* reports, uint64_t n) {
        for (uint64_t i = 0; i < n; ++i)
            if (reports[i].status == PCS_REPLAY_OK || reports[i].status == PCS_REPLAY_TABLE_CAP)
                rows += reports[i].table_size;
    }
};

// Summary of n_images whole reports, as one device call over the batch writes it.
inline void replay_summarize(const pcs_replay_report* reports, uint64_t n_images, pcs_replay_summary* out) {
    *out = pcs_replay_summary{};
    out->n_images = n_images;
    out->first_bad_image = out->invalid_image = UINT64_MAX;
    for (uint64_t i = 0; i < n_images; ++i) {
        const pcs_replay_report& r = reports[i];
        if (r.status < 4) ++out->n_by_status[r.status];
        if (r.status == PCS_REPLAY_OK || r.status == PCS_REPLAY_TABLE_CAP) {
            out->n_rows += r.table_size;
            out->n_log_entries += r.n_log_entries;
        }
        if (r.status == PCS_REPLAY_OK) {
            out->n_rows_written += r.table_size;
            out->n_mapped += r.n_mapped;
        } else if (out->first_bad_image == UINT64_MAX) {
            out->first_bad_image = i;
        }
    }
}

inline const char* replay_status_name(uint64_t s) {
    switch (s) {
        case PCS_REPLAY_OK: return "ok";
        case PCS_REPLAY_NOT_REPLAYABLE: return "not-replayable";
        case PCS_REPLAY_MALFORMED: return "malformed";
        case PCS_REPLAY_TABLE_CAP: return "table-cap";
    }
    return "unknown";
}

// ---- page_checksum_tool --live -------------------------------------------------
// A data file's base name is data_<file_id>_<term>, both decimal
// (ParseDataFileSuffix, include/common.h); the legacy data_<id> does not parse.
inline bool live_parse_uint(const std::string& s, uint64_t& out) {
    if (s.empty()) return false;
    for (char c : s)
        if (c < '0' || c > '9') return false;
    errno = 0;
    char* end = nullptr;
    out = strtoull(s.c_str(), &end, 10);
    return errno == 0 && end == s.c_str() + s.size();
}
inline bool live_parse_data_file(const std::string& path, uint64_t& file_id, uint64_t& term) {
    const size_t slash = path.find_last_of('/');
    const std::string name = slash == std::string::npos ? path : path.substr(slash + 1);
    if (name.compare(0, 5, "data_") != 0) return false;
    const std::string suffix = name.substr(5);
    const size_t sep = suffix.find('_');
    if (sep == std::string::npos) return false;
    return live_parse_uint(suffix.substr(0, sep), file_id) && live_parse_uint(suffix.substr(sep + 1), term);
}

inline const char* live_class_name(uint32_t c) {
    return c == PCS_PAGE_CORRUPT ? "corrupt" : c == PCS_PAGE_OK ? "ok" : c == PCS_PAGE_BLANK ? "blank" : "other";
}

// one line when the manifest cannot be replayed (exit 2), empty when it can
inline std::string live_tool_refusal(const std::string& path, const pcs_replay_report& r) {
    if (r.status == PCS_REPLAY_OK) return std::string();
    std::string why = replay_status_name(r.status);
    if (r.status == PCS_REPLAY_MALFORMED) why += " at record " + std::to_string(r.malformed_record);
    return path + ": manifest cannot be replayed: " + why + "\n";
}
inline std::string live_tool_file_line(const std::string& path, uint64_t file_id, const pcs_live_summary& s) {
    return path + ": file " + std::to_string(file_id) + " pages " + std::to_string(s.n_pages) + " live ok " +
           std::to_string(s.live_ok) + " blank " + std::to_string(s.live_blank) + " corrupt " +
           std::to_string(s.live_corrupt) + " dead ok " + std::to_string(s.dead_ok) + " blank " +
           std::to_string(s.dead_blank) + " corrupt " + std::to_string(s.dead_corrupt) + "\n";
}
inline std::string live_tool_page_line(uint64_t fp_first, const pcs_live_page& p) {
    return "  damaged: page_id " + std::to_string(p.page_id) + " file_page " + std::to_string(fp_first + p.index) +
           " class " + live_class_name(p.cls) + "\n";
}
inline std::string live_tool_footer(const pcs_replay_report& r, uint64_t mapped_in_given_files) {
    // the caller gives every file id once, so the difference cannot be negative; clamped all the same
    const uint64_t elsewhere = r.n_mapped > mapped_in_given_files ? r.n_mapped - mapped_in_given_files : 0;
    return "root " + std::to_string(r.root) + " ttl_root " + std::to_string(r.ttl_root) + " max_fp_id " +
           std::to_string(r.max_fp_id) + " mapped " + std::to_string(r.n_mapped) + " mapped_in_files_not_given " +
           std::to_string(elsewhere) + "\n";
}
// 2 when any live page is corrupt, else 3 when any live page is blank, else 0;
// dead damage never fails the run.
inline int live_tool_exit(const pcs_live_summary* files, uint64_t n) {
    bool corrupt = false, blank = false;
    for (uint64_t i = 0; i < n; ++i) {
        corrupt = corrupt || files[i].live_corrupt;
        blank = blank || files[i].live_blank;
    }
    return corrupt ? 2 : blank ? 3 : 0;
}

}  // namespace pcs
