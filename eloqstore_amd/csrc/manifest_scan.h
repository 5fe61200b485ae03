// manifest_scan.h — host-side logic of the manifest scan
// (pcs_manifest_scan_host in pcs_capi.cpp, page_checksum_tool
// --check-manifest): the argument rules, the plan that packs whole images
// into staging groups at multiples of `align`, the verdict that follows from
// a record's ok flags, the summary of whole reports, and the text and exit
// codes of the reference's tools/manifest_check_tool.cpp.  No HIP here:
// tests/cpp/manifest_scan_logic_test.cpp drives this header alone under
// ASAN + UBSan.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "eloqstore_pcs.h"

namespace pcs {

constexpr uint64_t kManifestHeaderBytes = 20;         // checksum(8) root(4) ttl_root(4) payload_len(4)
constexpr uint64_t kManifestStageBytes = 32ull << 20;  // packed images per staging group

inline bool manifest_align_ok(uint32_t align) { return align >= 64 && align <= 65536 && (align & (align - 1)) == 0; }
inline uint64_t manifest_round_up(uint64_t v, uint32_t align) { return (v + (align - 1)) & ~(uint64_t)(align - 1); }

// The scan's scratch indices are 32-bit: slots <= total / align + n_images,
// chunks <= slots + total / 2^20.
inline bool manifest_batch_fits(uint64_t total_bytes, uint64_t n_images, uint32_t align) {
    if (total_bytes >= (1ull << 62) || n_images >= (1ull << 31)) return false;
    return total_bytes / align + n_images + (total_bytes >> 20) <= 0x7FFFFFF0ull;
}

// One staging group: images [first, first + count) packed at off[k] (multiples
// of align, ascending) into `bytes` bytes.
struct ManifestGroup {
    uint64_t first = 0, count = 0, bytes = 0;
    std::vector<uint64_t> off;
};

// Whole images in order, a new group whenever the next image would carry the
// group past `budget`; an image above the budget is a group of its own.  Every
// image is in exactly one group; empty images travel with their neighbours.
inline std::vector<ManifestGroup> manifest_pack(const uint64_t* sizes, uint64_t n_images, uint32_t align,
                                                uint64_t budget = kManifestStageBytes) {
    std::vector<ManifestGroup> groups;
    ManifestGroup g;
    for (uint64_t i = 0; i < n_images; ++i) {
        const uint64_t need = manifest_round_up(sizes[i], align);
        if (g.count && g.bytes + need > budget) {
            groups.push_back(std::move(g));
            g = ManifestGroup{};
            g.first = i;
        }
        g.off.push_back(g.bytes);
        g.bytes += need;
        ++g.count;
    }
    if (g.count) groups.push_back(std::move(g));
    return groups;
}

// The report fields that follow from the ok flags of an image's n records, in
// walk order.
struct ManifestFlagsResult {
    uint64_t n_ok = 0, n_corrupt = 0, first_corrupt = UINT64_MAX, n_ok_after_corrupt = 0;
    uint64_t verdict = PCS_MANIFEST_EMPTY;
};
inline ManifestFlagsResult manifest_verdict(const uint8_t* ok, uint64_t n) {
    ManifestFlagsResult r;
    for (uint64_t k = 0; k < n; ++k) {
        if (ok[k]) {
            ++r.n_ok;
            if (r.first_corrupt != UINT64_MAX) ++r.n_ok_after_corrupt;
        } else {
            ++r.n_corrupt;
            if (r.first_corrupt == UINT64_MAX) r.first_corrupt = k;
        }
    }
    r.verdict = n == 0                          ? PCS_MANIFEST_EMPTY
                : r.first_corrupt == 0          ? PCS_MANIFEST_BAD_SNAPSHOT
                : r.first_corrupt == UINT64_MAX ? PCS_MANIFEST_CLEAN
                : r.n_ok_after_corrupt          ? PCS_MANIFEST_BROKEN
                                                : PCS_MANIFEST_TORN_TAIL;
    return r;
}

inline const char* manifest_verdict_name(uint64_t v) {
    switch (v) {
        case PCS_MANIFEST_CLEAN: return "clean";
        case PCS_MANIFEST_TORN_TAIL: return "torn-tail";
        case PCS_MANIFEST_BROKEN: return "broken";
        case PCS_MANIFEST_BAD_SNAPSHOT: return "bad-snapshot";
        case PCS_MANIFEST_EMPTY: return "empty";
    }
    return "unknown";
}

// Summary of n_images whole reports, as one device call over the batch writes
// it.  Sets every report's first_record to the exclusive sum of n_records.
inline void manifest_summarize(pcs_manifest_report* reports, uint64_t n_images, uint64_t record_cap,
                               pcs_manifest_summary* out) {
    *out = pcs_manifest_summary{};
    out->n_images = n_images;
    out->first_bad_image = out->invalid_image = UINT64_MAX;
    for (uint64_t i = 0; i < n_images; ++i) {
        pcs_manifest_report& r = reports[i];
        r.first_record = out->n_records;
        out->n_records += r.n_records;
        out->n_ok += r.n_ok;
        out->n_corrupt += r.n_corrupt;
        if (r.verdict < 5) ++out->n_by_verdict[r.verdict];
        if (r.verdict != PCS_MANIFEST_CLEAN && out->first_bad_image == UINT64_MAX) out->first_bad_image = i;
    }
    out->n_listed = out->n_records < record_cap ? out->n_records : record_cap;
}

// ---- tools/manifest_check_tool.cpp's output for one file --------------------
// `image` is the file's bytes, `recs` its report.n_records records.  The tool
// prints each record, then stops with 1 and a message on a truncated header or
// payload or when it found no record, and otherwise exits 2 when any checksum
// failed and 0 when none did.  It seeks over padding, so padding cut by the
// end of the file is not an error there.
struct ManifestToolText {
    std::string out, err;
    int exit_code = 0;
};
inline ManifestToolText manifest_tool_text(const std::string& path, const uint8_t* image,
                                           const pcs_manifest_report& rep, const pcs_manifest_record* recs) {
    static const char kHex[] = "0123456789abcdef";
    ManifestToolText t;
    bool failed = false;
    for (uint64_t k = 0; k < rep.n_records; ++k) {
        const pcs_manifest_record& r = recs[k];
        t.out += "Log #" + std::to_string(k) + " at offset " + std::to_string(r.offset) + "\n";
        t.out += "  record size: " + std::to_string(kManifestHeaderBytes + r.payload_len) + "\n";
        t.out += "  root: " + std::to_string(r.root) + "\n";
        t.out += "  ttl_root: " + std::to_string(r.ttl_root) + "\n";
        t.out += "  payload_bytes: " + std::to_string(r.payload_len) + "\n";
        t.out += std::string("  checksum: ") + (r.ok ? "OK" : "FAILED") + "\n";
        if (!r.ok) {
            failed = true;
            std::string hex;
            hex.reserve(2 * (size_t)r.payload_len);
            const uint8_t* p = image + r.offset + kManifestHeaderBytes;
            for (uint32_t b = 0; b < r.payload_len; ++b) {
                hex.push_back(kHex[p[b] >> 4]);
                hex.push_back(kHex[p[b] & 0xF]);
            }
            t.out += "  payload_hex: " + hex + "\n";
        }
    }
    if (rep.end_reason == PCS_MANIFEST_END_SHORT_HEADER) {
        t.err = "Manifest truncated while reading header at offset " + std::to_string(rep.end_offset) + "\n";
        t.exit_code = 1;
    } else if (rep.end_reason == PCS_MANIFEST_END_SHORT_PAYLOAD) {
        t.err = "Manifest truncated while reading payload at offset " +
                std::to_string(rep.end_offset + kManifestHeaderBytes) + "\n";
        t.exit_code = 1;
    } else if (rep.n_records == 0) {
        t.err = "No manifest logs found in " + path + "\n";
        t.exit_code = 1;
    } else {
        t.out += "Parsed " + std::to_string(rep.n_records) + " logs from " + path + "\n";
        t.exit_code = failed ? 2 : 0;
    }
    return t;
}

// ---- several files: one line per file and the worst verdict's exit code ----
inline std::string manifest_tool_line(const std::string& path, const pcs_manifest_report& rep) {
    return path + ": records " + std::to_string(rep.n_records) + " corrupt " + std::to_string(rep.n_corrupt) +
           " verdict " + manifest_verdict_name(rep.verdict) + " valid_prefix_bytes " +
           std::to_string(rep.valid_prefix_bytes) + "\n";
}
// 2 when any verdict is BROKEN or BAD_SNAPSHOT, else 3 when any is TORN_TAIL,
// else 1 when any is EMPTY or a file could not be read, else 0.
inline int manifest_tool_exit(const pcs_manifest_report* reports, uint64_t n, bool any_unreadable) {
    bool fatal = false, torn = false, empty = any_unreadable;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t v = reports[i].verdict;
        fatal = fatal || v == PCS_MANIFEST_BROKEN || v == PCS_MANIFEST_BAD_SNAPSHOT;
        torn = torn || v == PCS_MANIFEST_TORN_TAIL;
        empty = empty || v == PCS_MANIFEST_EMPTY;
    }
    return fatal ? 2 : torn ? 3 : empty ? 1 : 0;
}

}  // namespace pcs
