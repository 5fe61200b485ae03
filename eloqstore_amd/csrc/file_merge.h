// file_merge.h — host-side merge of per-file scrub reports
// (pcs_pages_scrub_files_host in pcs_capi.cpp, page_checksum_tool
// --scrub-files).  A data file that crosses a chunk edge comes back as one
// pcs_file_report per part; the parts are added in page order.  Counts add;
// first_corrupt, first_hole and written_pages shift by the part's offset
// inside the file.  The hole fields are not summed: one part's blank tail is a
// hole as soon as a later part holds a non-blank page, and two parts that meet
// blank-to-blank share one blank run, so they are derived again after every
// part.  The 16-word report carries all that this needs:
//   ends blank     written_pages < n_pages
//   blank runs     n_holes + (ends blank)
//   first blank    first_hole when there is a hole, else written_pages when
//                  the report ends blank, else none
//   starts blank   first blank == 0
// The result for any cut equals one pass over the file.  files_summarize
// builds the totals and the capped list of bad files from whole reports.  No
// HIP here: tests/cpp/file_merge_test.cpp drives this header alone under
// ASAN + UBSan.
#pragma once

#include <stdint.h>

#include "eloqstore_pcs.h"

namespace pcs {

class FileMerge {
public:
    // A file of no pages yet that starts at batch page `first_page`.
    static pcs_file_report empty(uint64_t first_page) {
        pcs_file_report r{};
        r.first_page = first_page;
        r.first_corrupt = r.first_hole = UINT64_MAX;
        return r;
    }
    static bool ends_blank(const pcs_file_report& r) { return r.written_pages < r.n_pages; }
    static uint64_t blank_runs(const pcs_file_report& r) { return r.n_holes + (ends_blank(r) ? 1 : 0); }
    static uint64_t first_blank(const pcs_file_report& r) {
        return r.n_holes ? r.first_hole : ends_blank(r) ? r.written_pages : UINT64_MAX;
    }

    // Add the part that follows the o.n_pages pages merged so far; the part's
    // first_page is ignored.
    static void add(pcs_file_report& o, const pcs_file_report& c) {
        if (c.n_pages == 0) return;
        const uint64_t off = o.n_pages;
        const bool joint = off != 0 && ends_blank(o) && first_blank(c) == 0;
        const uint64_t runs = blank_runs(o) + blank_runs(c) - (joint ? 1 : 0);
        uint64_t first = first_blank(o);
        if (first == UINT64_MAX && first_blank(c) != UINT64_MAX) first = off + first_blank(c);
        o.n_ok += c.n_ok;
        o.n_corrupt += c.n_corrupt;
        o.n_blank += c.n_blank;
        for (int k = 0; k < 6; ++k) o.ok_by_type[k] += c.ok_by_type[k];
        if (o.first_corrupt == UINT64_MAX && c.first_corrupt != UINT64_MAX) o.first_corrupt = off + c.first_corrupt;
        if (c.written_pages) o.written_pages = off + c.written_pages;
        o.n_pages = off + c.n_pages;
        // every blank run but the tail (the one that starts at written_pages) is a hole
        o.n_holes = runs - (ends_blank(o) ? 1 : 0);
        o.n_hole_pages = o.n_blank - (o.n_pages - o.written_pages);
        o.first_hole = o.n_holes ? first : UINT64_MAX;
    }
};

// Totals of n_files whole reports and the min(n_bad_files, cap) smallest bad
// file indices, ascending, into `bad` (may be null iff cap == 0).
inline void files_summarize(const pcs_file_report* reports, uint64_t n_files, pcs_files_summary* out, uint64_t* bad,
                            uint64_t cap) {
    *out = pcs_files_summary{};
    out->n_files = n_files;
    out->first_bad_file = out->invalid_file = UINT64_MAX;
    for (uint64_t f = 0; f < n_files; ++f) {
        const pcs_file_report& r = reports[f];
        out->n_pages += r.n_pages;
        out->n_ok += r.n_ok;
        out->n_corrupt += r.n_corrupt;
        out->n_blank += r.n_blank;
        out->n_corrupt_files += r.n_corrupt ? 1 : 0;
        out->n_hole_files += r.n_holes ? 1 : 0;
        out->n_unwritten_files += r.written_pages ? 0 : 1;
        if (r.n_corrupt || r.n_holes) {
            if (out->first_bad_file == UINT64_MAX) out->first_bad_file = f;
            if (out->n_listed < cap) bad[out->n_listed++] = f;
            ++out->n_bad_files;
        }
    }
}

}  // namespace pcs
