// extent_merge.h — host-side merge of per-chunk scrub extents
// (pcs_pages_scrub_extents_host in pcs_capi.cpp, page_checksum_tool
// --extents).  Each chunk comes back with a pcs_extent_summary and a capped
// ascending run list in chunk-local page indices; chunks are added in page
// order.  A chunk whose first class equals the previous chunk's last class
// continues that run: the run is extended (in the list too, when it is
// listed, however full the list is) and counted once.  The hole fields are
// not summed: a chunk's blank tail is a hole as soon as a later chunk holds a
// non-blank page, so they are derived again from the merged written_pages,
// n_blank, n_blank_runs, first_blank and last_class after every chunk.  The
// result for any chunking equals one pass over the whole class array.  No HIP
// here: tests/cpp/extent_merge_test.cpp drives this header alone under ASAN +
// UBSan.
#pragma once

#include <stdint.h>

#include "eloqstore_pcs.h"

namespace pcs {

class ExtentMerge {
public:
    // `runs` (may be null iff cap == 0) receives the global list.
    ExtentMerge(pcs_extent_summary* out, pcs_extent* runs, uint64_t cap) : out_(out), runs_(runs), cap_(cap) {
        *out_ = pcs_extent_summary{};
        out_->first_blank = out_->first_hole = out_->first_class = out_->last_class = UINT64_MAX;
    }

    // How many runs to ask of a chunk of `chunk_pages` pages: one more than
    // the global cap, since the chunk's first run may only extend a run that
    // is already listed; nothing when no run is listed at all.
    static uint64_t chunk_cap(uint64_t cap, uint64_t chunk_pages) {
        if (cap == 0 || chunk_pages == 0) return 0;
        return (cap < chunk_pages ? cap : chunk_pages - 1) + 1;
    }

    // Add the chunk that starts at global page `first_page`.  `chunk_runs`
    // holds the chunk's first c.n_listed runs (chunk-local, ascending, each
    // with its full length inside the chunk), listed with a cap of at least
    // chunk_cap(cap, c.n_pages); chunks must be added in ascending page order.
    void add(const pcs_extent_summary& c, const pcs_extent* chunk_runs, uint64_t first_page) {
        if (c.n_pages == 0) return;
        pcs_extent_summary& o = *out_;
        const bool joint = o.n_pages != 0 && c.first_class == o.last_class;
        uint64_t j = 0;
        if (joint) {
            // the open run is global run n_runs - 1: listed iff n_runs <= cap
            if (o.n_runs <= cap_) runs_[o.n_runs - 1].n_pages += chunk_runs[0].n_pages;
            j = 1;
        }
        // the chunk's next run is global run n_runs, at that place in the list
        uint64_t at = o.n_runs;
        for (; j < c.n_listed && at < cap_; ++j, ++at) {
            runs_[at] = chunk_runs[j];
            runs_[at].first_page += first_page;
        }
        if (o.n_pages == 0) o.first_class = c.first_class;
        o.last_class = c.last_class;
        o.n_runs += c.n_runs - (joint ? 1 : 0);
        o.n_listed = o.n_runs < cap_ ? o.n_runs : cap_;
        o.n_blank += c.n_blank;
        o.n_blank_runs += c.n_blank_runs - (joint && c.first_class == PCS_PAGE_BLANK ? 1 : 0);
        if (o.first_blank == UINT64_MAX && c.first_blank != UINT64_MAX) o.first_blank = first_page + c.first_blank;
        if (c.written_pages) o.written_pages = first_page + c.written_pages;
        o.n_pages += c.n_pages;
        // every blank run but the tail (the one that starts at written_pages) is a hole
        o.n_holes = o.n_blank_runs - (o.last_class == PCS_PAGE_BLANK ? 1 : 0);
        o.n_hole_pages = o.n_blank - (o.n_pages - o.written_pages);
        o.first_hole = o.n_holes ? o.first_blank : UINT64_MAX;
    }

private:
    pcs_extent_summary* out_;
    pcs_extent* runs_;
    uint64_t cap_;
};

}  // namespace pcs
