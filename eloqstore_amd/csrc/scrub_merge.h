// scrub_merge.h — host-side merge of per-chunk scrub results
// (pcs_pages_scrub_host, pcs_capi.cpp).  The host form scrubs a batch in
// 32 MiB chunks; each chunk comes back with a summary and a capped ascending
// list in chunk-local page indices.  Chunks are added in page order, so
// appending each chunk's list shifted by the chunk's first page keeps the
// global list ascending, and the first `cap` corrupt pages of the batch are
// exactly what the appends keep.  No HIP here: tests/cpp/scrub_merge_test.cpp
// drives this header alone under ASAN + UBSan.
#pragma once

#include <stdint.h>

#include "eloqstore_pcs.h"

namespace pcs {

class ScrubMerge {
public:
    // `list` (may be null iff cap == 0) receives the global list.
    ScrubMerge(pcs_scrub_summary* out, uint64_t* list, uint64_t cap) : out_(out), list_(list), cap_(cap) {
        *out_ = pcs_scrub_summary{};
        out_->first_corrupt = UINT64_MAX;
    }

    // How many list entries of a chunk can still matter: a chunk never needs
    // to list more than the room left in the global list.
    uint64_t room() const { return cap_ - out_->n_listed; }

    // Add the chunk that starts at global page `first_page`.  `chunk_list`
    // holds the chunk's c.n_listed smallest corrupt pages (chunk-local,
    // ascending); chunks must be added in ascending page order.
    void add(const pcs_scrub_summary& c, const uint64_t* chunk_list, uint64_t first_page) {
        out_->n_pages += c.n_pages;
        out_->n_ok += c.n_ok;
        out_->n_corrupt += c.n_corrupt;
        out_->n_blank += c.n_blank;
        for (int k = 0; k < 6; ++k) out_->ok_by_type[k] += c.ok_by_type[k];
        if (out_->first_corrupt == UINT64_MAX && c.first_corrupt != UINT64_MAX)
            out_->first_corrupt = first_page + c.first_corrupt;
        const uint64_t take = c.n_listed < room() ? c.n_listed : room();
        for (uint64_t i = 0; i < take; ++i) list_[out_->n_listed + i] = first_page + chunk_list[i];
        out_->n_listed += take;
    }

private:
    pcs_scrub_summary* out_;
    uint64_t* list_;
    uint64_t cap_;
};

}  // namespace pcs
