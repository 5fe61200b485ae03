// extents_test — eloqstore::TryScrubExtents / ScrubExtents (include/eloqstore/
// page_checksum.h) on scattered host pages, checked against runs taken from a
// classification made with the CPU oracle.  Needs a GPU; run by
// tests/test_gpu_extents.py.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "eloqstore/page_checksum.h"
#include "eloqstore_pcs.h"
#include "xxh_oracle.h"

namespace {

int g_fail = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                \
        }                                                            \
    } while (0)

}  // namespace

int main() {
    constexpr size_t P = 4096, N = 301, kRuns = 4;
    std::vector<std::unique_ptr<char[]>> store;  // one allocation per page: scattered
    std::vector<const char*> pages;
    for (size_t i = 0; i < N; ++i) {
        store.emplace_back(new char[P]);
        char* p = store.back().get();
        for (size_t b = 0; b < P; ++b) p[b] = (char)((i * 131 + b * 7 + (b >> 8)) & 0xFF);
        p[8] = (char)(i % 4);
        oracle_set_checksum(p, P);
        if (i >= 40 && i < 43) p[10] ^= 0x5A;             // a corrupt run of 3
        if (i == 100) p[P - 1] ^= 1;                      // a corrupt run of 1
        if (i == 0 || (i >= 70 && i < 75)) std::memset(p, 0, P);  // two holes
        if (i >= 250) std::memset(p, 0, P);               // the blank tail
        pages.push_back(p);
    }
    // expectation from the oracle
    std::vector<uint8_t> cls(N);
    uint64_t want_corrupt = 0, want_blank = 0;
    for (size_t i = 0; i < N; ++i) {
        bool zero = true;
        for (size_t b = 0; b < P && zero; ++b) zero = pages[i][b] == 0;
        cls[i] = oracle_validate_checksum(pages[i], P) ? PCS_PAGE_OK : zero ? PCS_PAGE_BLANK : PCS_PAGE_CORRUPT;
        want_corrupt += cls[i] == PCS_PAGE_CORRUPT;
        want_blank += cls[i] == PCS_PAGE_BLANK;
    }
    std::vector<eloqstore::PageExtent> want;
    for (size_t i = 0; i < N; ++i) {
        if (i == 0 || cls[i] != cls[i - 1]) want.push_back(eloqstore::PageExtent{i, 0, cls[i]});
        ++want.back().n_pages;
    }
    CHECK(want.size() == 9 && want_corrupt == 4);

    eloqstore::ExtentReport r;
    const int rc = eloqstore::TryScrubExtents(pages, P, r, kRuns, 2);
    if (rc != PCS_OK) {
        std::fprintf(stderr, "TryScrubExtents failed (%d): %s\n", rc, eloqstore::LastChecksumError());
        return 1;
    }
    CHECK(r.n_pages == N && r.n_corrupt == want_corrupt && r.n_blank == want_blank);
    CHECK(r.n_ok == N - want_corrupt - want_blank);
    CHECK(r.first_corrupt == 40 && r.corrupt.size() == 2 && r.corrupt[0] == 40 && r.corrupt[1] == 41);
    CHECK(r.n_runs == want.size() && r.runs.size() == kRuns);
    for (size_t i = 0; i < r.runs.size() && i < want.size(); ++i) {
        CHECK(r.runs[i].first_page == want[i].first_page);
        CHECK(r.runs[i].n_pages == want[i].n_pages);
        CHECK(r.runs[i].page_class == want[i].page_class);
    }
    CHECK(r.written_pages == 250 && r.n_blank_runs == 3 && r.first_blank == 0);
    CHECK(r.n_holes == 2 && r.n_hole_pages == 6 && r.first_hole == 0);

    // the aborting form, default caps: every run; an empty batch
    const eloqstore::ExtentReport all = eloqstore::ScrubExtents(pages, P);
    CHECK(all.runs.size() == want.size());
    uint64_t covered = 0;
    for (const auto& e : all.runs) covered += e.n_pages;
    CHECK(covered == N && all.corrupt.size() == want_corrupt);
    const eloqstore::ExtentReport none = eloqstore::ScrubExtents(std::span<const char* const>(), P);
    CHECK(none.n_pages == 0 && none.n_runs == 0 && none.runs.empty() && none.first_blank == UINT64_MAX &&
          none.first_hole == UINT64_MAX && none.written_pages == 0);
    // a page size off the XXH3 long path is refused, not aborted on
    CHECK(eloqstore::TryScrubExtents(pages, 128, r) == PCS_ERR_INVALID);

    if (g_fail) {
        std::fprintf(stderr, "extents_test: %d failures\n", g_fail);
        return 1;
    }
    std::printf("extents_test ok\n");
    return 0;
}
