// scrub_test — eloqstore::TryScrubPages / ScrubPages (include/eloqstore/
// page_checksum.h) on scattered host pages, checked against a classification
// made with the CPU oracle.  Needs a GPU; run by tests/test_gpu_scrub.py.
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

int bucket(uint8_t t) { return t < 4 ? t : t == 255 ? 4 : 5; }

}  // namespace

int main() {
    constexpr size_t P = 4096, N = 301, kCap = 5;
    const uint8_t types[6] = {0, 1, 2, 3, 255, 9};
    std::vector<std::unique_ptr<char[]>> store;  // one allocation per page: scattered
    std::vector<const char*> pages;
    for (size_t i = 0; i < N; ++i) {
        store.emplace_back(new char[P]);
        char* p = store.back().get();
        for (size_t b = 0; b < P; ++b) p[b] = (char)((i * 131 + b * 7 + (b >> 8)) & 0xFF);
        p[8] = (char)types[i % 6];
        oracle_set_checksum(p, P);
        if (i % 23 == 4) p[10] ^= 0x5A;               // corrupt
        if (i % 17 == 0 || i == N - 1) std::memset(p, 0, P);  // blank
        if (i == 50) {                                 // near-blank: one byte set, zero header
            std::memset(p, 0, P);
            p[P - 1] = 1;
        }
        if (i == 60) {                                 // zero body under its correct header: ok, type 0
            std::memset(p, 0, P);
            oracle_set_checksum(p, P);
        }
        pages.push_back(p);
    }
    // expectation from the oracle
    uint64_t want_ok = 0, want_corrupt = 0, want_blank = 0, want_type[6] = {};
    std::vector<uint64_t> want_list;
    std::vector<uint8_t> want_cls(N);
    for (size_t i = 0; i < N; ++i) {
        bool zero = true;
        for (size_t b = 0; b < P && zero; ++b) zero = pages[i][b] == 0;
        if (oracle_validate_checksum(pages[i], P)) {
            want_cls[i] = PCS_PAGE_OK;
            ++want_ok;
            ++want_type[bucket((uint8_t)pages[i][8])];
        } else if (zero) {
            want_cls[i] = PCS_PAGE_BLANK;
            ++want_blank;
        } else {
            want_cls[i] = PCS_PAGE_CORRUPT;
            ++want_corrupt;
            want_list.push_back(i);
        }
    }
    CHECK(want_ok && want_blank && want_corrupt > kCap);

    eloqstore::ScrubReport r;
    const int rc = eloqstore::TryScrubPages(pages, P, r, kCap);
    if (rc != PCS_OK) {
        std::fprintf(stderr, "TryScrubPages failed (%d): %s\n", rc, eloqstore::LastChecksumError());
        return 1;
    }
    CHECK(r.n_pages == N);
    CHECK(r.n_ok == want_ok);
    CHECK(r.n_corrupt == want_corrupt);
    CHECK(r.n_blank == want_blank);
    for (int k = 0; k < 6; ++k) CHECK(r.ok_by_type[k] == want_type[k]);
    CHECK(r.first_corrupt == want_list[0]);
    CHECK(r.corrupt.size() == kCap);
    for (size_t i = 0; i < r.corrupt.size() && i < kCap; ++i) CHECK(r.corrupt[i] == want_list[i]);
    CHECK(r.page_class == want_cls);
    for (size_t i = 0; i < N; ++i) CHECK(r.page_type[i] == (uint8_t)pages[i][8]);

    // the aborting form, default cap: the whole list; an empty batch
    const eloqstore::ScrubReport all = eloqstore::ScrubPages(pages, P);
    CHECK(all.corrupt == want_list);
    CHECK(all.n_corrupt == want_corrupt);
    const eloqstore::ScrubReport none = eloqstore::ScrubPages(std::span<const char* const>(), P);
    CHECK(none.n_pages == 0 && none.n_corrupt == 0 && none.first_corrupt == UINT64_MAX && none.corrupt.empty());
    // a page size off the XXH3 long path is refused, not aborted on
    CHECK(eloqstore::TryScrubPages(pages, 128, r) == PCS_ERR_INVALID);

    if (g_fail) {
        std::fprintf(stderr, "scrub_test: %d failures\n", g_fail);
        return 1;
    }
    std::printf("scrub_test ok\n");
    return 0;
}
