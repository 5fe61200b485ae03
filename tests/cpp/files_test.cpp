// files_test — eloqstore::TryScrubFiles / ScrubFiles (include/eloqstore/
// page_checksum.h), both overloads, on scattered host pages cut into data
// files, checked against a per-file loop over a classification made with the
// CPU oracle.  Needs a GPU; run by tests/test_gpu_files.py.
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

eloqstore::FileReport naive(const std::vector<uint8_t>& cls, const std::vector<const char*>& pages, uint64_t first,
                            uint64_t cnt) {
    eloqstore::FileReport r;
    r.first_page = first;
    r.n_pages = cnt;
    for (uint64_t i = 0; i < cnt; ++i) {
        const uint8_t c = cls[first + i], t = (uint8_t)pages[first + i][8];
        if (c == PCS_PAGE_OK) {
            ++r.n_ok;
            ++r.ok_by_type[t < 4 ? t : t == 255 ? 4 : 5];
        } else if (c == PCS_PAGE_CORRUPT) {
            ++r.n_corrupt;
            if (r.first_corrupt == UINT64_MAX) r.first_corrupt = i;
        } else {
            ++r.n_blank;
        }
        if (c != PCS_PAGE_BLANK) r.written_pages = i + 1;
    }
    for (uint64_t i = 0; i < r.written_pages; ++i) {
        if (cls[first + i] != PCS_PAGE_BLANK) continue;
        ++r.n_hole_pages;
        if (i == 0 || cls[first + i - 1] != PCS_PAGE_BLANK) {
            ++r.n_holes;
            if (r.first_hole == UINT64_MAX) r.first_hole = i;
        }
    }
    return r;
}

bool same(const eloqstore::FileReport& a, const eloqstore::FileReport& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

void check(const eloqstore::FilesReport& r, const std::vector<uint8_t>& cls, const std::vector<const char*>& pages,
           const std::vector<uint64_t>& first, size_t max_listed) {
    const size_t n_files = first.size() - 1;
    CHECK(r.files.size() == n_files);
    uint64_t corrupt_files = 0, hole_files = 0, unwritten = 0, first_bad = UINT64_MAX;
    std::vector<uint64_t> bad;
    for (size_t f = 0; f < n_files && f < r.files.size(); ++f) {
        const eloqstore::FileReport want = naive(cls, pages, first[f], first[f + 1] - first[f]);
        CHECK(same(r.files[f], want));
        corrupt_files += want.n_corrupt != 0;
        hole_files += want.n_holes != 0;
        unwritten += want.written_pages == 0;
        if (want.n_corrupt || want.n_holes) bad.push_back(f);
    }
    if (!bad.empty()) first_bad = bad[0];
    CHECK(r.n_pages == pages.size());
    CHECK(r.n_corrupt_files == corrupt_files && r.n_hole_files == hole_files && r.n_unwritten_files == unwritten);
    CHECK(r.n_bad_files == bad.size() && r.first_bad_file == first_bad);
    if (bad.size() > max_listed) bad.resize(max_listed);
    CHECK(r.bad_files == bad);
}

}  // namespace

int main() {
    constexpr size_t P = 4096, N = 301;
    std::vector<std::unique_ptr<char[]>> store;  // one allocation per page: scattered
    std::vector<const char*> pages;
    for (size_t i = 0; i < N; ++i) {
        store.emplace_back(new char[P]);
        char* p = store.back().get();
        for (size_t b = 0; b < P; ++b) p[b] = (char)((i * 131 + b * 7 + (b >> 8)) & 0xFF);
        p[8] = (char)(i % 5 == 4 ? 255 : i % 5);
        oracle_set_checksum(p, P);
        if (i >= 39 && i < 42) p[10] ^= 0x5A;             // a corrupt run across the boundary at 40
        if (i == 100) p[P - 1] ^= 1;
        if (i >= 76 && i < 84) std::memset(p, 0, P);      // blank across the boundary at 80: a tail and a hole
        if (i >= 120 && i < 160) std::memset(p, 0, P);    // a whole file unwritten
        if (i >= 250) std::memset(p, 0, P);               // the blank tail of the last files
        pages.push_back(p);
    }
    std::vector<uint8_t> cls(N);
    for (size_t i = 0; i < N; ++i) {
        bool zero = true;
        for (size_t b = 0; b < P && zero; ++b) zero = pages[i][b] == 0;
        cls[i] = oracle_validate_checksum(pages[i], P) ? PCS_PAGE_OK : zero ? PCS_PAGE_BLANK : PCS_PAGE_CORRUPT;
    }

    // equal-size files of 40 pages, the last one short
    eloqstore::FilesReport r;
    int rc = eloqstore::TryScrubFiles(pages, P, uint64_t{40}, r, 2);
    if (rc != PCS_OK) {
        std::fprintf(stderr, "TryScrubFiles failed (%d): %s\n", rc, eloqstore::LastChecksumError());
        return 1;
    }
    std::vector<uint64_t> even;
    for (uint64_t p = 0; p < N; p += 40) even.push_back(p);
    even.push_back(N);
    CHECK(even.size() == 9);
    check(r, cls, pages, even, 2);
    CHECK(r.files[0].first_corrupt == 39 && r.files[1].first_corrupt == 0 && r.files[1].n_corrupt == 2);
    CHECK(r.files[1].written_pages == 36 && r.files[1].n_holes == 0);    // blank up to its end: a tail
    CHECK(r.files[2].n_holes == 1 && r.files[2].first_hole == 0 && r.files[2].n_hole_pages == 4);
    CHECK(r.files[3].written_pages == 0 && r.files[7].n_pages == 21);
    CHECK(r.n_bad_files == 3 && r.bad_files.size() == 2 && r.bad_files[0] == 0 && r.bad_files[1] == 1);

    // explicit boundaries with empty files, the aborting form, default cap
    const std::vector<uint64_t> cut = {0, 0, 40, 40, 41, 80, 250, 250, N, N};
    const eloqstore::FilesReport all = eloqstore::ScrubFiles(pages, P, std::span<const uint64_t>(cut));
    check(all, cls, pages, cut, 1024);
    CHECK(all.files[0].n_pages == 0 && all.files[0].first_corrupt == UINT64_MAX && all.files[0].first_hole == UINT64_MAX);
    const eloqstore::FilesReport by40 = eloqstore::ScrubFiles(pages, P, uint64_t{40});
    check(by40, cls, pages, even, 1024);

    // no pages, no files; boundaries that do not cover the batch; a bad page size: refused, not aborted on
    const std::vector<uint64_t> zero = {0};
    const eloqstore::FilesReport none = eloqstore::ScrubFiles(std::span<const char* const>(), P, std::span<const uint64_t>(zero));
    CHECK(none.files.empty() && none.n_pages == 0 && none.n_bad_files == 0 && none.first_bad_file == UINT64_MAX);
    const std::vector<uint64_t> short_cut = {0, 40, 300}, back = {0, 50, 40, N};
    CHECK(eloqstore::TryScrubFiles(pages, P, std::span<const uint64_t>(short_cut), r) == PCS_ERR_INVALID);
    CHECK(eloqstore::TryScrubFiles(pages, P, std::span<const uint64_t>(back), r) == PCS_ERR_INVALID);
    CHECK(eloqstore::TryScrubFiles(pages, P, uint64_t{0}, r) == PCS_ERR_INVALID);
    CHECK(eloqstore::TryScrubFiles(pages, 128, uint64_t{40}, r) == PCS_ERR_INVALID);

    if (g_fail) {
        std::fprintf(stderr, "files_test: %d failures\n", g_fail);
        return 1;
    }
    std::printf("files_test ok\n");
    return 0;
}
