// scrub_merge_test — pcs::ScrubMerge (eloqstore_amd/csrc/scrub_merge.h) fed
// with synthetic per-chunk scrub results and checked against a direct count
// over the same synthetic classes.  No HIP: built with ASAN + UBSan
// (eloqstore_amd/Makefile `sanitize`) and run by tests/test_scrub_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scrub_merge.h"

namespace {

int g_fail = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                \
        }                                                            \
    } while (0)

uint64_t rnd(uint64_t& s) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int bucket(uint8_t t) { return t < 4 ? t : t == 255 ? 4 : 5; }

// What one device chunk reports for pages [first, first + cnt): exact-size
// buffers, so an overrun of either list is an ASAN report.
void chunk_result(const std::vector<uint8_t>& cls, const std::vector<uint8_t>& type, uint64_t first, uint64_t cnt,
                  uint64_t chunk_cap, pcs_scrub_summary& s, std::vector<uint64_t>& list) {
    s = pcs_scrub_summary{};
    s.first_corrupt = UINT64_MAX;
    s.n_pages = cnt;
    list.clear();
    for (uint64_t i = 0; i < cnt; ++i) {
        const uint8_t c = cls[first + i];
        if (c == PCS_PAGE_OK) {
            ++s.n_ok;
            ++s.ok_by_type[bucket(type[first + i])];
        } else if (c == PCS_PAGE_BLANK) {
            ++s.n_blank;
        } else {
            ++s.n_corrupt;
            if (s.first_corrupt == UINT64_MAX) s.first_corrupt = i;
            if (list.size() < chunk_cap) list.push_back(i);
        }
    }
    s.n_listed = list.size();
    list.shrink_to_fit();
}

void run_case(uint64_t n, uint64_t chunk, uint64_t cap, unsigned corrupt_per_1024, uint64_t seed) {
    std::vector<uint8_t> cls(n), type(n);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t r = rnd(seed);
        cls[i] = (r & 1023) < corrupt_per_1024 ? PCS_PAGE_CORRUPT : ((r >> 10) & 7) == 0 ? PCS_PAGE_BLANK : PCS_PAGE_OK;
        const uint8_t types[8] = {0, 1, 2, 3, 255, 7, 2, 2};
        type[i] = types[(r >> 20) & 7];
    }
    pcs_scrub_summary want;
    std::vector<uint64_t> want_list;
    chunk_result(cls, type, 0, n, cap, want, want_list);

    pcs_scrub_summary got;
    got.n_pages = 0xDEAD;  // the merge overwrites whatever the summary held
    std::vector<uint64_t> got_list(cap, 0xABABABABABABABABull);
    got_list.shrink_to_fit();
    pcs::ScrubMerge merge(&got, cap ? got_list.data() : nullptr, cap);
    for (uint64_t first = 0; first < n; first += chunk) {
        const uint64_t cnt = n - first < chunk ? n - first : chunk;
        pcs_scrub_summary c;
        std::vector<uint64_t> clist;
        chunk_result(cls, type, first, cnt, cap < cnt ? cap : cnt, c, clist);
        merge.add(c, clist.data(), first);
    }
    CHECK(got.n_pages == n);
    CHECK(got.n_ok == want.n_ok);
    CHECK(got.n_corrupt == want.n_corrupt);
    CHECK(got.n_blank == want.n_blank);
    for (int k = 0; k < 6; ++k) CHECK(got.ok_by_type[k] == want.ok_by_type[k]);
    CHECK(got.first_corrupt == want.first_corrupt);
    CHECK(got.n_listed == want.n_listed);
    CHECK(got.n_listed == (want.n_corrupt < cap ? want.n_corrupt : cap));
    for (uint64_t i = 0; i < got.n_listed; ++i) CHECK(got_list[i] == want_list[i]);
    for (uint64_t i = got.n_listed; i < cap; ++i) CHECK(got_list[i] == 0xABABABABABABABABull);
}

}  // namespace

int main() {
    run_case(0, 8192, 16, 10, 1);          // no chunk at all: zero counts, first_corrupt = UINT64_MAX
    run_case(9000, 8192, 5, 3, 2);         // cap reached inside the first chunk
    run_case(9000, 8192, 1024, 8, 3);      // list spans the chunk boundary, cap not reached
    run_case(30000, 8192, 100, 10, 4);     // cap reached in a later chunk
    run_case(30000, 8192, 0, 10, 5);       // cap 0, null list
    run_case(30000, 8192, 40000, 1024, 6); // every page corrupt, cap above the page count
    run_case(5000, 512, 7, 0, 7);          // nothing corrupt
    run_case(777, 1, 50, 300, 8);          // one page per chunk
    if (g_fail) {
        std::fprintf(stderr, "scrub_merge_test: %d failures\n", g_fail);
        return 1;
    }
    std::printf("scrub_merge_test ok\n");
    return 0;
}
