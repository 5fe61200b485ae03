// extent_merge_test — pcs::ExtentMerge (eloqstore_amd/csrc/extent_merge.h)
// fed with per-chunk extents of synthetic class arrays, built by a naive loop,
// and checked against the same loop over the whole array.  No HIP: built with
// ASAN + UBSan (eloqstore_amd/Makefile `sanitize`) and run by
// tests/test_extents_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "extent_merge.h"

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

constexpr uint64_t kGarbage = 0xABABABABABABABABull;

// What the device reports for the class bytes [first, first + cnt) with a
// list cap of `cap`, by the definitions of include/eloqstore_pcs.h; the list
// is an exact-size buffer, so an overrun of it is an ASAN report.
void naive(const std::vector<uint8_t>& cls, uint64_t first, uint64_t cnt, uint64_t cap, pcs_extent_summary& s,
           std::vector<pcs_extent>& runs) {
    s = pcs_extent_summary{};
    s.first_blank = s.first_hole = s.first_class = s.last_class = UINT64_MAX;
    s.n_pages = cnt;
    std::vector<pcs_extent> all;
    for (uint64_t i = 0; i < cnt; ++i) {
        const uint8_t c = cls[first + i];
        if (i == 0 || c != cls[first + i - 1]) all.push_back(pcs_extent{i, 0, c, 0});
        ++all.back().n_pages;
        if (c == PCS_PAGE_BLANK) {
            ++s.n_blank;
            if (s.first_blank == UINT64_MAX) s.first_blank = i;
        } else {
            s.written_pages = i + 1;
        }
    }
    for (const pcs_extent& r : all) {
        if (r.cls != PCS_PAGE_BLANK) continue;
        ++s.n_blank_runs;
        if (r.first_page < s.written_pages) {
            ++s.n_holes;
            s.n_hole_pages += r.n_pages;
            if (s.first_hole == UINT64_MAX) s.first_hole = r.first_page;
        }
    }
    s.n_runs = all.size();
    s.n_listed = s.n_runs < cap ? s.n_runs : cap;
    if (cnt) {
        s.first_class = cls[first];
        s.last_class = cls[first + cnt - 1];
    }
    runs.assign(all.begin(), all.begin() + (long)s.n_listed);
    runs.shrink_to_fit();
}

bool same(const pcs_extent_summary& a, const pcs_extent_summary& b) {
    return a.n_pages == b.n_pages && a.n_runs == b.n_runs && a.n_listed == b.n_listed &&
           a.written_pages == b.written_pages && a.n_blank == b.n_blank && a.n_blank_runs == b.n_blank_runs &&
           a.first_blank == b.first_blank && a.n_holes == b.n_holes && a.n_hole_pages == b.n_hole_pages &&
           a.first_hole == b.first_hole && a.first_class == b.first_class && a.last_class == b.last_class;
}

// Merge `cls` cut at `edges` (ascending chunk starts, the first one 0) with a
// global cap and compare with one pass.
void check_split(const std::vector<uint8_t>& cls, const std::vector<uint64_t>& edges, uint64_t cap) {
    const uint64_t n = cls.size();
    pcs_extent_summary want;
    std::vector<pcs_extent> want_runs;
    naive(cls, 0, n, cap, want, want_runs);

    pcs_extent_summary got;
    got.n_pages = 0xDEAD;  // the merge overwrites whatever the summary held
    std::vector<pcs_extent> got_runs(cap, pcs_extent{kGarbage, kGarbage, 0xABABABABu, 0xABABABABu});
    got_runs.shrink_to_fit();
    pcs::ExtentMerge merge(&got, cap ? got_runs.data() : nullptr, cap);
    for (size_t k = 0; k < edges.size(); ++k) {
        const uint64_t first = edges[k], end = k + 1 < edges.size() ? edges[k + 1] : n;
        pcs_extent_summary c;
        std::vector<pcs_extent> cruns;
        naive(cls, first, end - first, pcs::ExtentMerge::chunk_cap(cap, end - first), c, cruns);
        merge.add(c, cruns.data(), first);
    }
    const bool ok = same(got, want);
    CHECK(ok);
    if (!ok)
        std::fprintf(stderr, "  n=%llu cap=%llu chunks=%zu runs %llu/%llu holes %llu/%llu written %llu/%llu\n",
                     (unsigned long long)n, (unsigned long long)cap, edges.size(), (unsigned long long)got.n_runs,
                     (unsigned long long)want.n_runs, (unsigned long long)got.n_holes,
                     (unsigned long long)want.n_holes, (unsigned long long)got.written_pages,
                     (unsigned long long)want.written_pages);
    for (uint64_t i = 0; i < want.n_listed && i < cap; ++i) {
        CHECK(got_runs[i].first_page == want_runs[i].first_page);
        CHECK(got_runs[i].n_pages == want_runs[i].n_pages);  // the full length, also of the last listed run
        CHECK(got_runs[i].cls == want_runs[i].cls && got_runs[i].reserved == 0);
    }
    for (uint64_t i = want.n_listed; i < cap; ++i) CHECK(got_runs[i].first_page == kGarbage && got_runs[i].n_pages == kGarbage);
}

void check_array(const std::vector<uint8_t>& cls, uint64_t& seed) {
    const uint64_t n = cls.size();
    pcs_extent_summary whole;
    std::vector<pcs_extent> whole_runs;
    naive(cls, 0, n, n + 1, whole, whole_runs);
    const uint64_t caps[] = {0, 1, 2, whole.n_runs, whole.n_runs + 1, whole.n_runs + 100, 7};
    std::vector<std::vector<uint64_t>> splits;
    splits.push_back({0});  // one chunk
    for (uint64_t chunk : {uint64_t(1), uint64_t(2), uint64_t(3), uint64_t(16), uint64_t(100)}) {
        std::vector<uint64_t> e;
        for (uint64_t f = 0; f < n; f += chunk) e.push_back(f);
        splits.push_back(e);
    }
    {   // chunk edges exactly at every run start (a run's start is the previous run's end)
        std::vector<uint64_t> e;
        for (const pcs_extent& r : whole_runs) e.push_back(r.first_page);
        splits.push_back(e);
    }
    {   // chunk edges inside runs only, where a run is long enough
        std::vector<uint64_t> e{0};
        for (const pcs_extent& r : whole_runs)
            if (r.n_pages >= 2 && r.first_page + 1 > e.back()) e.push_back(r.first_page + 1 + rnd(seed) % (r.n_pages - 1));
        splits.push_back(e);
    }
    for (int k = 0; k < 4; ++k) {  // random chunk sizes
        std::vector<uint64_t> e;
        const uint64_t span = 1 + rnd(seed) % (n / 2 + 2);
        for (uint64_t f = 0; f < n; f += 1 + rnd(seed) % span) e.push_back(f);
        splits.push_back(e);
    }
    for (const auto& e : splits) {
        if (n && (e.empty() || e[0] != 0)) continue;
        for (uint64_t cap : caps) check_split(cls, e, cap);
    }
}

}  // namespace

int main() {
    uint64_t seed = 12345;
    auto arr = [](std::initializer_list<int> v) {
        std::vector<uint8_t> a;
        for (int x : v) a.push_back((uint8_t)x);
        return a;
    };
    // hand-written: empty, all blank, tail only, hole at page 0, hole + corrupt run + tail, a foreign byte,
    // a blank tail that turns into a hole at the very last page
    for (const auto& a : {arr({}), arr({2}), arr({2, 2, 2, 2, 2}), arr({1, 1, 2, 2}), arr({2, 1}),
                          arr({1, 2, 1, 0, 0, 2, 2}), arr({1, 7, 7, 1}), arr({1, 1, 2, 2, 2, 2, 2, 2, 1}),
                          arr({0, 0, 0, 0, 0, 0, 0, 0, 0, 0})})
        check_array(a, seed);
    // the last listed run extended by later chunks, by hand: cap 2, one page per chunk
    {
        const std::vector<uint8_t> a = arr({1, 0, 0, 0, 0, 0, 2});
        std::vector<uint64_t> e{0, 1, 2, 3, 4, 5, 6};
        check_split(a, e, 2);
    }
    for (int round = 0; round < 60; ++round) {
        const uint64_t n = 1 + rnd(seed) % 400;
        std::vector<uint8_t> a(n);
        const int kind = round % 6;
        uint64_t i = 0;
        while (i < n) {
            uint64_t len;
            uint8_t c;
            const uint64_t r = rnd(seed);
            switch (kind) {
                case 0: len = 1; c = (uint8_t)(i & 1 ? 2 : 1); break;              // alternating bytes
                case 1: len = n; c = 2; break;                                    // all blank
                case 2: len = 1 + r % 150; c = (uint8_t)((r >> 20) % 3); break;   // long constant stretches
                case 3: len = 1 + r % 4; c = (uint8_t)((r >> 20) % 3); break;     // short runs
                case 4: len = 1 + r % 40; c = (uint8_t)(((r >> 20) & 7) == 0 ? 7 : (r >> 24) % 3); break;  // a foreign byte
                default: len = i == 0 ? 1 + r % n : n; c = (uint8_t)(i == 0 ? 1 : 2); break;               // ok prefix, blank tail
            }
            for (uint64_t k = 0; k < len && i < n; ++k) a[i++] = c;
        }
        check_array(a, seed);
    }
    if (g_fail) {
        std::fprintf(stderr, "extent_merge_test: %d failures\n", g_fail);
        return 1;
    }
    std::printf("extent_merge_test ok\n");
    return 0;
}
