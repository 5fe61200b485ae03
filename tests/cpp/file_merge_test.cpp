// file_merge_test — pcs::FileMerge and pcs::files_summarize
// (eloqstore_amd/csrc/file_merge.h) fed with the reports of a file's parts,
// built by a naive loop, and checked against the same loop over the whole
// file.  No HIP: built with ASAN + UBSan (eloqstore_amd/Makefile `sanitize`)
// and run by tests/test_files_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "file_merge.h"

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

// What the device reports for pages [first, first + cnt) as one file, by the
// definitions of include/eloqstore_pcs.h.
pcs_file_report naive(const std::vector<uint8_t>& cls, const std::vector<uint8_t>& type, uint64_t first, uint64_t cnt) {
    pcs_file_report r = pcs::FileMerge::empty(first);
    r.n_pages = cnt;
    for (uint64_t i = 0; i < cnt; ++i) {
        const uint8_t c = cls[first + i], t = type[first + i];
        if (c == PCS_PAGE_OK) {
            ++r.n_ok;
            ++r.ok_by_type[t < 4 ? t : t == 255 ? 4 : 5];
        } else if (c == PCS_PAGE_CORRUPT) {
            ++r.n_corrupt;
            if (r.first_corrupt == UINT64_MAX) r.first_corrupt = i;
        } else if (c == PCS_PAGE_BLANK) {
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

bool same(const pcs_file_report& a, const pcs_file_report& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// Merge the file cls[0 .. n) cut at `edges` (ascending part starts, the first
// one 0) and compare with one pass.
void check_cut(const std::vector<uint8_t>& cls, const std::vector<uint8_t>& type, const std::vector<uint64_t>& edges,
               const char* what) {
    const uint64_t n = cls.size();
    const pcs_file_report want = naive(cls, type, 0, n);
    pcs_file_report got = pcs::FileMerge::empty(0);
    for (size_t k = 0; k < edges.size(); ++k) {
        const uint64_t a = edges[k], b = k + 1 < edges.size() ? edges[k + 1] : n;
        pcs_file_report part = naive(cls, type, a, b - a);
        part.first_page = 0x7777;  // ignored by the merge
        pcs::FileMerge::add(got, part);
    }
    if (!same(got, want)) {
        std::fprintf(stderr, "FAIL %s: n=%llu parts=%zu holes %llu/%llu hole pages %llu/%llu first hole %llu/%llu written %llu/%llu\n",
                     what, (unsigned long long)n, edges.size(), (unsigned long long)got.n_holes,
                     (unsigned long long)want.n_holes, (unsigned long long)got.n_hole_pages,
                     (unsigned long long)want.n_hole_pages, (unsigned long long)got.first_hole,
                     (unsigned long long)want.first_hole, (unsigned long long)got.written_pages,
                     (unsigned long long)want.written_pages);
        ++g_fail;
    }
}

std::vector<uint8_t> from_runs(std::initializer_list<std::pair<int, int>> runs) {
    std::vector<uint8_t> v;
    for (auto [c, k] : runs) v.insert(v.end(), (size_t)k, (uint8_t)c);
    return v;
}

void every_cut(const std::vector<uint8_t>& cls, const char* what) {
    std::vector<uint8_t> type(cls.size());
    for (size_t i = 0; i < type.size(); ++i) type[i] = (uint8_t)(i % 7 == 6 ? 255 : i % 7);
    const uint64_t n = cls.size();
    check_cut(cls, type, {0}, what);
    std::vector<uint64_t> ones;  // parts of 1 page
    for (uint64_t i = 0; i < n; ++i) ones.push_back(i);
    if (n) check_cut(cls, type, ones, what);
    for (uint64_t a = 1; a < n; ++a) {
        check_cut(cls, type, {0, a}, what);  // every single cut: inside, at the start and at the end of every run
        for (uint64_t b = a + 1; b < n; ++b) check_cut(cls, type, {0, a, b}, what);
    }
}

}  // namespace

int main() {
    constexpr int C = PCS_PAGE_CORRUPT, O = PCS_PAGE_OK, B = PCS_PAGE_BLANK;
    every_cut({}, "empty");
    every_cut(from_runs({{B, 1}}), "one blank");
    every_cut(from_runs({{O, 5}, {B, 4}}), "tail only");
    every_cut(from_runs({{O, 3}, {B, 4}, {O, 1}}), "a blank tail that a later part turns into a hole");
    every_cut(from_runs({{B, 3}, {O, 2}, {B, 5}, {O, 2}, {B, 2}}), "hole at 0, hole, tail");
    every_cut(from_runs({{B, 12}}), "all blank: every part is blank");
    every_cut(from_runs({{B, 6}, {C, 1}}), "all-blank parts ended by a corrupt page");
    every_cut(from_runs({{O, 8}, {C, 2}, {O, 3}, {C, 1}}), "a corrupt page first seen in a later part");
    every_cut(from_runs({{O, 2}, {7, 3}, {B, 2}, {9, 1}, {B, 1}}), "foreign class bytes are written pages");
    every_cut(from_runs({{B, 1}, {O, 1}, {B, 1}, {O, 1}, {B, 1}, {O, 1}, {B, 1}}), "alternating");
    {
        // a corrupt page first seen in the third part, by hand
        const std::vector<uint8_t> cls = from_runs({{O, 4}, {B, 4}, {O, 2}, {C, 1}, {O, 1}}), type(cls.size(), 2);
        pcs_file_report got = pcs::FileMerge::empty(100);
        pcs::FileMerge::add(got, naive(cls, type, 0, 4));
        CHECK(got.n_holes == 0 && got.written_pages == 4 && got.first_corrupt == UINT64_MAX);
        pcs::FileMerge::add(got, naive(cls, type, 4, 4));
        CHECK(got.n_holes == 0 && got.written_pages == 4 && got.n_blank == 4 && got.n_pages == 8);  // a tail so far
        pcs::FileMerge::add(got, naive(cls, type, 8, 4));
        CHECK(got.n_holes == 1 && got.n_hole_pages == 4 && got.first_hole == 4 && got.written_pages == 12);
        CHECK(got.first_corrupt == 10 && got.n_corrupt == 1 && got.first_page == 100 && got.ok_by_type[2] == 7);
    }
    // random files, random cuts
    uint64_t seed = 0xF11E5;
    for (int rep = 0; rep < 400; ++rep) {
        const uint64_t n = rnd(seed) % 200;
        std::vector<uint8_t> cls(n), type(n);
        uint8_t c = (uint8_t)(rnd(seed) % 3);
        for (uint64_t i = 0; i < n; ++i) {
            if (rnd(seed) % 4 == 0) c = (uint8_t)(rnd(seed) % 8 == 0 ? 5 : rnd(seed) % 3);
            cls[i] = c;
            type[i] = (uint8_t)(rnd(seed) % 2 ? rnd(seed) % 6 : 255);
        }
        std::vector<uint64_t> edges{0};
        for (uint64_t i = 1; i < n; ++i)
            if (rnd(seed) % 9 == 0) edges.push_back(i);
        check_cut(cls, type, edges, "random");
    }
    {
        // files_summarize: totals and the capped ascending list; the list is an exact-size buffer
        const std::vector<uint8_t> cls = from_runs({{O, 3}, {C, 1}, {B, 2}, {B, 1}, {O, 1}, {O, 2}, {B, 2}}), type(cls.size(), 1);
        const uint64_t first[] = {0, 4, 4, 6, 8, 10, 12, 12};  // corrupt | empty | unwritten | hole | clean | unwritten | empty
        std::vector<pcs_file_report> reps;
        for (int f = 0; f < 7; ++f) reps.push_back(naive(cls, type, first[f], first[f + 1] - first[f]));
        for (uint64_t cap : {0ull, 1ull, 2ull, 5ull}) {
            std::vector<uint64_t> bad(cap, 0xABABull);
            bad.shrink_to_fit();
            pcs_files_summary s;
            std::memset(&s, 0xAB, sizeof s);
            pcs::files_summarize(reps.data(), reps.size(), &s, cap ? bad.data() : nullptr, cap);
            CHECK(s.n_files == 7 && s.n_pages == 12 && s.n_ok == 6 && s.n_corrupt == 1 && s.n_blank == 5);
            CHECK(s.n_corrupt_files == 1 && s.n_hole_files == 1 && s.n_bad_files == 2 && s.n_unwritten_files == 4);
            CHECK(s.first_bad_file == 0 && s.invalid_file == UINT64_MAX && s.n_listed == (cap < 2 ? cap : 2));
            if (cap >= 1) CHECK(bad[0] == 0);
            if (cap >= 2) CHECK(bad[1] == 3);
            if (cap > 2) CHECK(bad[2] == 0xABABull);
        }
        pcs_files_summary s;
        pcs::files_summarize(nullptr, 0, &s, nullptr, 0);
        CHECK(s.n_files == 0 && s.n_bad_files == 0 && s.first_bad_file == UINT64_MAX && s.invalid_file == UINT64_MAX);
    }
    if (g_fail) {
        std::fprintf(stderr, "file_merge_test: %d failures\n", g_fail);
        return 1;
    }
    std::printf("file_merge_test ok\n");
    return 0;
}
