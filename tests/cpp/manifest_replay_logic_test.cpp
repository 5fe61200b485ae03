// manifest_replay_logic_test — the host-side logic of the manifest replay and
// the liveness-aware scrub (eloqstore_amd/csrc/manifest_replay.h): the argument
// rules, the carry of table rows across staging groups against one pass over
// the whole batch, the summary, the data-file name rule and the --live tool's
// text and exit codes.  No HIP: built with ASAN + UBSan (eloqstore_amd/Makefile
// `sanitize`) and run by tests/test_replay_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "manifest_replay.h"

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

bool has(const char* msg, const char* part) { return msg && std::strstr(msg, part); }

void test_arguments() {
    alignas(8) static uint8_t mem[64];
    void* p = mem;
    // device form
    CHECK(!pcs::replay_dev_args(p, 64, p, p, 1, 64, nullptr, p, p, p, 8));
    CHECK(!pcs::replay_dev_args(nullptr, 0, nullptr, nullptr, 0, 4096, nullptr, nullptr, p, nullptr, 0));
    CHECK(has(pcs::replay_dev_args(p, 64, p, p, 1, 64, nullptr, p, nullptr, p, 8), "d_summary"));
    CHECK(has(pcs::replay_dev_args(p, 64, p, p, 1, 100, nullptr, p, p, p, 8), "power of two"));
    CHECK(has(pcs::replay_dev_args(nullptr, 64, p, p, 1, 64, nullptr, p, p, p, 8), "d_base is null"));
    CHECK(has(pcs::replay_dev_args(mem + 4, 64, p, p, 1, 64, nullptr, p, p, p, 8), "8-byte aligned"));
    CHECK(has(pcs::replay_dev_args(p, 64, nullptr, p, 1, 64, nullptr, p, p, p, 8), "d_img_off"));
    CHECK(has(pcs::replay_dev_args(p, 64, p, p, 1, 64, nullptr, nullptr, p, p, 8), "d_reports"));
    CHECK(has(pcs::replay_dev_args(p, 64, p, p, 1, 64, mem + 4, p, p, p, 8), "8-byte aligned"));
    CHECK(has(pcs::replay_dev_args(p, 64, p, p, 1, 64, nullptr, p, p, nullptr, 8), "d_table is null"));
    CHECK(!pcs::replay_dev_args(p, 64, p, p, 1, 64, nullptr, p, p, nullptr, 0));
    CHECK(has(pcs::replay_dev_args(p, 1ull << 32, p, p, 1, 4096, nullptr, p, p, p, 8), "below 2^32"));
    CHECK(!pcs::replay_dev_args(p, (1ull << 32) - 4096, p, p, 1, 4096, nullptr, p, p, p, 8));
    CHECK(has(pcs::replay_dev_args(p, 64, p, p, 1, 64, nullptr, p, p, p, 1ull << 60), "table_cap"));
    // host form
    const void* imgs[2] = {mem, mem};
    uint64_t sizes[2] = {10, 20};
    CHECK(!pcs::replay_host_args(imgs, sizes, 2, 4096, p, p, p, 8));
    CHECK(!pcs::replay_host_args(nullptr, nullptr, 0, 4096, nullptr, p, nullptr, 0));
    CHECK(has(pcs::replay_host_args(imgs, sizes, 2, 4096, p, nullptr, p, 8), "summary is null"));
    CHECK(has(pcs::replay_host_args(nullptr, sizes, 2, 4096, p, p, p, 8), "images / sizes"));
    CHECK(has(pcs::replay_host_args(imgs, sizes, 2, 4096, nullptr, p, p, 8), "reports is null"));
    CHECK(has(pcs::replay_host_args(imgs, sizes, 2, 4096, p, p, nullptr, 8), "table is null"));
    CHECK(has(pcs::replay_host_args(imgs, sizes, 2, 32, p, p, p, 8), "power of two"));
    const void* hole[2] = {mem, nullptr};
    CHECK(has(pcs::replay_host_args(hole, sizes, 2, 4096, p, p, p, 8), "non-zero size is null"));
    uint64_t big[2] = {10, 1ull << 32};
    CHECK(has(pcs::replay_host_args(imgs, big, 2, 4096, p, p, p, 8), "too large"));
    // live
    CHECK(!pcs::live_args(p, 10, 5, p, 3, p, p, 4));
    CHECK(!pcs::live_args(nullptr, 0, 0, nullptr, 0, p, nullptr, 0));
    CHECK(has(pcs::live_args(p, 10, 5, p, 3, nullptr, p, 4), "summary is null"));
    CHECK(has(pcs::live_args(nullptr, 10, 5, p, 3, p, p, 4), "class bytes"));
    CHECK(has(pcs::live_args(p, 10, 5, nullptr, 3, p, p, 4), "table is null"));
    CHECK(has(pcs::live_args(p, 10, 5, p, 1ull << 32, p, p, 4), "2^32 - 1"));
    CHECK(!pcs::live_args(p, 10, 5, p, 0xFFFFFFFFull, p, p, 4));
    CHECK(has(pcs::live_args(p, 10, 5, p, 3, p, nullptr, 4), "damaged list is null"));
    CHECK(has(pcs::live_args(p, 10, (1ull << 61) - 5, p, 3, p, p, 4), "file page ids"));
    CHECK(has(pcs::live_args(p, 10, UINT64_MAX - 3, p, 3, p, p, 4), "file page ids"));
}

// One pass over a batch: table_first, the TABLE_CAP rule and the summary, as the device form defines them.
void one_pass(std::vector<pcs_replay_report>& r, uint64_t base, uint64_t cap) {
    uint64_t first = base;
    for (pcs_replay_report& x : r) {
        x.table_first = first;
        if (x.status == PCS_REPLAY_OK || x.status == PCS_REPLAY_TABLE_CAP) {
            x.status = first + x.table_size > cap ? PCS_REPLAY_TABLE_CAP : PCS_REPLAY_OK;
            first += x.table_size;
        }
    }
}

void test_carry_and_summary() {
    uint64_t seed = 11;
    for (int round = 0; round < 300; ++round) {
        const uint64_t n = rnd(seed) % 40;
        std::vector<pcs_replay_report> whole(n);
        uint64_t total = 0;
        for (pcs_replay_report& x : whole) {
            x = pcs_replay_report{};
            const uint64_t kind = rnd(seed) % 6;
            x.status = kind == 0 ? PCS_REPLAY_NOT_REPLAYABLE : kind == 1 ? PCS_REPLAY_MALFORMED : PCS_REPLAY_OK;
            if (x.status == PCS_REPLAY_OK) {
                x.table_size = rnd(seed) % 50;
                x.n_mapped = x.table_size / 2;
                x.n_log_entries = rnd(seed) % 9;
                total += x.table_size;
            }
        }
        const uint64_t cap = total ? rnd(seed) % (total + 10) : rnd(seed) % 3;
        std::vector<pcs_replay_report> groups = whole;
        one_pass(whole, 0, cap);
        // the same batch cut into groups, each counted from the carry
        pcs::ReplayCarry carry;
        for (uint64_t g0 = 0; g0 < n;) {
            const uint64_t g = 1 + rnd(seed) % 7, g1 = g0 + g < n ? g0 + g : n;
            std::vector<pcs_replay_report> part(groups.begin() + g0, groups.begin() + g1);
            one_pass(part, carry.rows, cap);
            carry.add(part.data(), part.size());
            std::copy(part.begin(), part.end(), groups.begin() + g0);
            g0 = g1;
        }
        uint64_t rows = 0, written = 0, mapped = 0, entries = 0, first_bad = UINT64_MAX, by[4] = {};
        for (uint64_t i = 0; i < n; ++i) {
            CHECK(groups[i].status == whole[i].status && groups[i].table_first == whole[i].table_first);
            if (whole[i].status == PCS_REPLAY_TABLE_CAP) groups[i].n_mapped = 0;  // as the device reports it
            ++by[groups[i].status];
            if (groups[i].status == PCS_REPLAY_OK || groups[i].status == PCS_REPLAY_TABLE_CAP) {
                rows += groups[i].table_size;
                entries += groups[i].n_log_entries;
            }
            if (groups[i].status == PCS_REPLAY_OK) {
                written += groups[i].table_size;
                mapped += groups[i].n_mapped;
            } else if (first_bad == UINT64_MAX) {
                first_bad = i;
            }
        }
        CHECK(carry.rows == rows);
        pcs_replay_summary s;
        std::memset(&s, 0xEE, sizeof s);
        pcs::replay_summarize(groups.data(), n, &s);
        CHECK(s.n_images == n && s.n_rows == rows && s.n_rows_written == written && s.n_mapped == mapped);
        CHECK(s.n_log_entries == entries && s.first_bad_image == first_bad && s.invalid_image == UINT64_MAX);
        CHECK(s.reserved == 0 && written <= cap);
        for (int k = 0; k < 4; ++k) CHECK(s.n_by_status[k] == by[k]);
    }
    pcs_replay_summary s;
    pcs::replay_summarize(nullptr, 0, &s);
    CHECK(s.n_images == 0 && s.n_rows == 0 && s.first_bad_image == UINT64_MAX && s.invalid_image == UINT64_MAX);
}

void test_names() {
    uint64_t id = 99, term = 99;
    CHECK(pcs::live_parse_data_file("data_123_5", id, term) && id == 123 && term == 5);
    CHECK(pcs::live_parse_data_file("/a/b.c/data_0_0", id, term) && id == 0 && term == 0);
    CHECK(pcs::live_parse_data_file("x/data_18446744073709551615_7", id, term) && id == UINT64_MAX && term == 7);
    for (const char* bad : {"data_123", "data__5", "data_12_", "data_1_2_3", "manifest_5", "data_12x_5", "data_-1_5",
                            "data_ 1_5", "data_18446744073709551616_1", "", "data_", "dir/", "xdata_1_2", "data_1_+2"})
        CHECK(!pcs::live_parse_data_file(bad, id, term));
    CHECK(!std::strcmp(pcs::replay_status_name(0), "ok") && !std::strcmp(pcs::replay_status_name(3), "table-cap"));
    CHECK(!std::strcmp(pcs::replay_status_name(17), "unknown"));
    CHECK(!std::strcmp(pcs::live_class_name(0), "corrupt") && !std::strcmp(pcs::live_class_name(1), "ok") &&
          !std::strcmp(pcs::live_class_name(2), "blank") && !std::strcmp(pcs::live_class_name(200), "other"));
}

void test_tool_text() {
    pcs_replay_report r{};
    r.status = PCS_REPLAY_OK;
    r.root = 4;
    r.ttl_root = 5;
    r.max_fp_id = 600;
    r.n_mapped = 70;
    CHECK(pcs::live_tool_refusal("m", r).empty());
    CHECK(pcs::live_tool_footer(r, 50) == "root 4 ttl_root 5 max_fp_id 600 mapped 70 mapped_in_files_not_given 20\n");
    CHECK(pcs::live_tool_footer(r, 70) == "root 4 ttl_root 5 max_fp_id 600 mapped 70 mapped_in_files_not_given 0\n");
    CHECK(pcs::live_tool_footer(r, 71) == "root 4 ttl_root 5 max_fp_id 600 mapped 70 mapped_in_files_not_given 0\n");
    r.status = PCS_REPLAY_MALFORMED;
    r.malformed_record = 3;
    CHECK(pcs::live_tool_refusal("dir/m", r) == "dir/m: manifest cannot be replayed: malformed at record 3\n");
    r.status = PCS_REPLAY_NOT_REPLAYABLE;
    CHECK(pcs::live_tool_refusal("m", r) == "m: manifest cannot be replayed: not-replayable\n");
    pcs_live_summary s{};
    s.n_pages = 64;
    s.live_ok = 1;
    s.live_blank = 2;
    s.live_corrupt = 3;
    s.dead_ok = 4;
    s.dead_blank = 5;
    s.dead_corrupt = 6;
    CHECK(pcs::live_tool_file_line("d/data_7_1", 7, s) ==
          "d/data_7_1: file 7 pages 64 live ok 1 blank 2 corrupt 3 dead ok 4 blank 5 corrupt 6\n");
    pcs_live_page p{};
    p.index = 9;
    p.page_id = 41;
    p.cls = PCS_PAGE_BLANK;
    CHECK(pcs::live_tool_page_line(7 << 6, p) == "  damaged: page_id 41 file_page 457 class blank\n");
    // exit codes: corrupt beats blank, dead damage is no failure
    pcs_live_summary files[3] = {};
    CHECK(pcs::live_tool_exit(files, 3) == 0 && pcs::live_tool_exit(nullptr, 0) == 0);
    files[1].dead_corrupt = 9;
    files[2].dead_blank = 9;
    CHECK(pcs::live_tool_exit(files, 3) == 0);
    files[0].live_blank = 1;
    CHECK(pcs::live_tool_exit(files, 3) == 3);
    files[2].live_corrupt = 1;
    CHECK(pcs::live_tool_exit(files, 3) == 2);
}

}  // namespace

int main() {
    test_arguments();
    test_carry_and_summary();
    test_names();
    test_tool_text();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("manifest replay logic ok\n");
    return 0;
}
