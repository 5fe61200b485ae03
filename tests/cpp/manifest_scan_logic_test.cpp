// manifest_scan_logic_test — the host-side logic of the manifest scan
// (eloqstore_amd/csrc/manifest_scan.h): the argument rules, the packing plan,
// the verdict derived from ok flags against a naive second formulation, the
// summary of whole reports, and the reference tool's text and exit codes on
// hand-written reports.  No HIP: built with ASAN + UBSan
// (eloqstore_amd/Makefile `sanitize`) and run by tests/test_manifest_scan_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "manifest_scan.h"

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

void test_arguments() {
    for (uint32_t a : {64u, 128u, 4096u, 65536u}) CHECK(pcs::manifest_align_ok(a));
    for (uint32_t a : {0u, 1u, 32u, 63u, 65u, 96u, 4097u, 131072u, 0x80000000u}) CHECK(!pcs::manifest_align_ok(a));
    CHECK(pcs::manifest_round_up(0, 64) == 0 && pcs::manifest_round_up(1, 64) == 64 &&
          pcs::manifest_round_up(64, 64) == 64 && pcs::manifest_round_up(4097, 4096) == 8192);
    CHECK(pcs::manifest_batch_fits(0, 0, 64) && pcs::manifest_batch_fits(8u << 20, 1, 4096));
    CHECK(pcs::manifest_batch_fits(1ull << 40, 1, 4096));   // 2^28 slots + 2^20 chunks
    CHECK(!pcs::manifest_batch_fits(1ull << 40, 1, 64));    // 2^34 slots
    CHECK(!pcs::manifest_batch_fits(1ull << 62, 1, 65536) && !pcs::manifest_batch_fits(UINT64_MAX, 1, 65536));
    CHECK(!pcs::manifest_batch_fits(0, 1ull << 31, 4096) && pcs::manifest_batch_fits(0, (1ull << 31) - 17, 4096));
}

void test_pack() {
    // every image in exactly one group, offsets aligned and ascending, groups within the budget
    uint64_t seed = 7;
    for (int round = 0; round < 200; ++round) {
        const uint32_t align = 64u << (rnd(seed) % 11);
        const uint64_t budget = (rnd(seed) % 64 + 1) * align;
        std::vector<uint64_t> sizes(rnd(seed) % 40);
        for (auto& s : sizes) s = rnd(seed) % 5 == 0 ? 0 : rnd(seed) % (budget * 2);
        const auto groups = pcs::manifest_pack(sizes.data(), sizes.size(), align, budget);
        uint64_t next = 0;
        for (const auto& g : groups) {
            CHECK(g.first == next && g.count > 0 && g.off.size() == g.count);
            uint64_t at = 0;
            for (uint64_t k = 0; k < g.count; ++k) {
                CHECK(g.off[k] == at && at % align == 0);
                at += pcs::manifest_round_up(sizes[g.first + k], align);
            }
            CHECK(g.bytes == at);
            CHECK(g.bytes <= budget || g.count == 1);  // an image above the budget is a group of its own
            next += g.count;
        }
        CHECK(next == sizes.size());
        // greedy: a group could not have taken its successor's first image
        for (size_t k = 0; k + 1 < groups.size(); ++k)
            CHECK(groups[k].bytes + pcs::manifest_round_up(sizes[groups[k + 1].first], align) > budget);
    }
    CHECK(pcs::manifest_pack(nullptr, 0, 4096).empty());
    const uint64_t three[3] = {5, 0, 4097};
    const auto g = pcs::manifest_pack(three, 3, 4096);
    CHECK(g.size() == 1 && g[0].bytes == 3 * 4096 && g[0].off[1] == 4096 && g[0].off[2] == 4096);
}

void test_verdict() {
    using V = pcs::ManifestFlagsResult;
    auto v = [](std::vector<uint8_t> f) { return pcs::manifest_verdict(f.data(), f.size()); };
    V r = v({});
    CHECK(r.verdict == PCS_MANIFEST_EMPTY && r.first_corrupt == UINT64_MAX && r.n_ok == 0 && r.n_corrupt == 0);
    CHECK(v({1}).verdict == PCS_MANIFEST_CLEAN && v({1, 1, 1}).verdict == PCS_MANIFEST_CLEAN);
    CHECK(v({0}).verdict == PCS_MANIFEST_BAD_SNAPSHOT && v({0, 1, 1}).verdict == PCS_MANIFEST_BAD_SNAPSHOT);
    r = v({1, 1, 0});
    CHECK(r.verdict == PCS_MANIFEST_TORN_TAIL && r.first_corrupt == 2 && r.n_ok_after_corrupt == 0);
    r = v({1, 0, 0, 0});
    CHECK(r.verdict == PCS_MANIFEST_TORN_TAIL && r.first_corrupt == 1 && r.n_corrupt == 3);
    r = v({1, 0, 1, 0});
    CHECK(r.verdict == PCS_MANIFEST_BROKEN && r.first_corrupt == 1 && r.n_ok_after_corrupt == 1 && r.n_ok == 2);
    // against the enum comments, spelled out the slow way
    uint64_t seed = 11;
    for (int round = 0; round < 2000; ++round) {
        std::vector<uint8_t> f(rnd(seed) % 9);
        for (auto& x : f) x = rnd(seed) % 3 != 0;
        r = v(f);
        uint64_t want;
        if (f.empty()) want = PCS_MANIFEST_EMPTY;
        else if (!f[0]) want = PCS_MANIFEST_BAD_SNAPSHOT;
        else {
            size_t fc = 0;
            while (fc < f.size() && f[fc]) ++fc;
            bool ok_after = false;
            for (size_t k = fc; k < f.size(); ++k) ok_after = ok_after || f[k];
            want = fc == f.size() ? PCS_MANIFEST_CLEAN : ok_after ? PCS_MANIFEST_BROKEN : PCS_MANIFEST_TORN_TAIL;
        }
        CHECK(r.verdict == want && r.n_ok + r.n_corrupt == f.size());
    }
}

pcs_manifest_report rep(uint64_t n, uint64_t corrupt, uint64_t verdict) {
    pcs_manifest_report r{};
    r.n_records = n;
    r.n_corrupt = corrupt;
    r.n_ok = n - corrupt;
    r.verdict = verdict;
    r.first_record = 999;  // a group-local value the summary must replace
    return r;
}

void test_summary() {
    std::vector<pcs_manifest_report> reps = {rep(3, 0, PCS_MANIFEST_CLEAN), rep(0, 0, PCS_MANIFEST_EMPTY),
                                             rep(5, 2, PCS_MANIFEST_TORN_TAIL), rep(1, 1, PCS_MANIFEST_BAD_SNAPSHOT),
                                             rep(4, 1, PCS_MANIFEST_BROKEN), rep(2, 0, PCS_MANIFEST_CLEAN)};
    pcs_manifest_summary s;
    std::memset(&s, 0xA5, sizeof s);
    pcs::manifest_summarize(reps.data(), reps.size(), 7, &s);
    CHECK(s.n_images == 6 && s.n_records == 15 && s.n_ok == 11 && s.n_corrupt == 4);
    CHECK(s.n_by_verdict[0] == 2 && s.n_by_verdict[1] == 1 && s.n_by_verdict[2] == 1 && s.n_by_verdict[3] == 1 &&
          s.n_by_verdict[4] == 1);
    CHECK(s.first_bad_image == 1 && s.n_listed == 7 && s.invalid_image == UINT64_MAX);
    const uint64_t first[6] = {0, 3, 3, 8, 9, 13};
    for (int i = 0; i < 6; ++i) CHECK(reps[i].first_record == first[i]);
    pcs::manifest_summarize(reps.data(), 1, 100, &s);
    CHECK(s.first_bad_image == UINT64_MAX && s.n_listed == 3);
    pcs::manifest_summarize(nullptr, 0, 0, &s);
    CHECK(s.n_images == 0 && s.n_records == 0 && s.n_listed == 0 && s.first_bad_image == UINT64_MAX);
}

void test_tool_text() {
    // a 3-record image at align 64: record 1 failed (its payload is dumped), then cut inside a header
    std::vector<uint8_t> img(64 * 3 + 7, 0);
    const uint8_t pay[3] = {0xAB, 0x01, 0xF0};
    std::memcpy(img.data() + 64 + 20, pay, 3);
    pcs_manifest_record recs[3] = {};
    recs[0] = {0, 1, 1, 0, 7, 9, 1};
    recs[1] = {64, 2, 3, 3, 0, 4294967295u, 0};
    recs[2] = {128, 5, 5, 44, 1, 2, 1};
    pcs_manifest_report r = rep(3, 1, PCS_MANIFEST_BROKEN);
    r.end_offset = 192;
    r.end_reason = PCS_MANIFEST_END_SHORT_HEADER;
    pcs::ManifestToolText t = pcs::manifest_tool_text("m.bin", img.data(), r, recs);
    const std::string body =
        "Log #0 at offset 0\n  record size: 20\n  root: 7\n  ttl_root: 9\n  payload_bytes: 0\n  checksum: OK\n"
        "Log #1 at offset 64\n  record size: 23\n  root: 0\n  ttl_root: 4294967295\n  payload_bytes: 3\n"
        "  checksum: FAILED\n  payload_hex: ab01f0\n"
        "Log #2 at offset 128\n  record size: 64\n  root: 1\n  ttl_root: 2\n  payload_bytes: 44\n  checksum: OK\n";
    CHECK(t.out == body && t.exit_code == 1);
    CHECK(t.err == "Manifest truncated while reading header at offset 192\n");
    r.end_reason = PCS_MANIFEST_END_SHORT_PAYLOAD;
    t = pcs::manifest_tool_text("m.bin", img.data(), r, recs);
    CHECK(t.out == body && t.exit_code == 1 && t.err == "Manifest truncated while reading payload at offset 212\n");
    for (uint64_t reason : {(uint64_t)PCS_MANIFEST_END_CLEAN, (uint64_t)PCS_MANIFEST_END_SHORT_PADDING}) {
        r.end_reason = reason;  // the tool seeks over padding: a cut padding is no error
        t = pcs::manifest_tool_text("m.bin", img.data(), r, recs);
        CHECK(t.out == body + "Parsed 3 logs from m.bin\n" && t.err.empty() && t.exit_code == 2);
    }
    recs[1].ok = 1;
    t = pcs::manifest_tool_text("m.bin", img.data(), r, recs);
    CHECK(t.exit_code == 0 && t.out.find("payload_hex") == std::string::npos);
    pcs_manifest_report none = rep(0, 0, PCS_MANIFEST_EMPTY);
    t = pcs::manifest_tool_text("dir/e.bin", img.data(), none, nullptr);
    CHECK(t.out.empty() && t.err == "No manifest logs found in dir/e.bin\n" && t.exit_code == 1);

    pcs_manifest_report line = rep(5, 2, PCS_MANIFEST_TORN_TAIL);
    line.valid_prefix_bytes = 12288;
    CHECK(pcs::manifest_tool_line("a", line) == "a: records 5 corrupt 2 verdict torn-tail valid_prefix_bytes 12288\n");
    const char* names[5] = {"clean", "torn-tail", "broken", "bad-snapshot", "empty"};
    for (uint64_t v = 0; v < 5; ++v) CHECK(std::string(pcs::manifest_verdict_name(v)) == names[v]);
    CHECK(std::string(pcs::manifest_verdict_name(5)) == "unknown");

    auto code = [](std::vector<uint64_t> verdicts, bool unreadable) {
        std::vector<pcs_manifest_report> reps;
        for (uint64_t v : verdicts) reps.push_back(rep(1, 0, v));
        return pcs::manifest_tool_exit(reps.data(), reps.size(), unreadable);
    };
    CHECK(code({0, 0}, false) == 0 && code({}, false) == 0 && code({0}, true) == 1 && code({0, 4}, false) == 1);
    CHECK(code({0, 1, 4}, false) == 3 && code({1}, true) == 3);
    CHECK(code({1, 2}, false) == 2 && code({3, 4}, true) == 2 && code({0, 3}, false) == 2);
}

}  // namespace

int main() {
    test_arguments();
    test_pack();
    test_verdict();
    test_summary();
    test_tool_text();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("manifest_scan_logic_test ok\n");
    return 0;
}
