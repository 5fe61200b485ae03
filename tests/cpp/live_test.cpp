// live_test — eloqstore::ReplayManifests / TryReplayManifests and ScrubLive /
// TryScrubLive through the C++ header (tests/test_gpu_scrub_live.py).
//   live_test <manifest_file> <max_rows> <fp_first> <class_bytes_file> <max_listed>
// replays the manifest, then asks which pages of the window the table points
// to, and prints every field as "name value" lines for the test to compare
// with tests/replay_ref.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <string_view>
#include <vector>

#include "eloqstore/page_checksum.h"

static std::string slurp(const char* path) {
    std::string out;
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(1);
    }
    char chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) out.append(chunk, got);
    std::fclose(f);
    return out;
}

#define SHOW(obj, field) std::printf(#field " %llu\n", (unsigned long long)(obj).field)

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: live_test <manifest> <max_rows> <fp_first> <class_bytes> <max_listed>\n");
        return 1;
    }
    const std::string image = slurp(argv[1]);
    const size_t max_rows = std::strtoull(argv[2], nullptr, 0);
    const uint64_t fp_first = std::strtoull(argv[3], nullptr, 0);
    const std::string classes = slurp(argv[4]);
    const size_t max_listed = std::strtoull(argv[5], nullptr, 0);

    const std::string_view images[1] = {image};
    eloqstore::ManifestsReplay bad;
    if (eloqstore::TryReplayManifests(images, bad, 100 /* not a power of two */) == 0) {
        std::fprintf(stderr, "an invalid align was accepted\n");
        return 1;
    }
    const eloqstore::ManifestsReplay rep = eloqstore::ReplayManifests(images, 4096, max_rows);
    const eloqstore::ManifestReplay& m = rep.manifests.at(0);
    std::printf("status %llu\n", (unsigned long long)m.status);
    SHOW(m, n_replayed);
    SHOW(m, malformed_record);
    SHOW(m, root);
    SHOW(m, ttl_root);
    SHOW(m, max_fp_id);
    SHOW(m, dict_bytes);
    SHOW(m, snapshot_pages);
    SHOW(m, n_log_entries);
    SHOW(m, table_size);
    SHOW(m, table_first);
    SHOW(m, n_mapped);
    SHOW(m, min_fp);
    SHOW(m, max_fp);
    SHOW(m, n_fp_beyond_max);
    SHOW(m, n_term_pairs);
    SHOW(rep, n_rows);
    std::printf("rows_written %zu\n", rep.table.size());
    std::printf("scan_verdict %llu\n", (unsigned long long)rep.scans.at(0).verdict);
    uint64_t fold = 0;
    for (uint64_t v : rep.table) fold = fold * 0x9E3779B97F4A7C15ull + v;
    std::printf("table_fold %llu\n", (unsigned long long)fold);

    const std::span<const uint8_t> cls(reinterpret_cast<const uint8_t*>(classes.data()), classes.size());
    eloqstore::LiveReport live;
    if (const int rc = eloqstore::TryScrubLive(cls, fp_first, rep.table, live, max_listed)) {
        std::fprintf(stderr, "TryScrubLive failed (%d): %s\n", rc, eloqstore::LastChecksumError());
        return 1;
    }
    SHOW(live, n_pages);
    SHOW(live, table_size);
    SHOW(live, n_mapped);
    SHOW(live, n_mapped_in_window);
    SHOW(live, n_duplicate);
    SHOW(live, live_ok);
    SHOW(live, live_blank);
    SHOW(live, live_corrupt);
    SHOW(live, dead_ok);
    SHOW(live, dead_blank);
    SHOW(live, dead_corrupt);
    SHOW(live, n_damaged);
    SHOW(live, first_damaged);
    SHOW(live, last_live);
    for (const eloqstore::LivePage& p : live.damaged)
        std::printf("damaged %llu %u %u\n", (unsigned long long)p.index, p.page_id, p.cls);
    uint64_t owners = 0;
    for (uint32_t o : live.owner) owners = owners * 0x9E3779B97F4A7C15ull + o;
    std::printf("owner_fold %llu\n", (unsigned long long)owners);
    return 0;
}
