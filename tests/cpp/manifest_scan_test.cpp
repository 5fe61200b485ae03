// manifest_scan_test — eloqstore::TryScanManifests / ScanManifests
// (include/eloqstore/page_checksum.h) on manifest images built record by
// record at odd host addresses, checked against a walk made with the CPU
// oracle's ManifestBuilder::CalcChecksum.  Needs a GPU; run by
// tests/test_gpu_manifest_scan.py.
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
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

constexpr uint32_t kAlign = 4096;

void put32(std::string& s, size_t at, uint32_t v) { std::memcpy(s.data() + at, &v, 4); }

// Appends one record (header, payload, checksum, padding) as ManifestBuilder::Finalize does.
void append(std::string& img, uint32_t payload_len, uint32_t seed) {
    const size_t o = img.size();
    img.resize(o + 20 + payload_len);
    put32(img, o + 8, seed);
    put32(img, o + 12, seed * 3 + 1);
    put32(img, o + 16, payload_len);
    for (uint32_t b = 0; b < payload_len; ++b) img[o + 20 + b] = (char)((seed * 31 + b * 7 + (b >> 9)) & 0xFF);
    const uint64_t h = oracle_manifest_checksum(img.data() + o + 8, 12 + payload_len);
    std::memcpy(img.data() + o, &h, 8);
    img.resize((img.size() + kAlign - 1) / kAlign * kAlign, '\0');
}

struct Walked {
    std::vector<eloqstore::ManifestRecord> recs;
    uint64_t end_offset = 0;
    eloqstore::ManifestEnd reason = eloqstore::ManifestEnd::kClean;
};
Walked walk(std::string_view img) {
    Walked w;
    uint64_t o = 0;
    for (;;) {
        w.end_offset = o;
        if (o == img.size()) return w;
        if (img.size() - o < 20) return w.reason = eloqstore::ManifestEnd::kShortHeader, w;
        eloqstore::ManifestRecord r;
        r.offset = o;
        std::memcpy(&r.stored, img.data() + o, 8);
        std::memcpy(&r.root, img.data() + o + 8, 4);
        std::memcpy(&r.ttl_root, img.data() + o + 12, 4);
        std::memcpy(&r.payload_len, img.data() + o + 16, 4);
        const uint64_t e = o + 20 + (uint64_t)r.payload_len;
        if (e > img.size()) return w.reason = eloqstore::ManifestEnd::kShortPayload, w;
        r.computed = oracle_manifest_checksum(img.data() + o + 8, e - o - 8);
        r.ok = r.stored == r.computed;
        w.recs.push_back(r);
        o = (e + kAlign - 1) / kAlign * kAlign;
        if (o > img.size()) {
            w.end_offset = img.size();
            return w.reason = eloqstore::ManifestEnd::kShortPadding, w;
        }
    }
}

}  // namespace

int main() {
    using eloqstore::ManifestVerdict;
    // five manifests: clean with a 1.5 MiB snapshot, torn tail, broken, bad snapshot cut in its padding, empty
    std::vector<std::string> imgs(5);
    append(imgs[0], (3u << 19) + 77, 1);
    for (uint32_t k = 0; k < 5; ++k) append(imgs[0], 10 + 37 * k, 10 + k);
    for (uint32_t k = 0; k < 4; ++k) append(imgs[1], 300 + k, 20 + k);
    imgs[1][2 * kAlign + 25] ^= 1;
    imgs[1][3 * kAlign + 3] ^= 0x80;
    for (uint32_t k = 0; k < 4; ++k) append(imgs[2], 5000 + k, 30 + k);
    imgs[2][3 * kAlign + 100] ^= 4;  // record 1 spans slots 2 and 3
    append(imgs[3], 100, 40);
    imgs[3][9] ^= 1;
    imgs[3].resize(200);
    // held at odd addresses in plain memory
    std::vector<std::string> store(5);
    std::vector<std::string_view> views;
    for (size_t i = 0; i < 5; ++i) {
        store[i] = std::string(i + 1, 'x') + imgs[i];
        views.emplace_back(store[i].data() + i + 1, imgs[i].size());
    }

    eloqstore::ManifestsReport r;
    int rc = eloqstore::TryScanManifests(views, r);
    if (rc != PCS_OK) {
        std::fprintf(stderr, "TryScanManifests failed (%d): %s\n", rc, eloqstore::LastChecksumError());
        return 1;
    }
    CHECK(r.manifests.size() == 5);
    const ManifestVerdict want[5] = {ManifestVerdict::kClean, ManifestVerdict::kTornTail, ManifestVerdict::kBroken,
                                     ManifestVerdict::kBadSnapshot, ManifestVerdict::kEmpty};
    uint64_t first = 0;
    for (size_t i = 0; i < 5 && i < r.manifests.size(); ++i) {
        const Walked w = walk(views[i]);
        const eloqstore::ManifestReport& m = r.manifests[i];
        CHECK(m.verdict == want[i]);
        CHECK(m.size == views[i].size() && m.n_records == w.recs.size() && m.first_record == first);
        CHECK(m.end_offset == w.end_offset && m.end_reason == w.reason);
        uint64_t ok = 0, fc = UINT64_MAX, largest = 0;
        for (size_t k = 0; k < w.recs.size(); ++k) {
            ok += w.recs[k].ok;
            if (!w.recs[k].ok && fc == UINT64_MAX) fc = k;
            if (20 + (uint64_t)w.recs[k].payload_len > largest) largest = 20 + (uint64_t)w.recs[k].payload_len;
            CHECK(first + k < r.records.size() &&
                  std::memcmp(&r.records[first + k], &w.recs[k], sizeof(eloqstore::ManifestRecord)) == 0);
        }
        CHECK(m.n_ok == ok && m.n_corrupt == w.recs.size() - ok && m.first_corrupt == fc && m.max_record_bytes == largest);
        CHECK(m.valid_prefix_bytes == (fc == UINT64_MAX ? w.end_offset : w.recs[fc].offset));
        first += w.recs.size();
    }
    CHECK(r.n_records == first && r.records.size() == first && r.n_records == 6 + 4 + 4 + 1);
    CHECK(r.manifests[0].max_record_bytes == 20 + (3u << 19) + 77);
    CHECK(r.manifests[1].first_corrupt == 2 && r.manifests[1].valid_prefix_bytes == 2 * kAlign);
    CHECK(r.manifests[2].first_corrupt == 1 && r.manifests[2].n_ok_after_corrupt == 2);
    CHECK(r.manifests[3].end_reason == eloqstore::ManifestEnd::kShortPadding && r.manifests[3].end_offset == 200);
    CHECK(r.manifests[4].first_corrupt == UINT64_MAX && r.manifests[4].end_reason == eloqstore::ManifestEnd::kClean);
    for (int v = 0; v < 5; ++v) CHECK(r.n_by_verdict[v] == 1);
    CHECK(r.first_bad_manifest == 1 && r.n_corrupt == 2 + 1 + 1);

    // the aborting form with a small cap: counts stay full, the list is cut
    const eloqstore::ManifestsReport capped = eloqstore::ScanManifests(views, kAlign, 7);
    CHECK(capped.n_records == first && capped.records.size() == 7);
    CHECK(std::memcmp(capped.records.data(), r.records.data(), 7 * sizeof(eloqstore::ManifestRecord)) == 0);
    // no images; a bad alignment is refused, not aborted on
    const eloqstore::ManifestsReport none = eloqstore::ScanManifests(std::span<const std::string_view>());
    CHECK(none.manifests.empty() && none.n_records == 0 && none.first_bad_manifest == UINT64_MAX);
    CHECK(eloqstore::TryScanManifests(views, r, 100) == PCS_ERR_INVALID);
    CHECK(eloqstore::TryScanManifests(views, r, 32) == PCS_ERR_INVALID);

    if (g_fail) {
        std::fprintf(stderr, "manifest_scan_test: %d failures\n", g_fail);
        return 1;
    }
    std::printf("manifest_scan_test ok\n");
    return 0;
}
