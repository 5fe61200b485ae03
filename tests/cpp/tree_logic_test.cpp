// tree_logic_test.cpp — the tree check's page rules (csrc/tree_check.h) on the
// CPU, under ASAN + UBSan, with no HIP: the device kernel compiles the same
// functions.  Every page sits in a heap allocation of exactly its own size, so
// any read outside [0, P) is reported by the sanitizer.
//
//   tree_logic_test pages FILE P   decode every P-byte page of FILE: one line
//                                  per page, "ok c0 c1 ..." or "malformed", and
//                                  the fold of all of them
//   tree_logic_test fuzz N [SEED]  N generated pages (tests/tree_ref.py makes
//                                  the same ones from the same seeds): random
//                                  bytes, and well-formed pages with one to
//                                  three random byte edits, of 32, 64, 1000 and
//                                  4096 bytes; prints the fold of the verdicts
//                                  and children and the number of well-formed
//                                  pages
// In both modes every page is also decoded region by region, as the device
// does it (validate all, then emit all), and the two decodes must agree.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "tree_check.h"

namespace {

constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull;

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        s += kGold;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
};

void put_varint(std::vector<uint8_t>& out, uint64_t v) {
    while (v >= 0x80) {
        out.push_back((uint8_t)((v & 0x7F) | 0x80));
        v >>= 7;
    }
    out.push_back((uint8_t)v);
}
void put_le16(std::vector<uint8_t>& out, uint32_t v) {
    out.push_back((uint8_t)v);
    out.push_back((uint8_t)(v >> 8));
}

// A well-formed index page written straight in the format from the generator's draws.
std::vector<uint8_t> fuzz_writer(uint32_t P, Rng& rng) {
    std::vector<uint8_t> buf(15, 0);
    buf[8] = (uint8_t)(rng.next() & 1);
    const uint32_t leftmost = (uint32_t)(rng.next() % (1ull << 31));
    for (int k = 0; k < 4; ++k) buf[11 + k] = (uint8_t)(leftmost >> (8 * k));
    const uint64_t interval = 1 + rng.next() % 17, want = rng.next() % 48;
    std::vector<uint32_t> restarts{15};
    uint64_t counter = 0, prev_len = 0, added = 0;
    int64_t last_id = 0;
    for (uint64_t e = 0; e < want; ++e) {
        const uint64_t a = rng.next();
        const uint64_t key_len = (a & 15) == 0 ? 1 + (a >> 8) % 200 : 1 + (a >> 8) % 12;
        const bool restart = counter >= interval;
        const uint64_t b = rng.next();
        const uint64_t shared = restart ? 0 : b % (std::min(prev_len, key_len - 1) + 1);
        const uint64_t non_shared = key_len - shared;
        const int64_t page_id = (int64_t)(rng.next() % (1ull << 31));
        std::vector<uint8_t> entry;
        put_varint(entry, shared);
        put_varint(entry, non_shared);
        uint64_t c = 0;
        for (uint64_t j = 0; j < non_shared; ++j) {
            if (j % 8 == 0) c = rng.next();
            entry.push_back((uint8_t)(c >> (8 * (j % 8))));
        }
        const int64_t delta = page_id - (restart ? 0 : last_id);
        put_varint(entry, delta >= 0 ? (uint64_t)delta << 1 : ((uint64_t)-delta << 1) | 1);
        if (buf.size() + entry.size() + 2 * (restarts.size() + (restart ? 1 : 0)) + 2 > P) break;
        if (restart) {
            restarts.push_back((uint32_t)buf.size());
            counter = 0;
        }
        buf.insert(buf.end(), entry.begin(), entry.end());
        prev_len = key_len;
        last_id = page_id;
        ++counter;
        ++added;
    }
    if (added == 0) restarts.clear();
    for (uint32_t r : restarts) put_le16(buf, r);
    put_le16(buf, (uint32_t)restarts.size());
    buf[9] = (uint8_t)buf.size();
    buf[10] = (uint8_t)(buf.size() >> 8);
    buf.resize(P, 0);
    return buf;
}

struct Folder {
    uint64_t fold = 0, n_ok = 0, n_pages = 0;
    bool print = false;

    // `bytes` is copied into a heap block of exactly P bytes and decoded there, twice.
    bool page(const uint8_t* bytes, uint32_t P) {
        std::unique_ptr<uint8_t[]> heap(new uint8_t[P]);
        std::memcpy(heap.get(), bytes, P);
        const uint8_t* p = heap.get();
        std::vector<uint32_t> seq, par;
        uint64_t n_children = 0;
        const bool ok = pcs::tree_index_decode(p, P, n_children, [&](uint32_t c) { seq.push_back(c); });
        // the device's order of work: the header, every region validated, then every region emitted
        uint32_t R = 0, E = 0, lo = 0, hi = 0;
        bool ok2 = pcs::tree_index_header(p, P, R, E);
        for (uint32_t k = 0; ok2 && k < R; ++k)
            ok2 = pcs::tree_region_bounds(p, R, E, R - 1 - k, lo, hi) &&
                  pcs::tree_region_decode(p, lo, hi, [](uint32_t) {}) >= 0;
        if (ok2) {
            par.push_back(pcs::tree_le32(p + pcs::kTreeLeftmostOffset));
            for (uint32_t k = 0; k < R; ++k) {
                pcs::tree_region_bounds(p, R, E, k, lo, hi);
                pcs::tree_region_decode(p, lo, hi, [&](uint32_t c) { par.push_back(c); });
            }
        }
        if (ok != ok2 || (ok && (seq != par || n_children != seq.size())) || (!ok && !seq.empty())) {
            std::fprintf(stderr, "page %llu: the sequential and the region-wise decode disagree\n",
                         (unsigned long long)n_pages);
            return false;
        }
        fold = fold * kGold + (ok ? 1 + seq.size() : 0);
        for (uint32_t c : seq) fold = fold * kGold + c;
        n_ok += ok;
        ++n_pages;
        if (print) {
            if (!ok) {
                std::printf("malformed\n");
            } else {
                std::printf("ok");
                for (uint32_t c : seq) std::printf(" %u", c);
                std::printf("\n");
            }
        }
        return true;
    }
};

int run_pages(const char* path, uint32_t P) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        return 1;
    }
    Folder folder;
    folder.print = true;
    std::vector<uint8_t> buf(P);
    while (std::fread(buf.data(), 1, P, f) == P)
        if (!folder.page(buf.data(), P)) return 1;
    std::fclose(f);
    std::printf("fold %llu ok %llu pages %llu\n", (unsigned long long)folder.fold, (unsigned long long)folder.n_ok,
                (unsigned long long)folder.n_pages);
    return 0;
}

int run_fuzz(uint64_t n, uint64_t seed) {
    static const uint32_t sizes[4] = {32, 64, 1000, 4096};
    Folder folder;
    for (uint64_t t = 0; t < n; ++t) {
        Rng rng{(seed + t) * 0xD6E8FEB86659FD93ull};
        const uint32_t P = sizes[t % 4];
        std::vector<uint8_t> page;
        if (((t >> 2) & 1) == 0) {
            page.resize((P + 7) / 8 * 8);
            for (uint32_t w = 0; w < page.size() / 8; ++w) {
                const uint64_t z = rng.next();
                for (int k = 0; k < 8; ++k) page[8 * w + k] = (uint8_t)(z >> (8 * k));
            }
            page.resize(P);
        } else {
            page = fuzz_writer(P, rng);
            const uint64_t edits = 1 + rng.next() % 3;
            for (uint64_t k = 0; k < edits; ++k) {
                const uint64_t pos = rng.next() % P;
                page[pos] = (uint8_t)(rng.next() & 0xFF);
            }
        }
        if (!folder.page(page.data(), P)) return 1;
    }
    std::printf("fold %llu ok %llu pages %llu\n", (unsigned long long)folder.fold, (unsigned long long)folder.n_ok,
                (unsigned long long)folder.n_pages);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "pages") return run_pages(argv[2], (uint32_t)std::strtoul(argv[3], nullptr, 10));
    if (argc >= 3 && std::string(argv[1]) == "fuzz")
        return run_fuzz(std::strtoull(argv[2], nullptr, 10), argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 20240607ull);
    std::fprintf(stderr, "usage: %s pages FILE P | fuzz N [SEED]\n", argv[0]);
    return 1;
}
