// leaf_logic_test.cpp — the leaf check's page rules (csrc/leaf_check.h) on the
// CPU, under ASAN + UBSan, with no HIP: the device kernel compiles the same
// functions.  Every page sits in a heap allocation of exactly its own size, so
// any read outside [0, P) is reported by the sanitizer.
//
//   leaf_logic_test pages FILE P   decode every P-byte page of FILE as a data
//                                  page: one line per page, "ok off/flags/len
//                                  ..." (entry offset, ValLenBit flags, value
//                                  length) or "malformed", and the fold of all
//                                  of them
//   leaf_logic_test fuzz N [SEED]  N generated pages (tests/leaf_ref.py makes
//                                  the same ones from the same seeds): random
//                                  bytes, and well-formed pages with zero to
//                                  two random byte edits, of 32, 64, 1000 and
//                                  4096 bytes; prints the fold of the verdicts
//                                  and entries and the number of well-formed
//                                  pages
// In both modes every page is also decoded region by region, as the device
// does it (validate all, last region first, then walk entry by entry without
// the previous key's length), and the two decodes must agree.  Every page is
// also put to the intrinsic overflow-page rule, whose pointers are then read.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "leaf_check.h"

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

// A well-formed data page written straight in the format from the generator's draws.
std::vector<uint8_t> fuzz_writer(uint32_t P, Rng& rng) {
    std::vector<uint8_t> buf(19, 0);
    buf[8] = 2;
    const uint64_t interval = 1 + rng.next() % 17, want = rng.next() % 48;
    std::vector<uint32_t> restarts{19};
    uint64_t counter = 0, prev_len = 0;
    for (uint64_t n = 0; n < want; ++n) {
        const uint64_t a = rng.next();
        const uint64_t key_len = (a & 15) == 0 ? 1 + (a >> 8) % 200 : 1 + (a >> 8) % 12;
        const bool restart = counter >= interval;
        const uint64_t b = rng.next();
        const uint64_t shared = restart ? 0 : b % (std::min(prev_len, key_len - 1) + 1);
        const uint64_t non_shared = key_len - shared;
        const uint64_t c = rng.next();
        const uint64_t flags = ((c & 7) == 0 ? 1 : 0) | ((c >> 3) & 1 ? 2 : 0) | (((c >> 4) % 3) << 2);
        uint64_t vlen;
        if (flags & 1) vlen = ((c >> 6) & 3) == 0 ? 4 * (1 + (c >> 8) % 128) : 4 * (1 + (c >> 8) % 4);
        else vlen = (c >> 8) % 40;
        std::vector<uint8_t> e;
        put_varint(e, shared);
        put_varint(e, non_shared);
        put_varint(e, vlen << 4 | flags);
        uint64_t d = 0;
        for (uint64_t j = 0; j < non_shared + vlen; ++j) {
            if (j % 8 == 0) d = rng.next();
            e.push_back((uint8_t)(d >> (8 * (j % 8))));
        }
        if (flags & 2) {
            const uint64_t x = rng.next();
            put_varint(e, x >> (x & 63));
        }
        const uint64_t t = rng.next();
        put_varint(e, t >> (t & 63));
        if (buf.size() + e.size() + 2 * (restarts.size() + (restart ? 1 : 0)) + 2 > P) break;
        if (restart) {
            restarts.push_back((uint32_t)buf.size());
            counter = 0;
        }
        buf.insert(buf.end(), e.begin(), e.end());
        prev_len = key_len;
        ++counter;
    }
    for (uint32_t r : restarts) put_le16(buf, r);
    put_le16(buf, (uint32_t)restarts.size());
    buf[9] = (uint8_t)buf.size();
    buf[10] = (uint8_t)(buf.size() >> 8);
    buf.resize(P, 0);
    return buf;
}

bool same(const pcs::LeafEntry& a, const pcs::LeafEntry& b) {
    return a.offset == b.offset && a.flags == b.flags && a.value_offset == b.value_offset &&
           a.value_len == b.value_len && a.expire_ts == b.expire_ts && a.ts_raw == b.ts_raw &&
           a.non_shared == b.non_shared && a.shared == b.shared;
}

struct Folder {
    uint64_t fold = 0, n_ok = 0, n_pages = 0, pointer_sum = 0;
    bool print = false;

    // `bytes` is copied into a heap block of exactly P bytes and decoded there, twice.
    bool page(const uint8_t* bytes, uint32_t P) {
        std::unique_ptr<uint8_t[]> heap(new uint8_t[P]);
        std::memcpy(heap.get(), bytes, P);
        const uint8_t* p = heap.get();
        std::vector<pcs::LeafEntry> seq, par;
        uint64_t n_entries = 0;
        const bool ok = pcs::leaf_data_decode(p, P, n_entries, [&](const pcs::LeafEntry& e) { seq.push_back(e); });
        // the device's order of work: the header, every region validated, then every region walked
        uint32_t R = 0, E = 0, lo = 0, hi = 0;
        bool ok2 = pcs::leaf_data_header(p, P, R, E);
        for (uint32_t k = 0; ok2 && k < R; ++k)
            ok2 = pcs::leaf_region_bounds(p, R, E, R - 1 - k, lo, hi) &&
                  pcs::leaf_region_decode(p, lo, hi, [](const pcs::LeafEntry&) {}) >= 0;
        if (ok2) {
            for (uint32_t k = 0; k < R; ++k) {
                pcs::leaf_region_bounds(p, R, E, k, lo, hi);
                uint32_t pos = lo;
                pcs::LeafEntry e;
                while (pos < hi && pcs::leaf_entry_decode(p, pos, hi, ~0ull, e)) par.push_back(e);
                if (pos != hi) ok2 = false;
            }
        }
        bool agree = ok == ok2 && (ok || seq.empty()) && (!ok || (n_entries == seq.size() && seq.size() == par.size()));
        for (size_t k = 0; agree && ok && k < seq.size(); ++k) agree = same(seq[k], par[k]);
        if (!agree) {
            std::fprintf(stderr, "page %llu: the sequential and the region-wise decode disagree\n",
                         (unsigned long long)n_pages);
            return false;
        }
        // every value and, for an overflow entry, every pointer lies in the page: read them
        for (const pcs::LeafEntry& e : seq)
            for (uint32_t j = 0; j < e.value_len; ++j) pointer_sum += p[e.value_offset + j];
        // the same bytes as an overflow page
        uint32_t V = 0, n = 0;
        if (P >= 32 && pcs::leaf_overflow_page(p, P, V, n)) {
            for (uint32_t j = 0; j < n; ++j) pointer_sum += pcs::tree_le32(p + pcs::leaf_pointer_offset(P, n) + 4 * j);
            for (uint32_t j = 0; j < V; ++j) pointer_sum += p[pcs::kLeafValueOffset + j];
        }
        fold = fold * kGold + (ok ? 1 + seq.size() : 0);
        for (const pcs::LeafEntry& e : seq) {
            const uint64_t f[8] = {e.offset, e.shared, e.non_shared, e.flags, e.value_offset, e.value_len, e.expire_ts,
                                   e.ts_raw};
            for (uint64_t x : f) fold = fold * kGold + x;
        }
        n_ok += ok;
        ++n_pages;
        if (print) {
            if (!ok) {
                std::printf("malformed\n");
            } else {
                std::printf("ok");
                for (const pcs::LeafEntry& e : seq) std::printf(" %u/%u/%u", e.offset, e.flags, e.value_len);
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
        if (((t >> 2) & 3) == 0) {
            page.resize((P + 7) / 8 * 8);
            for (uint32_t w = 0; w < page.size() / 8; ++w) {
                const uint64_t z = rng.next();
                for (int k = 0; k < 8; ++k) page[8 * w + k] = (uint8_t)(z >> (8 * k));
            }
            page.resize(P);
        } else {
            page = fuzz_writer(P, rng);
            const uint64_t edits = rng.next() % 3;
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
        return run_fuzz(std::strtoull(argv[2], nullptr, 10), argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 20250311ull);
    std::fprintf(stderr, "usage: %s pages FILE P | fuzz N [SEED]\n", argv[0]);
    return 1;
}
