// replay_cpu_loop — the honest alternative to pcs_manifest_replay_dev and
// pcs_scrub_live_dev for tools/lab/replay_rate.py: the images (or the class
// bytes and the table) copied to the host and a plain one-core loop of the same
// rules (include/eloqstore_pcs.h).  Lab code: it trusts the record headers as
// the device scan has already verified them, and takes no checksum.
//   g++ -O3 -std=c++20 -shared -fPIC replay_cpu_loop.cpp -o libreplay_cpu_loop.so
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

bool varint(const uint8_t* p, uint64_t end, uint64_t& pos, int limit, uint64_t& v) {
    v = 0;
    for (int n = 0; n < limit; ++n) {
        if (pos >= end) return false;
        const uint8_t b = p[pos++];
        v |= (uint64_t)(b & 0x7F) << (7 * n);
        if (b < 0x80) return true;
    }
    return false;
}

uint32_t le32(const uint8_t* p) {
    uint32_t v;
    std::memcpy(&v, p, 4);
    return v;
}

bool term(const uint8_t* p, uint64_t pos, uint64_t end) {
    uint64_t n = 0, v;
    while (pos < end) {
        if (!varint(p, end, pos, 10, v)) return false;
        ++n;
    }
    return n % 2 == 0;
}

}  // namespace

extern "C" {

// One image -> table (grown as needed), out[0..4) = status (0 ok, 2 malformed), table_size, max_fp_id, n_mapped.
int replay_cpu(const uint8_t* img, uint64_t size, uint32_t align, uint64_t* out) {
    std::vector<uint64_t> table;
    uint64_t o = 0, k = 0, max_fp = 0;
    out[0] = 2;
    while (size - o >= 20) {
        const uint64_t L = le32(img + o + 16);
        if (o + 20 + L > size) break;
        const uint8_t* p = img + o + 20;
        uint64_t pos = 0;
        if (k == 0) {
            uint64_t dict;
            if (!varint(p, L, pos, 10, max_fp) || !varint(p, L, pos, 5, dict)) return 1;
            dict &= 0xFFFFFFFFull;
            if (dict > L - pos) return 1;
            pos += dict;
        }
        const uint64_t rem = L - pos;
        if (rem < 8) return 1;
        const uint64_t mlen = le32(p + pos);
        if (mlen + 8 > rem) return 1;
        const uint64_t mend = pos + 4 + mlen;
        uint64_t q = pos + 4, v, pid;
        if (k == 0) {
            while (q < mend) {
                if (!varint(p, mend, q, 10, v)) return 1;
                table.push_back(v);
            }
        } else {
            while (q < mend) {
                if (!varint(p, mend, q, 5, pid) || q >= mend || !varint(p, mend, q, 10, v)) return 1;
                pid &= 0xFFFFFFFFull;
                if (pid >= table.size()) table.resize(pid + 1, 7);
                table[pid] = v;
                if ((v & 7) == 1 && (v >> 3) + 1 > max_fp) max_fp = (v >> 3) + 1;
            }
        }
        const uint64_t tlen = le32(p + mend);
        if (tlen > rem - mlen - 8 || !term(p, mend + 4, mend + 4 + tlen)) return 1;
        ++k;
        o = (o + 20 + L + align - 1) / align * align;
        if (o > size) break;
    }
    uint64_t mapped = 0;
    for (uint64_t v : table) mapped += (v & 7) == 1;
    out[0] = 0;
    out[1] = table.size();
    out[2] = max_fp;
    out[3] = mapped;
    return 0;
}

// owner[i] and out[0..8) = n_mapped, in window, live ok/blank/corrupt, dead ok/blank/corrupt
void live_cpu(const uint8_t* cls, uint64_t n, uint64_t fp_first, const uint64_t* table, uint64_t rows, uint32_t* owner,
              uint64_t* out) {
    std::memset(owner, 0xFF, n * 4);
    std::memset(out, 0, 8 * 8);
    for (uint64_t p = 0; p < rows; ++p) {
        const uint64_t v = table[p];
        if ((v & 7) != 1) continue;
        ++out[0];
        const uint64_t id = v >> 3;
        if (id < fp_first || id - fp_first >= n) continue;
        ++out[1];
        if (p < owner[id - fp_first]) owner[id - fp_first] = (uint32_t)p;
    }
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t c = cls[i];
        if (c > 2) continue;
        out[(owner[i] != 0xFFFFFFFFu ? 2 : 5) + (c == 1 ? 0 : c == 2 ? 1 : 2)]++;
    }
}

}  // extern "C"
