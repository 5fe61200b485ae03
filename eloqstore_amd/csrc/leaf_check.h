// leaf_check.h — the page rules of the leaf check (pcs_leaf_check_dev /
// pcs_leaf_check_host, page_checksum_tool --leaves), as plain host + device
// C++ in the style of tree_check.h, whose tree_le16, tree_le32 and
// tree_varint32 it reuses.  The device kernels (leaf_check.hip) and the CPU
// logic test (tests/cpp/leaf_logic_test.cpp, ASAN + UBSan) compile the same
// functions.  No HIP calls here.
//
// Data page (include/storage/data_page.h:17-51; DataPageBuilder::Add / Finish,
// src/storage/data_page_builder.cpp:129-236; DataPageIter::ParseNextKey and
// DecodeEntry, src/storage/data_page.cpp:337-469), all integers little-endian,
// P the page size:
//   [0, 8) checksum | 8 type (2) | LE16 @9 content length C | LE32 @11 prev |
//   LE32 @15 next | entries from 19 | restart offsets o[0 .. R) as LE16 from
//   E = C - 2 (1 + R) | LE16 @(C - 2) = R | padding.
// An entry is
//   varint32 shared | varint32 non_shared | varint32 stored_len |
//   non_shared key bytes | (stored_len >> 4) value bytes |
//   [varint64 expire_ts iff stored_len & 2] | varint64 zig-zag timestamp delta
// and the low four bits of stored_len are ValLenBit: bit 0 overflow, bit 1
// expire, bits 2-3 the compression kind.  The value bytes of an overflow entry
// are n x LE32 logical page ids (WriteOverflowValue, src/tasks/
// batch_write_task.cpp:1334-1402; DecodeOverflowPointers, src/tasks/task.cpp:
// 208-239).
//
// The strict rule: 21 <= C <= P; E >= 19 (signed); R == 0 requires E == 19; R
// == 1 with o[0] == E == 19 is the builder's empty page and is well-formed;
// otherwise o[0] == 19, o[k] < o[k + 1] and o[R - 1] < E, and every region
// [o[k], o[k + 1]) (o[R] = E) is a whole number of entries, every varint inside
// its region (a varint32 at most 5 bytes, value mod 2^32; a varint64 at most 10
// bytes, value mod 2^64); shared == 0 in a region's first entry and <= the
// previous entry's shared + non_shared in the others; non_shared + value_len
// fits in what is left of the region; the compression bits are not 3 (the
// reference CHECKs that); an overflow entry has value_len % 4 == 0 and 4 <=
// value_len <= 512 (max_overflow_pointers = 128).  This is stricter than the
// iterator, which bounds an entry by the end of the entries and not by its
// region: the strict form is what lets a lane own a region.  On a page the
// builder wrote both yield the same entries.  A page that breaks any rule is
// malformed and yields no entry and no pointer.  No byte outside [0, P) is
// read, whatever the page holds.  Key order is not checked: the reference's
// comparator is pluggable, so order is no property of the page format.
//
// Overflow page (data_page.h:161-200, data_page.cpp:518-609):
//   [0, 8) checksum | 8 type (3) | LE16 @9 value length V | the value from 11 |
//   n LE32 pointers ending at P - 1 | byte P - 1 = n.
// The intrinsic rule: n <= 128 and 11 + V + 4 n + 1 <= P.  Whether a page that
// is not the last of its group is full is NOT checked: that depends on
// KvOptions::overflow_pointers, which no file records.
#pragma once

#include <stdint.h>

#include "eloqstore_pcs.h"
#include "tree_check.h"

namespace pcs {

constexpr uint32_t kLeafHeaderBytes = 19;   // checksum 8, type 1, content length 2, prev 4, next 4
constexpr uint32_t kLeafMinContent = 21;    // the header and the restart count
constexpr uint32_t kLeafMaxPointers = 128;  // max_overflow_pointers
constexpr uint8_t kLeafOverflow = 3;        // PageType::Overflow
constexpr uint32_t kLeafValueOffset = 11;   // of an overflow page
constexpr uint32_t kLeafFlagOverflow = 1, kLeafFlagExpire = 2, kLeafFlagCompression = 12;

// One entry of a data page as the strict rule decodes it.
struct LeafEntry {
    uint32_t offset;      // of its first byte in the page
    uint32_t shared, non_shared;
    uint32_t flags;       // stored_len & 15
    uint32_t key_offset, value_offset, value_len;
    uint64_t expire_ts;   // 0 without the expire bit
    uint64_t ts_raw;      // the zig-zag timestamp delta as stored
};

// The header of a data page of P bytes: false when it breaks the rule, else R
// and E.  Every restart offset lies inside the page: E + 2 R + 2 = C <= P.
PCS_TREE_HD inline bool leaf_data_header(const uint8_t* page, uint32_t P, uint32_t& R, uint32_t& E) {
    if (P < kLeafMinContent) return false;
    const uint32_t C = tree_le16(page + 9);
    if (C < kLeafMinContent || C > P) return false;
    R = tree_le16(page + C - 2);
    const int64_t e = (int64_t)C - 2 * (1 + (int64_t)R);
    if (e < (int64_t)kLeafHeaderBytes) return false;
    E = (uint32_t)e;
    if (R == 0 && E != kLeafHeaderBytes) return false;
    return true;
}

// Region k of a page whose header passed: false when its restart offset breaks
// the rule, else its bytes [lo, hi) (empty only on the builder's empty page).
PCS_TREE_HD inline bool leaf_region_bounds(const uint8_t* page, uint32_t R, uint32_t E, uint32_t k, uint32_t& lo,
                                           uint32_t& hi) {
    lo = tree_le16(page + E + 2 * k);
    hi = k + 1 < R ? tree_le16(page + E + 2 * (k + 1)) : E;
    if (k == 0 && lo != kLeafHeaderBytes) return false;
    if (R == 1 && E == kLeafHeaderBytes) return true;  // Finish() with no Add(): one restart, no entry
    return lo < hi && hi <= E;
}

// One varint64 inside [pos, hi): false when it does not end within 10 bytes and before hi.
PCS_TREE_HD inline bool leaf_varint64(const uint8_t* page, uint32_t& pos, uint32_t hi, uint64_t& value) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < 10; ++i) {
        if (pos >= hi) return false;
        const uint64_t b = page[pos++];
        v |= (b & 0x7Fu) << (7 * i);  // bits above 63 fall off: the value mod 2^64
        if (b < 0x80u) {
            value = v;
            return true;
        }
    }
    return false;
}

// The entry at pos of region [.., hi) whose previous entry had a key of key_len
// bytes (0 at the region's start): false when it breaks the rule, else the
// entry, and pos moves past it.
PCS_TREE_HD inline bool leaf_entry_decode(const uint8_t* page, uint32_t& pos, uint32_t hi, uint64_t key_len,
                                          LeafEntry& e) {
    uint32_t stored;
    e.offset = pos;
    if (!tree_varint32(page, pos, hi, e.shared) || !tree_varint32(page, pos, hi, e.non_shared) ||
        !tree_varint32(page, pos, hi, stored))
        return false;
    if (e.shared > key_len) return false;  // 0 in a region's first entry
    e.flags = stored & 15u;
    e.value_len = stored >> 4;
    if ((e.flags & kLeafFlagCompression) == kLeafFlagCompression) return false;
    if ((uint64_t)e.non_shared + e.value_len > hi - pos) return false;
    e.key_offset = pos;
    e.value_offset = pos + e.non_shared;
    pos = e.value_offset + e.value_len;
    if ((e.flags & kLeafFlagOverflow) &&
        (e.value_len % 4 || e.value_len < 4 || e.value_len > 4 * kLeafMaxPointers))
        return false;
    e.expire_ts = 0;
    if ((e.flags & kLeafFlagExpire) && !leaf_varint64(page, pos, hi, e.expire_ts)) return false;
    return leaf_varint64(page, pos, hi, e.ts_raw);
}

// The entries of region [lo, hi): emit(entry) for each, in order.  Returns the
// number of entries, or -1 when the region breaks the rule (entries may have
// been emitted by then: validate with a no-op emit first).
template <class Emit>
PCS_TREE_HD inline int64_t leaf_region_decode(const uint8_t* page, uint32_t lo, uint32_t hi, Emit&& emit) {
    uint32_t pos = lo;
    uint64_t key_len = 0;
    int64_t n = 0;
    LeafEntry e;
    while (pos < hi) {
        if (!leaf_entry_decode(page, pos, hi, key_len, e)) return -1;
        key_len = (uint64_t)e.shared + e.non_shared;
        emit(e);
        ++n;
    }
    return n;
}

// A whole data page, sequentially: false when malformed (nothing emitted), else
// emit(entry) for every entry in page order and n_entries = their number.
template <class Emit>
PCS_TREE_HD inline bool leaf_data_decode(const uint8_t* page, uint32_t P, uint64_t& n_entries, Emit&& emit) {
    uint32_t R, E, lo, hi;
    if (!leaf_data_header(page, P, R, E)) return false;
    for (uint32_t k = 0; k < R; ++k) {
        if (!leaf_region_bounds(page, R, E, k, lo, hi)) return false;
        if (leaf_region_decode(page, lo, hi, [](const LeafEntry&) {}) < 0) return false;
    }
    n_entries = 0;
    for (uint32_t k = 0; k < R; ++k) {
        leaf_region_bounds(page, R, E, k, lo, hi);
        n_entries += (uint64_t)leaf_region_decode(page, lo, hi, emit);
    }
    return true;
}

// The intrinsic rule of an overflow page of P >= 32 bytes whose type byte is 3:
// false when it breaks the rule, else V and n; pointer j is the LE32 at
// leaf_pointer_offset(P, n) + 4 j.
PCS_TREE_HD inline bool leaf_overflow_page(const uint8_t* page, uint32_t P, uint32_t& V, uint32_t& n) {
    n = page[P - 1];
    V = tree_le16(page + 9);
    return n <= kLeafMaxPointers && kLeafValueOffset + V + 4 * n + 1 <= P;
}
PCS_TREE_HD inline uint32_t leaf_pointer_offset(uint32_t P, uint32_t n) { return P - 1 - 4 * n; }

// ---- argument rules: nullptr when the arguments are acceptable ---------------
// The window, table and class conventions and the limits are the tree check's.
inline const char* leaf_args(const void* pages, uint64_t page_size, uint64_t n_pages, uint64_t fp_first,
                             const void* table, uint64_t table_size, const void* summary, const void* problems,
                             uint64_t problem_cap) {
    if (!summary) return "summary is null";
    if (page_size < 32 || page_size > 65535) return "page_size must be in [32, 65535]";
    if (n_pages && !pages) return "pages are null";
    if (table_size && !table) return "table is null";
    if (table_size > 0xFFFFFFFFull) return "table_size must be at most 2^32 - 1";
    if (problem_cap && !problems) return "problem list is null with problem_cap > 0";
    if (n_pages >= (1ull << 43)) return "too many pages";
    if (fp_first + n_pages < fp_first || fp_first + n_pages > (1ull << 61)) return "the window leaves the file page ids";
    return nullptr;
}

// ---- page_checksum_tool --leaves: text and exit code ----------------------------
inline void leaf_bit_names(uint32_t bits, char* out /* >= 112 bytes */) {
    static const char* const names[9] = {"unmapped", "absent", "blank", "corrupt", "wrong-type", "malformed",
                                         "bad-pointer", "bad-chain", "shared"};
    char* p = out;
    for (int b = 0; b < 9; ++b)
        if (bits >> b & 1) {
            if (p != out) *p++ = '+';
            for (const char* s = names[b]; *s; ++s) *p++ = *s;
        }
    *p = 0;
}
// 2 when a row is unmapped, corrupt, of the wrong type, malformed or has a bad
// pointer, or when a chain points into the tree, carries pointers in a page that
// is not the last of its group, or was cut at the cap, or when --tree would exit
// 2 (corruption beats a blank page); else 3 when a row is blank; else the exit
// code of --tree.  ABSENT, SHARED and leaked overflow pages never change the
// status.
inline int leaf_tool_exit(const pcs_leaf_summary& s, int tree_exit) {
    if (s.n_by_bit[0] || s.n_by_bit[3] || s.n_by_bit[4] || s.n_by_bit[5] || s.n_by_bit[6] || s.n_refs_to_tree ||
        s.n_misplaced_pointers || s.n_chain_capped || tree_exit == 2)
        return 2;
    if (s.n_by_bit[2]) return 3;
    return tree_exit;
}

}  // namespace pcs
