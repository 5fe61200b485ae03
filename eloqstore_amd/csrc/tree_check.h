// tree_check.h — the page rules of the tree check (pcs_tree_check_dev /
// pcs_tree_check_host, page_checksum_tool --tree), as plain host + device C++.
// The device kernels (tree_check.hip) and the CPU logic test
// (tests/cpp/tree_logic_test.cpp, ASAN + UBSan) compile the same functions.
// No HIP calls here.
//
// Index page (IndexPageBuilder, src/storage/index_page_builder.cpp:44-204;
// IndexPageIter::ParseNextKey / DecodeEntry, src/storage/mem_index_page.cpp:
// 134-233; EncodeInt32Delta / DecodeInt32Delta, include/coding.h:161-192), all
// integers little-endian, P the page size:
//   [0, 8) checksum | 8 type (0 NonLeafIndex, 1 LeafIndex) | LE16 @9 content
//   length C | LE32 @11 leftmost child | entries from 15 | restart offsets
//   o[0 .. R) as LE16 from E = C - 2 (1 + R) | LE16 @(C - 2) = R | padding.
// The strict rule: 17 <= C <= P; E >= 15 (signed); R == 0 requires E == 15;
// otherwise o[0] == 15, o[k] < o[k + 1] and o[R - 1] < E, and every region
// [o[k], o[k + 1]) (o[R] = E) is a whole number of entries
//   varint32 shared | varint32 non_shared | non_shared key bytes | varint32 v
// each varint at most 5 bytes and inside the region, value mod 2^32; shared ==
// 0 in a region's first entry and <= the previous entry's shared + non_shared
// in the others; delta = (v & 1) ? -(v >> 1) : (v >> 1); the child id is delta
// in a region's first entry and previous id + delta otherwise, and lies in
// [0, INT32_MAX].  A page that breaks any rule is malformed and yields no
// child at all.  No byte outside [0, P) is read, whatever the page holds.
//
// Regions decode independently of one another (tree_region_bounds +
// tree_region_decode: one lane per region on the device), so a page is decoded
// in two passes: every region validated, then every region emitted.
//
// Data page (include/storage/data_page.h:26-51): type 2, LE32 @11 previous and
// LE32 @15 next sibling; nothing else of it is read.
#pragma once

#include <stdint.h>

#include "eloqstore_pcs.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCS_TREE_HD __host__ __device__
#else
#define PCS_TREE_HD
#endif

namespace pcs {

constexpr uint32_t kTreeHeaderBytes = 15;    // checksum 8, type 1, content length 2, leftmost child 4
constexpr uint32_t kTreeMinContent = 17;     // the header and the restart count
constexpr uint32_t kTreeNoPage = 0xFFFFFFFFu;
constexpr uint32_t kTreeTypeOffset = 8, kTreeLeftmostOffset = 11, kTreePrevOffset = 11, kTreeNextOffset = 15;
constexpr uint8_t kTreeNonLeaf = 0, kTreeLeafIndex = 1, kTreeData = 2;
constexpr uint32_t kTreeSixBits = PCS_TREE_UNMAPPED | PCS_TREE_ABSENT | PCS_TREE_BLANK | PCS_TREE_CORRUPT |
                                  PCS_TREE_WRONG_TYPE | PCS_TREE_MALFORMED;

PCS_TREE_HD inline uint32_t tree_le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
PCS_TREE_HD inline uint32_t tree_le32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// The header of an index page of P bytes: false when it breaks the rule, else R
// and E.  With R > 0 every restart offset lies inside the page: E + 2 R + 2 = C <= P.
PCS_TREE_HD inline bool tree_index_header(const uint8_t* page, uint32_t P, uint32_t& R, uint32_t& E) {
    if (P < kTreeMinContent) return false;
    const uint32_t C = tree_le16(page + 9);
    if (C < kTreeMinContent || C > P) return false;
    R = tree_le16(page + C - 2);
    const int64_t e = (int64_t)C - 2 * (1 + (int64_t)R);
    if (e < (int64_t)kTreeHeaderBytes) return false;
    E = (uint32_t)e;
    if (R == 0 && E != kTreeHeaderBytes) return false;
    return true;
}

// Region k of a page whose header passed: false when its restart offset breaks
// the rule, else its bytes [lo, hi).  All R calls together check the whole array.
PCS_TREE_HD inline bool tree_region_bounds(const uint8_t* page, uint32_t R, uint32_t E, uint32_t k, uint32_t& lo,
                                           uint32_t& hi) {
    lo = tree_le16(page + E + 2 * k);
    hi = k + 1 < R ? tree_le16(page + E + 2 * (k + 1)) : E;
    if (k == 0 && lo != kTreeHeaderBytes) return false;
    return lo < hi && hi <= E;
}

// One varint32 inside [pos, hi): false when it does not end within 5 bytes and before hi.
PCS_TREE_HD inline bool tree_varint32(const uint8_t* page, uint32_t& pos, uint32_t hi, uint32_t& value) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < 5; ++i) {
        if (pos >= hi) return false;
        const uint32_t b = page[pos++];
        v |= (b & 0x7Fu) << (7 * i);  // bits above 31 fall off: the value mod 2^32
        if (b < 0x80u) {
            value = v;
            return true;
        }
    }
    return false;
}

// The entries of region [lo, hi): emit(child id) for each, in order.  Returns
// the number of entries, or -1 when the region breaks the rule (children may
// have been emitted by then: validate with a no-op emit first).
template <class Emit>
PCS_TREE_HD inline int64_t tree_region_decode(const uint8_t* page, uint32_t lo, uint32_t hi, Emit&& emit) {
    uint32_t pos = lo;
    uint64_t key_len = 0;
    int64_t id = 0, n = 0;
    while (pos < hi) {
        uint32_t shared, non_shared, v;
        if (!tree_varint32(page, pos, hi, shared) || !tree_varint32(page, pos, hi, non_shared)) return -1;
        if (shared > key_len) return -1;  // 0 in a region's first entry
        if (non_shared > hi - pos) return -1;
        pos += non_shared;
        if (!tree_varint32(page, pos, hi, v)) return -1;
        const int64_t delta = (v & 1) ? -(int64_t)(v >> 1) : (int64_t)(v >> 1);
        id = n ? id + delta : delta;
        if (id < 0 || id > (int64_t)INT32_MAX) return -1;
        key_len = (uint64_t)shared + non_shared;
        emit((uint32_t)id);
        ++n;
    }
    return n;
}

// A whole index page, sequentially: false when malformed (nothing emitted),
// else emit(child) for the leftmost pointer and every entry in page order and
// n_children = their number.
template <class Emit>
PCS_TREE_HD inline bool tree_index_decode(const uint8_t* page, uint32_t P, uint64_t& n_children, Emit&& emit) {
    uint32_t R, E, lo, hi;
    if (!tree_index_header(page, P, R, E)) return false;
    for (uint32_t k = 0; k < R; ++k) {
        if (!tree_region_bounds(page, R, E, k, lo, hi)) return false;
        if (tree_region_decode(page, lo, hi, [](uint32_t) {}) < 0) return false;
    }
    n_children = 1;
    emit(tree_le32(page + kTreeLeftmostOffset));
    for (uint32_t k = 0; k < R; ++k) {
        tree_region_bounds(page, R, E, k, lo, hi);
        n_children += (uint64_t)tree_region_decode(page, lo, hi, emit);
    }
    return true;
}

// Which page types fit below a parent of type parent_type (a root: is_root).
PCS_TREE_HD inline bool tree_type_fits(bool is_root, uint8_t parent_type, uint8_t type) {
    if (is_root || parent_type == kTreeNonLeaf) return type == kTreeNonLeaf || type == kTreeLeafIndex;
    return type == kTreeData;
}

// The scrub's six type buckets: types 0..3, 255 (Deleted), anything else.
PCS_TREE_HD inline uint32_t tree_type_bucket(uint8_t type) { return type < 4 ? type : type == 255 ? 4 : 5; }

// ---- argument rules: nullptr when the arguments are acceptable ---------------
inline const char* tree_args(const void* pages, uint64_t page_size, uint64_t n_pages, uint64_t fp_first,
                             const void* table, uint64_t table_size, const void* roots, uint32_t n_roots,
                             const void* summary, const void* problems, uint64_t problem_cap) {
    if (!summary) return "summary is null";
    if (page_size < 32 || page_size > 65535) return "page_size must be in [32, 65535]";
    if (n_pages && !pages) return "pages are null";
    if (table_size && !table) return "table is null";
    if (table_size > 0xFFFFFFFFull) return "table_size must be at most 2^32 - 1";
    if (n_roots < 1 || n_roots > 8) return "n_roots must be in [1, 8]";
    if (!roots) return "roots are null";
    if (problem_cap && !problems) return "problem list is null with problem_cap > 0";
    if (n_pages >= (1ull << 43)) return "too many pages";
    if (fp_first + n_pages < fp_first || fp_first + n_pages > (1ull << 61)) return "the window leaves the file page ids";
    return nullptr;
}

// ---- page_checksum_tool --tree: text and exit code ------------------------------
inline void tree_bit_names(uint32_t bits, char* out /* >= 96 bytes */) {
    static const char* const names[8] = {"unmapped", "absent", "blank", "corrupt", "wrong-type", "malformed",
                                         "bad-child", "bad-link"};
    char* p = out;
    for (int b = 0; b < 8; ++b)
        if (bits >> b & 1) {
            if (p != out) *p++ = '+';
            for (const char* s = names[b]; *s; ++s) *p++ = *s;
        }
    *p = 0;
}
// 2 when a reached page is corrupt, malformed, of the wrong type, unmapped or has
// a bad child; else 3 when a reached page is blank; else 0.  ABSENT and BAD_LINK
// never change the status.
inline int tree_tool_exit(const pcs_tree_summary& s) {
    if (s.n_by_bit[0] || s.n_by_bit[3] || s.n_by_bit[4] || s.n_by_bit[5] || s.n_by_bit[6]) return 2;
    return s.n_by_bit[2] ? 3 : 0;
}

}  // namespace pcs
