// leaf_cpu_loop.cpp — the yardstick of tools/lab/leaf_rate.py: the tree check's
// and the leaf check's rules (csrc/tree_check.h, csrc/leaf_check.h: the very
// functions the kernels compile) as plain one-core host loops over the same
// bytes.  The walk orders differ from the device's (first come claims), the
// counts do not; leaf_rate.py compares them with the device's summaries.
//   make -C tools/lab "$PWD/tools/lab/libleaf_cpu_loop.so"
#include <cstdint>
#include <cstring>
#include <vector>

#include "leaf_check.h"
#include "tree_check.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

struct Window {
    const uint8_t* pages;
    uint64_t P, n_pages, fp_first;
    const uint8_t* cls;
    const uint64_t* table;
    uint64_t rows;
    // the first of UNMAPPED, ABSENT, BLANK, CORRUPT that applies to row c, else 0 and its page
    uint32_t readable(uint64_t c, const uint8_t*& pg) const {
        const uint64_t v = table[c];
        if ((v & 7) != 1) return PCS_TREE_UNMAPPED;
        const uint64_t fp = v >> 3;
        if (fp < fp_first || fp - fp_first >= n_pages || cls[fp - fp_first] > PCS_PAGE_BLANK) return PCS_TREE_ABSENT;
        if (cls[fp - fp_first] == PCS_PAGE_BLANK) return PCS_TREE_BLANK;
        if (cls[fp - fp_first] == PCS_PAGE_CORRUPT) return PCS_TREE_CORRUPT;
        pg = pages + (fp - fp_first) * P;
        return 0;
    }
};

}  // namespace

extern "C" {

// state[p]: 0 not reached, 1 reached, 2 reached as a data page with none of the six bits.
// out: n_reached, n_data (state 2 with sound sibling links), n_problems (any of the six bits, a bad child or a
// bad link), n_refs
void tree_cpu_loop(const uint8_t* pages, uint64_t P, uint64_t n_pages, uint64_t fp_first, const uint8_t* cls,
                   const uint64_t* table, uint64_t rows, const uint64_t* roots, uint32_t n_roots, uint8_t* state,
                   uint64_t* out) {
    const Window w{pages, P, n_pages, fp_first, cls, table, rows};
    std::memset(state, 0, rows);
    std::vector<uint8_t> ptype(rows, 0xFF), bad(rows, 0);
    std::vector<uint32_t> frontier, next;
    uint64_t n_reached = 0, n_refs = 0, n_problems = 0, n_data = 0;
    for (uint32_t t = 0; t < n_roots; ++t) {
        if (roots[t] >= kNone) continue;
        ++n_refs;
        if (roots[t] < rows && !state[roots[t]]) {
            state[roots[t]] = 1;
            frontier.push_back((uint32_t)roots[t]);
        }
    }
    for (uint32_t depth = 0; depth <= PCS_TREE_MAX_DEPTH && !frontier.empty(); ++depth) {
        next.clear();
        for (uint32_t c : frontier) {
            ++n_reached;
            const uint8_t* pg = nullptr;
            uint32_t bits = w.readable(c, pg);
            if (!bits) {
                const uint8_t type = pg[pcs::kTreeTypeOffset];
                if (!pcs::tree_type_fits(depth == 0, ptype[c], type)) {
                    bits = PCS_TREE_WRONG_TYPE;
                } else if (type == pcs::kTreeData) {
                    state[c] = 2;
                } else if (depth < PCS_TREE_MAX_DEPTH) {
                    uint64_t n = 0;
                    const bool ok = pcs::tree_index_decode(pg, (uint32_t)P, n, [&](uint32_t child) {
                        if (child >= rows) {
                            bits |= PCS_TREE_BAD_CHILD;
                        } else if (!state[child]) {
                            state[child] = 1;
                            ptype[child] = type;
                            next.push_back(child);
                        }
                    });
                    if (!ok) bits = PCS_TREE_MALFORMED;
                    n_refs += n;
                }
            }
            bad[c] = bits != 0;
        }
        frontier.swap(next);
    }
    for (uint64_t p = 0; p < rows; ++p) {  // the sibling links of the healthy data pages
        if (state[p] != 2) {
            n_problems += bad[p];
            continue;
        }
        const uint8_t* pg = nullptr;
        w.readable(p, pg);
        const uint32_t link[2] = {pcs::tree_le32(pg + pcs::kTreePrevOffset), pcs::tree_le32(pg + pcs::kTreeNextOffset)};
        bool good = true;
        for (int side = 0; side < 2; ++side) {
            const uint32_t q = link[side];
            if (q == kNone) continue;
            bool holds = false;
            if (q < rows && state[q] == 2) {
                const uint8_t* qg = nullptr;
                w.readable(q, qg);
                holds = pcs::tree_le32(qg + (side == 0 ? pcs::kTreeNextOffset : pcs::kTreePrevOffset)) == (uint32_t)p;
            }
            good = good && holds;
        }
        n_problems += !good;
        n_data += good;
    }
    out[0] = n_reached;
    out[1] = n_data;
    out[2] = n_problems;
    out[3] = n_refs;
}

// state is tree_cpu_loop's.  out: n_entries, n_overflow_values, n_refs, n_overflow_pages, n_problems,
// n_leaked_overflow, overflow_value_bytes, inline_value_bytes
void leaf_cpu_loop(const uint8_t* pages, uint64_t P, uint64_t n_pages, uint64_t fp_first, const uint8_t* cls,
                   const uint64_t* table, uint64_t rows, const uint8_t* state, uint64_t* out) {
    const Window w{pages, P, n_pages, fp_first, cls, table, rows};
    std::vector<uint64_t> key(rows, ~0ull);
    std::vector<uint32_t> refs(rows, 0);
    std::vector<uint16_t> bits(rows, 0);
    uint64_t n_entries = 0, n_values = 0, n_refs = 0, inline_bytes = 0;
    auto classify = [&](uint32_t c, uint32_t& V, uint32_t& n, const uint8_t*& pg) -> uint32_t {
        V = n = 0;
        if (const uint32_t b = w.readable(c, pg)) return b;
        if (pg[pcs::kTreeTypeOffset] != pcs::kLeafOverflow) return PCS_TREE_WRONG_TYPE;
        if (!pcs::leaf_overflow_page(pg, (uint32_t)P, V, n)) {
            V = n = 0;
            return PCS_TREE_MALFORMED;
        }
        return 0;
    };
    for (uint64_t p = 0; p < rows; ++p) {
        if (state[p] != 2) continue;
        const uint8_t* pg = nullptr;
        w.readable(p, pg);
        uint32_t dbits = 0;
        uint64_t n = 0;
        const bool ok = pcs::leaf_data_decode(pg, (uint32_t)P, n, [&](const pcs::LeafEntry& e) {
            if (!(e.flags & pcs::kLeafFlagOverflow)) {
                inline_bytes += e.value_len;
                return;
            }
            ++n_values;
            const uint64_t bid = p << 32 | (uint64_t)e.offset << 16;
            const uint8_t* group = pg + e.value_offset;
            uint32_t count = e.value_len / 4;
            for (uint32_t groups = 0; count; ++groups) {
                if (groups == PCS_LEAF_MAX_GROUPS) {
                    dbits |= PCS_LEAF_BAD_CHAIN;
                    break;
                }
                uint32_t next_count = 0;
                const uint8_t* next_group = nullptr;
                for (uint32_t j = 0; j < count; ++j) {
                    const uint32_t c = pcs::tree_le32(group + 4 * j);
                    ++n_refs;
                    if (c >= rows) {
                        dbits |= PCS_LEAF_BAD_POINTER;
                    } else if (state[c]) {
                        dbits |= PCS_LEAF_BAD_CHAIN;
                    } else {
                        if (bid < key[c]) key[c] = bid;
                        ++refs[c];
                        uint32_t V, nc;
                        const uint8_t* cg = nullptr;
                        const uint32_t cb = classify(c, V, nc, cg);
                        bits[c] = (uint16_t)cb;
                        if (cb || (nc && j + 1 != count)) {
                            dbits |= PCS_LEAF_BAD_CHAIN;
                        } else if (nc) {
                            next_count = nc;
                            next_group = cg + pcs::leaf_pointer_offset((uint32_t)P, nc);
                        }
                    }
                }
                count = next_count;
                group = next_group;
            }
        });
        if (!ok) dbits = PCS_TREE_MALFORMED;
        else n_entries += n;
        bits[p] = (uint16_t)dbits;
    }
    uint64_t n_overflow_pages = 0, n_problems = 0, n_leaked = 0, value_bytes = 0;
    for (uint64_t p = 0; p < rows; ++p) {
        if (state[p] == 2) {
            n_problems += bits[p] != 0;
        } else if (key[p] != ~0ull) {
            ++n_overflow_pages;
            uint32_t V, nc;
            const uint8_t* cg = nullptr;
            if (!classify((uint32_t)p, V, nc, cg)) value_bytes += V;
            n_problems += bits[p] != 0 || refs[p] > 1;
        } else if (!state[p]) {
            const uint8_t* pg = nullptr;
            if (!w.readable(p, pg) && pg[pcs::kTreeTypeOffset] == pcs::kLeafOverflow) ++n_leaked;
        }
    }
    out[0] = n_entries;
    out[1] = n_values;
    out[2] = n_refs;
    out[3] = n_overflow_pages;
    out[4] = n_problems;
    out[5] = n_leaked;
    out[6] = value_bytes;
    out[7] = inline_bytes;
}

}  // extern "C"
