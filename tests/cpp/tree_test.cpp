// tree_test.cpp — eloqstore::TryCheckTree / CheckTree through the C++ header
// (tests/test_gpu_tree_check.py compares the output with tests/tree_ref.py).
//   tree_test PAGES PAGE_SIZE FP_FIRST TABLE ROOT0,ROOT1,... CLASSES|- MAX_LISTED
// PAGES, TABLE (u64 rows) and CLASSES (one byte per page; "-" scrubs the pages
// on the device) are raw files.  Prints every report field, the listed problems
// and a fold of the nodes.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "eloqstore/page_checksum.h"
#include "eloqstore_pcs.h"

static std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s PAGES PAGE_SIZE FP_FIRST TABLE ROOTS CLASSES|- MAX_LISTED\n", argv[0]);
        return 1;
    }
    const std::vector<uint8_t> pages = slurp(argv[1]), raw_table = slurp(argv[4]);
    const size_t P = std::strtoull(argv[2], nullptr, 10);
    const uint64_t fp_first = std::strtoull(argv[3], nullptr, 10);
    std::vector<uint64_t> table(raw_table.size() / 8), roots;
    std::memcpy(table.data(), raw_table.data(), table.size() * 8);
    for (char* tok = std::strtok(argv[5], ","); tok; tok = std::strtok(nullptr, ","))
        roots.push_back(std::strtoull(tok, nullptr, 10));
    std::vector<uint8_t> classes;
    if (std::strcmp(argv[6], "-") != 0) classes = slurp(argv[6]);
    const size_t max_listed = std::strtoull(argv[7], nullptr, 10);

    eloqstore::TreeReport r;
    const int rc = eloqstore::TryCheckTree(pages, P, fp_first, classes, table, roots, r, max_listed);
    if (rc != PCS_OK) {
        std::fprintf(stderr, "TryCheckTree failed (%d): %s\n", rc, pcs_last_error());
        return 2;
    }
    // the throwing form gives the same report
    const eloqstore::TreeReport r2 = eloqstore::CheckTree(pages, P, fp_first, classes, table, roots, max_listed);
    if (r2.n_reached != r.n_reached || r2.n_problems != r.n_problems || r2.problems.size() != r.problems.size() ||
        std::memcmp(r2.nodes.data(), r.nodes.data(), r.nodes.size() * sizeof(eloqstore::TreeNode)) != 0) {
        std::fprintf(stderr, "CheckTree and TryCheckTree disagree\n");
        return 3;
    }
#define FIELD(name) std::printf(#name " %" PRIu64 "\n", (uint64_t)r.name)
    FIELD(n_pages); FIELD(table_size); FIELD(n_mapped); FIELD(n_reached); FIELD(n_nonleaf); FIELD(n_leaf_index);
    FIELD(n_data); FIELD(n_refs); FIELD(n_extra_refs); FIELD(n_out_of_range_refs); FIELD(max_depth);
    FIELD(n_depth_capped); FIELD(n_problems); FIELD(first_problem); FIELD(n_unreached_mapped);
    FIELD(n_unreached_unread); FIELD(n_chain_heads);
#undef FIELD
    for (int k = 0; k < 8; ++k) std::printf("n_by_bit_%d %" PRIu64 "\n", k, r.n_by_bit[k]);
    for (int k = 0; k < 6; ++k) std::printf("unreached_by_type_%d %" PRIu64 "\n", k, r.unreached_by_type[k]);
    for (const eloqstore::TreeProblem& p : r.problems)
        std::printf("problem %u %u %u %u\n", p.page_id, p.parent, p.bits, p.depth);
    uint64_t fold = 0;
    for (const eloqstore::TreeNode& n : r.nodes) {
        const uint64_t w0 = (uint64_t)n.parent | (uint64_t)n.depth << 32 | (uint64_t)n.tree << 40 |
                            (uint64_t)n.type << 48 | (uint64_t)n.bits << 56;
        fold = (fold * 0x9E3779B97F4A7C15ull + w0) * 0x9E3779B97F4A7C15ull + ((uint64_t)n.n_children | (uint64_t)n.n_bad_children << 32);
    }
    std::printf("node_fold %" PRIu64 "\n", fold);
    return 0;
}
