// leaf_test.cpp — eloqstore::TryCheckLeaves / CheckLeaves through the C++ header
// (tests/test_gpu_leaf_check.py compares the output with tests/leaf_ref.py).
//   leaf_test PAGES PAGE_SIZE FP_FIRST TABLE ROOT0,ROOT1,... CLASSES|- MAX_LISTED
// PAGES, TABLE (u64 rows) and CLASSES (one byte per page; "-" scrubs the pages
// on the device) are raw files.  Prints every report field, the listed
// problems, a fold of the leaves and, of the tree check that ran first, its
// reached pages, its problems and a fold of its nodes.
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

    eloqstore::LeafReport r;
    const int rc = eloqstore::TryCheckLeaves(pages, P, fp_first, classes, table, roots, r, max_listed);
    if (rc != PCS_OK) {
        std::fprintf(stderr, "TryCheckLeaves failed (%d): %s\n", rc, pcs_last_error());
        return 2;
    }
    // the throwing form gives the same report
    const eloqstore::LeafReport r2 = eloqstore::CheckLeaves(pages, P, fp_first, classes, table, roots, max_listed);
    if (r2.n_entries != r.n_entries || r2.n_problems != r.n_problems || r2.problems.size() != r.problems.size() ||
        r2.leaves.size() != r.leaves.size() ||
        std::memcmp(r2.leaves.data(), r.leaves.data(), r.leaves.size() * sizeof(eloqstore::LeafNode)) != 0 ||
        std::memcmp(r2.tree.nodes.data(), r.tree.nodes.data(), r.tree.nodes.size() * sizeof(eloqstore::TreeNode)) != 0) {
        std::fprintf(stderr, "CheckLeaves and TryCheckLeaves disagree\n");
        return 3;
    }
#define FIELD(name) std::printf(#name " %" PRIu64 "\n", (uint64_t)r.name)
    FIELD(n_pages); FIELD(table_size); FIELD(n_data_pages); FIELD(n_data_ok); FIELD(n_entries);
    FIELD(n_overflow_values); FIELD(n_expiring); FIELD(n_compressed); FIELD(inline_value_bytes);
    FIELD(overflow_value_bytes); FIELD(n_refs); FIELD(n_out_of_range_refs); FIELD(n_extra_refs);
    FIELD(n_refs_to_tree); FIELD(n_misplaced_pointers); FIELD(n_chain_capped); FIELD(max_groups);
    FIELD(n_overflow_pages); FIELD(n_problems); FIELD(first_problem); FIELD(n_leaked_overflow); FIELD(n_overflow_ok);
#undef FIELD
    for (int k = 0; k < 9; ++k) std::printf("n_by_bit_%d %" PRIu64 "\n", k, r.n_by_bit[k]);
    for (const eloqstore::LeafProblem& p : r.problems)
        std::printf("problem %u %u %u %u\n", p.page_id, p.owner, p.bits, p.owner_entry);
    uint64_t fold = 0;
    for (const eloqstore::LeafNode& n : r.leaves) {
        const uint64_t w0 = (uint64_t)n.owner | (uint64_t)n.owner_entry << 32 | (uint64_t)n.bits << 48;
        fold = (fold * 0x9E3779B97F4A7C15ull + w0) * 0x9E3779B97F4A7C15ull + ((uint64_t)n.a | (uint64_t)n.b << 32);
    }
    std::printf("leaf_fold %" PRIu64 "\n", fold);
    std::printf("tree_n_reached %" PRIu64 "\ntree_n_problems %" PRIu64 "\ntree_n_data %" PRIu64 "\n", r.tree.n_reached,
                r.tree.n_problems, r.tree.n_data);
    for (const eloqstore::TreeProblem& p : r.tree.problems)
        std::printf("tree_problem %u %u %u %u\n", p.page_id, p.parent, p.bits, p.depth);
    fold = 0;
    for (const eloqstore::TreeNode& n : r.tree.nodes) {
        const uint64_t w0 = (uint64_t)n.parent | (uint64_t)n.depth << 32 | (uint64_t)n.tree << 40 |
                            (uint64_t)n.type << 48 | (uint64_t)n.bits << 56;
        fold = (fold * 0x9E3779B97F4A7C15ull + w0) * 0x9E3779B97F4A7C15ull + ((uint64_t)n.n_children | (uint64_t)n.n_bad_children << 32);
    }
    std::printf("node_fold %" PRIu64 "\n", fold);
    return 0;
}
