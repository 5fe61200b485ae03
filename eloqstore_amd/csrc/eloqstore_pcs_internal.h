// eloqstore_pcs_internal.h — launch entry points shared by the C ABI
// (pcs_capi.cpp) and the kernels (pcs_kernels.hip).  Not installed.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pcs {

// mode: 0 digest, 1 validate, 2 stamp.  algo: 0 XXH3-64, 1 XXH64.
// Fixed-stride pages, any shape (odd shapes run as a descriptor batch built
// on the device).
hipError_t run_pages(int mode, int algo, const uint8_t* pages, uint64_t page_size, uint64_t n, uint64_t* out,
                     uint8_t* ok, unsigned long long* first_bad, hipStream_t s);

// Scrub of fixed-stride XXH3 pages (249 <= page_size < 2^32, any alignment):
// cls[i] = pcs_page_class, type[i] = page byte 8 (type may be null: scratch
// is leased for it), summary = the 12 words of pcs_scrub_summary, list[0 ..
// min(n_corrupt, cap)) = the smallest corrupt page indices, ascending.  All
// device memory; enqueues on s and never waits.
hipError_t run_scrub(const uint8_t* pages, uint64_t page_size, uint64_t n, uint8_t* cls, uint8_t* type,
                     uint64_t* summary, uint64_t* list, uint64_t cap, hipStream_t s);

// Extents of the class bytes cls[0 .. n) (a scrub's, or any sub-range of them
// at any byte alignment): summary = the 12 words of pcs_extent_summary,
// runs[0 .. min(n_runs, cap)) = the first maximal runs of equal byte as
// pcs_extent, each with its full length.  All device memory; enqueues on s
// and never waits.
hipError_t run_extents(const uint8_t* cls, uint64_t n, uint64_t* summary, uint64_t* runs, uint64_t cap,
                       hipStream_t s);

// Per-file reports of a scrub's class and type bytes cls / type[0 .. n): file f
// is pages [first[f], first[f + 1]) (first: n_files + 1 device words, checked
// on the device).  reports = 16 words per file (pcs_file_report), summary = the
// 12 words of pcs_files_summary, list[0 .. min(n_bad_files, cap)) = the
// smallest bad file indices, ascending.  All device memory; enqueues on s and
// never waits.
hipError_t run_files(const uint8_t* cls, const uint8_t* type, uint64_t n, const uint64_t* first, uint64_t n_files,
                     uint64_t* reports, uint64_t* summary, uint64_t* list, uint64_t cap, hipStream_t s);

// Descriptor batch: range i =[base + off[i], +len[i]).  skip = 8 applies the
// page convention (digest over [8, len), stored digest at [0, 8)); skip = 0
// hashes the raw range.  seed is used by XXH64 only (XXH3 path is seed 0).
hipError_t run_desc(int mode, int algo, const uint8_t* base, const uint64_t* off, const uint32_t* len, uint64_t n,
                    int skip, uint64_t seed, uint64_t* out, uint8_t* ok, unsigned long long* first_bad,
                    hipStream_t s);

// Page list: page i is the absolute device-visible address ptrs[i] (pool
// pages in registered host memory), all of size page_size.  ptrs, out and ok
// may live in pinned host memory.  No first_bad word: the caller scans the
// verdicts.  Only the fast shapes (list_shape_ok) are supported.
inline bool list_shape_ok(int algo, uint64_t P) {
    return algo == 0 ? (P % 256 == 0 && P >= 256 && P <= 0xFFFFFFFFull)
                     : (P % 64 == 0 && P >= 128 && P <= 0xFFFFFFFFull);
}
// host_ptrs, if given, is a host-readable copy of the list: small batches
// pass it in the kernel arguments instead.
hipError_t run_list(int mode, int algo, const uint64_t* ptrs, const uint64_t* host_ptrs, uint64_t page_size,
                    uint64_t n, uint64_t* out, uint8_t* ok, hipStream_t s);

hipError_t run_gen_pages(uint8_t* pages, uint64_t page_size, uint64_t n, uint64_t seed, uint64_t first_page,
                         hipStream_t s);
hipError_t run_gen_desc(uint8_t* base, const uint64_t* off, const uint32_t* len, uint64_t n, uint64_t seed,
                        uint64_t first_page, hipStream_t s);
hipError_t run_flip(uint8_t* pages, uint64_t page_size, uint64_t n, uint64_t every, uint64_t byte_off,
                    hipStream_t s);
// ManifestBuilder::CalcChecksum over a device-resident content buffer
hipError_t run_manifest(const uint8_t* content, uint64_t len, uint64_t* out, hipStream_t s);
// Manifest scan over n_images images [base + off[i], + size[i]) inside [base,
// base + total): off and size are device words, checked on the device; align
// is a power of two in [64, 65536] and base 8-byte aligned (the caller checks
// both).  reports = 12 words per image (pcs_manifest_report), summary = the 12
// words of pcs_manifest_summary, records[0 .. min(n_records, cap)) = 5 words
// each (pcs_manifest_record), in walk order with the images in order.  All
// device memory; enqueues on s and never waits.  hipErrorInvalidValue when
// total / align + n_images + total / 2^20 does not fit 31 bits.
hipError_t run_manifest_scan(const uint8_t* base, uint64_t total, const uint64_t* off, const uint64_t* size,
                             uint64_t n_images, uint32_t align, uint64_t* reports, uint64_t* summary,
                             uint64_t* records, uint64_t cap, hipStream_t s);
// Manifest replay over the same layout (total < 2^32): runs the scan with a
// record array of its own bound in scratch, then decodes and applies the
// mapping sections.  scan_reports (12 words per image) may be null; reports =
// 16 words per image (pcs_replay_report), summary = the 12 words of
// pcs_replay_summary.  Rows go to table[table_first + page_id] with
// table_first counted from table_base (the rows of earlier groups of a host
// batch; 0 for a whole batch) and tested against table_cap, both absolute row
// indices of `table`.  All device memory; enqueues on s and never waits.
hipError_t run_manifest_replay(const uint8_t* base, uint64_t total, const uint64_t* off, const uint64_t* size,
                               uint64_t n_images, uint32_t align, uint64_t* scan_reports, uint64_t* reports,
                               uint64_t* summary, uint64_t* table, uint64_t table_base, uint64_t table_cap,
                               hipStream_t s);
// Liveness of the file pages [fp_first, fp_first + n) whose class bytes are
// cls[0 .. n), against the mapping table table[0 .. rows) (rows < 2^32):
// owner[i] = the lowest row that maps page i, else UINT32_MAX (owner may be
// null: scratch is leased), summary = the 16 words of pcs_live_summary,
// list[0 .. min(n_damaged, cap)) = the damaged live pages as pcs_live_page,
// ascending.  All device memory; enqueues on s and never waits.
hipError_t run_scrub_live(const uint8_t* cls, uint64_t n, uint64_t fp_first, const uint64_t* table, uint64_t rows,
                          uint32_t* owner, uint64_t* summary, uint64_t* list, uint64_t cap, hipStream_t s);
// Tree check (tree_check.hip) of the file pages [fp_first, fp_first + n) of
// page_size bytes each (32 .. 65535) with class bytes cls[0 .. n), against the
// mapping table table[0 .. rows) (rows < 2^32) from the n_roots (1 .. 8) device
// words roots: nodes = 2 words per row (pcs_tree_node; may be null: scratch is
// leased), summary = the 32 words of pcs_tree_summary, list[0 ..
// min(n_problems, cap)) = pcs_tree_problem, ascending.  All device memory;
// enqueues on s and never waits.
hipError_t run_tree_check(const uint8_t* pages, uint64_t page_size, uint64_t n, uint64_t fp_first, const uint8_t* cls,
                          const uint64_t* table, uint64_t rows, const uint64_t* roots, uint32_t n_roots,
                          uint64_t* nodes, uint64_t* summary, uint64_t* list, uint64_t cap, hipStream_t s);
// Leaf check (leaf_check.hip) over the same window, class bytes and table, with
// tree_nodes = the 2 words per row a tree check wrote (required when rows > 0;
// only read): leaves = 2 words per row (pcs_leaf_node; may be null: scratch is
// leased), summary = the 32 words of pcs_leaf_summary, list[0 ..
// min(n_problems, cap)) = pcs_leaf_problem, ascending.  All device memory;
// enqueues on s and never waits.
hipError_t run_leaf_check(const uint8_t* pages, uint64_t page_size, uint64_t n, uint64_t fp_first, const uint8_t* cls,
                          const uint64_t* table, uint64_t rows, const uint64_t* tree_nodes, uint64_t* leaves,
                          uint64_t* summary, uint64_t* list, uint64_t cap, hipStream_t s);
// Event-fenced device scratch (see ScratchPool in pcs_kernels.hip): the
// buffer is reused only after the work queued on `s` at release completes.
hipError_t scratch_acquire(size_t bytes, void** out, int* id);
hipError_t scratch_release(int id, hipStream_t s);
int set_tuning(int key, int64_t value);
// Decrements a positive knob by one and returns true (PCS_TUNE_FAIL_INJECT).
bool take_tuning(int key);
int64_t get_tuning(int key);
// Plain streaming read of [buf, buf + bytes) (the HBM read ceiling): one
// folded word per 4 KiB page into out[0 .. ceil(bytes / 4096)).
hipError_t run_stream_read(const uint8_t* buf, uint64_t bytes, uint64_t* out, hipStream_t s);

// Pre-armed validate service (pcs_service_*): a mailbox in pinned host
// memory, read by the waiting kernel through its device alias.  It holds up
// to kServiceMaxLines request lines, one per concurrent caller; line k is
// served by workgroups [k * wpl, (k + 1) * wpl) of the kernel.  The first
// kServiceLineWords words of a line (two 64-byte lines) carry a whole small
// request: seq = generation << 32 | count, page count, page size, a check
// word and the first kServiceLinePtrs page addresses, so the poll that sees a
// new seq brings in a request of up to 12 pages.  The host writes seq last.
// The 16 words arrive as separate per-lane loads, so nothing makes them one
// snapshot: the check word (the sum of service_word_mix over the other 15
// words, written by the host just before seq) is what proves that a poll saw
// one request's words and not a new seq beside an older request's page
// addresses.  A poll whose words do not add up to their check word is
// ignored and the line is read again.  Verdicts are 32-bit words stored
// system-scope.  `gen` names the newest generation: a kernel of an older one
// leaves at its next poll.
constexpr int kServiceMaxPages = 256;
constexpr int kServiceMaxLines = 8;
constexpr int kServiceLineWords = 16;
constexpr int kServiceCheckWord = 3;
constexpr int kServiceLinePtrs = kServiceLineWords - 4;
constexpr uint32_t kServicePending = 0xA5A5A5A5u;
constexpr uint64_t kServiceStamp = 1ull << 32;  // in the page-size word: a stamp request
struct ServiceLine {
    alignas(64) uint64_t seq;
    uint64_t n;
    uint64_t page_size;               // | kServiceStamp for a stamp request
    uint64_t check;                   // sum of service_word_mix(word i, i) over the other line words
    uint64_t ptrs[kServiceMaxPages];  // device-visible page addresses
    alignas(64) uint32_t ok[kServiceMaxPages];
    alignas(64) uint64_t torn_seq;    // kernel: the last seq it saw beside words that failed the check
};
constexpr int kServiceMaxWorkgroups = 256;  // lines * workgroups per line
struct ServiceBox {
    alignas(64) uint64_t stop;  // host: 1 ends every waiting kernel
    uint64_t gen;               // host: the newest generation (written before its kernel is queued)
    ServiceLine line[kServiceMaxLines];
    // kernel: departed[w] = the generation of the last workgroup w to leave,
    // stored after every verdict / header store of it is visible system-wide
    alignas(64) uint32_t departed[kServiceMaxWorkgroups];
};
static_assert(offsetof(ServiceLine, ptrs) == 4 * sizeof(uint64_t), "line words: seq, n, page_size, check, ptrs");
static_assert(offsetof(ServiceBox, gen) == offsetof(ServiceBox, stop) + 8, "stop and gen are one poll's two words");
// murmur3's 64-bit finaliser over (word, position): a word read from an older
// request changes the sum by a pseudo-random 64-bit amount.
__host__ __device__ inline uint64_t service_word_mix(uint64_t w, uint64_t i) {
    uint64_t x = w ^ (i * 0x9E3779B97F4A7C15ull) ^ 0xD6E8FEB86659FD93ull;
    x ^= x >> 33;
    x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33;
    x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}
// Queue one service kernel of generation `gen`: lines * wpl workgroups,
// workgroup w serving line w / wpl.  Each serves its line's requests of that
// generation until idle_ticks pass without one or, between requests, it has
// lived life_ticks (both on the 100 MHz real-time clock), or stop is set, or
// the box names a newer generation; then it stores gen into departed[w].
// exit_ticks: test only (a kernel that serves nothing and leaves that many
// ticks late; 0 in production).
hipError_t run_service(ServiceBox* d_box, int lines, int wpl, uint32_t gen, uint64_t idle_ticks, uint64_t life_ticks,
                       uint64_t exit_ticks, hipStream_t s);

}  // namespace pcs
