/*
 * eloqstore_pcs.h — C ABI of the MI355X page-checksum engine (libeloqstore_pcs.so).
 *
 * The drop-in boundary for EloqStore's per-page checksum path.  Every entry
 * point takes plain pointers and sizes; no C++ or torch types cross it.  The
 * reference has no batched or device API: these functions replace the bodies
 * of
 *     void eloqstore::SetChecksum(std::string_view)      src/storage/page.cpp:18-23
 *     bool eloqstore::ValidateChecksum(std::string_view)  src/storage/page.cpp:25-31
 * (declared include/storage/page.h:25-26) at the batch points of their callers:
 *     IouringMgr::ReadPages validate loop        src/async_io_manager.cpp:353-366 (<=128 pages)
 *     IouringMgr::ReadPage validate              src/async_io_manager.cpp:239-244
 *     WriteTask::WritePage SetChecksum x3         src/tasks/write_task.cpp:58-79  (batched at
 *                                                 FlushBatchPages :155-167, <=256 pages)
 *     page_checksum_tool                         tools/page_checksum_tool.cpp:104-105
 * and the hash primitive they call, XXH3_64bits (external/xxhash.h:6185) /
 * XXH64 (external/xxhash.h:3678).
 *
 * Page convention (include/storage/page.h:11, include/coding.h:64-77,126-139):
 * digest = XXH3_64bits(page + 8, page_size - 8) (seed 0, default secret),
 * stored little-endian in page bytes [0, 8).  algo = PCS_XXH64 uses
 * XXH64(page + 8, page_size - 8, 0) with the same layout (BASELINE config 3).
 *
 * Conventions
 *  - Return value: PCS_OK (0) or a negative pcs_status.  pcs_last_error()
 *    gives a thread-local message for the last failure on the calling thread.
 *  - *_dev functions take caller-owned DEVICE pointers on the current HIP
 *    device and enqueue work on `stream` (0 = legacy default stream); they do
 *    not synchronise.  Results are valid after the stream is synchronised.
 *  - Validation never fails on a mismatch: mismatches are reported through
 *    d_ok[i] = 0 and *d_first_bad = smallest failing index (UINT64_MAX when all
 *    pages match).  d_first_bad may be NULL.  The caller maps a mismatch to
 *    KvError::Corrupted exactly as async_io_manager.cpp:243/362 does.
 *  - Thread-safety: reentrant; use one stream per host thread per device.
 *    The only global state is the immutable secret in device constant memory
 *    and a per-device CU-count cache.
 *  - The library has no CPU fallback: without a usable GPU every compute entry
 *    point returns PCS_ERR_NO_DEVICE.
 */
#ifndef ELOQSTORE_PCS_H
#define ELOQSTORE_PCS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* hipStream_t, kept opaque so that callers need no HIP headers. */
typedef struct ihipStream_t *pcs_stream_t;

enum pcs_status {
    PCS_OK = 0,
    PCS_ERR_INVALID = -1,     /* bad argument (null pointer, page_size < 8, ...) */
    PCS_ERR_NO_DEVICE = -2,   /* no usable GPU / HIP runtime failure at init */
    PCS_ERR_HIP = -3,         /* a HIP call or kernel launch failed */
    PCS_ERR_NOMEM = -4,       /* device or pinned-host allocation failed */
};

enum pcs_algo {
    PCS_XXH3_64 = 0, /* XXH3_64bits, seed 0 — the reference's page checksum */
    PCS_XXH64 = 1,   /* XXH64, seed 0 */
};

/* Flags of the validating host entry points (pcs_pages_validate_host_ex,
 * pcs_batch_submit_ex in PCS_BATCH_VALIDATE mode).  The flag-less names keep
 * their original 6-argument prototypes (= PCS_FLAG_NONE, always verify), so a
 * caller built against an older header can never pass a stray flag word.
 *   PCS_FLAG_SKIP_VERIFY  KvOptions::skip_verify_checksum (include/kv_options.h:41):
 *                         the reference skips the validate loop entirely
 *                         (async_io_manager.cpp:239, 353); here nothing is
 *                         hashed or copied, every verdict is 1 and first_bad is
 *                         UINT64_MAX.  Arguments are still checked; no GPU is
 *                         needed for this path (it computes nothing). */
enum pcs_flags {
    PCS_FLAG_NONE = 0,
    PCS_FLAG_SKIP_VERIFY = 1u << 0,
};

/* ---- library / device ----------------------------------------------------
 * ABI version of this header.  Compare pcs_abi_version() with PCS_ABI_VERSION
 * once at start-up: a library built from another header revision then fails
 * loudly instead of reading arguments it was not given.
 *   3  round 3: pcs_pages_validate_host and pcs_batch_submit lost the trailing
 *      flags word they had in round 2 (the flags moved to the _ex forms); a
 *      caller built against the old prototypes links but its flags are
 *      ignored, which pcs_abi_version() detects
 *   4  round 4: PCS_TUNE_SERVICE_TEAR_TEST / FAIL_INJECT / SERVICE_MAX_CALLERS,
 *      PCS_COUNTER_SERVICE_TORN_REQUESTS; the C++ single-page SetChecksum /
 *      ValidateChecksum moved to libeloqstore_pcs_dropin.so
 *   5  round 5: PCS_TUNE_SERVICE_REPOST_TEST, PCS_TUNE_ZC_STAMP_POLL_PAGES,
 *      PCS_COUNTER_SERVICE_REPOSTS (additive: no prototype changed)
 *   6  round 6: pcs_last_path / pcs_batch_path and the PCS_PATH_* bits,
 *      PCS_TUNE_SERVICE_SLOW_EXIT_TEST, PCS_TUNE_ZC_BATCH_EVENT, PCS_TUNE_SYNC_SPIN_US,
 *      PCS_TUNE_SERVICE_DEPARTURE, pcs_thread_prepare (additive);
 *      pcs_stream_read_dev writes
 *      one word per 4 KiB (was per 64 KiB: size d_out for the new count)
 *   7  page scrub: pcs_pages_scrub_dev / pcs_pages_scrub_host, enum
 *      pcs_page_class and struct pcs_scrub_summary; additive, no prototype changed.
 *      Added later under the same number, additive again (detect them by
 *      symbol): pcs_scrub_extents_dev / pcs_pages_scrub_extents_host, struct
 *      pcs_extent and struct pcs_extent_summary; pcs_scrub_files_dev /
 *      pcs_pages_scrub_files_host, struct pcs_file_report and struct
 *      pcs_files_summary; pcs_manifest_scan_dev / pcs_manifest_scan_host, struct
 *      pcs_manifest_record, pcs_manifest_report and pcs_manifest_summary, and
 *      PCS_TUNE_MANIFEST_WALK_TILE.  Added after 7 without a bump; detect with
 *      dlsym: pcs_manifest_replay_dev / pcs_manifest_replay_host, enum
 *      pcs_replay_status, struct pcs_replay_report and pcs_replay_summary;
 *      pcs_scrub_live_dev / pcs_scrub_live_host, struct pcs_live_page and
 *      pcs_live_summary; PCS_TUNE_REPLAY_TILE; pcs_tree_check_dev /
 *      pcs_tree_check_host, enum pcs_tree_bits, struct pcs_tree_node,
 *      pcs_tree_problem and pcs_tree_summary, PCS_TREE_MAX_DEPTH and
 *      PCS_TREE_CLASS_ABSENT; pcs_leaf_check_dev / pcs_leaf_check_host, enum
 *      pcs_leaf_bits, struct pcs_leaf_node, pcs_leaf_problem and
 *      pcs_leaf_summary, PCS_LEAF_MAX_GROUPS */
#define PCS_ABI_VERSION 7
int pcs_abi_version(void);
const char *pcs_version(void);
const char *pcs_last_error(void);
int pcs_device_count(int *count);
/* Select the HIP device for subsequent calls on this host thread. */
int pcs_set_device(int device);
int pcs_synchronize(pcs_stream_t stream);

/* ---- device-resident, fixed page size (pages contiguous, stride page_size) --
 * Fast paths: XXH3 runs a 16-lane group per page for every page size of its
 * long path (page_size >= 249) at any alignment; fastest at page_size % 256
 * == 0 on a 16-byte-aligned base (every power-of-two data_page_size and 64 KiB
 * chunks), 5-7 TB/s for other sizes.  XXH64 needs an
 * 8-byte-aligned base, page_size % 8 == 0 and page_size >= 40.  Any other
 * shape is still computed exactly (generic kernel), only slower. */

/* d_digests[i] = digest of page i over [8, page_size). */
int pcs_pages_digest_dev(const void *d_pages, uint64_t page_size, uint64_t n_pages, int algo,
                         uint64_t *d_digests, pcs_stream_t stream);
/* d_ok[i] = (stored LE u64 at page i [0,8)) == digest; batched ValidateChecksum. */
int pcs_pages_validate_dev(const void *d_pages, uint64_t page_size, uint64_t n_pages, int algo,
                           uint8_t *d_ok, uint64_t *d_first_bad, pcs_stream_t stream);
/* In place: page i bytes [0,8) = digest (LE); batched SetChecksum. */
int pcs_pages_stamp_dev(void *d_pages, uint64_t page_size, uint64_t n_pages, int algo,
                        pcs_stream_t stream);

/* ---- scrub: classify, census and list (XXH3 pages only) --------------------
 * A whole-file check must tell pages that were never written from pages that
 * are damaged: in append mode the store fallocates a data file to its full
 * size, so a file that is not full ends in all-zero pages, and a zero page
 * never validates (its stored digest is 0, XXH3 of a zero body is not).
 *   PCS_PAGE_OK       the stored digest matches: exactly the pages for which
 *                     pcs_pages_validate_dev writes 1
 *   PCS_PAGE_BLANK    EVERY byte of the page, header included, is zero.  Exact:
 *                     a zero body under its correct digest is OK, a zero header
 *                     over any non-zero body byte is CORRUPT
 *   PCS_PAGE_CORRUPT  neither
 * d_class[i] receives the class and d_type[i] the raw page byte 8 (PageType,
 * include/storage/page.h:14-21) of every page, whatever its class.  The
 * summary counts the classes and, for OK pages only, the types: ok_by_type[0..3]
 * = types 0..3 (NonLeafIndex, LeafIndex, Data, Overflow), [4] = type 255
 * (Deleted), [5] = any other byte.  d_corrupt[0 .. n_listed) receives the
 * n_listed = min(n_corrupt, corrupt_cap) SMALLEST corrupt page indices in
 * ascending order (the same from call to call); entries at n_listed and beyond
 * are not written; n_corrupt is always the full count.  Every call writes the
 * whole summary, whatever it held before; n_pages == 0 gives zero counts and
 * first_corrupt = UINT64_MAX.
 *
 * One pass reads every page byte once (the validate kernels with a second
 * output byte and, only on pages whose stored header is zero, an OR over the
 * loaded words); a second pass over the class and type bytes builds the
 * summary and the list on the device.  page_size must be >= 249 (the XXH3 long
 * path) and fit 32 bits, at any base alignment; anything else is
 * PCS_ERR_INVALID.  Not scrubbed in this revision: mixed-size descriptors,
 * XXH64 pages, the zero-copy page-list path, the validate service and
 * pcs_batch objects.
 *
 * The _dev form enqueues on `stream` and never synchronises (its scratch is
 * event-fenced per stream, so two streams may scrub concurrently); d_type may
 * be NULL, d_corrupt may be NULL iff corrupt_cap == 0.  The _host form is
 * synchronous and takes host pointers throughout: the pages go through the
 * staged pipeline of the other host batches only (gathered, or one contiguous
 * pinned run DMA'd directly, in 32 MiB chunks through the three slots; never
 * zero-copy, never the service), classes and types come back per chunk, and
 * the per-chunk summaries and lists are merged into global page indices,
 * ascending and capped.  PCS_TUNE_FAIL_INJECT applies to it. */
enum pcs_page_class { PCS_PAGE_CORRUPT = 0, PCS_PAGE_OK = 1, PCS_PAGE_BLANK = 2 };
typedef struct pcs_scrub_summary { /* 12 x u64, the same layout on device and host */
    uint64_t n_pages, n_ok, n_corrupt, n_blank;
    uint64_t ok_by_type[6];
    uint64_t first_corrupt; /* UINT64_MAX when none */
    uint64_t n_listed;      /* min(n_corrupt, corrupt_cap) */
} pcs_scrub_summary;
int pcs_pages_scrub_dev(const void *d_pages, uint64_t page_size, uint64_t n_pages, uint8_t *d_class,
                        uint8_t *d_type, pcs_scrub_summary *d_summary, uint64_t *d_corrupt,
                        uint64_t corrupt_cap, pcs_stream_t stream);
int pcs_pages_scrub_host(const void *const *pages, uint64_t page_size, uint64_t n_pages, uint8_t *cls,
                         uint8_t *type, pcs_scrub_summary *summary, uint64_t *corrupt,
                         uint64_t corrupt_cap);

/* ---- scrub extents: class runs, written extent and holes --------------------
 * A run-length view of a scrub's class bytes, computed on the device.  An
 * append-mode data file is written strictly in page order, so its written
 * pages form a prefix and its blank pages a suffix: a blank page BELOW the
 * last written page is a lost or trimmed write, and a scrub that only counts
 * blank pages cannot tell the two apart.
 *
 * A run is a maximal range of equal class bytes.  Only byte 2 (PCS_PAGE_BLANK)
 * is blank and only byte 0 is corrupt; any other byte value is a class of its
 * own kind: never blank, it splits runs by inequality and is reported as is in
 * `cls`.  d_runs[0 .. n_listed) receives the first n_listed = min(n_runs,
 * run_cap) runs in ascending order, each with its FULL length, also when it
 * extends far beyond the pages the other listed runs cover; entries at n_listed
 * and beyond are not written.  Every call writes the whole summary, whatever it
 * held before; n_pages == 0 gives zero counts and UINT64_MAX in first_blank,
 * first_hole, first_class and last_class.  The output is the same from call to
 * call (no atomic append).
 *
 * pcs_scrub_extents_dev reads only d_class[0 .. n_pages), about one byte per
 * page, never the pages: d_class is the class array a scrub wrote or any
 * sub-range of it at any byte alignment (one device batch may hold several
 * data files; take the extents per file).  It enqueues on `stream` and never
 * synchronises; its scratch is event-fenced per stream.  d_runs may be NULL
 * iff run_cap == 0 (the list pass is then skipped).
 *
 * pcs_pages_scrub_extents_host is pcs_pages_scrub_host (same pipeline, page
 * size rule, summary, corrupt list, PCS_TUNE_FAIL_INJECT and errors) that also
 * takes the extents of every 32 MiB chunk while its class bytes are still on
 * the device, and merges the chunks into global page indices: a run that
 * crosses a chunk edge is one run, and one chunk's blank tail is a hole as soon
 * as a later chunk holds a non-blank page, so the result is that of one pass
 * over the whole class array.  Here cls and type may both be NULL: a caller
 * that scrubs a whole store then allocates nothing per page.  summary and ext
 * must be non-NULL; runs may be NULL iff run_cap == 0. */
typedef struct pcs_extent {
    uint64_t first_page, n_pages;
    uint32_t cls;      /* the class byte of the run's pages */
    uint32_t reserved; /* 0 */
} pcs_extent;
typedef struct pcs_extent_summary { /* 12 x u64, the same layout on device and host */
    uint64_t n_pages;
    uint64_t n_runs;        /* all maximal runs, whatever the cap */
    uint64_t n_listed;      /* min(n_runs, run_cap) */
    uint64_t written_pages; /* 1 + index of the last non-blank page; 0 when every page is blank */
    uint64_t n_blank;       /* blank pages */
    uint64_t n_blank_runs;  /* blank runs, the tail included */
    uint64_t first_blank;   /* first blank page, UINT64_MAX when none */
    uint64_t n_holes;       /* blank runs that start below written_pages */
    uint64_t n_hole_pages;  /* blank pages below written_pages */
    uint64_t first_hole;    /* first page of the first hole, UINT64_MAX when none */
    uint64_t first_class, last_class; /* class byte of page 0 / page n-1; UINT64_MAX when n_pages == 0 */
} pcs_extent_summary;
int pcs_scrub_extents_dev(const uint8_t *d_class, uint64_t n_pages, pcs_extent_summary *d_summary,
                          pcs_extent *d_runs, uint64_t run_cap, pcs_stream_t stream);
int pcs_pages_scrub_extents_host(const void *const *pages, uint64_t page_size, uint64_t n_pages,
                                 uint8_t *cls, uint8_t *type, pcs_scrub_summary *summary,
                                 uint64_t *corrupt, uint64_t corrupt_cap, pcs_extent_summary *ext,
                                 pcs_extent *runs, uint64_t run_cap);

/* ---- scrub files: one report per data file of a batch ----------------------
 * A store holds data files, not one run of pages (KvOptions::pages_per_file_shift,
 * include/kv_options.h: 1 << 18 pages by default, "a smaller file size like
 * 4MB" recommended in append mode), so one device batch holds many files and
 * the operator's question is which of them are damaged.  File f is pages
 * [file_first[f], file_first[f + 1]) of the batch; file_first holds
 * n_files + 1 entries.  A file's report is what the two reductions above give
 * over that sub-range alone: the counting fields are pcs_pages_scrub_dev's
 * summary of the file's class and type bytes, with first_corrupt FILE-LOCAL;
 * written_pages, n_holes, n_hole_pages and first_hole are
 * pcs_scrub_extents_dev's over the same bytes, file-local too.  Class bytes
 * above 2 behave as there: counted nowhere, never blank.  A run never crosses
 * a file boundary: a blank page that ends file f is f's tail, not f + 1's
 * hole, and the byte before a file's first page is never read as its
 * predecessor.  Empty files (file_first[f] == file_first[f + 1]) are legal:
 * n_pages = 0, zero counts, UINT64_MAX in the three "first" fields.  A file is
 * bad when it has a corrupt page or a hole; d_bad[0 .. n_listed) receives the
 * n_listed = min(n_bad_files, bad_cap) SMALLEST bad file indices in ascending
 * order (the same from call to call, no atomic append); entries at n_listed
 * and beyond and reports at n_files and beyond are not written.
 *
 * pcs_scrub_files_dev reads only d_class and d_type[0 .. n_pages) (both
 * required, any byte alignment) and the boundaries, which are a DEVICE array:
 * a scrub can be followed by the cut with no host round trip.  The files need
 * not cover the batch; pages in no file are in no report.  It enqueues on
 * `stream`, never synchronises, and writes the whole summary on every call,
 * n_files == 0 included.  d_bad may be NULL iff bad_cap == 0.  The host cannot
 * see the boundaries, so the kernels check them: invalid_file is the first f
 * with file_first[f] > file_first[f + 1] or file_first[f + 1] > n_pages; when
 * it is set, every other summary word but n_files is 0 and no report or list
 * entry is written, whatever the boundaries hold.
 *
 * pcs_pages_scrub_files_host is pcs_pages_scrub_host's staged pipeline (same
 * page-size rule, PCS_TUNE_FAIL_INJECT and errors; never zero-copy, never the
 * service) with host pointers throughout.  file_first is checked on the host
 * (PCS_ERR_INVALID) and must cover the batch: file_first[0] == 0 and
 * file_first[n_files] == n_pages.  Each 32 MiB chunk is scrubbed and cut, on
 * the device, at the boundaries of the files that intersect it; only those
 * partial reports come back (no per-page array), and a file's parts are folded
 * in page order so that the result equals one pass over the file.  The summary
 * and the bad list are built on the host; invalid_file is UINT64_MAX. */
typedef struct pcs_file_report {          /* 16 x u64, the same layout on device and host */
    uint64_t first_page, n_pages;         /* the file's range in the batch */
    uint64_t n_ok, n_corrupt, n_blank;
    uint64_t ok_by_type[6];               /* as pcs_scrub_summary */
    uint64_t first_corrupt;               /* FILE-LOCAL page index, UINT64_MAX when none */
    uint64_t written_pages;               /* file-local: 1 + last non-blank page, 0 when none */
    uint64_t n_holes, n_hole_pages;       /* blank runs / pages below written_pages */
    uint64_t first_hole;                  /* file-local, UINT64_MAX when none */
} pcs_file_report;
typedef struct pcs_files_summary {        /* 12 x u64, the same layout on device and host */
    uint64_t n_files, n_pages;            /* n_pages = sum of the files' lengths */
    uint64_t n_ok, n_corrupt, n_blank;    /* pages, over all files */
    uint64_t n_corrupt_files;             /* files with n_corrupt > 0 */
    uint64_t n_hole_files;                /* files with n_holes > 0 */
    uint64_t n_bad_files;                 /* corrupt or hole */
    uint64_t n_unwritten_files;           /* written_pages == 0 (empty files included) */
    uint64_t first_bad_file;              /* UINT64_MAX when none */
    uint64_t n_listed;                    /* min(n_bad_files, bad_cap) */
    uint64_t invalid_file;                /* UINT64_MAX when the boundaries are valid */
} pcs_files_summary;
int pcs_scrub_files_dev(const uint8_t *d_class, const uint8_t *d_type, uint64_t n_pages,
                        const uint64_t *d_file_first, uint64_t n_files, pcs_file_report *d_reports,
                        pcs_files_summary *d_summary, uint64_t *d_bad, uint64_t bad_cap, pcs_stream_t stream);
int pcs_pages_scrub_files_host(const void *const *pages, uint64_t page_size, uint64_t n_pages,
                               const uint64_t *file_first, uint64_t n_files, pcs_file_report *reports,
                               pcs_files_summary *summary, uint64_t *bad, uint64_t bad_cap);

/* ---- device-resident descriptor batches (mixed page sizes) ----------------
 * Page i occupies [d_base + d_off[i], d_base + d_off[i] + d_len[i]).  Pages
 * shorter than 8 bytes never validate (ok = 0) and digest to 0. */
int pcs_desc_digest_dev(const void *d_base, const uint64_t *d_off, const uint32_t *d_len,
                        uint64_t n, int algo, uint64_t *d_digests, pcs_stream_t stream);
int pcs_desc_validate_dev(const void *d_base, const uint64_t *d_off, const uint32_t *d_len,
                          uint64_t n, int algo, uint8_t *d_ok, uint64_t *d_first_bad,
                          pcs_stream_t stream);
int pcs_desc_stamp_dev(void *d_base, const uint64_t *d_off, const uint32_t *d_len, uint64_t n,
                       int algo, pcs_stream_t stream);

/* ---- raw ranges (no page header): the hash primitive itself ---------------
 * d_out[i] = XXH3_64bits(range i)  (external/xxhash.h:6185), any length, or
 * XXH64(range i, seed)             (external/xxhash.h:3678). */
int pcs_xxh3_64_ranges_dev(const void *d_base, const uint64_t *d_off, const uint32_t *d_len,
                           uint64_t n, uint64_t *d_out, pcs_stream_t stream);
int pcs_xxh64_ranges_dev(const void *d_base, const uint64_t *d_off, const uint32_t *d_len,
                         uint64_t n, uint64_t seed, uint64_t *d_out, pcs_stream_t stream);

/* ---- host-memory batches (scattered pool pages, synchronous) --------------
 * The shape of IouringMgr::ReadPages / FlushBatchPages: an array of page
 * pointers into the caller's page pool (page.cpp:95-120).  Pages are gathered
 * into pinned staging, hashed on the current device and results copied back;
 * the call returns when done.  When the pages form one contiguous run in
 * pinned memory (hipHostMalloc / hipHostRegister, e.g. a registered io_uring
 * buffer ring), they are DMA'd directly with no gather copy.  32 MiB chunks
 * flow through three slots (H2D || kernel || D2H).  Safe to call concurrently
 * from several host threads (each thread owns its staging and streams). */
int pcs_pages_validate_host(const void *const *pages, uint64_t page_size, uint64_t n_pages,
                            int algo, uint8_t *ok, uint64_t *first_bad);
/* The same plus a flags word: PCS_FLAG_SKIP_VERIFY = KvOptions::skip_verify_checksum. */
int pcs_pages_validate_host_ex(const void *const *pages, uint64_t page_size, uint64_t n_pages,
                               int algo, uint8_t *ok, uint64_t *first_bad, uint32_t flags);
int pcs_pages_stamp_host(void *const *pages, uint64_t page_size, uint64_t n_pages, int algo);
int pcs_pages_digest_host(const void *const *pages, uint64_t page_size, uint64_t n_pages,
                          int algo, uint64_t *digests);

/* Pinned (page-locked) host memory, e.g. for an io_uring buffer ring or file
 * staging: batches over one contiguous pinned run are DMA'd with no gather.
 * The allocation is also a registered region (below). */
int pcs_host_alloc_pinned(uint64_t bytes, void **out);
int pcs_host_free_pinned(void *p);

/* Registered page pools (zero-copy).  EloqStore allocates its page pool in
 * chunks of 1024 pages (PagesPool::Extend, src/storage/page.cpp:95-120) and
 * its io_uring buffer rings once at start-up.  Registering such a region once
 * (page-locks it and maps it for the GPU) lets a host batch read and write its
 * pages in place over PCIe.  A host batch (pcs_pages_*_host, pcs_batch_submit)
 * whose pages all lie in registered regions, are 16-byte aligned and have a
 * fast size (XXH3: page_size % 256 == 0; XXH64: page_size % 64 == 0 and
 * >= 128) runs as ONE kernel launch.  That launch reads the page list and the
 * pages from host memory and writes the verdicts, digests or stamped headers
 * straight back: no gather copy and no staging DMA
 * (PCS_TUNE_ZERO_COPY).  Regions must not overlap.  A region must stay
 * registered until every batch over it has completed. */
int pcs_host_register(void *ptr, uint64_t bytes);
/* Optional, once per host thread that will issue host batches (a shard
 * thread at start-up): creates the thread's stream and the pinned result and
 * zero-copy buffers a batch of up to 256 pages uses on the current device,
 * and runs one 1-page zero-copy batch through them (the process's first
 * launch also loads the kernels).  Without it the thread's first host batch
 * pays for this: 16-35 ms with eight threads starting at once (soak
 * attribution).  Idempotent. */
int pcs_thread_prepare(void);
int pcs_host_unregister(void *ptr);  /* ptr = the base passed to pcs_host_register */

/* ---- asynchronous host batches (shard-loop integration) --------------------
 * EloqStore's shard thread never blocks: its work loop is Submit() ->
 * PollComplete() -> ExecuteReadyTasks() (src/storage/shard.cpp:67-130), and
 * a ReadPages / FlushBatchPages coroutine yields while I/O is in flight.  A
 * pcs_batch is the checksum analogue: submit gathers the pages (or DMAs a
 * pinned contiguous run directly), enqueues H2D + kernel + D2H on the batch's
 * own stream and returns; poll answers "done?" without blocking.  A batch
 * whose pages are one contiguous pinned run is DMA'd in place (the caller
 * must then not modify the pages until completion).  One batch
 * object holds one batch in flight; create several for more concurrency.
 * Pages must stay valid until the batch completes (stamp writes the digests
 * into them when poll/wait observes completion). */
typedef struct pcs_batch pcs_batch;
enum pcs_batch_mode { PCS_BATCH_DIGEST = 0, PCS_BATCH_VALIDATE = 1, PCS_BATCH_STAMP = 2 };
int pcs_batch_create(pcs_batch **out);  /* on the calling thread's current device */
/* A submit that fails leaves the batch idle: poll/wait/result then refuse
 * until a later submit succeeds. */
int pcs_batch_submit(pcs_batch *b, int mode, const void *const *pages, uint64_t page_size,
                     uint64_t n_pages, int algo);
/* flags: PCS_FLAG_SKIP_VERIFY (validate mode only) completes the batch at
 * submit with every verdict 1, sizing and pinning no staging. */
int pcs_batch_submit_ex(pcs_batch *b, int mode, const void *const *pages, uint64_t page_size,
                        uint64_t n_pages, int algo, uint32_t flags);
/* 1 = done, 0 = in flight, < 0 = error.  Never waits: on the service path a
 * poll that finds the service's lock held (another thread starting, stopping
 * or launching it) returns 0 and looks again at the next poll, and a service
 * stop or restart never drains the stream under that lock. */
int pcs_batch_poll(pcs_batch *b);
int pcs_batch_wait(pcs_batch *b);   /* blocks until done; PCS_OK or error */
/* After completion: verdicts / digests (either may be NULL) and the first
 * failing index (UINT64_MAX if none, validate mode). */
int pcs_batch_result(pcs_batch *b, uint8_t *ok, uint64_t *digests, uint64_t *first_bad);
int pcs_batch_destroy(pcs_batch *b);

/* ---- which path served a host batch (diagnostics) ------------------------
 * PCS_PATH_* bits of the calling thread's last synchronous host validate or
 * stamp (pcs_pages_validate_host(_ex), pcs_pages_stamp_host), or of a batch's
 * last submission (pcs_batch_path, complete or not).  0 before any call. */
enum pcs_path {
    PCS_PATH_SERVED = 1,          /* answered by the resident service kernel */
    PCS_PATH_LAUNCHED = 2,        /* ran on the launch path (a kernel launch of its own) */
    PCS_PATH_FALLBACK = 4,        /* posted to the service, then re-run on the launch path */
    PCS_PATH_REPOSTED = 8,        /* re-posted to a newer service generation at least once */
    PCS_PATH_NEW_GENERATION = 16, /* queued a new service kernel: none was certainly waiting */
    PCS_PATH_LOCK_SKIPPED = 32,   /* a poll found the service's lock held and returned without it, or a
                                     submit gave up waiting for it (20 us) and took the launch path */
};
int pcs_last_path(void);
int pcs_batch_path(const pcs_batch *b);

/* ---- pre-armed validate service (small read batches, opt-in) --------------
 * A launch per host batch costs ~14 µs before its first page is read.  While
 * the service is on, pcs_pages_validate_host(_ex) and pcs_pages_stamp_host
 * (and so eloqstore::ValidateChecksums / SetChecksums) serve eligible batches
 * through a resident
 * kernel of `workgroups` workgroups that polls a request line in pinned host
 * memory between requests.  Eligible: XXH3, 1-256 pages, all in registered
 * regions, 16-byte aligned, page_size % 256 == 0, called on a device whose
 * service is on; everything else takes the launch path.  Each device has its
 * own service: pcs_service_start / stop / running act on the calling
 * thread's current device (pcs_set_device).  One request per request line is
 * in flight at a time (one line by default, up to 8 with
 * pcs_service_start_ex); a call that finds every line owned, or arrives while
 * more eligible calls are in progress on the device than
 * PCS_TUNE_SERVICE_MAX_CALLERS + lines - 1 (a decaying average), takes the
 * launch path.  The kernel leaves
 * after idle_us (0 = 1000; else 200 .. 1000000) without a request and, between
 * requests, after 2 * idle_us of life, and the next request starts a new one:
 * it holds its CUs, and delays any device-synchronising HIP call of the
 * process, by at most 2 * idle_us.  Results are identical to the launch
 * path's.  PCS_ERR_INVALID for workgroups outside [1, 256] or
 * an idle_us out of range, or when the device's service is already running.
 * Services still running at exit are stopped by an atexit handler. */
int pcs_service_start(int workgroups, uint32_t idle_us);
/* The same with `lines` request lines (1 .. 8), each served by its own
 * `workgroups_per_line` workgroups (lines x workgroups_per_line <= 256): up
 * to `lines` calls on the device are in flight through the service at once,
 * each on a line of its own.  pcs_service_start(wg, idle) = _ex(1, wg, idle). */
int pcs_service_start_ex(int lines, int workgroups_per_line, uint32_t idle_us);
/* Turns the device's service off at once (new calls take the launch path),
 * then waits, without holding anything another thread's call needs, up to 2 s
 * for its kernels to leave; PCS_ERR_HIP if they have not.  Requests still in
 * flight re-run on the launch path. */
int pcs_service_stop(void);
int pcs_service_running(void); /* 1 while the service is on, 0 otherwise */

/* ---- manifest record checksum (next row: SURVEY.md §8f-3) -----------------
 * ManifestBuilder::CalcChecksum (src/storage/root_meta.cpp:150-174): XXH3-64
 * of each <= 1 MiB chunk of the content, folded as agg = rotl(agg, 1) ^ h;
 * agg *= 0x9e3779b97f4a7c15; empty content -> 0.  Chunks >= 2 KiB at 8-byte
 * alignment run on the long-range kernel (a workgroup per chunk). */
int pcs_manifest_checksum_dev(const void *d_content, uint64_t len, uint64_t *d_out, pcs_stream_t stream);
int pcs_manifest_checksum_host(const void *content, uint64_t len, uint64_t *out);
/* ManifestBuilder::ValidateChecksum (root_meta.cpp:138-148): a record is
 * checksum(8) | root(4) | ttl_root(4) | len(4) | payload; records shorter than
 * the 20-byte header never validate. */
int pcs_manifest_validate_host(const void *record, uint64_t size, int *valid);

/* ---- manifest scan: walk and verify every record of many manifests ---------
 * A store directory holds one manifest per partition: a snapshot record
 * followed by appended log records, each checksum(8) | root(4) | ttl_root(4) |
 * payload_len(4) | payload and padded to `align` (page_align, 4096).  The scan
 * finds the records of every image of a batch and checks each, as
 * Replayer::ParseNextRecord does one record at a time (src/replayer.cpp:74-140)
 * and tools/manifest_check_tool.cpp does for one file.
 *
 * Walk rule, per image of `size` bytes, from offset o = 0:
 *   o == size                -> stop, PCS_MANIFEST_END_CLEAN
 *   size - o < 20            -> stop, PCS_MANIFEST_END_SHORT_HEADER
 *   len = LE32 at o + 16, e = o + 20 + len in 64 bits (len may be any uint32_t)
 *   e > size                 -> stop, PCS_MANIFEST_END_SHORT_PAYLOAD; the
 *                               incomplete record is not a record
 *   otherwise [o, e) is a record, ok iff the LE64 at o equals
 *   ManifestBuilder::CalcChecksum of bytes [o + 8, e) (the 1 MiB chunks counted
 *   from o + 8, pcs_manifest_checksum_dev's aggregate)
 *   o' = e rounded up to align; o' > size -> stop, PCS_MANIFEST_END_SHORT_PADDING
 *   with end_offset = size; otherwise o = o' and go on.
 * end_offset is the offset at which the walk stopped.  The verdict follows
 * from the ok flags alone.  A length is followed only after its bounds test,
 * so no payload_len causes a read outside [d_base, d_base + total_bytes), and
 * bytes inside a record's payload that look like a header are never a record.
 *
 * Layout (pcs_manifest_scan_dev): image i is [d_base + d_img_off[i], +
 * d_img_size[i]); align is a power of two in [64, 65536]; d_base and d_records
 * are 8-byte aligned; every offset is a multiple of align; the images ascend
 * and are disjoint, d_img_off[i] >= roundup(d_img_off[i - 1] + d_img_size[i -
 * 1], align); d_img_off[i] + d_img_size[i] <= total_bytes.  Offsets and sizes
 * are DEVICE arrays which the host cannot see, so the kernels check them:
 * invalid_image is the first i that breaks a rule, and when it is set every
 * other summary word but n_images is 0 and no report or record is written.
 * d_img_size[i] == 0 is legal: PCS_MANIFEST_EMPTY, END_CLEAN, first_corrupt
 * UINT64_MAX.  total_bytes / align + n_images + total_bytes / 2^20 must stay
 * below 2^31 (PCS_ERR_INVALID otherwise).
 *
 * d_records[first_record + k] is record k of the image, in walk order with the
 * images in order, for every index below record_cap; entries at n_listed and
 * beyond are not written; the counts are always full.  The output is the same
 * from call to call (no atomic append).  d_records may be NULL iff record_cap
 * == 0.  The _dev form enqueues on `stream` and never synchronises; its
 * scratch is event-fenced per stream and sized from total_bytes, align and
 * n_images alone.  Every call writes the whole summary, n_images == 0
 * included.  The walk reads one aligned word per align-slot of every image,
 * all independent, and follows the chain through those words in LDS, never
 * through the image.
 *
 * pcs_manifest_scan_host is synchronous and takes host pointers throughout
 * (plain or pinned, any alignment).  It checks its arguments on the host,
 * copies the images into the calling thread's pinned staging at multiples of
 * align, DMAs them and runs the _dev form; never zero-copy, never the service.
 * Staging budget: 32 MiB of packed images per group; a batch above it goes
 * through in groups of whole images (an image larger than the budget is a
 * group of its own), and first_record and the summary are those of one call
 * over the whole batch.  invalid_image is UINT64_MAX.  PCS_TUNE_FAIL_INJECT
 * applies to it. */
enum pcs_manifest_end {               /* why an image's walk stopped */
    PCS_MANIFEST_END_CLEAN = 0,         /* next record offset == size */
    PCS_MANIFEST_END_SHORT_HEADER = 1,  /* 0 < size - offset < 20 */
    PCS_MANIFEST_END_SHORT_PAYLOAD = 2, /* offset + 20 + payload_len > size */
    PCS_MANIFEST_END_SHORT_PADDING = 3, /* last record complete, its padding cut by the end of the image */
};
enum pcs_manifest_verdict {
    PCS_MANIFEST_CLEAN = 0,        /* >= 1 record, every record ok */
    PCS_MANIFEST_TORN_TAIL = 1,    /* record 0 ok; every record from the first corrupt one on is corrupt:
                                      the replayer drops them and cuts the file back */
    PCS_MANIFEST_BROKEN = 2,       /* record 0 ok; an ok record follows a corrupt one (replayer.cpp:60-63) */
    PCS_MANIFEST_BAD_SNAPSHOT = 3, /* record 0 corrupt (replayer.cpp:37-38) */
    PCS_MANIFEST_EMPTY = 4,        /* no complete record */
};
typedef struct pcs_manifest_record { /* 40 bytes, the same layout on device and host */
    uint64_t offset;                 /* in its image; a multiple of align */
    uint64_t stored, computed;       /* LE u64 at [0, 8) / CalcChecksum(record[8 .. 20 + payload_len)) */
    uint32_t payload_len, root, ttl_root, ok;
} pcs_manifest_record;
typedef struct pcs_manifest_report { /* 12 x u64, one per image */
    uint64_t size, n_records, n_ok, n_corrupt;
    uint64_t first_corrupt;          /* record index in the image, UINT64_MAX when none */
    uint64_t n_ok_after_corrupt;     /* ok records after the first corrupt one */
    uint64_t valid_prefix_bytes;     /* offset of the first corrupt record, else the offset where the walk stopped */
    uint64_t end_offset, end_reason, verdict;
    uint64_t first_record;           /* index of the image's record 0 in d_records (exclusive sum of n_records) */
    uint64_t max_record_bytes;       /* largest 20 + payload_len walked, 0 when none */
} pcs_manifest_report;
typedef struct pcs_manifest_summary { /* 12 x u64 */
    uint64_t n_images, n_records, n_ok, n_corrupt;
    uint64_t n_by_verdict[5];
    uint64_t first_bad_image;        /* first image whose verdict is not CLEAN, UINT64_MAX when none */
    uint64_t n_listed;               /* min(n_records, record_cap) */
    uint64_t invalid_image;          /* UINT64_MAX when the layout is valid */
} pcs_manifest_summary;
int pcs_manifest_scan_dev(const void *d_base, uint64_t total_bytes, const uint64_t *d_img_off,
                          const uint64_t *d_img_size, uint64_t n_images, uint32_t align,
                          pcs_manifest_report *d_reports, pcs_manifest_summary *d_summary,
                          pcs_manifest_record *d_records, uint64_t record_cap, pcs_stream_t stream);
int pcs_manifest_scan_host(const void *const *images, const uint64_t *sizes, uint64_t n_images,
                           uint32_t align, pcs_manifest_report *reports, pcs_manifest_summary *summary,
                           pcs_manifest_record *records, uint64_t record_cap);

/* ---- manifest replay: the mapping table a manifest describes ----------------
 * What Replayer::Replay computes (src/replayer.cpp:27-72, 142-228, with
 * ManifestBuilder's layout, src/storage/root_meta.cpp:29-105), for every image
 * of a batch, on the device.  The call runs the scan above internally (its
 * record scratch is sized by the scan's own bound, total_bytes / align +
 * n_images; the caller passes no record array) and writes the scan's reports to
 * d_scan_reports when that is given.
 *
 * Which records: verdict CLEAN or TORN_TAIL replays n_replayed = (first_corrupt
 * == UINT64_MAX ? n_records : first_corrupt) records, record 0 as the snapshot
 * and the others as logs; any other verdict is PCS_REPLAY_NOT_REPLAYABLE.  root
 * and ttl_root are those of record n_replayed - 1.
 *
 * Varints (src/coding.cpp:141-201): little-endian base 128, a byte below 0x80
 * ends one; a varint64 has at most 10 bytes and its value is the sum of
 * (b_i & 0x7F) << 7i mod 2^64, a varint32 at most 5 bytes, value mod 2^32.
 * Snapshot payload of L bytes: varint64 max_fp_id; varint32 dict_len (<= the
 * bytes that remain, skipped); with rem bytes left, LE32 mapping_len with
 * mapping_len + 8 <= rem; mapping_len bytes of varint64s, value j = table[j];
 * LE32 term_len (<= the bytes after it); term_len bytes holding an even count
 * of varint64s, only framed and counted; bytes after it are ignored.  Log
 * payload: L >= 8, LE32 mapping_len with mapping_len + 8 <= L, the mapping
 * section holds alternating varint32 page_id and varint64 value (whole varints,
 * an even count), then the term section as in the snapshot.  A section must be
 * a whole number of varints, none longer than its limit.  Where the reference
 * asserts, CHECKs or LOG(FATAL)s on one of these, the image is
 * PCS_REPLAY_MALFORMED with malformed_record the lowest record that breaks a
 * rule; nothing outside the record is read and other images are unaffected.
 *
 * Apply: entries in record order, then byte order; a page's final value is that
 * of its last entry.  table_size = max(snapshot count, 1 + largest page_id of a
 * replayed log); a page nobody wrote is 7 (MappingSnapshot::InvalidValue).  A
 * value maps a file page iff value & 7 == 1, its id is value >> 3.  max_fp_id =
 * max(the snapshot's, id + 1 over EVERY replayed log entry that is a file page,
 * overwritten ones included), as ReplayLog does.  n_term_pairs sums the term
 * pairs of every replayed record.
 *
 * Rows: table_first is the exclusive sum of table_size over the images that are
 * neither NOT_REPLAYABLE nor MALFORMED (for those two it is the running sum at
 * that image, and every field but status, n_replayed, malformed_record and
 * table_first is 0, min_fp / max_fp UINT64_MAX).  An image with table_first +
 * table_size > table_cap gets PCS_REPLAY_TABLE_CAP: table_size, max_fp_id,
 * root, ttl_root, dict_bytes, snapshot_pages, n_log_entries and n_term_pairs
 * are still reported, it writes no rows and n_mapped, min_fp, max_fp and
 * n_fp_beyond_max are 0, UINT64_MAX, UINT64_MAX and 0.  OK images write
 * d_table[table_first + page_id]; rows of other images and everything at
 * n_rows_written and beyond are not written.  d_table may be NULL iff table_cap
 * == 0.  The output is identical from call to call: last-writer-wins is an
 * atomicMax over a per-row sequence number, then the winner stores.
 *
 * The layout, alignment rules and limits are pcs_manifest_scan_dev's, plus
 * total_bytes < 2^32 (PCS_ERR_INVALID otherwise).  The _dev form never
 * synchronises; every grid and scratch size comes from the arguments alone
 * (table_cap included: four bytes of scratch per row of d_table, so pass the
 * table's real capacity); scratch is event-fenced per stream.  An invalid
 * layout sets invalid_image, leaves every other summary word but n_images 0 and
 * writes nothing else.  Sized for what a store holds (thousands of manifests of
 * up to manifest_limit): the prelude pass runs one workgroup per image with a
 * lane per record, and two exclusive sums, over 2 x records and over the decode
 * tiles, run in one workgroup each, so a batch of millions of align-slots or one
 * image of millions of records spends its time there on one CU; the record
 * scratch is 72 bytes per align-slot of total_bytes.
 *
 * pcs_manifest_replay_host packs whole images into 32 MiB staging groups as
 * pcs_manifest_scan_host does and carries table_first and the TABLE_CAP rule
 * across the groups, so the result equals one call over the batch.
 * PCS_TUNE_FAIL_INJECT applies to it. */
enum pcs_replay_status {
    PCS_REPLAY_OK = 0,
    PCS_REPLAY_NOT_REPLAYABLE = 1, /* the scan's verdict is neither CLEAN nor TORN_TAIL */
    PCS_REPLAY_MALFORMED = 2,      /* a replayed record breaks a decode rule */
    PCS_REPLAY_TABLE_CAP = 3,      /* its rows do not fit below table_cap */
};
typedef struct pcs_replay_report { /* 16 x u64, one per image */
    uint64_t status, n_replayed;
    uint64_t malformed_record;     /* UINT64_MAX unless status is MALFORMED */
    uint64_t root, ttl_root, max_fp_id, dict_bytes;
    uint64_t snapshot_pages;       /* values in the snapshot's mapping section */
    uint64_t n_log_entries;        /* (page_id, value) pairs of the replayed logs */
    uint64_t table_size, table_first;
    uint64_t n_mapped;             /* rows that map a file page */
    uint64_t min_fp, max_fp;       /* smallest / largest mapped file page id, UINT64_MAX when n_mapped == 0 */
    uint64_t n_fp_beyond_max;      /* mapped ids >= max_fp_id */
    uint64_t n_term_pairs;
} pcs_replay_report;
typedef struct pcs_replay_summary { /* 12 x u64 */
    uint64_t n_images, n_by_status[4];
    uint64_t n_rows;               /* sum of table_size over OK and TABLE_CAP images */
    uint64_t n_rows_written;       /* over OK images: rows [0, n_rows_written) of d_table */
    uint64_t n_mapped, n_log_entries;
    uint64_t first_bad_image;      /* first image whose status is not OK, UINT64_MAX when none */
    uint64_t invalid_image;        /* UINT64_MAX when the layout is valid */
    uint64_t reserved;             /* 0 */
} pcs_replay_summary;
int pcs_manifest_replay_dev(const void *d_base, uint64_t total_bytes, const uint64_t *d_img_off,
                            const uint64_t *d_img_size, uint64_t n_images, uint32_t align,
                            pcs_manifest_report *d_scan_reports /* may be NULL */, pcs_replay_report *d_reports,
                            pcs_replay_summary *d_summary, uint64_t *d_table, uint64_t table_cap,
                            pcs_stream_t stream);
int pcs_manifest_replay_host(const void *const *images, const uint64_t *sizes, uint64_t n_images, uint32_t align,
                             pcs_manifest_report *scan_reports /* may be NULL */, pcs_replay_report *reports,
                             pcs_replay_summary *summary, uint64_t *table, uint64_t table_cap);

/* ---- scrub live: which damaged pages the tree still points to ---------------
 * In append mode a data file is mostly superseded copies: a corrupt dead page
 * is harmless, a blank or corrupt MAPPED page is data loss.  d_class is a
 * scrub's class bytes for file pages fp_first .. fp_first + n_pages, d_table a
 * replayed mapping table of table_size rows (<= 2^32 - 1).  Page i is live iff
 * some table[p] == ((fp_first + i) << 3 | 1); d_owner[i] is the lowest such p,
 * else UINT32_MAX (d_owner may be NULL: scratch is used).  n_mapped counts the
 * mapped rows of the whole table, n_mapped_in_window those that point into the
 * window, n_duplicate those of them that are not the owner.  The six cells
 * count class bytes 0, 1 and 2 only; d_damaged lists every live page whose
 * class byte is not PCS_PAGE_OK, ascending by index with page_id its owner,
 * capped at damaged_cap (n_damaged is always full; the same from call to
 * call).  d_damaged may be NULL iff damaged_cap == 0; table_size == 0 and
 * n_pages == 0 are legal.  The _dev form never synchronises; the _host form
 * copies the class bytes and the table to the device and runs it. */
typedef struct pcs_live_page {
    uint64_t index;        /* page index in the window */
    uint32_t page_id, cls; /* its owner and its class byte */
} pcs_live_page;
typedef struct pcs_live_summary { /* 16 x u64 */
    uint64_t n_pages, table_size, n_mapped, n_mapped_in_window, n_duplicate;
    uint64_t live_ok, live_blank, live_corrupt, dead_ok, dead_blank, dead_corrupt;
    uint64_t n_damaged;
    uint64_t first_damaged; /* UINT64_MAX when none */
    uint64_t last_live;     /* UINT64_MAX when no page is live */
    uint64_t n_listed;      /* min(n_damaged, damaged_cap) */
    uint64_t reserved;      /* 0 */
} pcs_live_summary;
int pcs_scrub_live_dev(const uint8_t *d_class, uint64_t n_pages, uint64_t fp_first, const uint64_t *d_table,
                       uint64_t table_size, uint32_t *d_owner /* may be NULL */, pcs_live_summary *d_summary,
                       pcs_live_page *d_damaged, uint64_t damaged_cap, pcs_stream_t stream);
int pcs_scrub_live_host(const uint8_t *cls, uint64_t n_pages, uint64_t fp_first, const uint64_t *table,
                        uint64_t table_size, uint32_t *owner /* may be NULL */, pcs_live_summary *summary,
                        pcs_live_page *damaged, uint64_t damaged_cap);

/* ---- tree check: walk the index tree from the replayed roots ------------------
 * After a replay the device holds the mapping table, root and ttl_root; after a
 * scrub a class byte per file page.  The tree check looks inside the pages: it
 * walks the B-tree that hangs off every root breadth-first, level by level, and
 * reports what does not hold together.  d_pages / d_class describe the file
 * pages fp_first .. fp_first + n_pages (scrub live's window convention),
 * d_table is a replayed table (a row maps file page value >> 3 iff value & 7 ==
 * 1), d_roots a DEVICE array of n_roots logical page ids: root and ttl_root are
 * adjacent words of a pcs_replay_report, so &report->root with n_roots = 2
 * chains a replay into the check with no host round trip.  A root >= UINT32_MAX
 * is an empty tree; a smaller root >= table_size is counted in n_refs and
 * n_out_of_range_refs and reaches nothing.
 *
 * Page rules (IndexPageBuilder, src/storage/index_page_builder.cpp:44-204;
 * IndexPageIter, src/storage/mem_index_page.cpp:134-233; the data-page header,
 * include/storage/data_page.h:26-51), little-endian: an index page has type
 * byte (offset 8) 0 (NonLeafIndex) or 1 (LeafIndex), content length C = LE16
 * @9 with 17 <= C <= page_size, R = LE16 @(C - 2) restart offsets o[k] = LE16
 * @(E + 2k) from E = C - 2 (1 + R) >= 15, and child 0 = LE32 @11.  R == 0
 * requires E == 15; otherwise o[0] == 15, o[k] < o[k + 1], o[R - 1] < E, and
 * every region [o[k], o[k + 1]) (o[R] = E) is a whole number of entries varint32
 * shared | varint32 non_shared | non_shared key bytes | varint32 v, each varint
 * at most 5 bytes and inside the region, shared == 0 in a region's first entry
 * and <= the previous entry's key length otherwise; delta = (v & 1) ? -(v >> 1)
 * : (v >> 1); the child id is delta in a region's first entry, previous id +
 * delta otherwise, and lies in [0, INT32_MAX].  On such a page the regions
 * decode independently and yield exactly the children the reference's
 * sequential iterator yields.  A page that breaks any rule is MALFORMED and
 * contributes NO child; no byte outside the page is read.  Key order is not
 * checked.  Of a data page (type 2) only prev = LE32 @11 and next = LE32 @15
 * are read.
 *
 * The walk: a logical page c < table_size referenced at depth d by parent p
 * bids the key (d << 32 | p); the smallest key claims it (a root bids depth 0
 * with its own id as parent; of equal roots the lowest tree index wins), so the
 * winner is the smallest depth, then the lowest parent id, whatever the
 * schedule; `tree` is the winner's tree.  Every page is decoded once: cycles
 * are harmless.  At most PCS_TREE_MAX_DEPTH levels are decoded: an index page
 * claimed at depth 16 is typed, counted in n_depth_capped and not decoded.  For
 * a claimed page the first rule that applies sets one bit, and the page is then
 * neither read nor followed:
 *   UNMAPPED    its table value is not a file page
 *   ABSENT      the file page lies outside the window, or its class byte is
 *               none of 0, 1, 2 (PCS_TREE_CLASS_ABSENT is the byte to write for
 *               pages that were not loaded)
 *   BLANK       class byte 2
 *   CORRUPT     class byte 0
 *   WRONG_TYPE  class byte 1 and the type byte does not fit: a root and a child
 *               of a type-0 page are of type 0 or 1, a child of a type-1 page
 *               is of type 2
 *   MALFORMED   an index page of the right type that breaks the page rule
 * A well-formed index page at depth < 16 has its children bid; a child id >=
 * table_size sets BAD_CHILD on the PARENT.  After the walk a reached data page
 * d with none of the six bits above gets BAD_LINK unless next == UINT32_MAX or
 * next is a reached data page with none of those bits whose prev == d, and the
 * same for prev with the roles swapped.  Chain heads (prev == UINT32_MAX) are
 * counted; tails equal heads in any consistent chain set and are not reported.
 *
 * d_nodes[p] (one per table row, may be NULL) describes row p; a row reached
 * from no root has parent UINT32_MAX, depth, tree and type 0xFF and zeros
 * elsewhere.  d_problems[0 .. n_listed) are the reached nodes with bits != 0 in
 * ascending page_id, capped at problem_cap (may be NULL iff problem_cap == 0);
 * entries at n_listed and beyond are not written.  Every output is the same
 * from call to call (claims by atomicMin, the list by ordered compaction).
 * unreached_by_type counts the mapped rows no root reaches whose page is in the
 * window with class byte 1, by the scrub's six type buckets; overflow pages hang
 * off data-page entries, which this call does not decode, so bucket 3 is
 * non-zero for any store with large values: the leaf check (below) walks them
 * and says which of them no value claims (n_leaked_overflow).  An unreached
 * mapped index or data page is a leak or a lost subtree.
 *
 * Limits (PCS_ERR_INVALID): 32 <= page_size <= 65535, table_size <= 2^32 - 1,
 * 1 <= n_roots <= 8; n_pages == 0 and table_size == 0 are legal.  d_table,
 * d_roots, d_nodes, d_summary and d_problems are 8-byte aligned; d_pages and
 * d_class may have any alignment.  The _dev form never synchronises: a fixed
 * number of launches of fixed size, no count read back; its scratch is
 * event-fenced per stream (at most 28 bytes per table row).  One wavefront decodes one
 * page, so one huge page keeps one CU busy.
 *
 * pcs_tree_check_host takes host pointers; `pages` is ONE contiguous buffer of
 * n_pages * page_size bytes, copied to the device with one plain copy (the
 * whole window must be resident: PCS_ERR_NOMEM when it does not fit; the staged
 * pipeline of the other host batches is not used).  With cls == NULL the pages
 * are scrubbed on the device first (page_size >= 249 then).  roots is a host
 * array.  PCS_TUNE_FAIL_INJECT applies to it. */
#define PCS_TREE_MAX_DEPTH 16
#define PCS_TREE_CLASS_ABSENT 3
enum pcs_tree_bits {
    PCS_TREE_UNMAPPED = 1, PCS_TREE_ABSENT = 2, PCS_TREE_BLANK = 4, PCS_TREE_CORRUPT = 8,
    PCS_TREE_WRONG_TYPE = 16, PCS_TREE_MALFORMED = 32, PCS_TREE_BAD_CHILD = 64, PCS_TREE_BAD_LINK = 128,
};
typedef struct pcs_tree_node { /* 16 bytes, one per table row */
    uint32_t parent;           /* UINT32_MAX: reached from no root; a root is its own parent */
    uint8_t depth, tree;       /* 0xFF when not reached */
    uint8_t type;              /* page byte 8; 0xFF when the page was not read */
    uint8_t bits;              /* pcs_tree_bits */
    uint32_t n_children;       /* child pointers decoded, leftmost included; 0 unless a well-formed index page */
    uint32_t n_bad_children;   /* of them >= table_size */
} pcs_tree_node;
typedef struct pcs_tree_problem { /* reached nodes with bits != 0, ascending page_id, capped */
    uint32_t page_id, parent, bits, depth;
} pcs_tree_problem;
typedef struct pcs_tree_summary { /* 32 x u64, the same layout on device and host; n_roots, the caller's own
                                    argument, has no word here */
    uint64_t n_pages, table_size, n_mapped, n_reached;
    uint64_t n_nonleaf, n_leaf_index, n_data; /* reached, bits == 0, by type */
    uint64_t n_refs;                /* child pointers decoded plus the non-empty roots */
    uint64_t n_extra_refs;          /* in-range refs beyond the first to a page */
    uint64_t n_out_of_range_refs;   /* refs >= table_size */
    uint64_t max_depth;             /* UINT64_MAX when nothing was reached */
    uint64_t n_depth_capped;
    uint64_t n_by_bit[8];           /* reached nodes with bit 1 << k set */
    uint64_t n_problems;
    uint64_t first_problem;         /* smallest page_id with bits != 0, UINT64_MAX when none */
    uint64_t n_listed;              /* min(n_problems, problem_cap) */
    uint64_t n_unreached_mapped;    /* mapped rows reached from no root = the sum of the next seven words */
    uint64_t unreached_by_type[6];  /* in the window, class byte 1: the scrub's six type buckets */
    uint64_t n_unreached_unread;    /* outside the window or class byte != 1 */
    uint64_t n_chain_heads;
} pcs_tree_summary;
int pcs_tree_check_dev(const void *d_pages, uint64_t page_size, uint64_t n_pages, uint64_t fp_first,
                       const uint8_t *d_class, const uint64_t *d_table, uint64_t table_size,
                       const uint64_t *d_roots, uint32_t n_roots, pcs_tree_node *d_nodes /* may be NULL */,
                       pcs_tree_summary *d_summary, pcs_tree_problem *d_problems, uint64_t problem_cap,
                       pcs_stream_t stream);
int pcs_tree_check_host(const void *pages, uint64_t page_size, uint64_t n_pages, uint64_t fp_first,
                        const uint8_t *cls /* may be NULL */, const uint64_t *table, uint64_t table_size,
                        const uint64_t *roots, uint32_t n_roots, pcs_tree_node *nodes /* may be NULL */,
                        pcs_tree_summary *summary, pcs_tree_problem *problems, uint64_t problem_cap);

/* ---- leaf check: decode data pages and follow overflow chains -----------------
 * The last layer of the offline check.  The tree check stops at the data pages;
 * every call a reader makes after the index descent goes through DataPageIter
 * and, for large values, GetOverflowValue.  The leaf check decodes every data
 * page the tree reached in good health and walks the overflow chain of every
 * large value.  It reuses what the tree check produced: d_pages, d_class,
 * d_table and the window follow the tree check's conventions and limits, and
 * d_tree_nodes is the node array of a tree check over the same inputs
 * (required; it is only read).
 *
 * Page rules, little-endian (DataPageBuilder, src/storage/
 * data_page_builder.cpp:129-236; DataPageIter, src/storage/data_page.cpp:
 * 337-469; OverflowPage, data_page.cpp:518-609).  A data page has type byte 2,
 * content length C = LE16 @9 with 21 <= C <= page_size, prev and next at 11 and
 * 15, R = LE16 @(C - 2) restart offsets o[k] = LE16 @(E + 2k) from E = C - 2 (1
 * + R) >= 19.  R == 0 requires E == 19; R == 1 with o[0] == E == 19 is the
 * builder's empty page; otherwise o[0] == 19, o[k] < o[k + 1], o[R - 1] < E, and
 * every region [o[k], o[k + 1]) (o[R] = E) is a whole number of entries
 *   varint32 shared | varint32 non_shared | varint32 stored_len | non_shared
 *   key bytes | stored_len >> 4 value bytes | [varint64 expire_ts iff
 *   stored_len & 2] | varint64 timestamp delta
 * every varint inside the region (a varint32 at most 5 bytes, a varint64 at
 * most 10), shared == 0 in a region's first entry and <= the previous key
 * length otherwise, non_shared + value_len within the rest of the region, the
 * compression bits (stored_len >> 2 & 3) not 3, and for an overflow entry
 * (stored_len & 1) value_len % 4 == 0 and 4 <= value_len <= 512: its value
 * bytes are value_len / 4 LE32 logical page ids.  This is stricter than the
 * reference's iterator (which bounds an entry by the end of the entries, not by
 * its region) and yields the same entries on every page the builder writes.  A
 * page that breaks any rule is MALFORMED and yields no entry and no pointer; no
 * byte outside the page is read.  Key order is not checked (the comparator is
 * pluggable: include/comparator.h), values are not decompressed.  An overflow
 * page has type byte 3, V = LE16 @9 value bytes from offset 11, n = byte
 * (page_size - 1) pointers as LE32 ending at page_size - 1; the intrinsic rule
 * is n <= 128 and 11 + V + 4 n + 1 <= page_size.  Whether a page that is not
 * the last of its group is full is not checked: that depends on
 * KvOptions::overflow_pointers, which no file records.
 *
 * Data pages: row p is checked iff the tree reached it as a data page with none
 * of the six bits UNMAPPED .. MALFORMED.  Its node has owner = p, a = its
 * entries and b = its overflow values (both 0 when MALFORMED).
 *
 * Overflow chains (GetOverflowValue, src/tasks/task.cpp:117-155): for every
 * overflow entry of a well-formed page the chain is walked group by group, the
 * entry's pointers being the first group and the pointers of a group's LAST
 * page the next.  The entry's key is (data page id << 32 | entry byte offset <<
 * 16).  Every pointer c of a group is counted in n_refs and takes the first of
 *   c >= table_size          n_out_of_range_refs, BAD_POINTER on the data page
 *   the tree reached c       n_refs_to_tree, BAD_CHAIN on the data page; c is
 *                            not claimed
 *   otherwise                c is claimed: its owner is the smallest key that
 *                            names it, `a` counts the pointers to it (mod 2^32),
 *                            and it gets the first that applies of UNMAPPED,
 *                            ABSENT, BLANK, CORRUPT (as in the tree check),
 *                            WRONG_TYPE (type byte != 3) and MALFORMED (the
 *                            intrinsic rule); any of them sets BAD_CHAIN on the
 *                            data page.  A page with none of them that is not
 *                            the last of its group and has n != 0 is counted in
 *                            n_misplaced_pointers and sets BAD_CHAIN.
 * The walk goes on iff the group's last pointer was claimed, its page has none
 * of the six bits and n > 0.  After PCS_LEAF_MAX_GROUPS groups a walk that
 * would go on stops: the value is counted in n_chain_capped and sets BAD_CHAIN
 * (a cycle ends there).  Whether a walk goes on depends on pages, table and
 * class bytes only, never on who won a claim, so every owner is the minimum
 * over the same bids and every counter the same integer sum on every call.  A
 * claimed row named by more than one pointer gets SHARED.  Counters that follow
 * pointers (n_refs, n_misplaced_pointers, ...) count every visit.
 *
 * d_leaves[p] (one per table row, may be NULL) describes row p; a row that is
 * neither a checked data page nor claimed has owner UINT32_MAX and zeros
 * elsewhere.  d_problems[0 .. n_listed) are the checked or claimed rows with
 * bits != 0 in ascending page_id, capped at problem_cap (may be NULL iff
 * problem_cap == 0); entries at n_listed and beyond are not written.  n_by_bit
 * counts those rows by bit.  n_leaked_overflow counts the rows that are mapped,
 * in the window, of class 1 and type 3, that no value claimed and the tree did
 * not reach: the overflow pages the tree check could say nothing about.
 *
 * Limits and alignment are the tree check's (d_tree_nodes and d_leaves 8-byte
 * aligned).  The _dev form never synchronises: five launches of fixed size, no
 * count read back; its scratch is event-fenced per stream (at most 28 bytes per
 * table row).  One wavefront decodes one data page and walks its chains, so a
 * page full of values that each run into the group cap keeps one wavefront busy
 * for 4096 dependent loads per value.
 *
 * pcs_leaf_check_host takes host pointers as pcs_tree_check_host does, scrubs
 * the pages on the device when cls == NULL (page_size >= 249 then), runs the
 * tree check and then the leaf check there, and returns both summaries
 * (tree_summary may be NULL; its n_listed is 0, the tree's problems being
 * exactly its reached nodes with bits != 0), optionally both node arrays, and
 * the leaf problems.  PCS_TUNE_FAIL_INJECT applies to it. */
#define PCS_LEAF_MAX_GROUPS 4096
enum pcs_leaf_bits { /* the low six are pcs_tree_bits' UNMAPPED .. MALFORMED */
    PCS_LEAF_BAD_POINTER = 64, PCS_LEAF_BAD_CHAIN = 128, PCS_LEAF_SHARED = 256,
};
typedef struct pcs_leaf_node { /* 16 bytes, one per table row */
    uint32_t owner;        /* data page checked: its own id; overflow row claimed: the data page of its smallest
                              bidder; else UINT32_MAX */
    uint16_t owner_entry;  /* byte offset of that entry in the owner; 0 for a data page */
    uint16_t bits;         /* pcs_leaf_bits */
    uint32_t a;            /* data page: entries;         overflow row: references */
    uint32_t b;            /* data page: overflow values; overflow row: V | n << 16 (0 unless the page has none of
                              the six bits) */
} pcs_leaf_node;
typedef struct pcs_leaf_problem { /* checked or claimed rows with bits != 0, ascending page_id, capped */
    uint32_t page_id, owner, bits, owner_entry;
} pcs_leaf_problem;
typedef struct pcs_leaf_summary { /* 32 x u64, the same layout on device and host */
    uint64_t n_pages, table_size;
    uint64_t n_data_pages;          /* rows checked */
    uint64_t n_data_ok;             /* of them with bits == 0 */
    uint64_t n_entries, n_overflow_values, n_expiring, n_compressed; /* over the well-formed data pages */
    uint64_t inline_value_bytes;    /* value bytes of the entries that do not overflow */
    uint64_t overflow_value_bytes;  /* V summed once per claimed row with none of the six bits */
    uint64_t n_refs;                /* pointers followed, the entries' own included */
    uint64_t n_out_of_range_refs;
    uint64_t n_extra_refs;          /* pointers to a claimed row beyond the first */
    uint64_t n_refs_to_tree;
    uint64_t n_misplaced_pointers;
    uint64_t n_chain_capped;
    uint64_t max_groups;            /* the longest walk, in groups */
    uint64_t n_overflow_pages;      /* claimed rows */
    uint64_t n_by_bit[9];           /* checked or claimed rows with bit 1 << k set */
    uint64_t n_problems;
    uint64_t first_problem;         /* smallest page_id with bits != 0, UINT64_MAX when none */
    uint64_t n_listed;              /* min(n_problems, problem_cap) */
    uint64_t n_leaked_overflow;     /* mapped, in the window, class 1, type 3, neither claimed here nor reached by
                                       the tree */
    uint64_t n_overflow_ok;         /* claimed rows with bits == 0 */
} pcs_leaf_summary;
int pcs_leaf_check_dev(const void *d_pages, uint64_t page_size, uint64_t n_pages, uint64_t fp_first,
                       const uint8_t *d_class, const uint64_t *d_table, uint64_t table_size,
                       const pcs_tree_node *d_tree_nodes /* required: a tree check's output over the same inputs */,
                       pcs_leaf_node *d_leaves /* may be NULL */, pcs_leaf_summary *d_summary,
                       pcs_leaf_problem *d_problems, uint64_t problem_cap, pcs_stream_t stream);
int pcs_leaf_check_host(const void *pages, uint64_t page_size, uint64_t n_pages, uint64_t fp_first,
                        const uint8_t *cls /* may be NULL */, const uint64_t *table, uint64_t table_size,
                        const uint64_t *roots, uint32_t n_roots, pcs_tree_node *tree_nodes /* may be NULL */,
                        pcs_tree_summary *tree_summary /* may be NULL */, pcs_leaf_node *leaves /* may be NULL */,
                        pcs_leaf_summary *summary, pcs_leaf_problem *problems, uint64_t problem_cap);

/* ---- sharding ------------------------------------------------------------
 * Contiguous page range [begin, end) of rank `rank` of `world` for n pages:
 * begin = floor(rank * n / world).  Pages are independent, so G GPUs hash G
 * disjoint ranges with no collective. */
int pcs_shard_range(uint64_t n, int world, int rank, uint64_t *begin, uint64_t *end);

/* ---- tuning -------------------------------------------------------------
 * Process-wide launch knobs, read at every launch (defaults in brackets):
 *   PCS_TUNE_XXH3_BLOCKS_PER_CU   [0] grid cap in 256-thread blocks per CU for
 *                                     the XXH3 page kernels (grid-stride loop
 *                                     beyond it); 0 = auto: one block per 16
 *                                     pages up to 16 KiB pages, 8 per CU above
 *   PCS_TUNE_XXH64_BLOCKS_PER_CU  [0] same for XXH64 (one block per 64 pages)
 *   PCS_TUNE_NT_LOADS             [1] XXH3 page loads non-temporal (1) or
 *                                     default cache policy (0)
 *   PCS_TUNE_XXH64_LAYOUT         [0] segments in flight per XXH64 LDS-kernel
 *                                     step: 0 or 1 = default (2), 2 -> 1,
 *                                     3 -> 2, 4 -> 4, 5 -> 3
 *   PCS_TUNE_ZERO_COPY            [1] host batches over registered pages:
 *                                     1 = zero-copy (one launch, pages read in
 *                                     place); 0 = stage through device memory
 *                                     (gather or direct DMA)
 *   PCS_TUNE_XXH3_RT_BATCH        [1] XXH3 pages whose size is not a compiled
 *                                     case (mixed-size descriptors, odd
 *                                     multiples of 256): 1 = load 4 blocks per
 *                                     step like the fixed kernels; 0 = one
 *                                     block per step
 *   PCS_TUNE_XXH3_SPLIT_PAGES  [8192] fixed-size XXH3 pages of at least this
 *                                     many bytes (power of two, 8-64 KiB) are
 *                                     split over P/4096 groups, one 4 KiB slice
 *                                     each, with the scramble chain run from
 *                                     block sums in LDS; 0 = never
 *   PCS_TUNE_INLINE_LIST          [1] zero-copy XXH3 batches of <= 256 pages
 *                                     pass the page list in the kernel
 *                                     arguments (0 = read it from host memory)
 *   PCS_TUNE_MANIFEST_WIDE        [1] manifests at 8-byte alignment: block
 *                                     sums over the whole GPU, then one chain
 *                                     per chunk (0 = one workgroup per chunk)
 *   PCS_TUNE_XXH64_WAVES          [4] waves per workgroup of the XXH64 LDS
 *                                     kernel (1, 2 or 4; 16 pages per wave)
 *   PCS_TUNE_ZC_POLL              [1] validate batches from host memory, sync
 *                                     and async, zero-copy AND staged (gather
 *                                     or direct DMA), plus zero-copy XXH3
 *                                     stamps of <= PCS_TUNE_ZC_STAMP_POLL_PAGES
 *                                     pages: complete once
 *                                     every verdict / done byte has landed in
 *                                     host memory (1) or on the launch's
 *                                     completion signal (0)
 *   PCS_TUNE_ZC_STAMP_POLL_PAGES [256] zero-copy XXH3 stamps of up to this
 *                                     many pages complete from per-page done
 *                                     bytes (with PCS_TUNE_ZC_POLL on), larger
 *                                     ones on the launch's completion signal
 *   PCS_TUNE_SERVICE_STREAM       [1] stream of the validate service, read at
 *                                     pcs_service_start: 1 highest priority
 *                                     (hardware queues of its own), 0 plain
 *   PCS_TUNE_SERVICE_MAX_CALLERS  [2] validate service contention gate: while
 *                                     the decaying average of concurrent
 *                                     eligible calls on the device exceeds
 *                                     this + lines - 1 + 0.5, the service
 *                                     declines and calls take the launch
 *                                     path; 0 = off (values above 2^20 act
 *                                     as 2^20: the gate never closes)
 *   PCS_TUNE_SERVICE_TEAR_TEST    [0] test only: microseconds the service's
 *                                     host side waits between posting seq and
 *                                     writing the request words (the kernel
 *                                     must ignore the torn line meanwhile)
 *   PCS_TUNE_FAIL_INJECT          [0] test only: the next k host-batch calls
 *                                     (pcs_pages_*_host scrub included, pcs_batch_submit*,
 *                                     pcs_batch_poll / wait,
 *                                     pcs_manifest_*_host) fail with
 *                                     PCS_ERR_HIP; decremented per failure
 *   PCS_TUNE_SERVICE_REPOST_TEST  [0] test only: the next k service requests
 *                                     are posted as if an earlier generation
 *                                     had answered part of them and left: seq
 *                                     names the previous generation (no
 *                                     waiting kernel serves it) and the
 *                                     verdict words of pages 16 and up hold a
 *                                     stale answer (validate 0, stamp 1); the
 *                                     host must re-arm and re-post the whole
 *                                     request (PCS_COUNTER_SERVICE_REPOSTS)
 *   PCS_TUNE_SERVICE_SLOW_EXIT_TEST [0] test only: service kernels queued while
 *                                     this is > 0 serve no request and stay
 *                                     this many microseconds after deciding to
 *                                     leave (a stop or restart must not make
 *                                     pollers wait for them)
 *   PCS_TUNE_ZC_BATCH_EVENT       [0] asynchronous zero-copy batches that
 *                                     complete from their landed verdicts /
 *                                     done bytes: 1 records an event behind
 *                                     the kernel (round 5), 0 queries the
 *                                     batch's stream instead (one runtime
 *                                     call less per batch)
 *   PCS_TUNE_SYNC_SPIN_US         [0] synchronous host calls (validate, stamp,
 *                                     pcs_batch_wait) spin on their results
 *                                     for this many microseconds, then sleep
 *                                     ~10 µs between checks; 0 = spin
 *                                     throughout (lowest latency; a loaded
 *                                     store's sync callers then burn their
 *                                     cores)
 *   PCS_TUNE_SERVICE_DEPARTURE    [1] a service kernel's workgroups store
 *                                     their generation into the mailbox as
 *                                     they leave; 1: a waiting request learns
 *                                     that its line's workgroups have gone
 *                                     from those words (re-posting at once)
 *                                     and asks the runtime about the kernel
 *                                     every 1 ms; 0: asks the runtime every
 *                                     50 µs (round 6 before this key)
 *   PCS_TUNE_MANIFEST_WALK_TILE [2048] manifest scan: align-slots per LDS tile
 *                                     of the chain walk, a power of two in
 *                                     [64, 4096] (any other value runs at the
 *                                     default); results do not depend on it
 *   PCS_TUNE_REPLAY_TILE        [4096] manifest replay: bytes of a mapping
 *                                     section per decode work item (one wave),
 *                                     a power of two in [64, 4096]; setting any
 *                                     other value fails; results do not depend
 *                                     on it (sweep: profiles/replay/replay_rate.txt)
 * Keys 4, 5, 10, 12, 14, 16-22, 25, 29 and 32 selected variants that measured slower or no
 * better (XXH64 quad nt loads, in-place stamp widths, descriptor tile sorts,
 * 4 KiB slices, wave-dealt pages and slice streams, pipelined split-page
 * tiles, plain result stores, 4 KiB-aligned descriptor steps, a 4-waves-
 * per-SIMD descriptor body; round 3: an XXH64 direct-to-LDS segment ring,
 * XXH64 tile-order chunks; round 4: XXH64 equal-byte runs per quad; round 5:
 * validate-service polls kept in flight);
 * they were retired: setting one fails and reading one
 * returns -1. */
enum pcs_tune_key {
    PCS_TUNE_XXH3_BLOCKS_PER_CU = 1,
    PCS_TUNE_XXH64_BLOCKS_PER_CU = 2,
    PCS_TUNE_NT_LOADS = 3,
    PCS_TUNE_XXH64_LAYOUT = 6,
    PCS_TUNE_ZERO_COPY = 7,
    PCS_TUNE_XXH3_RT_BATCH = 8,
    PCS_TUNE_XXH3_SPLIT_PAGES = 9,
    PCS_TUNE_INLINE_LIST = 11,
    PCS_TUNE_MANIFEST_WIDE = 13,
    PCS_TUNE_XXH64_WAVES = 15,
    PCS_TUNE_ZC_POLL = 23,
    PCS_TUNE_SERVICE_STREAM = 24,
    PCS_TUNE_SERVICE_TEAR_TEST = 26,
    PCS_TUNE_FAIL_INJECT = 27,
    PCS_TUNE_SERVICE_MAX_CALLERS = 28,
    PCS_TUNE_SERVICE_REPOST_TEST = 30,
    PCS_TUNE_ZC_STAMP_POLL_PAGES = 31,
    PCS_TUNE_SERVICE_SLOW_EXIT_TEST = 33,
    PCS_TUNE_ZC_BATCH_EVENT = 34,
    PCS_TUNE_SYNC_SPIN_US = 35,
    PCS_TUNE_SERVICE_DEPARTURE = 36,
    PCS_TUNE_MANIFEST_WALK_TILE = 38, /* 37 was never assigned and stays unknown */
    PCS_TUNE_REPLAY_TILE = 39,
};
int pcs_set_tuning(int key, int64_t value);
int64_t pcs_get_tuning(int key); /* -1 for an unknown key */

/* ---- path counters ----------------------------------------------------------
 * Process-wide counts of how host batches were served (monotonic). */
enum pcs_counter {
    PCS_COUNTER_ZERO_COPY_LAUNCHES = 0, /* registered pages hashed in place */
    PCS_COUNTER_DIRECT_DMA_CHUNKS = 1,  /* contiguous pinned runs DMA'd as is */
    PCS_COUNTER_GATHER_CHUNKS = 2,      /* pages gathered into pinned staging */
    PCS_COUNTER_SERVICE_BATCHES = 3,    /* validate / stamp batches served by the pre-armed service */
    PCS_COUNTER_SERVICE_TORN_REQUESTS = 4, /* served requests whose line the kernel first saw torn
                                              (new seq, words failing the check word) and ignored */
    PCS_COUNTER_SERVICE_REPOSTS = 5,       /* service requests re-posted to a newer generation after
                                              the kernel they were posted to left unanswered */
};
uint64_t pcs_counter(int which); /* 0 for an unknown counter */

/* ---- workload tooling (benchmarks, tests, scrub drills) -------------------
 * Synthetic pages: word w of page p = splitmix64((seed ^ p) + (w+1) *
 * 0x9E3779B97F4A7C15), p = first_page_index + i. */
int pcs_gen_pages_dev(void *d_pages, uint64_t page_size, uint64_t n_pages, uint64_t seed,
                      uint64_t first_page_index, pcs_stream_t stream);
int pcs_gen_desc_dev(void *d_base, const uint64_t *d_off, const uint32_t *d_len, uint64_t n,
                     uint64_t seed, uint64_t first_page_index, pcs_stream_t stream);
/* XOR 0xFF into byte `byte_offset` of every `every`-th page (pages 0, every, ...). */
int pcs_flip_byte_dev(void *d_pages, uint64_t page_size, uint64_t n_pages, uint64_t every,
                      uint64_t byte_offset, pcs_stream_t stream);
/* Streaming-read ceiling: a plain read of [d_buf, d_buf + bytes) (16-byte
 * aligned; a trailing partial 16 bytes is ignored) with the headline hash
 * kernel's exact structure and load pattern (256-thread workgroups of 16 four-
 * KiB "pages", XCD-contiguous tile order, nt dwordx4 loads, one 128-byte
 * result store per tile) and no hash: each 4 KiB page folded into one word,
 * d_out[0 .. ceil(bytes / 4096)).  The roofline's measured companion: the
 * hash kernels are compared with the rate at which the same bytes can merely
 * be read the same way.  (ABI 6: one word per 4 KiB; rounds 2-5 wrote one
 * per 64 KiB window.) */
int pcs_stream_read_dev(const void *d_buf, uint64_t bytes, uint64_t *d_out, pcs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ELOQSTORE_PCS_H */
