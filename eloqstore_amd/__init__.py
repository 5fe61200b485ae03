"""eloqstore_amd — Python binding of the MI355X page-checksum engine.

The product is the native library ``libeloqstore_pcs.so`` (HIP kernels for
gfx950 + C ABI declared in ``include/eloqstore_pcs.h`` + the C++ drop-in
``include/eloqstore/page_checksum.h``).  This module is the thin ctypes layer
the tests and ``bench.py`` drive it through; device memory and streams come
from PyTorch (plumbing only).  There is no CPU fallback: every compute call
raises ``PcsError`` when the library or the GPU is unavailable.

Mirrors the reference call surface (src/storage/page.cpp:18-31):
``set_checksum`` / ``validate_checksum`` on one host page, plus batched
device and host forms.
"""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np

import torch  # noqa: F401  (loads the process's HIP runtime before the library)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(HERE, "libeloqstore_pcs.so")
DROPIN_LIB_PATH = os.path.join(HERE, "libeloqstore_pcs_dropin.so")  # opt-in single-page C++ symbols
TOOL_PATH = os.path.join(HERE, "page_checksum_tool")
HEADER_PATH = os.path.join(ROOT, "include", "eloqstore_pcs.h")

XXH3_64 = 0
XXH64 = 1
PCS_OK = 0
PCS_ERR_INVALID = -1
PCS_ERR_NO_DEVICE = -2
PCS_ERR_HIP = -3
PCS_ERR_NOMEM = -4

_u64, _u32, _i32, _vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p
_P = ctypes.POINTER

# name -> argtypes (restype int unless listed in _STR)
_SIGS = {
    "pcs_device_count": [_P(_i32)],
    "pcs_set_device": [_i32],
    "pcs_synchronize": [_vp],
    "pcs_pages_digest_dev": [_vp, _u64, _u64, _i32, _vp, _vp],
    "pcs_pages_validate_dev": [_vp, _u64, _u64, _i32, _vp, _vp, _vp],
    "pcs_pages_stamp_dev": [_vp, _u64, _u64, _i32, _vp],
    "pcs_pages_scrub_dev": [_vp, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _vp],
    "pcs_pages_scrub_host": [_vp, _u64, _u64, _vp, _vp, _vp, _vp, _u64],
    "pcs_scrub_extents_dev": [_vp, _u64, _vp, _vp, _u64, _vp],
    "pcs_pages_scrub_extents_host": [_vp, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64],
    "pcs_scrub_files_dev": [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp],
    "pcs_pages_scrub_files_host": [_vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _u64],
    "pcs_desc_digest_dev": [_vp, _vp, _vp, _u64, _i32, _vp, _vp],
    "pcs_desc_validate_dev": [_vp, _vp, _vp, _u64, _i32, _vp, _vp, _vp],
    "pcs_desc_stamp_dev": [_vp, _vp, _vp, _u64, _i32, _vp],
    "pcs_xxh3_64_ranges_dev": [_vp, _vp, _vp, _u64, _vp, _vp],
    "pcs_xxh64_ranges_dev": [_vp, _vp, _vp, _u64, _u64, _vp, _vp],
    "pcs_pages_validate_host": [_vp, _u64, _u64, _i32, _vp, _vp],
    "pcs_pages_validate_host_ex": [_vp, _u64, _u64, _i32, _vp, _vp, _u32],
    "pcs_pages_stamp_host": [_vp, _u64, _u64, _i32],
    "pcs_pages_digest_host": [_vp, _u64, _u64, _i32, _vp],
    "pcs_shard_range": [_u64, _i32, _i32, _P(_u64), _P(_u64)],
    "pcs_gen_pages_dev": [_vp, _u64, _u64, _u64, _u64, _vp],
    "pcs_gen_desc_dev": [_vp, _vp, _vp, _u64, _u64, _u64, _vp],
    "pcs_flip_byte_dev": [_vp, _u64, _u64, _u64, _u64, _vp],
    "pcs_stream_read_dev": [_vp, _u64, _vp, _vp],
    "pcs_host_alloc_pinned": [_u64, _P(_vp)],
    "pcs_host_free_pinned": [_vp],
    "pcs_host_register": [_vp, _u64],
    "pcs_host_unregister": [_vp],
    "pcs_batch_create": [_P(_vp)],
    "pcs_batch_submit": [_vp, _i32, _vp, _u64, _u64, _i32],
    "pcs_batch_submit_ex": [_vp, _i32, _vp, _u64, _u64, _i32, _u32],
    "pcs_batch_poll": [_vp],
    "pcs_batch_wait": [_vp],
    "pcs_batch_result": [_vp, _vp, _vp, _vp],
    "pcs_batch_destroy": [_vp],
    "pcs_manifest_checksum_dev": [_vp, _u64, _vp, _vp],
    "pcs_manifest_checksum_host": [_vp, _u64, _P(_u64)],
    "pcs_manifest_validate_host": [_vp, _u64, _P(_i32)],
    "pcs_manifest_scan_dev": [_vp, _u64, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _u64, _vp],
    "pcs_manifest_scan_host": [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _u64],
    "pcs_manifest_replay_dev": [_vp, _u64, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _u64, _vp],
    "pcs_manifest_replay_host": [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _u64],
    "pcs_scrub_live_dev": [_vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp],
    "pcs_scrub_live_host": [_vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _u64],
    "pcs_tree_check_dev": [_vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _u64, _vp],
    "pcs_tree_check_host": [_vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _u64],
    "pcs_leaf_check_dev": [_vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp],
    "pcs_leaf_check_host": [_vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u64],
    "pcs_set_tuning": [_i32, ctypes.c_int64],
    "pcs_get_tuning": [_i32],
    "pcs_counter": [_i32],
    "pcs_service_start": [_i32, _u32],
    "pcs_service_start_ex": [_i32, _i32, _u32],
    "pcs_service_stop": [],
    "pcs_service_running": [],
    "pcs_last_path": [],
    "pcs_thread_prepare": [],
    "pcs_batch_path": [_vp],
    "pcs_version": [],
    "pcs_abi_version": [],
    "pcs_last_error": [],
}
_STR = {"pcs_version", "pcs_last_error"}
_I64 = {"pcs_get_tuning", "pcs_counter"}


class PcsError(RuntimeError):
    def __init__(self, fn: str, code: int, msg: str):
        super().__init__(f"{fn} failed ({code}): {msg}")
        self.code = code


_lib = None


def lib() -> ctypes.CDLL:
    """Load libeloqstore_pcs.so (built by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PcsError("load", PCS_ERR_NO_DEVICE,
                           f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        so = ctypes.CDLL(LIB_PATH)
        for name, args in _SIGS.items():
            f = getattr(so, name)
            f.argtypes = args
            f.restype = ctypes.c_char_p if name in _STR else ctypes.c_int64 if name in _I64 else ctypes.c_int
        _lib = so
    return _lib


def header_functions(path: str = HEADER_PATH) -> list[str]:
    """Every pcs_* function declared in the public C header."""
    with open(path) as f:
        text = f.read()
    return sorted(set(re.findall(r"\b(pcs_[a-z0-9_]+)\s*\(", text)))


def _check(fn: str, rc: int) -> None:
    if rc != PCS_OK:
        raise PcsError(fn, rc, lib().pcs_last_error().decode(errors="replace"))


def _call(fn: str, *args) -> None:
    _check(fn, getattr(lib(), fn)(*args))


def _ptr(t) -> int:
    if t is None:
        return 0
    if isinstance(t, int):
        return t
    return t.data_ptr()


def _stream(stream) -> int:
    if stream is None:
        return torch.cuda.current_stream().cuda_stream
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


TUNE_XXH3_BLOCKS_PER_CU = 1
TUNE_XXH64_BLOCKS_PER_CU = 2
TUNE_NT_LOADS = 3
TUNE_XXH64_LAYOUT = 6
TUNE_ZERO_COPY = 7
TUNE_XXH3_RT_BATCH = 8
TUNE_XXH3_SPLIT_PAGES = 9
TUNE_INLINE_LIST = 11
TUNE_MANIFEST_WIDE = 13
TUNE_XXH64_WAVES = 15
TUNE_ZC_POLL = 23
TUNE_SERVICE_STREAM = 24
TUNE_SERVICE_TEAR_TEST = 26  # test only
TUNE_FAIL_INJECT = 27  # test only
TUNE_SERVICE_MAX_CALLERS = 28
TUNE_SERVICE_REPOST_TEST = 30  # test only
TUNE_ZC_STAMP_POLL_PAGES = 31
TUNE_SERVICE_SLOW_EXIT_TEST = 33  # test only
TUNE_ZC_BATCH_EVENT = 34
TUNE_SYNC_SPIN_US = 35
TUNE_SERVICE_DEPARTURE = 36
TUNE_MANIFEST_WALK_TILE = 38
TUNE_REPLAY_TILE = 39

# PCS_PATH_* bits (pcs_last_path / pcs_batch_path)
PATH_SERVED = 1
PATH_LAUNCHED = 2
PATH_FALLBACK = 4
PATH_REPOSTED = 8
PATH_NEW_GENERATION = 16
PATH_LOCK_SKIPPED = 32

COUNTER_ZERO_COPY_LAUNCHES = 0
COUNTER_DIRECT_DMA_CHUNKS = 1
COUNTER_GATHER_CHUNKS = 2
COUNTER_SERVICE_BATCHES = 3
COUNTER_SERVICE_TORN_REQUESTS = 4
COUNTER_SERVICE_REPOSTS = 5


def counter(which: int) -> int:
    """pcs_counter: how host batches were served (process-wide, monotonic)."""
    return int(lib().pcs_counter(which))


def set_tuning(key: int, value: int) -> None:
    _call("pcs_set_tuning", key, value)


def get_tuning(key: int) -> int:
    return int(lib().pcs_get_tuning(key))


def version() -> str:
    return lib().pcs_version().decode()


ABI_VERSION = 7  # PCS_ABI_VERSION of include/eloqstore_pcs.h this binding was written for


def abi_version() -> int:
    return int(lib().pcs_abi_version())


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = lib().pcs_device_count(ctypes.byref(n))
    return n.value if rc == PCS_OK else 0


def shard_range(n: int, world: int, rank: int) -> tuple[int, int]:
    b, e = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _call("pcs_shard_range", n, world, rank, ctypes.byref(b), ctypes.byref(e))
    return b.value, e.value


# ---- device-resident batches (torch tensors on cuda) ------------------------

def pages_digest(pages, page_size: int, n: int, algo: int = XXH3_64, out=None, stream=None):
    """digests[i] = hash of page i over [8, page_size); pages: uint8 device tensor."""
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=pages.device)
    _call("pcs_pages_digest_dev", _ptr(pages), page_size, n, algo, _ptr(out), _stream(stream))
    return out


def pages_validate(pages, page_size: int, n: int, algo: int = XXH3_64, ok=None, first_bad=None, stream=None):
    if ok is None:
        ok = torch.empty(n, dtype=torch.uint8, device=pages.device)
    if first_bad is None:
        first_bad = torch.empty(1, dtype=torch.int64, device=pages.device)
    _call("pcs_pages_validate_dev", _ptr(pages), page_size, n, algo, _ptr(ok), _ptr(first_bad), _stream(stream))
    return ok, first_bad


def pages_stamp(pages, page_size: int, n: int, algo: int = XXH3_64, stream=None) -> None:
    _call("pcs_pages_stamp_dev", _ptr(pages), page_size, n, algo, _stream(stream))


PAGE_CORRUPT, PAGE_OK, PAGE_BLANK = 0, 1, 2  # pcs_page_class
_SUMMARY_WORDS = 12  # pcs_scrub_summary
TYPE_BUCKETS = ("nonleaf_index", "leaf_index", "data", "overflow", "deleted", "other")
NO_PAGE = (1 << 64) - 1  # first_corrupt when no page is corrupt


def summary_dict(words) -> dict:
    """pcs_scrub_summary (12 u64 words) as a dict."""
    w = [int(x) & NO_PAGE for x in words]
    return {"n_pages": w[0], "n_ok": w[1], "n_corrupt": w[2], "n_blank": w[3], "ok_by_type": w[4:10],
            "first_corrupt": w[10], "n_listed": w[11]}


def pages_scrub_async(pages, page_size: int, n: int, cls=None, types=None, summary=None, corrupt=None,
                      corrupt_cap: int = 1024, stream=None):
    """pcs_pages_scrub_dev, enqueue only: returns the device tensors (cls,
    types, summary words, corrupt list), valid once the stream is synchronised.
    types=False passes a NULL type array; cap 0 passes a NULL list."""
    if cls is None:
        cls = torch.empty(n, dtype=torch.uint8, device=pages.device)
    if types is None:
        types = torch.empty(n, dtype=torch.uint8, device=pages.device)
    if summary is None:
        summary = torch.empty(_SUMMARY_WORDS, dtype=torch.int64, device=pages.device)
    if corrupt is None and corrupt_cap:
        corrupt = torch.empty(corrupt_cap, dtype=torch.int64, device=pages.device)
    _call("pcs_pages_scrub_dev", _ptr(pages), page_size, n, _ptr(cls), _ptr(None if types is False else types),
          _ptr(summary), _ptr(corrupt) if corrupt_cap else 0, corrupt_cap, _stream(stream))
    return cls, (None if types is False else types), summary, corrupt


def pages_scrub(pages, page_size: int, n: int, cls=None, types=None, corrupt_cap: int = 1024, stream=None):
    """Classify n device pages (PAGE_OK / PAGE_BLANK / PAGE_CORRUPT), report
    their type bytes, count them and list the smallest corrupt page indices:
    -> (cls, types, summary dict, corrupt tensor of n_listed indices).  Waits
    for the stream (the summary is read on the host)."""
    cls, types, summary, corrupt = pages_scrub_async(pages, page_size, n, cls, types, None, None, corrupt_cap, stream)
    if stream is not None:  # the copy below is ordered on torch's current stream only
        _call("pcs_synchronize", _stream(stream))
    d = summary_dict(summary.cpu().tolist())
    listed = corrupt[: d["n_listed"]] if corrupt is not None else torch.empty(0, dtype=torch.int64, device=pages.device)
    return cls, types, d, listed


_EXTENT_WORDS = 12  # pcs_extent_summary
_EXTENT_FIELDS = ("n_pages", "n_runs", "n_listed", "written_pages", "n_blank", "n_blank_runs", "first_blank",
                  "n_holes", "n_hole_pages", "first_hole", "first_class", "last_class")
# pcs_extent: 24 bytes, 3 u64 words on the device
EXTENT_DTYPE = np.dtype([("first_page", "<u8"), ("n_pages", "<u8"), ("cls", "<u4"), ("reserved", "<u4")])


def extent_dict(words) -> dict:
    """pcs_extent_summary (12 u64 words) as a dict."""
    return {k: int(x) & NO_PAGE for k, x in zip(_EXTENT_FIELDS, words)}


def scrub_extents_async(cls, n: int | None = None, summary=None, runs=None, run_cap: int = 1024, stream=None):
    """pcs_scrub_extents_dev, enqueue only: cls is a device uint8 tensor of
    class bytes (or any slice of one); returns the device tensors (summary
    words, runs as run_cap x 3 int64 words), valid once the stream is
    synchronised.  run_cap 0 passes a NULL run list."""
    if n is None:
        n = cls.numel()
    if summary is None:
        summary = torch.empty(_EXTENT_WORDS, dtype=torch.int64, device=cls.device)
    if runs is None and run_cap:
        runs = torch.empty((run_cap, 3), dtype=torch.int64, device=cls.device)
    _call("pcs_scrub_extents_dev", _ptr(cls), n, _ptr(summary), _ptr(runs) if run_cap else 0, run_cap,
          _stream(stream))
    return summary, runs


def scrub_extents(cls, n: int | None = None, run_cap: int = 1024, stream=None):
    """The maximal runs of equal class in a scrub's class bytes and the
    written extent / blank tail / holes summary: -> (summary dict, structured
    array (EXTENT_DTYPE) of the n_listed first runs).  Waits for the stream."""
    summary, runs = scrub_extents_async(cls, n, None, None, run_cap, stream)
    if stream is not None:  # the copies below are ordered on torch's current stream only
        _call("pcs_synchronize", _stream(stream))
    d = extent_dict(summary.cpu().tolist())
    if runs is None or d["n_listed"] == 0:
        return d, np.zeros(0, dtype=EXTENT_DTYPE)
    words = np.ascontiguousarray(runs[: d["n_listed"]].cpu().numpy())
    return d, words.view(EXTENT_DTYPE).reshape(-1)


_FILE_REPORT_WORDS = 16  # pcs_file_report
_FILES_SUMMARY_WORDS = 12  # pcs_files_summary
_FILES_SUMMARY_FIELDS = ("n_files", "n_pages", "n_ok", "n_corrupt", "n_blank", "n_corrupt_files", "n_hole_files",
                         "n_bad_files", "n_unwritten_files", "first_bad_file", "n_listed", "invalid_file")
# pcs_file_report: 128 bytes, 16 u64 words on the device and on the host
FILE_REPORT_DTYPE = np.dtype([("first_page", "<u8"), ("n_pages", "<u8"), ("n_ok", "<u8"), ("n_corrupt", "<u8"),
                              ("n_blank", "<u8"), ("ok_by_type", "<u8", (6,)), ("first_corrupt", "<u8"),
                              ("written_pages", "<u8"), ("n_holes", "<u8"), ("n_hole_pages", "<u8"),
                              ("first_hole", "<u8")])


def file_report_dict(rec) -> dict:
    """One pcs_file_report (a FILE_REPORT_DTYPE record or 16 u64 words) as a dict."""
    if getattr(rec, "dtype", None) != FILE_REPORT_DTYPE:
        rec = np.array([int(x) & NO_PAGE for x in rec], dtype=np.uint64).view(FILE_REPORT_DTYPE)[0]
    return {k: rec[k].tolist() if k == "ok_by_type" else int(rec[k]) for k in FILE_REPORT_DTYPE.names}


def files_summary_dict(words) -> dict:
    """pcs_files_summary (12 u64 words) as a dict."""
    return {k: int(x) & NO_PAGE for k, x in zip(_FILES_SUMMARY_FIELDS, words)}


def scrub_files_async(cls, types, file_first, n: int | None = None, n_files: int | None = None, reports=None,
                      summary=None, bad=None, bad_cap: int = 1024, stream=None):
    """pcs_scrub_files_dev, enqueue only: cls and types are device uint8
    tensors of a scrub's class and type bytes, file_first a device int64
    tensor of n_files + 1 page boundaries; returns the device tensors (reports
    as n_files x 16 int64 words, summary words, bad file indices), valid once
    the stream is synchronised.  bad_cap 0 passes a NULL list."""
    if n is None:
        n = cls.numel()
    if n_files is None:
        n_files = file_first.numel() - 1
    if reports is None:
        reports = torch.empty((max(n_files, 1), _FILE_REPORT_WORDS), dtype=torch.int64, device=cls.device)
    if summary is None:
        summary = torch.empty(_FILES_SUMMARY_WORDS, dtype=torch.int64, device=cls.device)
    if bad is None and bad_cap:
        bad = torch.empty(bad_cap, dtype=torch.int64, device=cls.device)
    _call("pcs_scrub_files_dev", _ptr(cls), _ptr(types), n, _ptr(file_first), n_files, _ptr(reports), _ptr(summary),
          _ptr(bad) if bad_cap else 0, bad_cap, _stream(stream))
    return reports, summary, bad


def scrub_files(cls, types, file_first, bad_cap: int = 1024, stream=None):
    """One report per data file of a scrubbed batch: -> (structured array
    (FILE_REPORT_DTYPE) of n_files reports, summary dict, array of the
    n_listed smallest bad file indices).  file_first may be a device tensor or
    any host sequence of n_files + 1 ascending page boundaries.  Waits for the
    stream.  With invalid boundaries (summary["invalid_file"] set) the reports
    are not written and come back empty."""
    if not isinstance(file_first, torch.Tensor):
        host = np.ascontiguousarray(file_first, dtype=np.uint64).view(np.int64)
        file_first = torch.from_numpy(host).to(cls.device)
    n_files = file_first.numel() - 1
    reports, summary, bad = scrub_files_async(cls, types, file_first, None, n_files, None, None, None, bad_cap, stream)
    if stream is not None:  # the copies below are ordered on torch's current stream only
        _call("pcs_synchronize", _stream(stream))
    d = files_summary_dict(summary.cpu().tolist())
    if d["invalid_file"] != NO_PAGE:
        return np.zeros(0, dtype=FILE_REPORT_DTYPE), d, np.zeros(0, dtype=np.uint64)
    recs = np.ascontiguousarray(reports[:n_files].cpu().numpy()).view(np.uint64).view(FILE_REPORT_DTYPE).reshape(-1)
    listed = bad[: d["n_listed"]].cpu().numpy().view(np.uint64) if bad is not None else np.zeros(0, dtype=np.uint64)
    return recs, d, listed


def desc_digest(base, off, length, n: int, algo: int = XXH3_64, out=None, stream=None):
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=base.device)
    _call("pcs_desc_digest_dev", _ptr(base), _ptr(off), _ptr(length), n, algo, _ptr(out), _stream(stream))
    return out


def desc_validate(base, off, length, n: int, algo: int = XXH3_64, ok=None, first_bad=None, stream=None):
    if ok is None:
        ok = torch.empty(n, dtype=torch.uint8, device=base.device)
    if first_bad is None:
        first_bad = torch.empty(1, dtype=torch.int64, device=base.device)
    _call("pcs_desc_validate_dev", _ptr(base), _ptr(off), _ptr(length), n, algo, _ptr(ok), _ptr(first_bad),
          _stream(stream))
    return ok, first_bad


def desc_stamp(base, off, length, n: int, algo: int = XXH3_64, stream=None) -> None:
    _call("pcs_desc_stamp_dev", _ptr(base), _ptr(off), _ptr(length), n, algo, _stream(stream))


def xxh3_64_ranges(base, off, length, n: int, out=None, stream=None):
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=base.device)
    _call("pcs_xxh3_64_ranges_dev", _ptr(base), _ptr(off), _ptr(length), n, _ptr(out), _stream(stream))
    return out


def xxh64_ranges(base, off, length, n: int, seed: int = 0, out=None, stream=None):
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=base.device)
    _call("pcs_xxh64_ranges_dev", _ptr(base), _ptr(off), _ptr(length), n, seed, _ptr(out), _stream(stream))
    return out


def gen_pages(pages, page_size: int, n: int, seed: int, first_page: int = 0, stream=None) -> None:
    _call("pcs_gen_pages_dev", _ptr(pages), page_size, n, seed, first_page, _stream(stream))


def gen_desc(base, off, length, n: int, seed: int, first_page: int = 0, stream=None) -> None:
    _call("pcs_gen_desc_dev", _ptr(base), _ptr(off), _ptr(length), n, seed, first_page, _stream(stream))


def flip_byte(pages, page_size: int, n: int, every: int, byte_offset: int = 10, stream=None) -> None:
    _call("pcs_flip_byte_dev", _ptr(pages), page_size, n, every, byte_offset, _stream(stream))


def stream_read(buf, nbytes: int, out, stream=None) -> None:
    """pcs_stream_read_dev: plain streaming read of nbytes (the read ceiling);
    out receives one folded u64 per 4 KiB page (ceil(nbytes / 4096) words)."""
    _call("pcs_stream_read_dev", _ptr(buf), nbytes, _ptr(out), _stream(stream))


def manifest_checksum_host(content: bytes) -> int:
    """ManifestBuilder::CalcChecksum (root_meta.cpp:150-174) on the GPU."""
    buf = (ctypes.c_char * max(1, len(content))).from_buffer_copy(content or b"\0")
    out = ctypes.c_uint64(0)
    _call("pcs_manifest_checksum_host", buf, len(content), ctypes.byref(out))
    return out.value


def manifest_validate_host(record: bytes) -> bool:
    buf = (ctypes.c_char * max(1, len(record))).from_buffer_copy(record or b"\0")
    v = ctypes.c_int(0)
    _call("pcs_manifest_validate_host", buf, len(record), ctypes.byref(v))
    return bool(v.value)


# pcs_manifest_record (40 bytes), pcs_manifest_report and pcs_manifest_summary (12 u64 words each)
MANIFEST_RECORD_DTYPE = np.dtype([("offset", "<u8"), ("stored", "<u8"), ("computed", "<u8"), ("payload_len", "<u4"),
                                  ("root", "<u4"), ("ttl_root", "<u4"), ("ok", "<u4")])
MANIFEST_REPORT_DTYPE = np.dtype([(k, "<u8") for k in (
    "size", "n_records", "n_ok", "n_corrupt", "first_corrupt", "n_ok_after_corrupt", "valid_prefix_bytes",
    "end_offset", "end_reason", "verdict", "first_record", "max_record_bytes")])
MANIFEST_SUMMARY_DTYPE = np.dtype([("n_images", "<u8"), ("n_records", "<u8"), ("n_ok", "<u8"), ("n_corrupt", "<u8"),
                                   ("n_by_verdict", "<u8", (5,)), ("first_bad_image", "<u8"), ("n_listed", "<u8"),
                                   ("invalid_image", "<u8")])
MANIFEST_END = ("clean", "short_header", "short_payload", "short_padding")
MANIFEST_VERDICT = ("clean", "torn_tail", "broken", "bad_snapshot", "empty")


def manifest_scan_async(base, img_off, img_size, align: int = 4096, total_bytes: int | None = None,
                        n_images: int | None = None, reports=None, summary=None, records=None,
                        record_cap: int = 1024, stream=None):
    """pcs_manifest_scan_dev, enqueue only: base is a device uint8 tensor that
    holds the images, img_off / img_size device int64 tensors of their offsets
    and sizes; returns the device tensors (reports as n_images x 12 int64
    words, the 12 summary words, records as record_cap x 40 bytes), valid once
    the stream is synchronised.  record_cap 0 passes a NULL record array."""
    if total_bytes is None:
        total_bytes = base.numel()
    if n_images is None:
        n_images = img_off.numel()
    if reports is None:
        reports = torch.empty((max(n_images, 1), 12), dtype=torch.int64, device=base.device)
    if summary is None:
        summary = torch.empty(12, dtype=torch.int64, device=base.device)
    if records is None and record_cap:
        records = torch.empty((record_cap, 5), dtype=torch.int64, device=base.device)
    _call("pcs_manifest_scan_dev", _ptr(base), total_bytes, _ptr(img_off), _ptr(img_size), n_images, align,
          _ptr(reports), _ptr(summary), _ptr(records) if record_cap else 0, record_cap, _stream(stream))
    return reports, summary, records


def manifest_scan_dev(base, img_off, img_size, align: int = 4096, record_cap: int = 1024, total_bytes: int | None = None,
                      stream=None):
    """Walk and verify every record of the manifest images held in the device
    tensor base -> (reports (MANIFEST_REPORT_DTYPE, one per image), summary
    (one MANIFEST_SUMMARY_DTYPE record), the n_listed records
    (MANIFEST_RECORD_DTYPE)).  img_off / img_size may be device tensors or host
    sequences.  Waits for the stream.  With an invalid layout
    (summary["invalid_image"] set) reports and records come back empty."""
    def dev(x):
        if isinstance(x, torch.Tensor):
            return x
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).to(base.device)
    img_off, img_size = dev(img_off), dev(img_size)
    n = img_off.numel()
    reports, summary, records = manifest_scan_async(base, img_off, img_size, align, total_bytes, n, None, None, None,
                                                    record_cap, stream)
    if stream is not None:  # the copies below are ordered on torch's current stream only
        _call("pcs_synchronize", _stream(stream))
    s = np.ascontiguousarray(summary.cpu().numpy()).view(np.uint64).view(MANIFEST_SUMMARY_DTYPE)[0]
    if int(s["invalid_image"]) != NO_PAGE:
        return np.zeros(0, dtype=MANIFEST_REPORT_DTYPE), s, np.zeros(0, dtype=MANIFEST_RECORD_DTYPE)
    reps = np.ascontiguousarray(reports[:n].cpu().numpy()).view(np.uint64).view(MANIFEST_REPORT_DTYPE).reshape(-1)
    listed = int(s["n_listed"])
    recs = (np.ascontiguousarray(records[:listed].cpu().numpy()).view(np.uint8).view(MANIFEST_RECORD_DTYPE).reshape(-1)
            if listed else np.zeros(0, dtype=MANIFEST_RECORD_DTYPE))
    return reps, s, recs


def manifest_scan_host(images: list, align: int = 4096, record_cap: int = 1024):
    """pcs_manifest_scan_host over whole manifest images in host memory (bytes,
    bytearray, memoryview or uint8 numpy arrays, any alignment) -> (reports,
    summary, records) as manifest_scan_dev."""
    n = len(images)
    views = [np.frombuffer(b, dtype=np.uint8) if not isinstance(b, np.ndarray) else b for b in images]
    ptrs = np.array([v.ctypes.data if v.size else 0 for v in views], dtype=np.uint64)
    sizes = np.array([v.size for v in views], dtype=np.uint64)
    reports = np.zeros(max(1, n), dtype=MANIFEST_REPORT_DTYPE)
    summary = np.zeros(1, dtype=MANIFEST_SUMMARY_DTYPE)
    records = np.zeros(max(1, record_cap), dtype=MANIFEST_RECORD_DTYPE)
    _call("pcs_manifest_scan_host", ptrs.ctypes.data, sizes.ctypes.data, n, align, reports.ctypes.data,
          summary.ctypes.data, records.ctypes.data if record_cap else 0, record_cap)
    return reports[:n], summary[0], records[: int(summary[0]["n_listed"])]


# pcs_replay_report (16 u64 words), pcs_replay_summary (12), pcs_live_page (16 bytes), pcs_live_summary (16)
REPLAY_REPORT_DTYPE = np.dtype([(k, "<u8") for k in (
    "status", "n_replayed", "malformed_record", "root", "ttl_root", "max_fp_id", "dict_bytes", "snapshot_pages",
    "n_log_entries", "table_size", "table_first", "n_mapped", "min_fp", "max_fp", "n_fp_beyond_max", "n_term_pairs")])
REPLAY_SUMMARY_DTYPE = np.dtype([("n_images", "<u8"), ("n_by_status", "<u8", (4,)), ("n_rows", "<u8"),
                                 ("n_rows_written", "<u8"), ("n_mapped", "<u8"), ("n_log_entries", "<u8"),
                                 ("first_bad_image", "<u8"), ("invalid_image", "<u8"), ("reserved", "<u8")])
LIVE_PAGE_DTYPE = np.dtype([("index", "<u8"), ("page_id", "<u4"), ("cls", "<u4")])
LIVE_SUMMARY_DTYPE = np.dtype([(k, "<u8") for k in (
    "n_pages", "table_size", "n_mapped", "n_mapped_in_window", "n_duplicate", "live_ok", "live_blank",
    "live_corrupt", "dead_ok", "dead_blank", "dead_corrupt", "n_damaged", "first_damaged", "last_live", "n_listed",
    "reserved")])
REPLAY_OK, REPLAY_NOT_REPLAYABLE, REPLAY_MALFORMED, REPLAY_TABLE_CAP = range(4)
REPLAY_STATUS = ("ok", "not_replayable", "malformed", "table_cap")
MAPPING_INVALID = 7  # MappingSnapshot::InvalidValue: a table row nobody wrote
NO_OWNER = 0xFFFFFFFF


def manifest_replay_async(base, img_off, img_size, align: int = 4096, table_cap: int = 0, total_bytes: int | None = None,
                          n_images: int | None = None, scan_reports=None, reports=None, summary=None, table=None,
                          stream=None):
    """pcs_manifest_replay_dev, enqueue only: base, img_off and img_size as for
    manifest_scan_async; returns the device tensors (scan reports n x 12 int64
    words, or None when scan_reports is False; reports n x 16; the 12 summary
    words; the table of table_cap int64 rows, None when table_cap is 0), valid
    once the stream is synchronised."""
    if total_bytes is None:
        total_bytes = base.numel()
    if n_images is None:
        n_images = img_off.numel()
    if scan_reports is None:
        scan_reports = torch.empty((max(n_images, 1), 12), dtype=torch.int64, device=base.device)
    if reports is None:
        reports = torch.empty((max(n_images, 1), 16), dtype=torch.int64, device=base.device)
    if summary is None:
        summary = torch.empty(12, dtype=torch.int64, device=base.device)
    if table is None and table_cap:
        table = torch.empty(table_cap, dtype=torch.int64, device=base.device)
    _call("pcs_manifest_replay_dev", _ptr(base), total_bytes, _ptr(img_off), _ptr(img_size), n_images, align,
          _ptr(None if scan_reports is False else scan_reports), _ptr(reports), _ptr(summary),
          _ptr(table) if table_cap else 0, table_cap, _stream(stream))
    return (None if scan_reports is False else scan_reports), reports, summary, (table if table_cap else None)


def manifest_replay_dev(base, img_off, img_size, align: int = 4096, table_cap: int = 0, total_bytes: int | None = None,
                        stream=None):
    """Replay the manifest images held in the device tensor base -> (reports
    (REPLAY_REPORT_DTYPE, one per image), summary (one REPLAY_SUMMARY_DTYPE
    record), the n_rows_written table rows (uint64), scan reports
    (MANIFEST_REPORT_DTYPE)).  Image i's rows are table[table_first :
    table_first + table_size] when its status is REPLAY_OK.  Waits for the
    stream.  With an invalid layout everything but the summary is empty."""
    def dev(x):
        if isinstance(x, torch.Tensor):
            return x
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).to(base.device)
    img_off, img_size = dev(img_off), dev(img_size)
    n = img_off.numel()
    scan_reports, reports, summary, table = manifest_replay_async(base, img_off, img_size, align, table_cap,
                                                                  total_bytes, n, stream=stream)
    if stream is not None:  # the copies below are ordered on torch's current stream only
        _call("pcs_synchronize", _stream(stream))
    s = np.ascontiguousarray(summary.cpu().numpy()).view(np.uint64).view(REPLAY_SUMMARY_DTYPE)[0]
    if int(s["invalid_image"]) != NO_PAGE:
        return (np.zeros(0, dtype=REPLAY_REPORT_DTYPE), s, np.zeros(0, dtype=np.uint64),
                np.zeros(0, dtype=MANIFEST_REPORT_DTYPE))
    reps = np.ascontiguousarray(reports[:n].cpu().numpy()).view(np.uint64).view(REPLAY_REPORT_DTYPE).reshape(-1)
    sreps = np.ascontiguousarray(scan_reports[:n].cpu().numpy()).view(np.uint64).view(MANIFEST_REPORT_DTYPE).reshape(-1)
    rows = int(s["n_rows_written"])
    tab = (np.ascontiguousarray(table[:rows].cpu().numpy()).view(np.uint64) if rows else np.zeros(0, dtype=np.uint64))
    return reps, s, tab, sreps


def manifest_replay_host(images: list, align: int = 4096, table_cap: int = 0):
    """pcs_manifest_replay_host over whole manifest images in host memory ->
    (reports, summary, table rows, scan reports) as manifest_replay_dev."""
    n = len(images)
    views = [np.frombuffer(b, dtype=np.uint8) if not isinstance(b, np.ndarray) else b for b in images]
    ptrs = np.array([v.ctypes.data if v.size else 0 for v in views], dtype=np.uint64)
    sizes = np.array([v.size for v in views], dtype=np.uint64)
    scan_reports = np.zeros(max(1, n), dtype=MANIFEST_REPORT_DTYPE)
    reports = np.zeros(max(1, n), dtype=REPLAY_REPORT_DTYPE)
    summary = np.zeros(1, dtype=REPLAY_SUMMARY_DTYPE)
    table = np.zeros(max(1, table_cap), dtype=np.uint64)
    _call("pcs_manifest_replay_host", ptrs.ctypes.data, sizes.ctypes.data, n, align, scan_reports.ctypes.data,
          reports.ctypes.data, summary.ctypes.data, table.ctypes.data if table_cap else 0, table_cap)
    return reports[:n], summary[0], table[: int(summary[0]["n_rows_written"])], scan_reports[:n]


def scrub_live_async(cls, n_pages: int, fp_first: int, table, table_size: int | None = None, owner=None,
                     summary=None, damaged=None, damaged_cap: int = 1024, stream=None):
    """pcs_scrub_live_dev, enqueue only: cls is a scrub's device class bytes
    for file pages fp_first .. fp_first + n_pages, table a device int64 mapping
    table (None with table_size 0); returns the device tensors (owner uint32 as
    int32 words, or None when owner is False; the 16 summary words; the damaged
    list as damaged_cap x 2 int64 words), valid once the stream is synchronised."""
    device = cls.device
    if table_size is None:
        table_size = 0 if table is None else table.numel()
    if owner is None:
        owner = torch.empty(max(n_pages, 1), dtype=torch.int32, device=device)
    if summary is None:
        summary = torch.empty(16, dtype=torch.int64, device=device)
    if damaged is None and damaged_cap:
        damaged = torch.empty((damaged_cap, 2), dtype=torch.int64, device=device)
    _call("pcs_scrub_live_dev", _ptr(cls), n_pages, fp_first, _ptr(table) if table_size else 0, table_size,
          _ptr(None if owner is False else owner), _ptr(summary), _ptr(damaged) if damaged_cap else 0, damaged_cap,
          _stream(stream))
    return (None if owner is False else owner), summary, damaged


def scrub_live(cls, n_pages: int, fp_first: int, table, table_size: int | None = None, owner=None,
               damaged_cap: int = 1024, stream=None):
    """Which pages of a scrubbed window a replayed table still points to ->
    (owner (uint32 numpy array, NO_OWNER for dead pages; None when owner is
    False), summary (one LIVE_SUMMARY_DTYPE record), the n_listed damaged live
    pages (LIVE_PAGE_DTYPE)).  cls and table may be device tensors or host
    arrays.  Waits for the stream."""
    if not isinstance(cls, torch.Tensor):
        cls = torch.from_numpy(np.ascontiguousarray(cls, dtype=np.uint8)).cuda()
    if table is not None and not isinstance(table, torch.Tensor):
        table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint64).view(np.int64)).to(cls.device)
    owner, summary, damaged = scrub_live_async(cls, n_pages, fp_first, table, table_size, owner, None, None,
                                               damaged_cap, stream)
    if stream is not None:
        _call("pcs_synchronize", _stream(stream))
    s = np.ascontiguousarray(summary.cpu().numpy()).view(np.uint64).view(LIVE_SUMMARY_DTYPE)[0]
    listed = int(s["n_listed"])
    pages = (np.ascontiguousarray(damaged[:listed].cpu().numpy()).view(np.uint8).view(LIVE_PAGE_DTYPE).reshape(-1)
             if listed else np.zeros(0, dtype=LIVE_PAGE_DTYPE))
    own = None if owner is None else np.ascontiguousarray(owner[:n_pages].cpu().numpy()).view(np.uint32)
    return own, s, pages


def scrub_live_host(cls, fp_first: int, table, damaged_cap: int = 1024, want_owner: bool = True):
    """pcs_scrub_live_host over host arrays -> (owner, summary, damaged) as scrub_live."""
    cls = np.ascontiguousarray(cls, dtype=np.uint8)
    table = np.ascontiguousarray(table, dtype=np.uint64)
    n = cls.size
    owner = np.zeros(max(1, n), dtype=np.uint32)
    summary = np.zeros(1, dtype=LIVE_SUMMARY_DTYPE)
    damaged = np.zeros(max(1, damaged_cap), dtype=LIVE_PAGE_DTYPE)
    _call("pcs_scrub_live_host", cls.ctypes.data if n else 0, n, fp_first, table.ctypes.data if table.size else 0,
          table.size, owner.ctypes.data if want_owner else 0, summary.ctypes.data,
          damaged.ctypes.data if damaged_cap else 0, damaged_cap)
    return (owner[:n] if want_owner else None), summary[0], damaged[: int(summary[0]["n_listed"])]


# pcs_tree_node (16 bytes), pcs_tree_problem (16 bytes), pcs_tree_summary (32 u64 words)
TREE_NODE_DTYPE = np.dtype([("parent", "<u4"), ("depth", "u1"), ("tree", "u1"), ("type", "u1"), ("bits", "u1"),
                            ("n_children", "<u4"), ("n_bad_children", "<u4")])
TREE_PROBLEM_DTYPE = np.dtype([("page_id", "<u4"), ("parent", "<u4"), ("bits", "<u4"), ("depth", "<u4")])
TREE_SUMMARY_DTYPE = np.dtype([
    ("n_pages", "<u8"), ("table_size", "<u8"), ("n_mapped", "<u8"), ("n_reached", "<u8"), ("n_nonleaf", "<u8"),
    ("n_leaf_index", "<u8"), ("n_data", "<u8"), ("n_refs", "<u8"), ("n_extra_refs", "<u8"),
    ("n_out_of_range_refs", "<u8"), ("max_depth", "<u8"), ("n_depth_capped", "<u8"), ("n_by_bit", "<u8", (8,)),
    ("n_problems", "<u8"), ("first_problem", "<u8"), ("n_listed", "<u8"), ("n_unreached_mapped", "<u8"),
    ("unreached_by_type", "<u8", (6,)), ("n_unreached_unread", "<u8"), ("n_chain_heads", "<u8")])
(TREE_UNMAPPED, TREE_ABSENT, TREE_BLANK, TREE_CORRUPT, TREE_WRONG_TYPE, TREE_MALFORMED, TREE_BAD_CHILD,
 TREE_BAD_LINK) = (1 << k for k in range(8))
TREE_MAX_DEPTH = 16
TREE_CLASS_ABSENT = 3  # the class byte of a page that was not loaded


def tree_check_async(pages, page_size: int, n_pages: int, fp_first: int, cls, table, roots, n_roots: int = 2,
                     table_size: int | None = None, nodes=None, summary=None, problems=None, problem_cap: int = 1024,
                     stream=None):
    """pcs_tree_check_dev, enqueue only: pages and cls are the device bytes of
    the window's file pages and their scrub classes, table a device int64
    mapping table (None with table_size 0), roots a device int64 tensor or a
    device ADDRESS (for instance that of a replay report's root word) of
    n_roots words; returns the device tensors (nodes table_size x 2 int64 words,
    or None when nodes is False; the 32 summary words; the problems as
    problem_cap x 2 int64 words), valid once the stream is synchronised."""
    device = summary.device if summary is not None else cls.device if cls is not None else table.device
    if table_size is None:
        table_size = 0 if table is None else table.numel()
    if nodes is None:
        nodes = torch.empty((max(table_size, 1), 2), dtype=torch.int64, device=device)
    if summary is None:
        summary = torch.empty(32, dtype=torch.int64, device=device)
    if problems is None and problem_cap:
        problems = torch.empty((problem_cap, 2), dtype=torch.int64, device=device)
    _call("pcs_tree_check_dev", _ptr(pages) if n_pages else 0, page_size, n_pages, fp_first,
          _ptr(cls) if n_pages else 0, _ptr(table) if table_size else 0, table_size, _ptr(roots), n_roots,
          _ptr(None if nodes is False else nodes), _ptr(summary), _ptr(problems) if problem_cap else 0, problem_cap,
          _stream(stream))
    return (None if nodes is False else nodes), summary, problems


def _tree_roots(roots, device):
    if isinstance(roots, (torch.Tensor, int)):
        return roots, None
    r = np.ascontiguousarray(roots, dtype=np.uint64)
    return torch.from_numpy(r.view(np.int64).copy()).to(device), r.size


def tree_check(pages, page_size: int, n_pages: int, fp_first: int, cls, table, roots, n_roots: int | None = None,
               nodes=None, problem_cap: int = 1024, stream=None):
    """Walk the index tree from `roots` over device pages -> (nodes
    (TREE_NODE_DTYPE, one per table row; None when nodes is False), summary
    (one TREE_SUMMARY_DTYPE record), the n_listed problems
    (TREE_PROBLEM_DTYPE)).  table and roots may be device tensors or host
    arrays.  Waits for the stream."""
    device = pages.device
    if table is not None and not isinstance(table, torch.Tensor):
        table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint64).view(np.int64).copy()).to(device)
    roots, n = _tree_roots(roots, device)
    if n_roots is None:
        n_roots = n if n is not None else roots.numel() if isinstance(roots, torch.Tensor) else 2
    table_size = 0 if table is None else table.numel()
    nodes, summary, problems = tree_check_async(pages, page_size, n_pages, fp_first, cls, table, roots, n_roots,
                                                table_size, nodes, None, None, problem_cap, stream)
    if stream is not None:
        _call("pcs_synchronize", _stream(stream))
    s = np.ascontiguousarray(summary.cpu().numpy()).view(np.uint64).view(TREE_SUMMARY_DTYPE)[0]
    listed = int(s["n_listed"])
    probs = (np.ascontiguousarray(problems[:listed].cpu().numpy()).view(np.uint8).view(TREE_PROBLEM_DTYPE).reshape(-1)
             if listed else np.zeros(0, dtype=TREE_PROBLEM_DTYPE))
    nd = None
    if nodes is not None:
        nd = (np.ascontiguousarray(nodes[:table_size].cpu().numpy()).view(np.uint8).view(TREE_NODE_DTYPE).reshape(-1)
              if table_size else np.zeros(0, dtype=TREE_NODE_DTYPE))
    return nd, s, probs


def tree_check_host(pages, page_size: int, fp_first: int, cls, table, roots, problem_cap: int = 1024,
                    want_nodes: bool = True):
    """pcs_tree_check_host over host arrays (pages one contiguous uint8 buffer;
    cls None scrubs the pages on the device) -> (nodes, summary, problems) as
    tree_check."""
    pages = np.ascontiguousarray(pages, dtype=np.uint8).reshape(-1)
    n = pages.size // page_size
    if cls is not None:
        cls = np.ascontiguousarray(cls, dtype=np.uint8)
    table = np.ascontiguousarray(table, dtype=np.uint64)
    roots = np.ascontiguousarray(roots, dtype=np.uint64)
    nodes = np.zeros(max(1, table.size), dtype=TREE_NODE_DTYPE)
    summary = np.zeros(1, dtype=TREE_SUMMARY_DTYPE)
    problems = np.zeros(max(1, problem_cap), dtype=TREE_PROBLEM_DTYPE)
    _call("pcs_tree_check_host", pages.ctypes.data if n else 0, page_size, n, fp_first,
          cls.ctypes.data if cls is not None and n else 0, table.ctypes.data if table.size else 0, table.size,
          roots.ctypes.data, roots.size, nodes.ctypes.data if want_nodes else 0, summary.ctypes.data,
          problems.ctypes.data if problem_cap else 0, problem_cap)
    return (nodes[: table.size] if want_nodes else None), summary[0], problems[: int(summary[0]["n_listed"])]


# pcs_leaf_node (16 bytes), pcs_leaf_problem (16 bytes), pcs_leaf_summary (32 u64 words)
LEAF_NODE_DTYPE = np.dtype([("owner", "<u4"), ("owner_entry", "<u2"), ("bits", "<u2"), ("a", "<u4"), ("b", "<u4")])
LEAF_PROBLEM_DTYPE = np.dtype([("page_id", "<u4"), ("owner", "<u4"), ("bits", "<u4"), ("owner_entry", "<u4")])
LEAF_SUMMARY_DTYPE = np.dtype([
    ("n_pages", "<u8"), ("table_size", "<u8"), ("n_data_pages", "<u8"), ("n_data_ok", "<u8"), ("n_entries", "<u8"),
    ("n_overflow_values", "<u8"), ("n_expiring", "<u8"), ("n_compressed", "<u8"), ("inline_value_bytes", "<u8"),
    ("overflow_value_bytes", "<u8"), ("n_refs", "<u8"), ("n_out_of_range_refs", "<u8"), ("n_extra_refs", "<u8"),
    ("n_refs_to_tree", "<u8"), ("n_misplaced_pointers", "<u8"), ("n_chain_capped", "<u8"), ("max_groups", "<u8"),
    ("n_overflow_pages", "<u8"), ("n_by_bit", "<u8", (9,)), ("n_problems", "<u8"), ("first_problem", "<u8"),
    ("n_listed", "<u8"), ("n_leaked_overflow", "<u8"), ("n_overflow_ok", "<u8")])
LEAF_BAD_POINTER, LEAF_BAD_CHAIN, LEAF_SHARED = 64, 128, 256   # the low six bits are TREE_UNMAPPED .. TREE_MALFORMED
LEAF_MAX_GROUPS = 4096


def leaf_check_async(pages, page_size: int, n_pages: int, fp_first: int, cls, table, tree_nodes,
                     table_size: int | None = None, leaves=None, summary=None, problems=None,
                     problem_cap: int = 1024, stream=None):
    """pcs_leaf_check_dev, enqueue only: pages, cls and table as for
    tree_check_async, tree_nodes the node tensor a tree check over the same
    inputs wrote (on the same stream, or one this stream waits for); returns the
    device tensors (leaves table_size x 2 int64 words, or None when leaves is
    False; the 32 summary words; the problems as problem_cap x 2 int64 words),
    valid once the stream is synchronised."""
    device = summary.device if summary is not None else cls.device if cls is not None else table.device
    if table_size is None:
        table_size = 0 if table is None else table.numel()
    if leaves is None:
        leaves = torch.empty((max(table_size, 1), 2), dtype=torch.int64, device=device)
    if summary is None:
        summary = torch.empty(32, dtype=torch.int64, device=device)
    if problems is None and problem_cap:
        problems = torch.empty((problem_cap, 2), dtype=torch.int64, device=device)
    _call("pcs_leaf_check_dev", _ptr(pages) if n_pages else 0, page_size, n_pages, fp_first,
          _ptr(cls) if n_pages else 0, _ptr(table) if table_size else 0, table_size,
          _ptr(tree_nodes) if table_size else 0, _ptr(None if leaves is False else leaves), _ptr(summary),
          _ptr(problems) if problem_cap else 0, problem_cap, _stream(stream))
    return (None if leaves is False else leaves), summary, problems


def leaf_check(pages, page_size: int, n_pages: int, fp_first: int, cls, table, tree_nodes, leaves=None,
               problem_cap: int = 1024, stream=None):
    """Decode the data pages a tree check reached and walk their overflow chains
    over device pages -> (leaves (LEAF_NODE_DTYPE, one per table row; None when
    leaves is False), summary (one LEAF_SUMMARY_DTYPE record), the n_listed
    problems (LEAF_PROBLEM_DTYPE)).  table may be a device tensor or a host
    array; tree_nodes is tree_check_async's device tensor.  Waits for the
    stream."""
    device = pages.device
    if table is not None and not isinstance(table, torch.Tensor):
        table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint64).view(np.int64).copy()).to(device)
    table_size = 0 if table is None else table.numel()
    leaves, summary, problems = leaf_check_async(pages, page_size, n_pages, fp_first, cls, table, tree_nodes,
                                                 table_size, leaves, None, None, problem_cap, stream)
    if stream is not None:
        _call("pcs_synchronize", _stream(stream))
    s = np.ascontiguousarray(summary.cpu().numpy()).view(np.uint64).view(LEAF_SUMMARY_DTYPE)[0]
    listed = int(s["n_listed"])
    probs = (np.ascontiguousarray(problems[:listed].cpu().numpy()).view(np.uint8).view(LEAF_PROBLEM_DTYPE).reshape(-1)
             if listed else np.zeros(0, dtype=LEAF_PROBLEM_DTYPE))
    lv = None
    if leaves is not None:
        lv = (np.ascontiguousarray(leaves[:table_size].cpu().numpy()).view(np.uint8).view(LEAF_NODE_DTYPE).reshape(-1)
              if table_size else np.zeros(0, dtype=LEAF_NODE_DTYPE))
    return lv, s, probs


def leaf_check_host(pages, page_size: int, fp_first: int, cls, table, roots, problem_cap: int = 1024,
                    want_nodes: bool = True):
    """pcs_leaf_check_host over host arrays (pages one contiguous uint8 buffer;
    cls None scrubs the pages on the device): the tree check and the leaf check
    in one call -> (tree nodes, tree summary, leaves, leaf summary, leaf
    problems); both node arrays are None when want_nodes is False."""
    pages = np.ascontiguousarray(pages, dtype=np.uint8).reshape(-1)
    n = pages.size // page_size
    if cls is not None:
        cls = np.ascontiguousarray(cls, dtype=np.uint8)
    table = np.ascontiguousarray(table, dtype=np.uint64)
    roots = np.ascontiguousarray(roots, dtype=np.uint64)
    tree_nodes = np.zeros(max(1, table.size), dtype=TREE_NODE_DTYPE)
    tree_summary = np.zeros(1, dtype=TREE_SUMMARY_DTYPE)
    leaves = np.zeros(max(1, table.size), dtype=LEAF_NODE_DTYPE)
    summary = np.zeros(1, dtype=LEAF_SUMMARY_DTYPE)
    problems = np.zeros(max(1, problem_cap), dtype=LEAF_PROBLEM_DTYPE)
    _call("pcs_leaf_check_host", pages.ctypes.data if n else 0, page_size, n, fp_first,
          cls.ctypes.data if cls is not None and n else 0, table.ctypes.data if table.size else 0, table.size,
          roots.ctypes.data, roots.size, tree_nodes.ctypes.data if want_nodes else 0, tree_summary.ctypes.data,
          leaves.ctypes.data if want_nodes else 0, summary.ctypes.data, problems.ctypes.data if problem_cap else 0,
          problem_cap)
    return ((tree_nodes[: table.size] if want_nodes else None), tree_summary[0],
            (leaves[: table.size] if want_nodes else None), summary[0], problems[: int(summary[0]["n_listed"])])


class Batch:
    """Asynchronous host batch (pcs_batch_*): submit, poll without blocking, read results."""

    DIGEST, VALIDATE, STAMP = 0, 1, 2

    def __init__(self):
        self._b = ctypes.c_void_p()
        _call("pcs_batch_create", ctypes.byref(self._b))
        self._keep = None
        self.n = 0

    def submit(self, mode: int, pages: list, page_size: int, algo: int = XXH3_64, skip_verify: bool = False) -> None:
        arr, keep = _page_ptrs(pages)
        self._keep = (arr, keep)
        self.n = len(pages)
        self.mode = mode
        _call("pcs_batch_submit_ex", self._b, mode, arr, page_size, len(pages), algo, _flags(skip_verify))

    def submit_ptrs(self, mode: int, ptrs, page_size: int, algo: int = XXH3_64, skip_verify: bool = False) -> None:
        """Submit raw page addresses (a uint64 array of host pointers)."""
        ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
        self._keep = ptrs
        self.n = len(ptrs)
        self.mode = mode
        _call("pcs_batch_submit_ex", self._b, mode, ptrs.ctypes.data, page_size, len(ptrs), algo,
              _flags(skip_verify))

    def poll(self) -> bool:
        rc = lib().pcs_batch_poll(self._b)
        if rc < 0:
            _check("pcs_batch_poll", rc)
        return rc == 1

    def wait(self) -> None:
        _call("pcs_batch_wait", self._b)

    def path(self) -> int:
        """PCS_PATH_* bits of the last submission (which path served it)."""
        return int(lib().pcs_batch_path(self._b))

    def result(self):
        fb = ctypes.c_uint64(0)
        if self.mode == self.VALIDATE:
            ok = (ctypes.c_uint8 * max(1, self.n))()
            _call("pcs_batch_result", self._b, ok, None, ctypes.byref(fb))
            return list(ok)[: self.n], (None if fb.value == (1 << 64) - 1 else fb.value)
        dig = (ctypes.c_uint64 * max(1, self.n))()
        _call("pcs_batch_result", self._b, None, dig, ctypes.byref(fb))
        return list(dig)[: self.n]

    def close(self) -> None:
        if self._b:
            lib().pcs_batch_destroy(self._b)
            self._b = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- host-memory forms (reference call surface) ------------------------------

FLAG_NONE, FLAG_SKIP_VERIFY = 0, 1  # pcs_flags


def _flags(skip_verify: bool) -> int:
    """KvOptions::skip_verify_checksum (kv_options.h:41) -> PCS_FLAG_SKIP_VERIFY."""
    return FLAG_SKIP_VERIFY if skip_verify else FLAG_NONE


def _page_ptrs(pages: list) -> tuple:
    bufs = [p if isinstance(p, ctypes.Array) else (ctypes.c_char * len(p)).from_buffer(p) for p in pages]
    arr = (ctypes.c_void_p * len(bufs))(*[ctypes.addressof(b) for b in bufs])
    return arr, bufs


def set_checksum(page: bytearray) -> None:
    """eloqstore::SetChecksum (page.cpp:18-23) on one writable host page."""
    arr, _keep = _page_ptrs([page])
    _call("pcs_pages_stamp_host", arr, len(page), 1, XXH3_64)


def validate_checksum(page) -> bool:
    """eloqstore::ValidateChecksum (page.cpp:25-31) on one host page."""
    buf = page if isinstance(page, bytearray) else bytearray(page)
    arr, _keep = _page_ptrs([buf])
    ok = (ctypes.c_uint8 * 1)()
    _call("pcs_pages_validate_host", arr, len(buf), 1, XXH3_64, ok, None)
    return bool(ok[0])


def validate_checksums(pages: list, page_size: int, algo: int = XXH3_64, skip_verify: bool = False):
    """Batched ValidateChecksum over scattered host pages -> (ok list, first_bad or None)."""
    arr, _keep = _page_ptrs(pages)
    ok = (ctypes.c_uint8 * max(1, len(pages)))()
    fb = ctypes.c_uint64(0)
    _call("pcs_pages_validate_host_ex", arr, page_size, len(pages), algo, ok, ctypes.byref(fb),
          _flags(skip_verify))
    return list(ok), (None if fb.value == (1 << 64) - 1 else fb.value)


def set_checksums(pages: list, page_size: int, algo: int = XXH3_64) -> None:
    arr, _keep = _page_ptrs(pages)
    _call("pcs_pages_stamp_host", arr, page_size, len(pages), algo)


def page_digests_host(pages: list, page_size: int, algo: int = XXH3_64) -> list:
    arr, _keep = _page_ptrs(pages)
    out = (ctypes.c_uint64 * len(pages))()
    _call("pcs_pages_digest_host", arr, page_size, len(pages), algo, out)
    return list(out)


# ---- raw pointer arrays and registered page pools -----------------------------

def host_register(addr: int, nbytes: int) -> None:
    """pcs_host_register: page-lock + map a host region for zero-copy batches."""
    _call("pcs_host_register", addr, nbytes)


def host_unregister(addr: int) -> None:
    _call("pcs_host_unregister", addr)


def validate_ptrs(ptrs, page_size: int, algo: int = XXH3_64, skip_verify: bool = False):
    """pcs_pages_validate_host_ex over raw host page addresses -> (ok array, first_bad or None)."""
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    ok = np.zeros(max(1, len(ptrs)), dtype=np.uint8)
    fb = ctypes.c_uint64(0)
    _call("pcs_pages_validate_host_ex", ptrs.ctypes.data, page_size, len(ptrs), algo, ok.ctypes.data,
          ctypes.byref(fb), _flags(skip_verify))
    return ok[: len(ptrs)], (None if fb.value == (1 << 64) - 1 else fb.value)


def stamp_ptrs(ptrs, page_size: int, algo: int = XXH3_64) -> None:
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    _call("pcs_pages_stamp_host", ptrs.ctypes.data, page_size, len(ptrs), algo)


def digest_ptrs(ptrs, page_size: int, algo: int = XXH3_64) -> np.ndarray:
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    out = np.zeros(max(1, len(ptrs)), dtype=np.uint64)
    _call("pcs_pages_digest_host", ptrs.ctypes.data, page_size, len(ptrs), algo, out.ctypes.data)
    return out[: len(ptrs)]


def scrub_ptrs(ptrs, page_size: int, corrupt_cap: int = 1024):
    """pcs_pages_scrub_host over raw host page addresses ->
    (cls array, types array, summary dict, corrupt index array)."""
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    n = len(ptrs)
    cls = np.zeros(max(1, n), dtype=np.uint8)
    types = np.zeros(max(1, n), dtype=np.uint8)
    summary = np.zeros(_SUMMARY_WORDS, dtype=np.uint64)
    corrupt = np.zeros(max(1, corrupt_cap), dtype=np.uint64)
    _call("pcs_pages_scrub_host", ptrs.ctypes.data, page_size, n, cls.ctypes.data, types.ctypes.data,
          summary.ctypes.data, corrupt.ctypes.data if corrupt_cap else 0, corrupt_cap)
    d = summary_dict(summary)
    return cls[:n], types[:n], d, corrupt[: d["n_listed"]]


def scrub_pages_host(pages: list, page_size: int, corrupt_cap: int = 1024):
    """Scrub scattered host buffers (bytearrays): see scrub_ptrs."""
    arr, _keep = _page_ptrs(pages)
    ptrs = np.array([arr[i] or 0 for i in range(len(pages))], dtype=np.uint64)
    return scrub_ptrs(ptrs, page_size, corrupt_cap)


def scrub_extents_ptrs(ptrs, page_size: int, run_cap: int = 1024, corrupt_cap: int = 1024, per_page: bool = False):
    """pcs_pages_scrub_extents_host over raw host page addresses ->
    (summary dict, corrupt index array, extent summary dict, runs array) and,
    with per_page, the cls and types arrays behind them (NULL otherwise)."""
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    n = len(ptrs)
    cls = np.zeros(max(1, n), dtype=np.uint8) if per_page else None
    types = np.zeros(max(1, n), dtype=np.uint8) if per_page else None
    summary = np.zeros(_SUMMARY_WORDS, dtype=np.uint64)
    corrupt = np.zeros(max(1, corrupt_cap), dtype=np.uint64)
    ext = np.zeros(_EXTENT_WORDS, dtype=np.uint64)
    runs = np.zeros(max(1, run_cap), dtype=EXTENT_DTYPE)
    _call("pcs_pages_scrub_extents_host", ptrs.ctypes.data, page_size, n, cls.ctypes.data if per_page else 0,
          types.ctypes.data if per_page else 0, summary.ctypes.data, corrupt.ctypes.data if corrupt_cap else 0,
          corrupt_cap, ext.ctypes.data, runs.ctypes.data if run_cap else 0, run_cap)
    d, e = summary_dict(summary), extent_dict(ext)
    out = (d, corrupt[: d["n_listed"]], e, runs[: e["n_listed"]])
    return out + (cls[:n], types[:n]) if per_page else out


def scrub_extents_host(pages: list, page_size: int, run_cap: int = 1024, corrupt_cap: int = 1024,
                       per_page: bool = False):
    """Scrub scattered host buffers (bytearrays) with extents: see scrub_extents_ptrs."""
    arr, _keep = _page_ptrs(pages)
    ptrs = np.array([arr[i] or 0 for i in range(len(pages))], dtype=np.uint64)
    return scrub_extents_ptrs(ptrs, page_size, run_cap, corrupt_cap, per_page)


def scrub_files_ptrs(ptrs, page_size: int, file_first, bad_cap: int = 1024):
    """pcs_pages_scrub_files_host over raw host page addresses and n_files + 1
    page boundaries that cover them -> (structured array (FILE_REPORT_DTYPE) of
    n_files reports, summary dict, array of the n_listed smallest bad files)."""
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    first = np.ascontiguousarray(file_first, dtype=np.uint64)
    n_files = len(first) - 1
    reports = np.zeros(max(1, n_files), dtype=FILE_REPORT_DTYPE)
    summary = np.zeros(_FILES_SUMMARY_WORDS, dtype=np.uint64)
    bad = np.zeros(max(1, bad_cap), dtype=np.uint64)
    _call("pcs_pages_scrub_files_host", ptrs.ctypes.data, page_size, len(ptrs), first.ctypes.data, n_files,
          reports.ctypes.data, summary.ctypes.data, bad.ctypes.data if bad_cap else 0, bad_cap)
    d = files_summary_dict(summary)
    return reports[:n_files], d, bad[: d["n_listed"]]


def scrub_files_host(pages: list, page_size: int, file_first, bad_cap: int = 1024):
    """Scrub scattered host buffers (bytearrays) cut into files: see scrub_files_ptrs."""
    arr, _keep = _page_ptrs(pages)
    ptrs = np.array([arr[i] or 0 for i in range(len(pages))], dtype=np.uint64)
    return scrub_files_ptrs(ptrs, page_size, file_first, bad_cap)


class ValidateService:
    """pcs_service_start / pcs_service_stop as a context manager: while it is
    open, validate_ptrs / validate_checksums batches of up to 256 registered
    XXH3 pages go to a resident kernel instead of a launch each."""

    def __init__(self, workgroups: int = 4, idle_us: int = 1000, lines: int = 1):
        self.workgroups, self.idle_us, self.lines = workgroups, idle_us, lines

    def __enter__(self):
        _call("pcs_service_start_ex", self.lines, self.workgroups, self.idle_us)
        return self

    def __exit__(self, *exc):
        _call("pcs_service_stop")


class PagePool:
    """A page-aligned host region of n_pages x page_size, like one chunk of
    EloqStore's PagesPool (page.cpp:95-120), registered for zero-copy batches.
    `.pages` is a (n_pages, page_size) uint8 view; `.ptr(i)` a page address."""

    def __init__(self, n_pages: int, page_size: int, register: bool = True):
        import mmap
        self.n, self.P = n_pages, page_size
        self._map = mmap.mmap(-1, max(1, n_pages * page_size))
        self.pages = np.frombuffer(self._map, dtype=np.uint8)[: n_pages * page_size].reshape(n_pages, page_size)
        self.base = self.pages.ctypes.data
        self.registered = False
        if register:
            host_register(self.base, n_pages * page_size)
            self.registered = True

    def ptr(self, i) -> np.ndarray:
        return np.uint64(self.base) + np.asarray(i, dtype=np.uint64) * np.uint64(self.P)

    def close(self) -> None:
        if self.registered:
            host_unregister(self.base)
            self.registered = False
        self.pages = None
        if self._map is not None:
            try:
                self._map.close()
            except BufferError:  # a view is still alive; let GC unmap it
                pass
            self._map = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
