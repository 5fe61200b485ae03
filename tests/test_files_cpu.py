"""Scrub files, the parts that need no GPU: the numpy reference on
hand-written batches, the new symbols under the unchanged ABI revision, the
no-device and argument behaviour of both entry points, the CLI's --scrub-files
usage and I/O errors, and the host-side merge of a file's parts under ASAN +
UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import eloqstore_amd as pcs
import file_ref

HERE = os.path.dirname(os.path.abspath(__file__))
HAVE_GPU = pcs.device_count() > 0
NO = file_ref.NO_PAGE


def _report(first_page, n_pages, n_ok, n_corrupt, n_blank, by_type, first_corrupt, written, n_holes, n_hole_pages,
            first_hole):
    return {"first_page": first_page, "n_pages": n_pages, "n_ok": n_ok, "n_corrupt": n_corrupt, "n_blank": n_blank,
            "ok_by_type": by_type, "first_corrupt": first_corrupt, "written_pages": written, "n_holes": n_holes,
            "n_hole_pages": n_hole_pages, "first_hole": first_hole}


def test_reference_on_a_hand_written_batch():
    #            file 0      | 1 (empty) | file 2   | file 3      | file 4
    cls = [1, 1, 2, 2,                     2, 1,      0, 2, 2, 1,   2, 2, 7]
    typ = [0, 2, 9, 9,                     9, 255,    1, 0, 0, 77,  0, 0, 3]
    first = [0, 4, 4, 6, 10, 13]
    reps, s, bad = file_ref.files(np.array(cls, np.uint8), np.array(typ, np.uint8), first)
    assert reps == [
        _report(0, 4, 2, 0, 2, [1, 0, 1, 0, 0, 0], NO, 2, 0, 0, NO),    # a blank tail: healthy
        _report(4, 0, 0, 0, 0, [0] * 6, NO, 0, 0, 0, NO),
        _report(4, 2, 1, 0, 1, [0, 0, 0, 0, 1, 0], NO, 2, 1, 1, 0),     # file 0's tail is not part of this hole
        _report(6, 4, 1, 1, 2, [0, 0, 0, 0, 0, 1], 0, 4, 1, 2, 1),
        _report(10, 3, 0, 0, 2, [0] * 6, NO, 3, 1, 2, 0),               # a foreign class byte is written, counted nowhere
    ]
    assert s == {"n_files": 5, "n_pages": 13, "n_ok": 4, "n_corrupt": 1, "n_blank": 7, "n_corrupt_files": 1,
                 "n_hole_files": 3, "n_bad_files": 3, "n_unwritten_files": 1, "first_bad_file": 2, "n_listed": 3,
                 "invalid_file": NO}
    assert bad.tolist() == [2, 3, 4]
    reps1, s1, bad1 = file_ref.files(np.array(cls, np.uint8), np.array(typ, np.uint8), first, bad_cap=1)
    assert reps1 == reps and s1 == dict(s, n_listed=1) and bad1.tolist() == [2]
    # a partial cover: pages in no file are in no report
    reps, s, bad = file_ref.files(np.array(cls, np.uint8), np.array(typ, np.uint8), [6, 7])
    assert reps == [_report(6, 1, 0, 1, 0, [0] * 6, 0, 1, 0, 0, NO)] and s["n_pages"] == 1
    # no file at all
    reps, s, bad = file_ref.files(np.array(cls, np.uint8), np.array(typ, np.uint8), [0])
    assert reps == [] and s == dict.fromkeys(file_ref.SUMMARY_FIELDS, 0) | {"first_bad_file": NO, "invalid_file": NO}


def test_reference_on_invalid_boundaries():
    cls, typ = np.ones(10, np.uint8), np.zeros(10, np.uint8)
    for first, inv in (([0, 5, 4, 10], 1), ([0, 11], 0), ([0, 3, 12, 10], 1), ([11, 11], 0)):
        reps, s, bad = file_ref.files(cls, typ, first)
        assert reps == [] and len(bad) == 0
        assert s == dict.fromkeys(file_ref.SUMMARY_FIELDS, 0) | {"n_files": len(first) - 1, "invalid_file": inv}
    assert file_ref.invalid_file([0, 0, 10, 10], 10) is None
    assert file_ref.even_cut(10, 4).tolist() == [0, 4, 8, 10] and file_ref.even_cut(8, 4).tolist() == [0, 4, 8]
    recs = file_ref.as_records(file_ref.files(cls, typ, [0, 10])[0])
    assert recs.dtype.itemsize == 128 and recs.view(np.uint64).tolist() == [0, 10, 10, 0, 0, 10, 0, 0, 0, 0, 0, NO,
                                                                            10, 0, 0, NO]


def test_new_symbols_under_abi_7():
    so = pcs.lib()
    names = {"pcs_scrub_files_dev", "pcs_pages_scrub_files_host"}
    for name in names:
        assert hasattr(so, name) and name in pcs._SIGS
    assert names <= set(pcs.header_functions())
    assert pcs.abi_version() == 7 == pcs.ABI_VERSION
    text = open(pcs.HEADER_PATH).read()
    assert "#define PCS_ABI_VERSION 7" in text
    assert "typedef struct pcs_file_report {" in text and "typedef struct pcs_files_summary {" in text
    assert pcs.FILE_REPORT_DTYPE.itemsize == 128 and pcs.FILE_REPORT_DTYPE == file_ref.REPORT_DTYPE
    assert pcs._FILES_SUMMARY_FIELDS == file_ref.SUMMARY_FIELDS and pcs._FILES_SUMMARY_WORDS == 12
    d = pcs.file_report_dict(list(range(16)))
    assert d["ok_by_type"] == [5, 6, 7, 8, 9, 10] and d["first_hole"] == 15 and tuple(d) == file_ref.REPORT_FIELDS
    assert pcs.files_summary_dict(range(12))["invalid_file"] == 11
    for fn in ("scrub_files_async", "scrub_files", "scrub_files_ptrs", "scrub_files_host"):
        assert callable(getattr(pcs, fn))


def test_cpp_file_symbols_in_batch_library_only():
    nm = lambda path: subprocess.run(["nm", "-D", "-C", "--defined-only", path], capture_output=True, text=True,
                                     check=True).stdout
    out, drop = nm(pcs.LIB_PATH), nm(pcs.DROPIN_LIB_PATH)
    for sym in ("eloqstore::TryScrubFiles(", "eloqstore::ScrubFiles("):
        assert out.count(sym) == 2, sym  # the boundary form and the pages-per-file form
        assert sym not in drop, sym


def _host_args(n=3, P=4096):
    pages = [bytearray(P) for _ in range(n)]
    arr, keep = pcs._page_ptrs(pages)
    first = (ctypes.c_uint64 * 3)(0, 1, n)
    reports = (ctypes.c_uint64 * 32)()
    summary = (ctypes.c_uint64 * 12)()
    bad = (ctypes.c_uint64 * 4)()
    return arr, first, reports, summary, bad, (pages, keep)


@pytest.mark.skipif(HAVE_GPU, reason="checks the no-GPU failure path")
def test_file_entry_points_fail_loudly_without_a_gpu():
    so = pcs.lib()
    arr, first, reports, summary, bad, _keep = _host_args()
    assert so.pcs_scrub_files_dev(0, 0, 1, 0, 1, 0, 0, 0, 0, 0) == pcs.PCS_ERR_NO_DEVICE
    assert b"no usable HIP device" in so.pcs_last_error()
    assert so.pcs_pages_scrub_files_host(arr, 4096, 3, first, 2, reports, summary, bad, 4) == pcs.PCS_ERR_NO_DEVICE
    assert b"no usable HIP device" in so.pcs_last_error()
    assert so.pcs_pages_scrub_files_host(arr, 4096, 3, first, 2, reports, summary, None, 0) == pcs.PCS_ERR_NO_DEVICE
    with pytest.raises(pcs.PcsError):
        pcs.scrub_files_host([bytearray(4096)], 4096, [0, 1])


def test_files_host_argument_checks_and_fail_inject():
    """Null outputs and boundaries that decrease or do not cover the batch are
    refused before anything else; PCS_TUNE_FAIL_INJECT fails the call before it
    touches the GPU; the page-size rule is pcs_pages_scrub_host's."""
    so = pcs.lib()
    arr, first, reports, summary, bad, _keep = _host_args()
    f = so.pcs_pages_scrub_files_host
    assert f(arr, 4096, 3, None, 2, reports, summary, bad, 4) == pcs.PCS_ERR_INVALID
    assert f(arr, 4096, 3, first, 2, None, summary, bad, 4) == pcs.PCS_ERR_INVALID
    assert f(arr, 4096, 3, first, 2, reports, None, bad, 4) == pcs.PCS_ERR_INVALID
    assert f(arr, 4096, 3, first, 2, reports, summary, None, 4) == pcs.PCS_ERR_INVALID
    assert b"bad is null" in so.pcs_last_error()
    for cut, msg in (((0, 2, 1), b"decreases"), ((1, 2, 3), b"file_first[0] is not 0"),
                     ((0, 1, 2), b"is not n_pages"), ((0, 1, 4), b"is not n_pages")):
        assert f(arr, 4096, 3, (ctypes.c_uint64 * 3)(*cut), 2, reports, summary, bad, 4) == pcs.PCS_ERR_INVALID
        assert msg in so.pcs_last_error(), cut
    try:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 1)
        assert f(arr, 4096, 3, first, 2, reports, summary, None, 0) == pcs.PCS_ERR_HIP
        assert b"injected failure" in so.pcs_last_error()
        assert pcs.get_tuning(pcs.TUNE_FAIL_INJECT) == 0
    finally:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 0)
    if HAVE_GPU:
        assert f(arr, 248, 3, first, 2, reports, summary, None, 0) == pcs.PCS_ERR_INVALID
        assert b"249 <= page_size" in so.pcs_last_error()
        assert f(arr, 4096, 3, first, 2, reports, summary, bad, 4) == pcs.PCS_OK
        assert list(summary)[:5] == [2, 3, 0, 0, 3] and summary[8] == 2 and summary[11] == NO
    else:
        assert f(arr, 4096, 3, first, 2, reports, summary, None, 0) == pcs.PCS_ERR_NO_DEVICE


def run_tool(*args):
    return subprocess.run([pcs.TOOL_PATH, *args], capture_output=True, text=True)


def test_cli_scrub_files_usage_and_io_errors(tmp_path):
    r = run_tool()
    assert r.returncode == 1
    assert "--scrub-files <page_size_bytes> <file>..." in r.stderr
    assert "--scrub <file_path> [page_size_bytes]" in r.stderr and "--extents <file_path> [page_size_bytes]" in r.stderr
    for args in (("--scrub-files",), ("--scrub-files", "4096")):
        r = run_tool(*args)
        assert r.returncode == 1 and "Usage:" in r.stderr
    f = tmp_path / "f.bin"
    f.write_bytes(b"\0" * 8192)
    for bad in ("x", "0", "248"):
        r = run_tool("--scrub-files", bad, str(f))
        assert r.returncode == 1 and "Invalid page size" in r.stderr, bad
    # every file is opened before any GPU work: one missing file fails the call, wherever it stands
    r = run_tool("--scrub-files", "4096", str(f), str(tmp_path / "missing.bin"))
    assert r.returncode == 1 and "Failed to open" in r.stderr and "missing.bin" in r.stderr and r.stdout == ""


def test_file_merge_under_asan_ubsan():
    """pcs::FileMerge and pcs::files_summarize (csrc/file_merge.h), the host
    code that folds a file's parts and re-derives its holes, driven by a
    stand-alone program against a naive loop over the whole file, built with
    -fsanitize=address,undefined."""
    exe = os.path.join(HERE, "cpp", "file_merge_test_asan")
    if not os.path.exists(exe):
        pytest.skip("sanitizer build unavailable on this host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "file_merge_test ok" in r.stdout, r.stdout + r.stderr
