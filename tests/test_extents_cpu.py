"""Scrub extents, the parts that need no GPU: the numpy reference on
hand-written class arrays, the new symbols under the unchanged ABI revision,
the no-device and argument behaviour of both entry points, the CLI's
--extents usage and I/O errors, and the host-side merge of per-chunk extents
under ASAN + UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import eloqstore_amd as pcs
import extent_ref

HERE = os.path.dirname(os.path.abspath(__file__))
HAVE_GPU = pcs.device_count() > 0
NO = extent_ref.NO_PAGE


def _summary(n_pages, n_runs, written, n_blank, n_blank_runs, first_blank, n_holes, n_hole_pages, first_hole,
             first_class, last_class, n_listed=None):
    return {"n_pages": n_pages, "n_runs": n_runs, "n_listed": n_runs if n_listed is None else n_listed,
            "written_pages": written, "n_blank": n_blank, "n_blank_runs": n_blank_runs, "first_blank": first_blank,
            "n_holes": n_holes, "n_hole_pages": n_hole_pages, "first_hole": first_hole, "first_class": first_class,
            "last_class": last_class}


HAND = [
    ([], _summary(0, 0, 0, 0, 0, NO, 0, 0, NO, NO, NO), []),
    ([2], _summary(1, 1, 0, 1, 1, 0, 0, 0, NO, 2, 2), [(0, 1, 2)]),
    ([1, 1, 2, 2], _summary(4, 2, 2, 2, 1, 2, 0, 0, NO, 1, 2), [(0, 2, 1), (2, 2, 2)]),                # tail only
    ([2, 1], _summary(2, 2, 2, 1, 1, 0, 1, 1, 0, 2, 1), [(0, 1, 2), (1, 1, 1)]),                       # hole at page 0
    ([1, 2, 1, 0, 0, 2, 2], _summary(7, 5, 5, 3, 2, 1, 1, 1, 1, 1, 2),
     [(0, 1, 1), (1, 1, 2), (2, 1, 1), (3, 2, 0), (5, 2, 2)]),                                         # hole, corrupt run, tail
    ([1, 7, 7, 1], _summary(4, 3, 4, 0, 0, NO, 0, 0, NO, 1, 1), [(0, 1, 1), (1, 2, 7), (3, 1, 1)]),    # a foreign byte
]


@pytest.mark.parametrize("cls,want,want_runs", HAND, ids=[str(h[0]) for h in HAND])
def test_reference_on_hand_written_arrays(cls, want, want_runs):
    s, runs = extent_ref.extents(np.array(cls, dtype=np.uint8), run_cap=1024)
    assert s == want
    assert [(int(r["first_page"]), int(r["n_pages"]), int(r["cls"])) for r in runs] == want_runs
    assert (runs["reserved"] == 0).all()
    # a cap below the run count lists the first runs with their full lengths and keeps the counts
    s1, runs1 = extent_ref.extents(np.array(cls, dtype=np.uint8), run_cap=1)
    assert s1 == dict(want, n_listed=min(1, want["n_runs"]))
    assert [(int(r["first_page"]), int(r["n_pages"]), int(r["cls"])) for r in runs1] == want_runs[:1]
    s0, runs0 = extent_ref.extents(np.array(cls, dtype=np.uint8), run_cap=0)
    assert s0 == dict(want, n_listed=0) and len(runs0) == 0


def test_reference_builders():
    a = extent_ref.from_runs([(1, 3), (2, 2), (0, 1)])
    assert a.tolist() == [1, 1, 1, 2, 2, 0]
    g = extent_ref.geometric(5000, 9.0, 3)
    assert g.size == 5000 and set(np.unique(g).tolist()) == {0, 1, 2}
    s, runs = extent_ref.extents(g, run_cap=10 ** 6)
    assert int(runs["n_pages"].sum()) == 5000 and s["n_listed"] == s["n_runs"] == len(runs)
    assert (np.diff(runs["cls"].astype(np.int64)) != 0).all()  # maximal: neighbours differ


def test_new_symbols_under_abi_7():
    so = pcs.lib()
    names = {"pcs_scrub_extents_dev", "pcs_pages_scrub_extents_host"}
    for name in names:
        assert hasattr(so, name) and name in pcs._SIGS
    assert names <= set(pcs.header_functions())
    assert pcs.abi_version() == 7 == pcs.ABI_VERSION
    text = open(pcs.HEADER_PATH).read()
    assert "#define PCS_ABI_VERSION 7" in text
    assert "typedef struct pcs_extent {" in text and "typedef struct pcs_extent_summary {" in text
    assert pcs.EXTENT_DTYPE.itemsize == 24 == extent_ref.RUN_DTYPE.itemsize
    assert pcs._EXTENT_FIELDS == extent_ref.FIELDS


def test_cpp_extent_symbols_in_batch_library_only():
    nm = lambda path: subprocess.run(["nm", "-D", "-C", "--defined-only", path], capture_output=True, text=True,
                                     check=True).stdout
    out, drop = nm(pcs.LIB_PATH), nm(pcs.DROPIN_LIB_PATH)
    for sym in ("eloqstore::TryScrubExtents(", "eloqstore::ScrubExtents("):
        assert sym in out, sym
        assert sym not in drop, sym


def _host_args(n=3, P=4096):
    pages = [bytearray(P) for _ in range(n)]
    arr, keep = pcs._page_ptrs(pages)
    cls = (ctypes.c_uint8 * n)()
    summary = (ctypes.c_uint64 * 12)()
    ext = (ctypes.c_uint64 * 12)()
    lst = (ctypes.c_uint64 * 4)()
    runs = (ctypes.c_uint64 * 12)()  # 4 x pcs_extent
    return arr, cls, summary, ext, lst, runs, (pages, keep)


@pytest.mark.skipif(HAVE_GPU, reason="checks the no-GPU failure path")
def test_extent_entry_points_fail_loudly_without_a_gpu():
    so = pcs.lib()
    arr, cls, summary, ext, lst, runs, _keep = _host_args()
    assert so.pcs_scrub_extents_dev(0, 1, 0, 0, 0, 0) == pcs.PCS_ERR_NO_DEVICE
    assert b"no usable HIP device" in so.pcs_last_error()
    assert so.pcs_pages_scrub_extents_host(arr, 4096, 3, cls, None, summary, lst, 4, ext, runs, 4) == \
        pcs.PCS_ERR_NO_DEVICE
    assert b"no usable HIP device" in so.pcs_last_error()
    # NULL cls / type pass the argument checks
    assert so.pcs_pages_scrub_extents_host(arr, 4096, 3, None, None, summary, lst, 4, ext, runs, 4) == \
        pcs.PCS_ERR_NO_DEVICE
    with pytest.raises(pcs.PcsError):
        pcs.scrub_extents_host([bytearray(4096)], 4096)


def test_extents_host_argument_checks_and_fail_inject():
    """Null summaries and lists are refused before anything else; cls and type
    may be null; PCS_TUNE_FAIL_INJECT fails the call before it touches the GPU;
    the page-size rule is pcs_pages_scrub_host's."""
    so = pcs.lib()
    arr, cls, summary, ext, lst, runs, _keep = _host_args()
    f = so.pcs_pages_scrub_extents_host
    assert f(arr, 4096, 3, cls, None, None, lst, 4, ext, runs, 4) == pcs.PCS_ERR_INVALID
    assert f(arr, 4096, 3, cls, None, summary, lst, 4, None, runs, 4) == pcs.PCS_ERR_INVALID
    assert f(arr, 4096, 3, cls, None, summary, None, 4, ext, runs, 4) == pcs.PCS_ERR_INVALID
    assert f(arr, 4096, 3, cls, None, summary, lst, 4, ext, None, 4) == pcs.PCS_ERR_INVALID
    assert b"runs is null" in so.pcs_last_error()
    try:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 1)
        assert f(arr, 4096, 3, None, None, summary, None, 0, ext, None, 0) == pcs.PCS_ERR_HIP
        assert b"injected failure" in so.pcs_last_error()
        assert pcs.get_tuning(pcs.TUNE_FAIL_INJECT) == 0
    finally:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 0)
    if HAVE_GPU:
        assert f(arr, 248, 3, None, None, summary, None, 0, ext, None, 0) == pcs.PCS_ERR_INVALID
        assert b"249 <= page_size" in so.pcs_last_error()
        assert f(arr, 4096, 3, None, None, summary, None, 0, ext, None, 0) == pcs.PCS_OK
    else:
        assert f(arr, 4096, 3, None, None, summary, None, 0, ext, None, 0) == pcs.PCS_ERR_NO_DEVICE


def run_tool(*args):
    return subprocess.run([pcs.TOOL_PATH, *args], capture_output=True, text=True)


def test_cli_extents_usage_and_io_errors(tmp_path):
    r = run_tool()
    assert r.returncode == 1
    assert "--scrub <file_path> [page_size_bytes]" in r.stderr
    assert "--extents <file_path> [page_size_bytes]" in r.stderr
    assert "exit 3" in r.stderr and "append-mode" in r.stderr
    r = run_tool("--extents")
    assert r.returncode == 1 and "Usage:" in r.stderr
    r = run_tool("--extents", "a", "4096", "extra")
    assert r.returncode == 1 and "Usage:" in r.stderr
    r = run_tool("--extents", str(tmp_path / "missing.bin"))
    assert r.returncode == 1 and "Failed to open" in r.stderr
    f = tmp_path / "f.bin"
    f.write_bytes(b"\0" * 8192)
    for bad in ("x", "0", "248"):
        r = run_tool("--extents", str(f), bad)
        assert r.returncode == 1 and "Invalid page size" in r.stderr, bad
    r = run_tool("--extents", str(f), "16384")
    assert r.returncode == 1 and "holds no whole page" in r.stderr


def test_extent_merge_under_asan_ubsan():
    """pcs::ExtentMerge (csrc/extent_merge.h), the host code that folds
    per-chunk extents into global runs and re-derives the holes, driven by a
    stand-alone program against a naive loop over the whole class array, built
    with -fsanitize=address,undefined."""
    exe = os.path.join(HERE, "cpp", "extent_merge_test_asan")
    if not os.path.exists(exe):
        pytest.skip("sanitizer build unavailable on this host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "extent_merge_test ok" in r.stdout, r.stdout + r.stderr
