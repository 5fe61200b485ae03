"""Page scrub, the parts that need no GPU: the blank-page fixture, the
reference classifier the GPU tests compare with, the new symbols and ABI
revision, the no-device and argument behaviour of both entry points, the
CLI's --scrub usage and I/O errors, and the host-side merge of per-chunk
results under ASAN + UBSan."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import eloqstore_amd as pcs
import oracle
import scrub_ref

HERE = os.path.dirname(os.path.abspath(__file__))
HAVE_GPU = pcs.device_count() > 0
PAGE_SIZES = (249, 256, 1000, 4096, 5000, 8192, 16384, 32768, 65536)


def test_blank_fixture_matches_oracle_and_is_never_zero():
    with open(os.path.join(HERE, "golden", "scrub_blank.json")) as f:
        fx = json.load(f)
    rows = {int(P): int(h, 16) for P, h in fx["rows"]}
    assert tuple(sorted(rows)) == PAGE_SIZES
    assert rows[4096] == 0xE9B88C5D16960EE3 and rows[65536] == 0xF75F7D02ACCA5678
    for P, h in rows.items():
        assert h != 0, P
        assert oracle.xxh3_64(bytes(P - 8)) == h, P
        # so an all-zero page (stored digest 0) never validates
        assert int(oracle.pages_digest(np.zeros(P, dtype=np.uint8), P, 0)[0]) == h
    ref = oracle.ref_lib()
    if ref is not None:  # the reference's own xxhash.c, when it was built
        for P, h in rows.items():
            body = bytes(P - 8)
            assert int(ref.XXH3_64bits(body, len(body))) == h, P


def test_reference_classifier_on_hand_built_pages():
    P = 1000
    pg = np.zeros((8, P), dtype=np.uint8)
    pg[0, 100] = 7; pg[0, 8] = 2       # data page, stamped: ok, bucket 2
    pg[1, 200] = 9; pg[1, 8] = 255     # deleted, stamped: ok, bucket 4
    pg[2, 300] = 1; pg[2, 8] = 77      # unknown type, stamped: ok, bucket 5
    scrub_ref.stamp(pg, [0, 1, 2])
    # 3: blank.  4: zero body under its correct header: ok, type 0
    scrub_ref.stamp(pg, [4])
    pg[5, 500] = 1                     # zero header over a non-zero body: corrupt
    pg[6] = pg[0]; pg[6, 10] ^= 0xFF   # flipped after stamping: corrupt
    pg[7, 0] = 1                       # header byte only: corrupt, not blank
    cls, types, s, bad = scrub_ref.classify(pg, P, corrupt_cap=2)
    assert cls.tolist() == [1, 1, 1, 2, 1, 0, 0, 0]
    assert types.tolist() == [2, 255, 77, 0, 0, 0, 2, 0]
    assert s == {"n_pages": 8, "n_ok": 4, "n_corrupt": 3, "n_blank": 1, "ok_by_type": [1, 0, 1, 0, 1, 1],
                 "first_corrupt": 5, "n_listed": 2}
    assert bad.tolist() == [5, 6]
    cls, types, s, bad = scrub_ref.classify(np.zeros(0, dtype=np.uint8), P)
    assert s["n_pages"] == 0 and s["first_corrupt"] == scrub_ref.NO_PAGE and len(bad) == 0
    # every bucket rule
    assert [scrub_ref.bucket(t) for t in (0, 1, 2, 3, 4, 254, 255)] == [0, 1, 2, 3, 5, 5, 4]


@pytest.mark.parametrize("P,n", [(4096, 1003), (65536, 37), (249, 100)])
def test_built_batches_hold_every_case(P, n):
    near = scrub_ref.near_blank_offsets(P)
    pg, rows = scrub_ref.build_batch(P, n, near=near[:9] if n < 64 else None)
    cls, types, s, bad = scrub_ref.classify(pg, P)
    assert s["n_ok"] and s["n_corrupt"] and s["n_blank"] and all(s["ok_by_type"])
    assert (cls[rows["blank"]] == scrub_ref.BLANK).all() and s["n_blank"] == len(rows["blank"])
    assert cls[rows["zero_body_ok"]] == scrub_ref.OK and cls[rows["zero_header"]] == scrub_ref.CORRUPT
    assert all(cls[r] == scrub_ref.CORRUPT for r in rows["near_blank"].values())
    assert (cls[rows["flipped"]] == scrub_ref.CORRUPT).all()


def _has_all(offs, lo, hi):
    return np.isin(np.arange(max(lo, 0), hi), offs).all()


@pytest.mark.parametrize("P", [249, 1000, 4096, 5120, 8192, 65535, 65536, 131328, 135176])
def test_walk_offsets_cover_what_they_claim(P):
    offs = scrub_ref.walk_offsets(P)
    assert offs.ndim == 1 and (np.diff(offs) > 0).all() and offs[0] >= 0 and offs[-1] < P
    if P <= 5120:
        assert np.array_equal(offs, np.arange(P))
        return
    assert _has_all(offs, 0, 1100) and _has_all(offs, P - 1100, P)
    if P <= 65536:
        k = offs // 16
        assert np.array_equal(np.unique(k), np.arange((P + 15) // 16))  # every piece is hit
        pairs = lambda a: {(int(x), int(y)) for x, y in zip(a, offs % 16)}
        assert len(pairs(k % 16)) == 256            # (lane, byte-in-piece)
        assert len(pairs((k // 16) % 4)) == 64      # (chunk, byte-in-piece)
        for m in range(0, P + 1, 4096):
            assert _has_all(offs, m - 24, min(m + 25, P)), m
    else:
        assert np.array_equal(np.unique(offs // 64), np.arange((P + 63) // 64))  # every stripe is hit


@pytest.mark.parametrize("P", [249, 1000, 4096, 8192])
def test_walk_batches_hold_every_case(P):
    pg, rows = scrub_ref.build_walk_batch(P, seed=1)
    n = len(pg)
    offs, wrows = rows["offsets"], rows["walk_rows"]
    assert np.array_equal(offs, scrub_ref.walk_offsets(P)) and len(set(wrows.tolist())) == len(offs)
    assert rows["walk"] == dict(zip(offs.tolist(), wrows.tolist()))
    control = sorted(r for kind in scrub_ref.CONTROL_KINDS for r in rows[kind])
    assert control[:-1] == list(range(0, n - 1, 17)) and control[-1] == n - 1
    assert sorted(control + wrows.tolist()) == list(range(n))
    assert {0, n - 1} <= set(rows["blank"])
    assert {r % 16 for r in control} == set(range(16))
    # a walk page is zero but for one byte with one bit; all 8 bits at every byte-in-piece position
    vals = pg[wrows, offs]
    assert (pg[wrows].astype(bool).sum(axis=1) == 1).all() and np.isin(vals, 1 << np.arange(8)).all()
    assert {(int(p), int(v)) for p, v in zip(offs % 16, vals)} == {(p, 1 << b) for p in range(16) for b in range(8)}
    hb = pg[rows["header_bit"]]
    assert not hb[:, 8:].any()
    assert [int(x) for x in np.ascontiguousarray(hb[:, :8]).view("<u8").ravel()] == \
        [1 << ((r // 17) % 64) for r in rows["header_bit"]]
    cls, types, s, bad = scrub_ref.classify(pg, P)
    assert (cls[wrows] == scrub_ref.CORRUPT).all()
    assert (cls[rows["header_bit"]] == scrub_ref.CORRUPT).all() and len(rows["header_bit"]) >= 1
    assert (cls[rows["blank"]] == scrub_ref.BLANK).all() and s["n_blank"] == len(rows["blank"])
    assert (cls[rows["zero_body_ok"]] == scrub_ref.OK).all() and (cls[rows["random_ok"]] == scrub_ref.OK).all()
    assert s["n_ok"] == len(rows["zero_body_ok"]) + len(rows["random_ok"]) >= 2
    assert set(types[rows["random_ok"]].tolist()) <= set(scrub_ref.TYPE_BYTES)


def test_new_symbols_and_abi_7():
    so = pcs.lib()
    assert hasattr(so, "pcs_pages_scrub_dev") and hasattr(so, "pcs_pages_scrub_host")
    assert {"pcs_pages_scrub_dev", "pcs_pages_scrub_host"} <= set(pcs.header_functions())
    assert pcs.abi_version() == 7 == pcs.ABI_VERSION
    text = open(pcs.HEADER_PATH).read()
    assert "#define PCS_ABI_VERSION 7" in text
    assert "PCS_PAGE_CORRUPT = 0, PCS_PAGE_OK = 1, PCS_PAGE_BLANK = 2" in text
    assert (pcs.PAGE_CORRUPT, pcs.PAGE_OK, pcs.PAGE_BLANK) == (0, 1, 2)


def test_cpp_scrub_symbols_in_batch_library_only():
    nm = lambda path: subprocess.run(["nm", "-D", "-C", "--defined-only", path], capture_output=True, text=True,
                                     check=True).stdout
    out, drop = nm(pcs.LIB_PATH), nm(pcs.DROPIN_LIB_PATH)
    for sym in ("eloqstore::TryScrubPages(", "eloqstore::ScrubPages("):
        assert sym in out, sym
        assert sym not in drop, sym


def _host_args(n=3, P=4096):
    pages = [bytearray(P) for _ in range(n)]
    arr, keep = pcs._page_ptrs(pages)
    cls = (ctypes.c_uint8 * n)()
    summary = (ctypes.c_uint64 * 12)()
    lst = (ctypes.c_uint64 * 4)()
    return arr, cls, summary, lst, (pages, keep)


@pytest.mark.skipif(HAVE_GPU, reason="checks the no-GPU failure path")
def test_scrub_entry_points_fail_loudly_without_a_gpu():
    so = pcs.lib()
    arr, cls, summary, lst, _keep = _host_args()
    assert so.pcs_pages_scrub_dev(0, 4096, 1, 0, 0, 0, 0, 0, 0) == pcs.PCS_ERR_NO_DEVICE
    assert b"no usable HIP device" in so.pcs_last_error()
    assert so.pcs_pages_scrub_host(arr, 4096, 3, cls, None, summary, lst, 4) == pcs.PCS_ERR_NO_DEVICE
    assert b"no usable HIP device" in so.pcs_last_error()
    with pytest.raises(pcs.PcsError):
        pcs.scrub_pages_host([bytearray(4096)], 4096)


def test_scrub_host_argument_checks_and_fail_inject():
    """Null outputs are refused before anything else, as the other host entry
    points do; PCS_TUNE_FAIL_INJECT fails the call before it touches the GPU."""
    so = pcs.lib()
    arr, cls, summary, lst, _keep = _host_args()
    assert so.pcs_pages_scrub_host(arr, 4096, 3, None, None, summary, lst, 4) == pcs.PCS_ERR_INVALID
    assert so.pcs_pages_scrub_host(arr, 4096, 3, cls, None, None, lst, 4) == pcs.PCS_ERR_INVALID
    assert so.pcs_pages_scrub_host(arr, 4096, 3, cls, None, summary, None, 4) == pcs.PCS_ERR_INVALID
    try:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 1)
        assert so.pcs_pages_scrub_host(arr, 4096, 3, cls, None, summary, lst, 4) == pcs.PCS_ERR_HIP
        assert b"injected failure" in so.pcs_last_error()
        assert pcs.get_tuning(pcs.TUNE_FAIL_INJECT) == 0
    finally:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 0)


def run_tool(*args):
    return subprocess.run([pcs.TOOL_PATH, *args], capture_output=True, text=True)


def test_cli_scrub_usage_and_io_errors(tmp_path):
    r = run_tool()
    assert r.returncode == 1 and "--scrub <file_path> [page_size_bytes]" in r.stderr
    r = run_tool("--scrub")
    assert r.returncode == 1 and "Usage:" in r.stderr
    r = run_tool("--scrub", "a", "4096", "extra")
    assert r.returncode == 1 and "Usage:" in r.stderr
    r = run_tool("--scrub", str(tmp_path / "missing.bin"))
    assert r.returncode == 1 and "Failed to open" in r.stderr
    f = tmp_path / "f.bin"
    f.write_bytes(b"\0" * 8192)
    for bad in ("x", "0", "248"):
        r = run_tool("--scrub", str(f), bad)
        assert r.returncode == 1 and "Invalid page size" in r.stderr, bad
    r = run_tool("--scrub", str(f), "16384")
    assert r.returncode == 1 and "holds no whole page" in r.stderr


def test_chunk_merge_under_asan_ubsan():
    """pcs::ScrubMerge (csrc/scrub_merge.h), the host code that merges per-chunk
    summaries and lists into global indices, driven by a stand-alone program
    with synthetic chunk results, built with -fsanitize=address,undefined."""
    exe = os.path.join(HERE, "cpp", "scrub_merge_test_asan")
    if not os.path.exists(exe):
        pytest.skip("sanitizer build unavailable on this host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scrub_merge_test ok" in r.stdout, r.stdout + r.stderr
