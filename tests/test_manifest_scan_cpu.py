"""Manifest scan, the parts that need no GPU: the Python walker and builder on
hand-computed images, the new symbols and struct sizes under the unchanged ABI
revision, the no-device and argument behaviour of both entry points, the CLI's
--check-manifest usage and errors, and the host-side logic under ASAN + UBSan."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import eloqstore_amd as pcs
import manifest_ref as mr
import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
HAVE_GPU = pcs.device_count() > 0
NO = mr.NO


def test_builder_writes_what_finalize_writes():
    b = mr.Builder(4096)
    assert b.add(b"", root=7, ttl_root=9) == 0
    assert b.add(b"abc", root=1) == 4096
    assert b.add(bytes(4076)) == 8192      # fills its slot exactly: no padding
    assert b.add(bytes(4077)) == 12288     # one byte more: two slots
    img = b.data()
    assert len(img) == 5 * 4096 and b.offsets == [0, 4096, 8192, 12288]
    body0 = struct.pack("<III", 7, 9, 0)
    assert img[:20] == struct.pack("<Q", oracle.manifest_checksum(body0)) + body0
    assert img[20:4096] == bytes(4076)
    assert img[4096 + 8:4096 + 23] == struct.pack("<III", 1, 0, 3) + b"abc"
    assert struct.unpack_from("<Q", img, 4096)[0] == oracle.manifest_checksum(img[4096 + 8:4096 + 23])
    # the aggregate is per 1 MiB chunk: a one-chunk content is rotl(0, 1) ^ XXH3 times the constant
    assert oracle.manifest_checksum(body0) == (oracle.xxh3_64(body0) * 0x9E3779B97F4A7C15) & NO
    assert mr.image([0, 3], seed=5, align=64)[64 + 16:64 + 20] == struct.pack("<I", 3)
    assert len(mr.image([44, 45], align=64)) == 64 + 128


def test_walker_on_hand_computed_images():
    img = mr.image([10, 5000, 0], seed=3)
    rep, recs = mr.report(img)
    assert [r["offset"] for r in recs] == [0, 4096, 12288] and [r["payload_len"] for r in recs] == [10, 5000, 0]
    assert all(r["ok"] and r["stored"] == r["computed"] for r in recs)
    assert rep == {"size": 16384, "n_records": 3, "n_ok": 3, "n_corrupt": 0, "first_corrupt": NO,
                   "n_ok_after_corrupt": 0, "valid_prefix_bytes": 16384, "end_offset": 16384,
                   "end_reason": mr.END_CLEAN, "verdict": mr.CLEAN, "first_record": 0, "max_record_bytes": 5020}
    # every cut of the last record
    for size, n, end_off, reason in ((12288, 2, 12288, mr.END_CLEAN), (12289, 2, 12288, mr.END_SHORT_HEADER),
                                     (12307, 2, 12288, mr.END_SHORT_HEADER), (12308, 3, 12308, mr.END_SHORT_PADDING),
                                     (14000, 3, 14000, mr.END_SHORT_PADDING), (16384, 3, 16384, mr.END_CLEAN),
                                     (4096 + 5019, 1, 4096, mr.END_SHORT_PAYLOAD),
                                     (4096 + 5020, 2, 4096 + 5020, mr.END_SHORT_PADDING), (0, 0, 0, mr.END_CLEAN),
                                     (19, 0, 0, mr.END_SHORT_HEADER), (20, 0, 0, mr.END_SHORT_PAYLOAD)):
        r, rs = mr.report(img[:size])
        assert (r["n_records"], r["end_offset"], r["end_reason"]) == (n, end_off, reason), size
        assert r["verdict"] == (mr.CLEAN if n else mr.EMPTY) and r["valid_prefix_bytes"] == end_off
    # verdicts from the flags alone
    for flags, v in (([], mr.EMPTY), ([1], mr.CLEAN), ([0], mr.BAD_SNAPSHOT), ([0, 1], mr.BAD_SNAPSHOT),
                     ([1, 0], mr.TORN_TAIL), ([1, 0, 0], mr.TORN_TAIL), ([1, 0, 1], mr.BROKEN),
                     ([1, 1, 0, 0, 1], mr.BROKEN)):
        assert mr.verdict_of(flags) == v, flags
    # a corrupt middle record; a zero tail is walked as corrupt 20-byte records
    bad = bytearray(img)
    bad[4096 + 30] ^= 1
    r, rs = mr.report(bad)
    assert (r["verdict"], r["first_corrupt"], r["n_ok_after_corrupt"], r["valid_prefix_bytes"]) == (mr.BROKEN, 1, 1, 4096)
    r, rs = mr.report(bytes(img) + bytes(3 * 4096))
    assert (r["n_records"], r["n_corrupt"], r["verdict"], r["first_corrupt"]) == (6, 3, mr.TORN_TAIL, 3)
    assert rs[3]["payload_len"] == 0 and rs[3]["stored"] == 0 and rs[3]["computed"] == oracle.manifest_checksum(bytes(12))
    # a garbage length stops the walk; a payload that embeds a record is one record
    g = bytearray(img)
    g[4096 + 16:4096 + 20] = b"\xff\xff\xff\xff"
    r, rs = mr.report(g)
    assert (r["n_records"], r["end_offset"], r["end_reason"]) == (1, 4096, mr.END_SHORT_PAYLOAD)
    inner = mr.image([100], seed=9)
    outer = mr.Builder()
    outer.add(bytes(4076) + bytes(inner))
    outer.add_random(7, 1)
    r, rs = mr.report(outer.data())
    assert [x["offset"] for x in rs] == [0, 2 * 4096] and r["verdict"] == mr.CLEAN


def test_reference_scan_summary_and_layout():
    imgs = [mr.image([1, 2], 1), b"", mr.image([3], 2)[:50], bytes(100)]
    reps, s, recs = mr.scan(imgs, record_cap=2)
    assert reps["n_records"].tolist() == [2, 0, 1, 1] and reps["first_record"].tolist() == [0, 2, 2, 3]
    assert reps["verdict"].tolist() == [mr.CLEAN, mr.EMPTY, mr.CLEAN, mr.BAD_SNAPSHOT]
    assert reps["end_reason"].tolist() == [mr.END_CLEAN, mr.END_CLEAN, mr.END_SHORT_PADDING, mr.END_SHORT_PADDING]
    assert (int(s["n_records"]), int(s["n_ok"]), int(s["n_corrupt"]), int(s["n_listed"])) == (4, 3, 1, 2)
    assert s["n_by_verdict"].tolist() == [2, 0, 0, 1, 1] and int(s["first_bad_image"]) == 1 and len(recs) == 2
    buf, offs, sizes = mr.pack(imgs)
    assert offs == [0, 8192, 8192, 12288] and sizes == [8192, 0, 50, 100] and len(buf) == 16384
    assert mr.invalid_image(offs, sizes, len(buf), 4096) is None
    assert mr.invalid_image([0, 8192, 8192, 12288 + 64], sizes, 1 << 20, 4096) == 3   # misaligned
    assert mr.invalid_image([0, 4096], [8192, 10], 1 << 20, 4096) == 1                # overlapping
    assert mr.invalid_image([8192, 0], [10, 10], 1 << 20, 4096) == 1                  # descending
    assert mr.invalid_image([0, 8192], [8192, 8193], 16384, 4096) == 1                # past total_bytes


def test_new_symbols_and_struct_sizes_under_abi_7():
    so = pcs.lib()
    names = {"pcs_manifest_scan_dev", "pcs_manifest_scan_host"}
    for name in names:
        assert hasattr(so, name) and name in pcs._SIGS
    assert names <= set(pcs.header_functions())
    assert pcs.abi_version() == 7 == pcs.ABI_VERSION
    text = open(pcs.HEADER_PATH).read()
    for t in ("pcs_manifest_record", "pcs_manifest_report", "pcs_manifest_summary"):
        assert f"typedef struct {t} {{" in text

    class Record(ctypes.Structure):
        _fields_ = [("offset", ctypes.c_uint64), ("stored", ctypes.c_uint64), ("computed", ctypes.c_uint64),
                    ("payload_len", ctypes.c_uint32), ("root", ctypes.c_uint32), ("ttl_root", ctypes.c_uint32),
                    ("ok", ctypes.c_uint32)]

    class Report(ctypes.Structure):
        _fields_ = [(k, ctypes.c_uint64) for k in mr.REPORT_FIELDS]

    class Summary(ctypes.Structure):
        _fields_ = [("n_images", ctypes.c_uint64), ("n_records", ctypes.c_uint64), ("n_ok", ctypes.c_uint64),
                    ("n_corrupt", ctypes.c_uint64), ("n_by_verdict", ctypes.c_uint64 * 5),
                    ("first_bad_image", ctypes.c_uint64), ("n_listed", ctypes.c_uint64),
                    ("invalid_image", ctypes.c_uint64)]

    assert (ctypes.sizeof(Record), ctypes.sizeof(Report), ctypes.sizeof(Summary)) == (40, 96, 96)
    assert pcs.MANIFEST_RECORD_DTYPE == mr.RECORD_DTYPE and pcs.MANIFEST_RECORD_DTYPE.itemsize == 40
    assert pcs.MANIFEST_REPORT_DTYPE == mr.REPORT_DTYPE and pcs.MANIFEST_REPORT_DTYPE.itemsize == 96
    assert pcs.MANIFEST_SUMMARY_DTYPE == mr.SUMMARY_DTYPE and pcs.MANIFEST_SUMMARY_DTYPE.itemsize == 96
    for t, dt in ((Record, pcs.MANIFEST_RECORD_DTYPE), (Summary, pcs.MANIFEST_SUMMARY_DTYPE)):
        for name, _ in t._fields_:
            assert getattr(t, name).offset == dt.fields[name][1], name
    # the walk-tile key is new; the key before it was never assigned and stays unknown
    assert pcs.TUNE_MANIFEST_WALK_TILE == 38 and pcs.get_tuning(38) == 2048 and pcs.get_tuning(37) == -1
    pcs.set_tuning(pcs.TUNE_MANIFEST_WALK_TILE, 64)
    assert pcs.get_tuning(38) == 64
    pcs.set_tuning(pcs.TUNE_MANIFEST_WALK_TILE, 2048)
    for fn in ("manifest_scan_async", "manifest_scan_dev", "manifest_scan_host"):
        assert callable(getattr(pcs, fn))


def test_cpp_manifest_symbols_in_batch_library_only():
    nm = lambda path: subprocess.run(["nm", "-D", "-C", "--defined-only", path], capture_output=True, text=True,
                                     check=True).stdout
    out, drop = nm(pcs.LIB_PATH), nm(pcs.DROPIN_LIB_PATH)
    for sym in ("eloqstore::TryScanManifests(", "eloqstore::ScanManifests("):
        assert out.count(sym) == 1, sym
        assert sym not in drop, sym


def _host_args(n=2):
    imgs = [np.frombuffer(bytes(mr.image([5, 6], k + 1)), np.uint8) for k in range(n)]
    ptrs = (ctypes.c_uint64 * n)(*[i.ctypes.data for i in imgs])
    sizes = (ctypes.c_uint64 * n)(*[i.size for i in imgs])
    reports = (ctypes.c_uint64 * (12 * n))()
    summary = (ctypes.c_uint64 * 12)()
    records = (ctypes.c_uint64 * (5 * 8))()
    return ptrs, sizes, reports, summary, records, imgs


@pytest.mark.skipif(HAVE_GPU, reason="checks the no-GPU failure path")
def test_manifest_entry_points_fail_loudly_without_a_gpu(tmp_path):
    so = pcs.lib()
    ptrs, sizes, reports, summary, records, _keep = _host_args()
    assert so.pcs_manifest_scan_dev(0, 0, 0, 0, 0, 4096, 0, 0, 0, 0, 0) == pcs.PCS_ERR_NO_DEVICE
    assert b"no usable HIP device" in so.pcs_last_error()
    assert so.pcs_manifest_scan_host(ptrs, sizes, 2, 4096, reports, summary, records, 8) == pcs.PCS_ERR_NO_DEVICE
    assert b"no usable HIP device" in so.pcs_last_error()
    assert so.pcs_manifest_scan_host(None, None, 0, 4096, None, summary, None, 0) == pcs.PCS_ERR_NO_DEVICE
    with pytest.raises(pcs.PcsError):
        pcs.manifest_scan_host([bytes(mr.image([1]))])
    # the tool has no CPU fallback: a readable manifest is an error, not a verdict
    f = tmp_path / "manifest"
    f.write_bytes(bytes(mr.image([1, 2])))
    r = run_tool("--check-manifest", str(f))
    assert r.returncode == 1 and "Manifest scan failed" in r.stderr and r.stdout == ""


def test_manifest_host_argument_checks_and_fail_inject():
    """Null outputs, a bad alignment and a null image of non-zero size are
    refused before anything else; PCS_TUNE_FAIL_INJECT fails the call before it
    touches the GPU."""
    so = pcs.lib()
    ptrs, sizes, reports, summary, records, _keep = _host_args()
    f = so.pcs_manifest_scan_host
    assert f(ptrs, sizes, 2, 4096, reports, None, records, 8) == pcs.PCS_ERR_INVALID
    assert b"summary is null" in so.pcs_last_error()
    assert f(None, sizes, 2, 4096, reports, summary, records, 8) == pcs.PCS_ERR_INVALID
    assert f(ptrs, None, 2, 4096, reports, summary, records, 8) == pcs.PCS_ERR_INVALID
    assert f(ptrs, sizes, 2, 4096, None, summary, records, 8) == pcs.PCS_ERR_INVALID
    assert f(ptrs, sizes, 2, 4096, reports, summary, None, 8) == pcs.PCS_ERR_INVALID
    assert b"records is null" in so.pcs_last_error()
    for align in (0, 1, 32, 100, 4095, 131072):
        assert f(ptrs, sizes, 2, align, reports, summary, records, 8) == pcs.PCS_ERR_INVALID, align
        assert b"power of two in [64, 65536]" in so.pcs_last_error()
    assert f((ctypes.c_uint64 * 2)(ptrs[0], 0), sizes, 2, 4096, reports, summary, records, 8) == pcs.PCS_ERR_INVALID
    assert b"non-zero size is null" in so.pcs_last_error()
    try:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 1)
        assert f(ptrs, sizes, 2, 4096, reports, summary, None, 0) == pcs.PCS_ERR_HIP
        assert b"injected failure" in so.pcs_last_error()
        assert pcs.get_tuning(pcs.TUNE_FAIL_INJECT) == 0
    finally:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 0)
    if HAVE_GPU:
        assert f(ptrs, sizes, 2, 4096, reports, summary, records, 8) == pcs.PCS_OK
        assert list(summary) == [2, 4, 4, 0, 2, 0, 0, 0, 0, NO, 4, NO]
    else:
        assert f(ptrs, sizes, 2, 4096, reports, summary, None, 0) == pcs.PCS_ERR_NO_DEVICE


def run_tool(*args):
    return subprocess.run([pcs.TOOL_PATH, *args], capture_output=True, text=True)


def test_cli_check_manifest_usage_and_io_errors(tmp_path):
    r = run_tool()
    assert r.returncode == 1 and "--check-manifest <manifest_file>..." in r.stderr
    r = run_tool("--check-manifest")
    assert r.returncode == 1 and "Usage:" in r.stderr and r.stdout == ""
    # one file: the reference tool's message and exit code for a file it cannot open
    missing = str(tmp_path / "missing")
    r = run_tool("--check-manifest", missing)
    assert r.returncode == 1 and r.stderr.startswith(f"Failed to open {missing}: ") and r.stdout == ""


def test_manifest_scan_logic_under_asan_ubsan():
    """csrc/manifest_scan.h (argument rules, packing plan, verdict from flags,
    summary, the reference tool's text), driven by a stand-alone program built
    with -fsanitize=address,undefined."""
    exe = os.path.join(HERE, "cpp", "manifest_scan_logic_test_asan")
    if not os.path.exists(exe):
        pytest.skip("sanitizer build unavailable on this host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "manifest_scan_logic_test ok" in r.stdout, r.stdout + r.stderr
