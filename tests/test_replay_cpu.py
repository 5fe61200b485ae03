"""CPU-side contract of the manifest replay and the liveness-aware scrub: the
pure-Python model (tests/replay_ref.py) round-trips its own builder and trips
on every malformed rule, the additive symbols exist under ABI 7 with their
bindings and struct sizes, PCS_TUNE_REPLAY_TILE accepts only its range, both
_host calls check their arguments before they look for a device, and the
host-side logic (csrc/manifest_replay.h) runs under ASAN + UBSan."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
import manifest_ref as mr
import replay_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))
HAVE_GPU = torch.cuda.is_available()
NO = rr.NO
I32 = lambda v: struct.pack("<I", v)


# ---- the model -----------------------------------------------------------------
def test_varint_encoder_and_decoder_round_trip():
    for v in [0, 1, 127, 128, 300, (1 << 14) - 1, 1 << 14, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, NO]:
        b = rr.varint(v)
        assert len(b) == max(1, (v.bit_length() + 6) // 7) and b[-1] < 0x80 and all(x >= 0x80 for x in b[:-1])
        assert rr.read_varint(b, 0, len(b), 10) == (v, len(b))
        for n in range(len(b), 11):  # padded encodings decode to the same value
            p = rr.varint(v, length=n)
            assert len(p) == n and rr.read_varint(p, 0, n, 10)[0] == v
    # the tenth byte keeps one bit, the fifth byte of a varint32 four
    assert rr.read_section64(rr.varint(1 << 63, top=0x7E), 0, 10) == [1 << 63]
    entries, _ = rr.decode_log(rr.log_payload(rr.varint(9, length=5, top=0x70) + rr.varint(77)))
    assert entries == [(9, 77)]
    with pytest.raises(rr.Malformed):
        rr.read_varint(b"\x80" * 10 + b"\x01", 0, 11, 10)
    with pytest.raises(rr.Malformed):
        rr.read_varint(b"\x80\x80", 0, 2, 10)


def test_builder_and_decoder_round_trip():
    values = [rr.fp(k * 7) for k in range(100)] + [0, rr.INVALID, 1 << 63]
    term = [(1, 2), (300, 1 << 40)]
    p = rr.snapshot_payload(555, rr.values_section(values), rr.term_section(term), b"dictionary", b"ignored trailer")
    assert rr.decode_snapshot(p) == (555, 10, values, 2)
    entries = [(5, rr.fp(1)), (1 << 20, 0), (0xFFFFFFFF, NO)]
    assert rr.decode_log(rr.log_payload(rr.entries_section(entries), rr.term_section(term), b"xx")) == (entries, 2)
    img = rr.manifest(10, values, [[(2, rr.fp(900)), (110, rr.fp(3))], [(2, rr.INVALID)]], term=term)
    reps, s, rows = rr.replay([img, b"", img], table_cap=200)
    r = reps[0]
    assert (int(r["status"]), int(r["n_replayed"]), int(r["root"]), int(r["ttl_root"])) == (rr.OK, 3, 101, 201)
    assert (int(r["max_fp_id"]), int(r["snapshot_pages"]), int(r["n_log_entries"])) == (901, 103, 3)
    assert (int(r["table_size"]), int(r["n_term_pairs"]), int(r["n_mapped"])) == (111, 2, 100)
    assert int(rows[2]) == rr.INVALID and int(rows[110]) == rr.fp(3) and (rows[103:110] == rr.INVALID).all()
    assert reps["status"].tolist() == [rr.OK, rr.NOT_REPLAYABLE, rr.TABLE_CAP]
    assert reps["table_first"].tolist() == [0, 111, 111] and int(s["n_rows"]) == 222 and rows.size == 111
    assert int(reps[2]["max_fp_id"]) == 901 and int(reps[2]["n_mapped"]) == 0 and int(reps[2]["min_fp"]) == NO
    assert s["n_by_status"].tolist() == [1, 1, 0, 1] and int(s["first_bad_image"]) == 1


def test_each_malformed_rule_trips_in_the_model():
    good = rr.snapshot_payload(9, rr.values_section([1, 2, 3]))
    rr.decode_snapshot(good)
    bad_snapshots = [b"", b"\x80\x80", b"\x80" * 10 + b"\x01" + good,                         # max_fp_id
                     rr.varint(5) + rr.varint(100) + b"abc" + I32(0) + I32(0),               # dict_len too large
                     rr.varint(5) + b"\x80" * 5 + b"\x00" + I32(0) + I32(0),                 # dict_len of 6 bytes
                     rr.varint(5) + rr.varint(0) + I32(11) + b"\x01" * 10 + I32(0),          # mapping_len + 8 > rem
                     rr.varint(5) + rr.varint(0) + b"\x00" * 7,                              # no room for the lengths
                     rr.varint(5) + rr.varint(0) + I32(2) + b"\x01\x02" + I32(3) + b"\x01\x02",  # term_len
                     rr.snapshot_payload(9, b"\x01\x82"),                                    # dangling varint
                     rr.snapshot_payload(9, b"\x80" * 10 + b"\x01"),                         # 11-byte run
                     rr.snapshot_payload(9, b"\x01", b"\x01")]                               # odd term count
    for p in bad_snapshots:
        with pytest.raises(rr.Malformed):
            rr.decode_snapshot(p)
    rr.decode_log(rr.log_payload(b"\x80\x80\x80\x80\x01\x09"))  # a 5-byte page id is legal
    bad_logs = [b"\x00" * 7,                                     # shorter than 8
                I32(3) + b"\x01\x09" + I32(0),                   # mapping_len + 8 > L
                rr.log_payload(b"\x80" * 5 + b"\x01\x09"),       # 6-byte page id
                rr.log_payload(b"\x01\x09\x02"),                 # odd count
                rr.log_payload(b"\x01" + b"\x80" * 10 + b"\x01"),  # 11-byte value
                rr.log_payload(b"\x01\x89"),                     # dangling value
                rr.log_payload(b"", b"\x01\x02\x03"),            # odd term count
                I32(0) + I32(5) + b"\x01\x02"]                   # term_len too large
    for p in bad_logs:
        with pytest.raises(rr.Malformed):
            rr.decode_log(p)
    # in an image: the lowest bad record is named, nothing is replayed, the status is MALFORMED
    b = mr.Builder()
    b.add(good)
    b.add(rr.log_payload(rr.entries_section([(1, 9)])))
    b.add(bad_logs[3])
    b.add(bad_logs[0])
    reps, s, rows = rr.replay([b.data()])
    assert (int(reps[0]["status"]), int(reps[0]["malformed_record"]), rows.size) == (rr.MALFORMED, 2, 0)


def test_scrub_live_model():
    cls = np.array([1, 0, 2, 1], dtype=np.uint8)
    table = np.array([rr.fp(11), rr.INVALID, rr.fp(12), rr.fp(11), rr.fp(99), 12 << 3], dtype=np.uint64)
    own, s, pages = rr.scrub_live(cls, 10, table)
    assert own.tolist() == [rr.NO_OWNER, 0, 2, rr.NO_OWNER]
    assert [int(s[k]) for k in rr.LIVE_FIELDS] == [4, 6, 4, 3, 1, 0, 1, 1, 2, 0, 0, 2, 1, 2, 2, 0]
    assert pages.tolist() == [(1, 0, 0), (2, 2, 2)]
    assert rr.scrub_live(cls, 10, table, 1)[2].tolist() == [(1, 0, 0)]


# ---- symbols, bindings, sizes ---------------------------------------------------
def test_new_symbols_bindings_and_struct_sizes_under_abi_7():
    so = pcs.lib()
    names = {"pcs_manifest_replay_dev", "pcs_manifest_replay_host", "pcs_scrub_live_dev", "pcs_scrub_live_host"}
    for name in names:
        assert hasattr(so, name) and name in pcs._SIGS
    assert names <= set(pcs.header_functions())
    assert pcs.abi_version() == 7 == pcs.ABI_VERSION
    text = open(pcs.HEADER_PATH).read()
    assert "#define PCS_ABI_VERSION 7" in text and "detect with\n *      dlsym" in text
    for t in ("pcs_replay_report", "pcs_replay_summary", "pcs_live_page", "pcs_live_summary"):
        assert f"typedef struct {t} {{" in text
    assert (pcs.REPLAY_REPORT_DTYPE.itemsize, pcs.REPLAY_SUMMARY_DTYPE.itemsize) == (128, 96)
    assert (pcs.LIVE_PAGE_DTYPE.itemsize, pcs.LIVE_SUMMARY_DTYPE.itemsize) == (16, 128)
    assert pcs.REPLAY_REPORT_DTYPE == rr.REPORT_DTYPE and pcs.REPLAY_SUMMARY_DTYPE == rr.SUMMARY_DTYPE
    assert pcs.LIVE_PAGE_DTYPE == rr.LIVE_PAGE_DTYPE and pcs.LIVE_SUMMARY_DTYPE == rr.LIVE_SUMMARY_DTYPE
    # the field order of the header's structs is the dtypes'
    for t, dt in (("pcs_replay_report", rr.REPORT_DTYPE), ("pcs_replay_summary", rr.SUMMARY_DTYPE),
                  ("pcs_live_page", rr.LIVE_PAGE_DTYPE), ("pcs_live_summary", rr.LIVE_SUMMARY_DTYPE)):
        body = re.sub(r"/\*.*?\*/", "", text.split(f"typedef struct {t} {{")[1].split("}")[0], flags=re.S)
        assert tuple(re.findall(r"\b([a-z_0-9]+)\s*(?:\[\d+\])?\s*[,;]", body)) == dt.names, t
    for fn in ("manifest_replay_async", "manifest_replay_dev", "manifest_replay_host", "scrub_live_async",
               "scrub_live", "scrub_live_host"):
        assert callable(getattr(pcs, fn))
    assert (pcs.REPLAY_OK, pcs.REPLAY_NOT_REPLAYABLE, pcs.REPLAY_MALFORMED, pcs.REPLAY_TABLE_CAP) == (0, 1, 2, 3)


def test_replay_tile_key():
    assert pcs.TUNE_REPLAY_TILE == 39 and "PCS_TUNE_REPLAY_TILE = 39" in open(pcs.HEADER_PATH).read()
    default = pcs.get_tuning(39)
    assert default == 4096 and pcs.get_tuning(40) == -1
    for bad in (0, 32, 63, 65, 96, 1000, 8192, 1 << 20):
        with pytest.raises(pcs.PcsError):
            pcs.set_tuning(39, bad)
        assert pcs.get_tuning(39) == default
    try:
        for good in (64, 128, 4096):
            pcs.set_tuning(39, good)
            assert pcs.get_tuning(39) == good
    finally:
        pcs.set_tuning(39, default)


def test_cpp_symbols_in_batch_library_only():
    nm = lambda path: subprocess.run(["nm", "-D", "-C", "--defined-only", path], capture_output=True, text=True,
                                     check=True).stdout
    out, drop = nm(pcs.LIB_PATH), nm(pcs.DROPIN_LIB_PATH)
    for sym in ("eloqstore::TryReplayManifests(", "eloqstore::ReplayManifests(", "eloqstore::TryScrubLive(",
                "eloqstore::ScrubLive("):
        assert out.count(sym) == 1, sym
        assert sym not in drop, sym


# ---- arguments -------------------------------------------------------------------
def _replay_args(n=2):
    imgs = [np.frombuffer(bytes(rr.manifest(5, [rr.fp(k)], [[(1, rr.fp(2))]])), np.uint8) for k in range(n)]
    ptrs = (ctypes.c_uint64 * n)(*[i.ctypes.data for i in imgs])
    sizes = (ctypes.c_uint64 * n)(*[i.size for i in imgs])
    reports = (ctypes.c_uint64 * (16 * n))()
    summary = (ctypes.c_uint64 * 12)()
    table = (ctypes.c_uint64 * 16)()
    return ptrs, sizes, reports, summary, table, imgs


def test_replay_host_argument_checks_come_first():
    so = pcs.lib()
    ptrs, sizes, reports, summary, table, _keep = _replay_args()
    f = so.pcs_manifest_replay_host
    assert f(ptrs, sizes, 2, 4096, None, reports, None, table, 16) == pcs.PCS_ERR_INVALID
    assert b"summary is null" in so.pcs_last_error()
    assert f(None, sizes, 2, 4096, None, reports, summary, table, 16) == pcs.PCS_ERR_INVALID
    assert f(ptrs, None, 2, 4096, None, reports, summary, table, 16) == pcs.PCS_ERR_INVALID
    assert f(ptrs, sizes, 2, 4096, None, None, summary, table, 16) == pcs.PCS_ERR_INVALID
    assert b"reports is null" in so.pcs_last_error()
    assert f(ptrs, sizes, 2, 4096, None, reports, summary, None, 16) == pcs.PCS_ERR_INVALID
    assert b"table is null" in so.pcs_last_error()
    for align in (0, 1, 32, 100, 4095, 131072):
        assert f(ptrs, sizes, 2, align, None, reports, summary, table, 16) == pcs.PCS_ERR_INVALID, align
        assert b"power of two in [64, 65536]" in so.pcs_last_error()
    assert f((ctypes.c_uint64 * 2)(ptrs[0], 0), sizes, 2, 4096, None, reports, summary, table, 16) == pcs.PCS_ERR_INVALID
    assert b"non-zero size is null" in so.pcs_last_error()
    assert f(ptrs, (ctypes.c_uint64 * 2)(sizes[0], 1 << 32), 2, 4096, None, reports, summary, table,
             16) == pcs.PCS_ERR_INVALID
    assert b"too large" in so.pcs_last_error()
    # the device form checks its arguments before it looks for a device too
    g = so.pcs_manifest_replay_dev
    assert g(0, 0, 0, 0, 0, 4096, 0, 0, 0, 0, 0, 0) == pcs.PCS_ERR_INVALID
    assert g(8, 1 << 32, 8, 8, 1, 4096, 0, 8, 8, 8, 4, 0) == pcs.PCS_ERR_INVALID
    assert b"below 2^32" in so.pcs_last_error()
    try:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 1)
        assert f(ptrs, sizes, 2, 4096, None, reports, summary, None, 0) == pcs.PCS_ERR_HIP
        assert b"injected failure" in so.pcs_last_error() and pcs.get_tuning(pcs.TUNE_FAIL_INJECT) == 0
    finally:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 0)


def test_scrub_live_host_argument_checks_come_first():
    so = pcs.lib()
    cls = (ctypes.c_uint8 * 8)(*[1] * 8)
    table = (ctypes.c_uint64 * 4)(*[rr.fp(k) for k in range(4)])
    summary = (ctypes.c_uint64 * 16)()
    damaged = (ctypes.c_uint64 * 16)()
    f = so.pcs_scrub_live_host
    assert f(cls, 8, 0, table, 4, None, None, damaged, 8) == pcs.PCS_ERR_INVALID
    assert b"summary is null" in so.pcs_last_error()
    assert f(None, 8, 0, table, 4, None, summary, damaged, 8) == pcs.PCS_ERR_INVALID
    assert f(cls, 8, 0, None, 4, None, summary, damaged, 8) == pcs.PCS_ERR_INVALID
    assert f(cls, 8, 0, table, 4, None, summary, None, 8) == pcs.PCS_ERR_INVALID
    assert b"damaged list is null" in so.pcs_last_error()
    assert f(cls, 8, 0, table, 1 << 32, None, summary, damaged, 8) == pcs.PCS_ERR_INVALID
    assert b"2^32 - 1" in so.pcs_last_error()
    assert f(cls, 8, (1 << 61) - 3, table, 4, None, summary, damaged, 8) == pcs.PCS_ERR_INVALID
    assert so.pcs_scrub_live_dev(0, 8, 0, 0, 0, 0, 0, 0, 0, 0) == pcs.PCS_ERR_INVALID


@pytest.mark.skipif(HAVE_GPU, reason="checks the no-GPU failure path")
def test_entry_points_fail_loudly_without_a_gpu(tmp_path):
    so = pcs.lib()
    ptrs, sizes, reports, summary, table, _keep = _replay_args()
    assert so.pcs_manifest_replay_host(ptrs, sizes, 2, 4096, None, reports, summary, table, 16) == pcs.PCS_ERR_NO_DEVICE
    assert b"no usable HIP device" in so.pcs_last_error()
    assert so.pcs_manifest_replay_host(None, None, 0, 4096, None, None, summary, None, 0) == pcs.PCS_ERR_NO_DEVICE
    assert so.pcs_manifest_replay_dev(0, 0, 0, 0, 0, 4096, 0, 0, summary, 0, 0, 0) == pcs.PCS_ERR_NO_DEVICE
    cls = (ctypes.c_uint8 * 8)(*[1] * 8)
    live = (ctypes.c_uint64 * 16)()
    assert so.pcs_scrub_live_host(cls, 8, 0, None, 0, None, live, None, 0) == pcs.PCS_ERR_NO_DEVICE
    assert so.pcs_scrub_live_dev(cls, 8, 0, None, 0, None, live, None, 0, 0) == pcs.PCS_ERR_NO_DEVICE
    with pytest.raises(pcs.PcsError):
        pcs.manifest_replay_host([bytes(rr.manifest(1, [9]))], table_cap=4)
    with pytest.raises(pcs.PcsError):
        pcs.scrub_live_host(np.ones(4, np.uint8), 0, np.zeros(0, np.uint64))
    # the tool has no CPU fallback: a readable manifest is an error, not a verdict
    m = tmp_path / "manifest_1"
    m.write_bytes(bytes(rr.manifest(1, [9])))
    d = tmp_path / "data_0_1"
    d.write_bytes(bytes(4096))
    r = subprocess.run([pcs.TOOL_PATH, "--live", str(m), "4096", "6", str(d)], capture_output=True, text=True)
    assert r.returncode == 1 and "Manifest replay failed" in r.stderr and r.stdout == ""


def test_cli_live_usage_and_name_errors(tmp_path):
    run = lambda *a: subprocess.run([pcs.TOOL_PATH, *a], capture_output=True, text=True)
    r = run()
    assert r.returncode == 1 and "--live <manifest_file> <page_size_bytes> <pages_per_file_shift> <data_file>..." in r.stderr
    r = run("--live", "m", "4096", "6")
    assert r.returncode == 1 and "Usage:" in r.stderr and r.stdout == ""
    r = run("--live", str(tmp_path / "m"), "4096", "6", str(tmp_path / "data_12"))
    assert r.returncode == 1 and "Not a data file name" in r.stderr
    r = run("--live", str(tmp_path / "missing"), "4096", "6", str(tmp_path / "data_1_2"))
    assert r.returncode == 1 and r.stderr.startswith(f"Failed to open {tmp_path / 'missing'}: ")
    r = run("--live", str(tmp_path / "m"), "big", "6", str(tmp_path / "data_1_2"))
    assert r.returncode == 1 and "Invalid page size" in r.stderr
    r = run("--live", str(tmp_path / "m"), "0", "6", str(tmp_path / "data_1_2"))  # no division by a page size of 0
    assert r.returncode == 1 and "Invalid page size" in r.stderr
    r = run("--live", str(tmp_path / "m"), "4096", "6", str(tmp_path / "data_1_2"), str(tmp_path / "x" / "data_1_9"))
    assert r.returncode == 1 and "File id 1 is given twice" in r.stderr


def test_manifest_replay_logic_under_asan_ubsan():
    """csrc/manifest_replay.h (argument rules, the group carry, the summary,
    the data-file name rule, the tool's text and exit codes), driven by a
    stand-alone program built with -fsanitize=address,undefined."""
    exe = os.path.join(HERE, "cpp", "manifest_replay_logic_test_asan")
    if not os.path.exists(exe):
        pytest.skip("sanitizer build unavailable on this host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "manifest replay logic ok" in r.stdout
