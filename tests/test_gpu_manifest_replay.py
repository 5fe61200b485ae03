"""Manifest replay on the GPU: pcs_manifest_replay_dev / _host bit for bit
against tests/replay_ref.py (a sequential pure-Python decoder), with poisoned
outputs and sentinels behind them: every varint length, every alignment of the
mapping section, the decode tile's edges, last-writer-wins, every malformed
rule, every verdict, batches, the table cap, streams, a snapshot that crosses
the 1 MiB chunk edge, the host form above its staging budget and the injected
failure."""
import struct

import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
import manifest_ref as mr
import replay_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A
NO = rr.NO
DEFAULT_TILE = 4096


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(DEV)


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for k in want.dtype.names:
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist()[:8], want[k].tolist()[:8])


_ALIVE = []  # inputs of calls on side streams, until the next synchronize


def call_dev(images, align, cap, stream=None, scan=True):
    """One device call with poisoned outputs -> the raw output tensors."""
    n = len(images)
    buf, offs, sizes = mr.pack(images, align)
    base = torch.from_numpy(buf.copy()).to(DEV) if buf.size else torch.zeros(8, dtype=torch.uint8, device=DEV)
    o = (torch.full((n + 2, 12), SENTINEL, dtype=torch.int64, device=DEV) if scan else False,
         torch.full((n + 2, 16), SENTINEL, dtype=torch.int64, device=DEV),
         torch.full((12,), 0x1234567, dtype=torch.int64, device=DEV),
         torch.full((cap + 2,), SENTINEL, dtype=torch.int64, device=DEV))
    d_offs, d_sizes = to_dev(offs), to_dev(sizes)
    if stream is not None:
        # the inputs and the poison were written on torch's current stream: the call's stream waits for them, and
        # the inputs stay referenced until the caller has synchronised (a freed tensor's memory may be handed out
        # again while the call still reads it)
        stream.wait_stream(torch.cuda.current_stream())
        _ALIVE.append((base, d_offs, d_sizes))
    pcs.manifest_replay_async(base, d_offs, d_sizes, align, cap, buf.size, n, o[0], o[1], o[2],
                              o[3] if cap else None, stream)
    return o


def check(o, want, images, align, cap, what=""):
    wreps, ws, wrows = want
    n = len(images)
    scan_reports, reports, summary, table = (None if t is False else t.cpu().numpy().view(np.uint64) for t in o)
    same(np.array([summary.view(rr.SUMMARY_DTYPE)[0]]), np.array([ws]), what + " summary")
    same(np.ascontiguousarray(reports[:n]).view(rr.REPORT_DTYPE).reshape(-1), wreps, what + " reports")
    assert (reports[n:] == SENTINEL).all(), what
    rows = int(ws["n_rows_written"])
    assert rows == wrows.size
    assert np.array_equal(table[:rows], wrows), (what, "table")
    assert (table[rows:] == SENTINEL).all(), (what, "rows beyond n_rows_written")
    if scan_reports is not None:
        same(np.ascontiguousarray(scan_reports[:n]).view(mr.REPORT_DTYPE).reshape(-1), mr.scan(images, align)[0],
             what + " scan reports")
        assert (scan_reports[n:] == SENTINEL).all(), what


def replay_dev(images, align=4096, cap=None, stream=None, what="", scan=True):
    """One device call over `images`, checked against the model; cap None = the rows needed plus three."""
    want = rr.replay(images, align)
    if cap is None:
        cap = int(want[1]["n_rows"]) + 3
    want = rr.replay(images, align, cap)
    o = call_dev(images, align, cap, stream, scan)
    torch.cuda.synchronize()
    _ALIVE.clear()
    check(o, want, images, align, cap, what)
    return want


@pytest.fixture
def tile():
    def set_tile(v):
        pcs.set_tuning(pcs.TUNE_REPLAY_TILE, v)
    yield set_tile
    pcs.set_tuning(pcs.TUNE_REPLAY_TILE, DEFAULT_TILE)


def healthy(seed, pages=40, logs=2):
    rng = np.random.default_rng(seed)
    values = [rr.fp(int(x)) for x in rng.integers(0, 1 << 20, pages)]
    entries = [[(int(p), rr.fp(int(v))) for p, v in zip(rng.integers(0, pages + 10, 7), rng.integers(0, 1 << 20, 7))]
               for _ in range(logs)]
    return rr.manifest(1 << 20, values, entries, term=[(1, seed), (2, 9)])


# ---- varints ---------------------------------------------------------------------
def test_value_varints_of_every_length():
    values = [(1 << (7 * (n - 1))) | (rr.fp(n) if n == 1 else 0) for n in range(1, 10)] + [1 << 63]
    assert [len(rr.varint(v)) for v in values] == list(range(1, 11))
    # non-canonical encodings of a small value in every length, and a 10-byte one whose last byte wraps away
    section = rr.values_section(values) + b"".join(rr.varint(rr.fp(77), length=n) for n in range(1, 11))
    section += rr.varint((1 << 63) | rr.fp(3), top=0x7E)
    b = mr.Builder()
    b.add(rr.snapshot_payload(5, section), root=1, ttl_root=2)
    # the same values through a log, after page ids of every length; the 5-byte one carries bits above 2^32
    ids = [rr.varint(30 + n, length=n) for n in range(1, 6)] + [rr.varint(41, length=5, top=0x70)]
    vals = values[:3] + [rr.fp(1 << 40), (1 << 63) | 2, values[8]]
    b.add(rr.log_payload(b"".join(i + rr.varint(v) for i, v in zip(ids, vals))), root=3, ttl_root=4)
    reps, s, rows = replay_dev([b.data()])
    assert int(reps[0]["status"]) == rr.OK and int(reps[0]["snapshot_pages"]) == 21
    assert int(rows[20]) == rr.fp(3) | 1 << 63 and int(rows[41]) == values[8] and int(reps[0]["table_size"]) == 42
    assert int(reps[0]["max_fp_id"]) == (1 << 40) + 1


@pytest.mark.parametrize("align", [64, 4096])
def test_mapping_section_at_every_alignment(align):
    images = []
    for d in range(18):
        values = [rr.fp(1000 * d + k) if k % 3 else 1 << (7 * (k % 9)) for k in range(70)]
        images.append(rr.manifest(10, values, [[(k, rr.fp(5 * k + d)) for k in range(0, 80, 9)]], align,
                                  dict_bytes=bytes(range(200, 200 + d))))
    reps, s, rows = replay_dev(images, align)
    assert reps["dict_bytes"].tolist() == list(range(18)) and reps["status"].tolist() == [rr.OK] * 18


# ---- tile edges --------------------------------------------------------------------
def edge_images(t):
    one = lambda n: b"".join(rr.varint(rr.fp(k % 15)) for k in range(n))  # n one-byte values
    two = lambda n: b"".join(rr.varint(rr.fp(16 + k % 100)) for k in range(n))  # n two-byte values
    big = rr.varint((1 << 63) | rr.fp(12345))
    assert len(one(3)) == 3 and len(two(3)) == 6 and len(big) == 10
    sections = [two(t // 2) + one(1) + two(5),               # ends on the tile's last byte, then on the next one's first
                one(t - 5) + big + one(t),                    # a 10-byte value across the edge
                one(t - 9) + big + big,                       # ... ending on the last byte, the next from the first
                one(2 * t - 1) + big]
    sections += [one(n) for n in (0, 1, t - 1, t, t + 1, 3 * t)]
    images = []
    for k, sec in enumerate(sections):
        b = mr.Builder()
        b.add(rr.snapshot_payload(9, sec, dict_bytes=bytes(k)), root=k)
        images.append(b.data())
    # log sections of 0, 2, t - 1, t and t + 1 bytes (t = 1 mod 3), and a page id split from its value by the edge
    e3 = lambda n: b"".join(rr.varint(k % 100) + rr.varint(rr.fp(16 + k)) for k in range(n))      # 3 bytes each
    e2 = lambda n: b"".join(rr.varint(100 + k % 28) + rr.varint(rr.fp(k % 15)) for k in range(n))       # 2 bytes each
    logs = [b"", e2(1), e3((t - 1) // 3), e3((t - 4) // 3) + e2(2), e3((t - 1) // 3) + e2(1),
            e2((t - 2) // 2) + rr.varint(7) + big + e2(3), e2((t - 2) // 2) + rr.varint(8, length=5) + big]
    assert [len(x) for x in logs[:5]] == [0, 2, t - 1, t, t + 1]
    b = mr.Builder()
    b.add(rr.snapshot_payload(9, one(7)))
    for sec in logs:
        b.add(rr.log_payload(sec, rr.term_section([(1, 2)] * (t // 2))))
    images.append(b.data())
    return images


@pytest.mark.parametrize("t", [64, DEFAULT_TILE])
def test_tile_edges(tile, t):
    tile(t)
    assert pcs.get_tuning(pcs.TUNE_REPLAY_TILE) == t
    reps, s, rows = replay_dev(edge_images(t), what=f"tile {t}")
    assert reps["status"].tolist() == [rr.OK] * len(reps)


def test_results_do_not_depend_on_the_tile(tile):
    images = [healthy(k, pages=300, logs=3) for k in range(5)]
    for t in (64, 256, 4096):
        tile(t)
        replay_dev(images, what=f"tile {t}")


# ---- apply -------------------------------------------------------------------------
def test_last_writer_wins():
    values = [rr.fp(100 + k) for k in range(50)]
    logs = [[(5, rr.fp(1)), (5, rr.fp(2)), (5, rr.fp(3)), (6, rr.fp(9))],       # three times in one record
            [(5, rr.fp(4)), (7, rr.INVALID), (6, rr.fp(10))],                     # ... and across records; delete
            [(7, rr.fp(11)), (5, rr.fp(5)), (49, rr.fp(12)), (50, rr.fp(13))],    # map again; the table's end and one past
            [(1050, rr.fp(14))],                                                  # 1,000 beyond: gap rows are 7
            [(2, 0), (3, 2 << 3 | 2), (4, rr.INVALID), (8, 4 << 3)]]              # types 0, 2 and 7: not mapped
    reps, s, rows = replay_dev([rr.manifest(200, values, logs)])
    r = reps[0]
    assert [int(rows[k]) for k in (5, 6, 7, 49, 50, 1050)] == [rr.fp(x) for x in (5, 10, 11, 12, 13, 14)]
    assert int(r["table_size"]) == 1051 and (rows[51:1050] == rr.INVALID).all()
    assert int(r["n_mapped"]) == 50 - 4 + 2 and int(r["n_log_entries"]) == 16


def test_max_fp_id_from_an_overwritten_entry_and_pages_beyond_it():
    logs = [[(0, rr.fp(5000)), (0, rr.fp(7))], [(1, rr.fp(8))]]
    reps, s, rows = replay_dev([rr.manifest(10, [rr.fp(1), rr.fp(2), rr.fp(3)], logs)])
    assert int(reps[0]["max_fp_id"]) == 5001 and int(reps[0]["n_fp_beyond_max"]) == 0
    # the snapshot's own max_fp_id below what it maps: three pages at or above it
    reps, s, rows = replay_dev([rr.manifest(20, [rr.fp(19), rr.fp(20), rr.fp(21), rr.fp(900)], [[(9, rr.fp(3))]])])
    assert int(reps[0]["max_fp_id"]) == 20 and int(reps[0]["n_fp_beyond_max"]) == 3
    assert (int(reps[0]["min_fp"]), int(reps[0]["max_fp"])) == (3, 900)


# ---- malformed ---------------------------------------------------------------------
def snap_image(payload, logs=()):
    b = mr.Builder()
    b.add(payload, root=1)
    for p in logs:
        b.add(p, root=2)
    return b.data()


GOOD_SNAP = rr.snapshot_payload(9, rr.values_section([rr.fp(k) for k in range(20)]))
GOOD_LOG = rr.log_payload(rr.entries_section([(3, rr.fp(77))]))
I32 = lambda v: struct.pack("<I", v)
MALFORMED = {
    "max_fp_id cut short": (snap_image(b"\x80\x80"), 0),
    "max_fp_id of 11 bytes": (snap_image(b"\x80" * 10 + b"\x01" + GOOD_SNAP), 0),
    "dict_len too large": (snap_image(rr.varint(5) + rr.varint(100) + b"abc" + I32(0) + I32(0)), 0),
    "dict_len of 6 bytes": (snap_image(rr.varint(5) + b"\x80" * 5 + b"\x00" + I32(0) + I32(0)), 0),
    "mapping_len + 8 > rem": (snap_image(rr.varint(5) + rr.varint(0) + I32(11) + b"\x01" * 10 + I32(0)), 0),
    "no room for mapping_len": (snap_image(rr.varint(5) + rr.varint(0) + b"\x00" * 7), 0),
    "term_len too large": (snap_image(rr.varint(5) + rr.varint(0) + I32(2) + b"\x01\x02" + I32(3) + b"\x01\x02"), 0),
    "dangling varint": (snap_image(rr.snapshot_payload(9, b"\x01\x82")), 0),
    "11-byte run": (snap_image(rr.snapshot_payload(9, b"\x09" + b"\x80" * 10 + b"\x01")), 0),
    "11-byte run at the section's start": (snap_image(rr.snapshot_payload(9, b"\x80" * 10 + b"\x01")), 0),
    "6-byte page id": (snap_image(GOOD_SNAP, [GOOD_LOG, rr.log_payload(b"\x80" * 5 + b"\x01" + b"\x09")]), 2),
    "odd count in a log": (snap_image(GOOD_SNAP, [rr.log_payload(b"\x01\x09\x02"), GOOD_LOG]), 1),
    "odd term count": (snap_image(rr.snapshot_payload(9, b"\x09", b"\x01")), 0),
    "odd term count in a log": (snap_image(GOOD_SNAP, [rr.log_payload(b"\x01\x09", b"\x01\x02\x03")]), 1),
    "11-byte run in a term": (snap_image(GOOD_SNAP, [rr.log_payload(b"", b"\x80" * 10 + b"\x01\x01")]), 1),
    "log payload shorter than 8": (snap_image(GOOD_SNAP, [GOOD_LOG, GOOD_LOG, b"\x00" * 7]), 3),
    "log mapping_len + 8 > L": (snap_image(GOOD_SNAP, [I32(3) + b"\x01\x09" + I32(0)]), 1),
    "two bad records": (snap_image(GOOD_SNAP, [GOOD_LOG, b"\x00" * 7, rr.log_payload(b"\x01")]), 2),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed(case):
    img, record = MALFORMED[case]
    images = [healthy(1), img, healthy(2)]
    reps, s, rows = replay_dev(images, what=case)
    assert reps["status"].tolist() == [rr.OK, rr.MALFORMED, rr.OK] and int(reps[1]["malformed_record"]) == record
    alone = rr.replay([healthy(1), healthy(2)])[2]
    assert np.array_equal(rows, alone)  # the neighbours' rows are what they are without it


# ---- verdicts ------------------------------------------------------------------------
def flip(img, record, at=25):
    img = bytearray(img)
    img[mr.walk(img)[0][record]["offset"] + at] ^= 0x40
    return img


def test_verdicts():
    full = rr.manifest(50, [rr.fp(k) for k in range(30)], [[(k, rr.fp(100 * j + k))] for j in range(1, 4) for k in (2, 40)])
    snapshot_only = rr.manifest(50, [rr.fp(k) for k in range(30)])
    torn = flip(flip(flip(flip(full, 3), 4), 5), 6)
    # a malformed payload behind the first corrupt record is never looked at
    b = mr.Builder()
    b.add(GOOD_SNAP)
    b.add(GOOD_LOG)
    b.add(b"\x00" * 7)
    torn_bad = flip(b.data(), 2)
    broken = flip(full, 2)
    bad_snapshot = flip(full, 0)
    images = [snapshot_only, torn, torn_bad, broken, bad_snapshot, b"", full]
    reps, s, rows = replay_dev(images)
    assert reps["status"].tolist() == [0, 0, 0, 1, 1, 1, 0]
    assert reps["n_replayed"].tolist() == [1, 3, 2, 0, 0, 0, 7]
    assert reps["table_size"].tolist() == [30, 41, 20, 0, 0, 0, 41]
    assert int(s["first_bad_image"]) == 3 and s["n_by_status"].tolist() == [4, 3, 0, 0]


# ---- batches ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 257])
def test_batches(n):
    images = [b"" if k % 7 == 3 else healthy(k, pages=5 + k % 40, logs=k % 3) for k in range(n)]
    replay_dev(images, align=64 if n > 2 else 4096)
    replay_dev(images, align=64 if n > 2 else 4096, scan=False)  # NULL scan reports


def test_no_image_and_only_empty_images():
    replay_dev([])
    reps, s, rows = replay_dev([b"", b""])
    assert reps["status"].tolist() == [rr.NOT_REPLAYABLE] * 2 and int(s["n_rows"]) == 0


def test_invalid_layout():
    images = [healthy(1), healthy(2)]
    buf, offs, sizes = mr.pack(images, 4096)
    offs[1] -= 4096  # overlaps image 0
    base = torch.from_numpy(buf.copy()).to(DEV)
    reports = torch.full((4, 16), SENTINEL, dtype=torch.int64, device=DEV)
    table = torch.full((200,), SENTINEL, dtype=torch.int64, device=DEV)
    _, _, summary, _ = pcs.manifest_replay_async(base, to_dev(offs), to_dev(sizes), 4096, 200, buf.size, 2, None,
                                                 reports, None, table)
    torch.cuda.synchronize()
    assert summary.cpu().tolist() == [2] + [0] * 9 + [1, 0]
    assert (reports.cpu().numpy().view(np.uint64) == SENTINEL).all()
    assert (table.cpu().numpy().view(np.uint64) == SENTINEL).all()


# ---- table cap ---------------------------------------------------------------------------
def test_table_cap():
    images = [healthy(1, pages=30), healthy(2, pages=50), b"", healthy(3, pages=20), healthy(4, pages=10)]
    sizes = rr.replay(images)[0]["table_size"].tolist()
    total = sum(sizes)
    reps, s, rows = replay_dev(images, cap=total)  # exact
    assert reps["status"].tolist() == [0, 0, 1, 0, 0] and int(s["n_rows_written"]) == total
    reps, s, rows = replay_dev(images, cap=total - 1)  # one short: the last image does not fit
    assert reps["status"].tolist() == [0, 0, 1, 0, 3] and int(s["n_rows"]) == total
    reps, s, rows = replay_dev(images, cap=sizes[0] + sizes[1] - 1)  # image 1 and the later non-empty ones
    assert reps["status"].tolist() == [0, 3, 1, 3, 3] and int(s["n_rows_written"]) == sizes[0]
    assert reps["table_first"].tolist() == [0, sizes[0], sizes[0] + sizes[1], sizes[0] + sizes[1], total - sizes[4]]
    assert int(reps[1]["max_fp_id"]) == 1 << 20 and int(reps[1]["n_mapped"]) == 0 and int(reps[1]["min_fp"]) == NO
    reps, s, rows = replay_dev(images, cap=0)  # NULL table
    assert reps["status"].tolist() == [3, 3, 1, 3, 3] and int(s["n_rows_written"]) == 0


# ---- determinism ---------------------------------------------------------------------------
def test_two_streams_and_the_same_call_twice():
    a = [rr.manifest(99, [rr.fp(k) for k in range(500)],
                     [[(int(p), rr.fp(1000 * j + i)) for i, p in enumerate(np.random.default_rng(j).integers(0, 40, 300))]
                      for j in range(6)])]
    b = [healthy(k, pages=100, logs=4) for k in range(9)]
    wa, wb = rr.replay(a, 4096, 700), rr.replay(b, 4096, 2000)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        outs.append((call_dev(a, 4096, 700, s1), call_dev(b, 4096, 2000, s2)))
    torch.cuda.synchronize()
    _ALIVE.clear()
    for oa, ob in outs:
        check(oa, wa, a, 4096, 700, "stream 1")
        check(ob, wb, b, 4096, 2000, "stream 2")
    for x, y in zip(outs[0][0] + outs[0][1], outs[1][0] + outs[1][1]):
        assert torch.equal(x, y)


# ---- a larger image ------------------------------------------------------------------------
def test_a_snapshot_across_the_chunk_edge():
    rng = np.random.default_rng(5)
    values = [rr.fp(int(x)) for x in rng.integers(0, 1 << 26, 300_000)]
    logs = [[(int(p), rr.fp(int(v))) for p, v in zip(rng.integers(0, 300_500, 100), rng.integers(0, 1 << 27, 100))]
            for _ in range(50)]
    img = rr.manifest(1 << 26, values, logs)
    assert mr.walk(img)[0][0]["payload_len"] > (1 << 20)
    reps, s, rows = replay_dev([healthy(1), img, healthy(2)])
    assert int(reps[1]["snapshot_pages"]) == 300_000 and int(reps[1]["n_log_entries"]) == 5000


# ---- host form -----------------------------------------------------------------------------
def host_check(images, cap, what=""):
    want = rr.replay(images, 4096, cap)
    reps, s, rows, sreps = pcs.manifest_replay_host(images, 4096, cap)
    same(np.array([s]).view(rr.SUMMARY_DTYPE), np.array([want[1]]), what + " summary")
    same(reps.view(rr.REPORT_DTYPE), want[0], what + " reports")
    assert np.array_equal(rows, want[2]), what
    same(sreps.view(mr.REPORT_DTYPE), mr.scan(images, 4096)[0], what + " scan reports")
    return want


def test_host_form_above_the_staging_budget():
    # 40 images of 1 MiB (the dict carries the bulk): more than one 32 MiB staging group
    images = []
    for k in range(40):
        dict_bytes = bytes([k]) * ((1 << 20) - 8192)
        images.append(rr.manifest(500 + k, [rr.fp(k * 1000 + j) for j in range(60 + k)],
                                  [[(j, rr.fp(7 * j + k)) for j in range(0, 90, 11)]], dict_bytes=dict_bytes))
    images[17] = flip(images[17], 0)  # not replayable: table_first carries over it, and over the group edge
    assert all(len(i) == 1 << 20 for i in images) and sum(len(i) for i in images) > 32 << 20
    total = int(host_check(images, 1 << 14)[1]["n_rows"])
    # the cap runs out inside the second group
    want = host_check(images, total - 200, "short cap")
    assert int(want[0]["status"][39]) == rr.TABLE_CAP and int(want[0]["status"][3]) == rr.OK
    # and equals the device form over the whole batch
    replay_dev(images, cap=total - 200)


def test_host_form_small_and_empty():
    host_check([healthy(1), b"", MALFORMED["dangling varint"][0], healthy(2)], 300)
    host_check([], 0)
    host_check([healthy(3)], 0)


def test_fail_injection():
    images = [healthy(1)]
    pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 1)
    try:
        with pytest.raises(pcs.PcsError) as e:
            pcs.manifest_replay_host(images, 4096, 100)
        assert e.value.code == pcs.PCS_ERR_HIP
    finally:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 0)
    host_check(images, 100)
