"""Manifest scan on the GPU: pcs_manifest_scan_dev / _host, the C++ and CLI
layers, bit-exact against tests/manifest_ref.py (a pure-Python walker whose
records are checked with the reference's xxhash.c): every XXH3 length class of
a record, the 1 MiB chunk edges, every way an image can end, garbage lengths,
every verdict, the tile edges of the chain walk, batches, caps, streams and
invalid layouts."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
import manifest_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0x5A5A5A5A5A5A5A5A
NO = mr.NO
MIB = 1 << 20

# content length 12 + len: the XXH3 edges 16/17, 128/129, 240/241 and 248/249, the 1 KiB block edge and the
# records around the one that fills a 4096 slot exactly
LENGTHS = [0, 1, 4, 5, 116, 117, 228, 229, 236, 237, 1003, 1004, 1005, 1012, 1013, 4075, 4076, 4077]
# last chunk of 1 MiB - 1, exactly 1 MiB, 1 byte (after one and after two full chunks), a few hundred bytes
SNAPSHOTS = [MIB - 13, MIB - 12, MIB - 11, 2 * MIB - 12, 2 * MIB - 11, 3 * MIB + 500]


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(DEV)


def outputs(n_images, cap):
    return (torch.full((n_images + 2, 12), SENTINEL, dtype=torch.int64, device=DEV),
            torch.full((12,), 0x1234567, dtype=torch.int64, device=DEV),
            torch.full((cap + 2, 5), SENTINEL, dtype=torch.int64, device=DEV))


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for k in want.dtype.names:
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist()[:8], want[k].tolist()[:8])


def read_outputs(o, n_images, cap):
    reports, summary, records = (t.cpu().numpy().view(np.uint64) for t in o)
    s = summary.view(mr.SUMMARY_DTYPE)[0]
    return reports, s, records


def check_outputs(o, want, n_images, cap, what=""):
    """Poisoned reports, summary and records against the reference, and the sentinels behind them."""
    wreps, ws, wrecs = want
    reports, s, records = read_outputs(o, n_images, cap)
    same(np.array([s]), np.array([ws]), what + " summary")
    same(np.ascontiguousarray(reports[:n_images]).view(mr.REPORT_DTYPE).reshape(-1), wreps, what + " reports")
    assert (reports[n_images:] == SENTINEL).all(), what
    listed = int(ws["n_listed"])
    same(np.ascontiguousarray(records[:listed]).view(np.uint8).view(mr.RECORD_DTYPE).reshape(-1), wrecs[:listed],
         what + " records")
    assert (records[listed:] == SENTINEL).all(), what


def scan_dev(images, align=4096, cap=None, stream=None, what=""):
    """One device call over `images` packed at multiples of align, checked against the walker."""
    want = mr.scan(images, align, record_cap=1 << 30 if cap is None else cap)
    if cap is None:
        cap = int(want[1]["n_records"]) + 3
        want = mr.scan(images, align, record_cap=cap)
    buf, offs, sizes = mr.pack(images, align)
    base = torch.from_numpy(buf.copy()).to(DEV) if buf.size else torch.zeros(8, dtype=torch.uint8, device=DEV)
    o = outputs(len(images), cap)
    pcs.manifest_scan_async(base, to_dev(offs), to_dev(sizes), align, buf.size, len(images), o[0], o[1],
                            o[2] if cap else None, cap, stream)
    torch.cuda.synchronize()
    check_outputs(o, want, len(images), cap, what)
    return want


def logs(b, n, seed):
    for k in range(n):
        b.add_random((seed * 37 + k * 101) % 600, seed * 100 + k)


# ---- hash classes ---------------------------------------------------------------
def test_every_length_class():
    images = [mr.image([n], seed=n + 1) for n in LENGTHS] + [mr.image(LENGTHS, seed=99)]
    reps, s, recs = scan_dev(images)
    assert int(s["n_records"]) == 2 * len(LENGTHS) and int(s["n_corrupt"]) == 0
    assert reps["end_reason"].tolist() == [mr.END_CLEAN] * len(images)
    # the same records with one body byte flipped each: every class must notice
    for img in images:
        for r in mr.walk(img)[0]:
            img[r["offset"] + 8 + (r["payload_len"] + 11) // 2] ^= 0x10
    reps, s, recs = scan_dev(images)
    assert int(s["n_ok"]) == 0 and not recs["ok"].any()


@pytest.mark.parametrize("snap", SNAPSHOTS)
def test_chunk_edges(snap):
    b = mr.Builder()
    b.add_random(snap, snap)
    logs(b, 5, 3)
    img = b.data()
    reps, s, recs = scan_dev([img])
    assert int(reps[0]["verdict"]) == mr.CLEAN and int(reps[0]["max_record_bytes"]) == 20 + snap
    # a flipped byte in the last chunk, in the first, and on each side of the first chunk edge
    for at in (8 + 12 + snap - 1, 8 + 3, 8 + MIB - 1, 8 + MIB):
        bad = bytearray(img)
        bad[min(at, 20 + snap - 1)] ^= 1
        reps, s, recs = scan_dev([bad])
        assert int(reps[0]["verdict"]) == mr.BAD_SNAPSHOT and int(reps[0]["n_ok"]) == 5


# ---- ends -----------------------------------------------------------------------------
def test_every_way_an_image_ends():
    img = mr.image([300, 9000, 40], seed=5)  # records at 0, 4096, 16384
    images = [b"", bytes(1), bytes(19), bytes(img[:19])]
    for start, ln in ((0, 300), (4096, 9000), (16384, 40)):
        nxt = mr.round_up(start + 20 + ln, 4096)
        images += [img[:start], img[:start + 1], img[:start + 19], img[:start + 20], img[:start + 20 + ln // 2],
                   img[:start + 20 + ln - 1], img[:start + 20 + ln], img[:(start + 20 + ln + nxt) // 2], img[:nxt]]
    reps, s, recs = scan_dev(images)
    assert set(reps["end_reason"].tolist()) == {0, 1, 2, 3}
    assert reps["verdict"][:4].tolist() == [mr.EMPTY] * 4 and int(reps[0]["first_corrupt"]) == NO
    assert (reps["end_reason"][0], reps["end_reason"][1]) == (mr.END_CLEAN, mr.END_SHORT_HEADER)
    for k, img_k in enumerate(images):  # each one alone gives what it gives in the batch
        if k % 4 == 1:
            scan_dev([img_k], what=f"image {k}")


def test_garbage_lengths_stop_the_walk():
    base = mr.image([300, 700, 40, 80], seed=6)
    images = []
    for rec in (0, 2):
        o = mr.walk(base)[0][rec]["offset"]
        for ln in (0xFFFFFFFF, len(base) - o - 19, 0x7FFFFFF0, 0x80000000):
            img = bytearray(base)
            img[o + 16:o + 20] = struct.pack("<I", ln)
            images.append(img)
    # the last image of the buffer: a length that would run past total_bytes
    reps, s, recs = scan_dev(images)
    assert reps["end_reason"].tolist() == [mr.END_SHORT_PAYLOAD] * 8
    assert reps["n_records"].tolist() == [0] * 4 + [2] * 4
    scan_dev(images[:1])
    scan_dev(images[4:5])
    # one byte shorter fits: the record ends the image exactly and is corrupt
    img = bytearray(base)
    img[16:20] = struct.pack("<I", len(base) - 20)
    reps, s, recs = scan_dev([img])
    assert (int(reps[0]["n_records"]), int(reps[0]["end_reason"]), int(reps[0]["verdict"])) == (1, 0, mr.BAD_SNAPSHOT)


def test_headers_inside_a_payload_are_not_records():
    inner = mr.image([100, 200, 50], seed=9)  # three valid records at slot boundaries
    b = mr.Builder()
    b.add_random(10, 1)
    b.add(bytes(4076) + bytes(inner) + bytes(30), root=5)  # its payload holds the three at slots 2, 3, 4
    b.add_random(20, 2)
    img = b.data()
    assert img[2 * 4096:5 * 4096] == inner
    reps, s, recs = scan_dev([img, inner])
    assert reps["n_records"].tolist() == [3, 3] and recs["offset"].tolist() == [0, 4096, 6 * 4096, 0, 4096, 8192]
    # the same bytes from the embedded records on: there they are records
    reps, s, recs = scan_dev([img[2 * 4096:]])
    assert recs["offset"].tolist()[:3] == [0, 4096, 8192] and recs["ok"].tolist()[:3] == [1, 1, 1]


# ---- verdicts ---------------------------------------------------------------------------
def flipped(img, at, bit=1):
    out = bytearray(img)
    out[at] ^= bit
    return out


def test_every_verdict():
    img = mr.image([50, 5000, 0, 300, 7, 1200], seed=7)  # offsets 0, 4096, 12288, 16384, 20480, 24576
    offs = [r["offset"] for r in mr.walk(img)[0]]
    assert offs == [0, 4096, 12288, 16384, 20480, 24576]
    last3 = bytearray(img)
    for o in offs[3:]:
        last3[o + 21 if o != offs[4] else o + 20] ^= 0x40
    images = [img,
              flipped(img, 25), flipped(img, 3, 0x80),           # record 0: a body byte, the stored checksum
              flipped(img, 4096 + 4500), flipped(img, 12288 + 9),  # a middle record: ok records follow it
              flipped(img, offs[5] + 100), flipped(flipped(img, offs[5] + 100), offs[4] + 22), last3,
              bytes(img) + bytes(5 * 4096),                       # zero slots walk as corrupt 20-byte records
              bytes(img) + bytes(4096 + 7)]
    reps, s, recs = scan_dev(images)
    assert reps["verdict"].tolist() == [mr.CLEAN, mr.BAD_SNAPSHOT, mr.BAD_SNAPSHOT, mr.BROKEN, mr.BROKEN,
                                        mr.TORN_TAIL, mr.TORN_TAIL, mr.TORN_TAIL, mr.TORN_TAIL, mr.TORN_TAIL]
    assert reps["n_corrupt"].tolist() == [0, 1, 1, 1, 1, 1, 2, 3, 5, 1]
    assert reps["valid_prefix_bytes"].tolist()[5:] == [offs[5], offs[4], offs[3], len(img), len(img)]
    assert s["n_by_verdict"].tolist() == [1, 5, 2, 2, 0] and int(s["first_bad_image"]) == 1


def test_every_flipped_header_byte():
    img = mr.image([50, 5000, 0, 300], seed=8)
    images = [flipped(img, 4096 + k, bit) for k in range(20) for bit in (1, 0x80)]
    images += [flipped(img, k, 1) for k in range(20)]
    reps, s, recs = scan_dev(images)  # a flip in payload_len changes the walk: the walker decides
    assert len(set(reps["n_records"].tolist())) > 1 and mr.END_SHORT_PAYLOAD in reps["end_reason"].tolist()
    assert int(s["n_by_verdict"][mr.BROKEN]) and int(s["n_by_verdict"][mr.BAD_SNAPSHOT])


# ---- tile edges of the chain walk -------------------------------------------------------------
def tile_images():
    images = [mr.image([(k * 131) % 900 for k in range(n)], seed=n) for n in (63, 64, 65, 128, 129)]
    b = mr.Builder()
    logs(b, 60, 11)
    b.add_random(10 * 4096 + 100, 12)   # slots 60..70: across the edge of tile 0
    logs(b, 70, 13)                     # up to slot 140: across the edge of tile 1 one slot at a time
    images.append(b.data())
    b = mr.Builder()
    logs(b, 5, 14)
    b.add_random(3 * 64 * 4096 - 20, 15)  # slots 5..196: its next slot is three tiles on, at the same place
    logs(b, 3, 16)
    b.add_random(56 * 4096 - 20, 17)  # slots 200..255 exactly: its next slot is the first of a tile
    logs(b, 2, 18)
    images.append(b.data())
    # zero slots: 200 corrupt 20-byte records after 3 good ones
    images.append(bytes(mr.image([1, 2, 3])) + bytes(200 * 4096))
    return images


@pytest.fixture(scope="module")
def tile_reference():
    images = tile_images()
    return images, mr.scan(images, 4096, record_cap=1 << 20)


@pytest.mark.parametrize("tile", [64, 128, 0, 4096])
def test_tile_edges(tile_reference, tile):
    images, want = tile_reference
    cap = int(want[1]["n_records"]) + 1
    buf, offs, sizes = mr.pack(images)
    base = torch.from_numpy(buf).to(DEV)
    default = pcs.get_tuning(pcs.TUNE_MANIFEST_WALK_TILE)
    assert default == 2048
    try:
        if tile:
            pcs.set_tuning(pcs.TUNE_MANIFEST_WALK_TILE, tile)
        o = outputs(len(images), cap)
        pcs.manifest_scan_async(base, to_dev(offs), to_dev(sizes), 4096, buf.size, len(images), *o, cap)
        torch.cuda.synchronize()
        check_outputs(o, want, len(images), cap, f"tile {tile}")
        # one image per call as well: the span and the skip start in tile 0 there too
        for k in (1, 5, 6):
            one = mr.scan([images[k]], 4096, record_cap=cap)
            o = outputs(1, cap)
            pcs.manifest_scan_async(base[offs[k]:], to_dev([0]), to_dev([sizes[k]]), 4096, sizes[k], 1, *o, cap)
            torch.cuda.synchronize()
            check_outputs(o, one, 1, cap, f"tile {tile} image {k}")
    finally:
        pcs.set_tuning(pcs.TUNE_MANIFEST_WALK_TILE, default)


def test_a_tile_value_out_of_range_runs_at_the_default(tile_reference):
    images, _ = tile_reference
    try:
        for bad in (0, 1, 63, 100, 1 << 20):
            pcs.set_tuning(pcs.TUNE_MANIFEST_WALK_TILE, bad)
            scan_dev(images[4:6], what=f"tile {bad}")
    finally:
        pcs.set_tuning(pcs.TUNE_MANIFEST_WALK_TILE, 2048)


# ---- batches ------------------------------------------------------------------------------------
def mixed_images(n, seed=21):
    rng = np.random.default_rng(seed)
    images = []
    for k in range(n):
        kind = k % 7
        if kind == 3:
            images.append(b"")
            continue
        img = mr.image([int(x) for x in rng.integers(0, 6000, int(rng.integers(1, 9)))], seed=seed * 1000 + k)
        if kind == 1:
            img = flipped(img, int(rng.integers(0, len(img))))
        elif kind == 4:
            img = img[:int(rng.integers(1, len(img)))]
        elif kind == 5:
            img = bytes(img) + bytes(4096 * int(rng.integers(1, 4)))
        images.append(img)
    return images


@pytest.mark.parametrize("n", [1, 2, 257])
def test_batches_of_mixed_images(n):
    images = mixed_images(n)
    reps, s, recs = scan_dev(images)
    total = int(s["n_records"])
    if n == 257:
        assert all(int(x) for x in s["n_by_verdict"])  # every verdict occurs
        inside = int(reps[100]["first_record"]) + 1
        for cap in (0, 1, inside, total, total + 5):
            scan_dev(images, cap=cap, what=f"cap {cap}")


def test_no_images_writes_the_whole_summary():
    o = outputs(0, 4)
    pcs.manifest_scan_async(torch.zeros(8, dtype=torch.uint8, device=DEV), None, None, 4096, 0, 0, *o, 4)
    torch.cuda.synchronize()
    check_outputs(o, mr.scan([], record_cap=4), 0, 4)
    assert o[1].cpu().numpy().view(np.uint64).tolist() == [0] * 9 + [NO, 0, NO]


def test_two_streams_interleaved():
    work = []
    for n, seed, cap in ((40, 31, 50), (9, 32, 1000)):
        images = mixed_images(n, seed)
        buf, offs, sizes = mr.pack(images)
        work.append((torch.from_numpy(buf).to(DEV), to_dev(offs), to_dev(sizes), buf.size, n, cap,
                     mr.scan(images, record_cap=cap)))
    streams = [torch.cuda.Stream(device=DEV) for _ in work]
    torch.cuda.synchronize()
    outs = [[outputs(w[4], w[5]) for _ in range(8)] for w in work]
    for rep in range(8):
        for k, (base, off, size, total, n, cap, want) in enumerate(work):
            pcs.manifest_scan_async(base, off, size, 4096, total, n, *outs[k][rep], cap, stream=streams[k])
    torch.cuda.synchronize()
    for k, (base, off, size, total, n, cap, want) in enumerate(work):
        for o in outs[k]:
            check_outputs(o, want, n, cap, f"stream {k}")


def test_invalid_layouts_are_reported_not_followed():
    images = mixed_images(6, 41)
    images[3] = mr.image([10])
    buf, offs, sizes = mr.pack(images)
    total = buf.size
    base = torch.from_numpy(buf).to(DEV)
    cases = []
    bad = list(offs); bad[2] += 64; cases.append((bad, sizes, total, "misaligned"))
    bad = list(sizes); bad[1] = offs[2] - offs[1] + 1; cases.append((offs, bad, total, "overlapping"))
    bad = list(offs); bad[3], bad[4] = bad[4], bad[3]; cases.append((bad, sizes, total, "descending"))
    cases.append((offs, sizes, total - 1 - (4096 - sizes[5] % 4096) % 4096, "past total_bytes"))
    bad = list(sizes); bad[5] = 1 << 63; cases.append((offs, bad, total, "a huge size"))
    bad = list(offs); bad[0] = NO - 4095; cases.append((bad, sizes, total, "a huge offset"))
    bad = list(offs); bad[4] = offs[3]; cases.append((bad, sizes, total, "equal offsets of non-empty images"))
    for o_, s_, t_, what in cases:
        inv = mr.invalid_image(o_, s_, t_, 4096)
        assert inv is not None, what
        o = outputs(6, 8)
        pcs.manifest_scan_async(base, to_dev(o_), to_dev(s_), 4096, t_, 6, *o, 8)
        torch.cuda.synchronize()
        reports, s, records = read_outputs(o, 6, 8)
        assert o[1].cpu().numpy().view(np.uint64).tolist() == [6] + [0] * 10 + [inv], what
        assert (reports == SENTINEL).all() and (records == SENTINEL).all(), what
    # the valid layout right after, on the same scratch
    o = outputs(6, 8)
    pcs.manifest_scan_async(base, to_dev(offs), to_dev(sizes), 4096, total, 6, *o, 8)
    torch.cuda.synchronize()
    check_outputs(o, mr.scan(images, record_cap=8), 6, 8)
    # images need not cover the buffer; an empty image may share its successor's offset
    sub = [images[1], b"", images[4]]
    o = outputs(3, 64)
    pcs.manifest_scan_async(base, to_dev([offs[1], offs[4], offs[4]]), to_dev([sizes[1], 0, sizes[4]]), 4096, total, 3,
                            *o, 64)
    torch.cuda.synchronize()
    check_outputs(o, mr.scan(sub, record_cap=64), 3, 64)


def test_dev_argument_checks():
    base = torch.zeros(8192 + 8, dtype=torch.uint8, device=DEV)
    off, size = to_dev([0]), to_dev([100])
    rep, summ, rec = outputs(1, 4)
    ok = [base.data_ptr(), 8192, off.data_ptr(), size.data_ptr(), 1, 4096, rep.data_ptr(), summ.data_ptr(),
          rec.data_ptr(), 4, 0]
    pcs._call("pcs_manifest_scan_dev", *ok)
    for at, value in ((0, base.data_ptr() + 4), (2, 0), (3, 0), (5, 100), (5, 32), (5, 131072), (6, 0), (7, 0), (8, 0),
                      (8, rec.data_ptr() + 4), (1, 1 << 62)):
        args = list(ok)
        args[at] = value
        with pytest.raises(pcs.PcsError) as e:
            pcs._call("pcs_manifest_scan_dev", *args)
        assert e.value.code == pcs.PCS_ERR_INVALID, (at, value)
    torch.cuda.synchronize()


@pytest.mark.parametrize("align", [64, 65536])
def test_other_alignments(align):
    images = [mr.image([0, 44, 45, 500, 70000, 3], seed=51, align=align), b"", mr.image([10], 52, align)[:30],
              bytes(mr.image([7, 8], 53, align)) + bytes(3 * align)]
    reps, s, recs = scan_dev(images, align=align)
    assert reps["verdict"].tolist() == [mr.CLEAN, mr.EMPTY, mr.CLEAN, mr.TORN_TAIL]


# ---- host form, C++ and CLI -------------------------------------------------------------------------
def unaligned(images):
    """Each image in plain memory at an odd address."""
    keep = []
    for k, img in enumerate(images):
        a = np.zeros(len(img) + 16, np.uint8)
        a[1 + k % 7:1 + k % 7 + len(img)] = np.frombuffer(bytes(img), np.uint8)
        keep.append(a[1 + k % 7:1 + k % 7 + len(img)])
    return keep


def test_host_form_equals_the_device_form():
    images = mixed_images(40, 61)
    for cap in (0, 7, 1 << 16):
        want = mr.scan(images, record_cap=cap)
        reps, s, recs = pcs.manifest_scan_host(unaligned(images), record_cap=cap)
        same(reps, want[0], "host reports")
        same(np.array([s]), np.array([want[1]]), "host summary")
        same(recs, want[2], "host records")
    drep, ds, drecs = pcs.manifest_scan_dev(torch.from_numpy(mr.pack(images)[0]).to(DEV), mr.pack(images)[1],
                                            mr.pack(images)[2], record_cap=1 << 16)
    same(drep, want[0], "dev reports")
    same(drecs, want[2], "dev records")
    reps, s, recs = pcs.manifest_scan_host([], record_cap=4)
    assert len(reps) == 0 and len(recs) == 0 and int(s["first_bad_image"]) == NO and int(s["invalid_image"]) == NO
    reps, s, recs = pcs.manifest_scan_host([b"", b""], align=64)
    assert reps["verdict"].tolist() == [mr.EMPTY] * 2 and int(s["n_records"]) == 0


def test_host_form_in_groups_of_whole_images():
    """More than the 32 MiB staging budget: three groups, first_record and the cap across them."""
    images = []
    for k in range(5):
        b = mr.Builder()
        b.add_random(13 * MIB + 4096 * k + 5, 70 + k)
        logs(b, 3 + k, 71 + k)
        images.append(b.data())
    images.insert(2, b"")
    images[4] = flipped(images[4], 9 * MIB)
    want = mr.scan(images, record_cap=1 << 16)
    assert sum(len(i) for i in images) > 2 * (32 << 20)
    reps, s, recs = pcs.manifest_scan_host(unaligned(images), record_cap=1 << 16)
    same(reps, want[0], "grouped reports")
    same(np.array([s]), np.array([want[1]]), "grouped summary")
    same(recs, want[2], "grouped records")
    inside = int(want[0][3]["first_record"]) + 2
    reps, s, recs = pcs.manifest_scan_host(unaligned(images), record_cap=inside)
    assert int(s["n_listed"]) == inside and int(s["n_records"]) == int(want[1]["n_records"])
    same(recs, want[2][:inside], "grouped records under a cap")


def test_host_fail_inject_is_a_clean_error():
    images = unaligned(mixed_images(3, 81))
    try:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 1)
        with pytest.raises(pcs.PcsError) as e:
            pcs.manifest_scan_host(images)
        assert e.value.code == pcs.PCS_ERR_HIP and "injected failure" in str(e.value)
    finally:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 0)
    reps, s, recs = pcs.manifest_scan_host(images)
    same(reps, mr.scan(mixed_images(3, 81))[0], "after the injected failure")


def test_cpp_scan_manifests():
    exe = os.path.join(HERE, "cpp", "manifest_scan_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "manifest_scan_test ok" in r.stdout, r.stdout + r.stderr


def run_tool(*args):
    return subprocess.run([pcs.TOOL_PATH, *args], capture_output=True, text=True)


def test_cli_one_file_prints_what_the_reference_tool_prints(tmp_path):
    img = mr.image([10, 5000, 0, 300], seed=91)
    cases = {"clean": (img, 0), "failed": (flipped(img, 4096 + 40), 2), "failed-last": (flipped(img, 16384 + 2), 2),
             "cut-header": (img[:16384 + 7], 1), "cut-payload": (img[:4096 + 3000], 1),
             "cut-padding": (img[:16384 + 320 + 5], 0), "no-padding": (img[:16384 + 320], 0),
             "failed-then-cut": (flipped(img, 25)[:12288 + 19], 1), "empty": (b"", 1), "tiny": (bytes(5), 1),
             "zero-slot": (bytes(4096), 2)}
    for name, (data, code) in cases.items():
        path = tmp_path / name
        path.write_bytes(bytes(data))
        out, err, want_code = mr.tool_text(str(path), data)
        assert want_code == code, name
        r = run_tool("--check-manifest", str(path))
        assert (r.returncode, r.stdout, r.stderr) == (want_code, out, err), name


def test_cli_several_files_one_line_each(tmp_path):
    img = mr.image([10, 5000, 0, 300], seed=92)
    files = {"a-clean": img, "b-torn": flipped(img, 16384 + 30), "c-broken": flipped(img, 4096 + 30),
             "d-bad": flipped(img, 9), "e-empty": b"", "f-clean": mr.image([1], 93)}
    paths = {}
    for name, data in files.items():
        paths[name] = str(tmp_path / name)
        (tmp_path / name).write_bytes(bytes(data))
    def run(*names):
        r = run_tool("--check-manifest", *[paths[n] for n in names])
        assert r.stdout == "".join(mr.tool_line(paths[n], files[n]) for n in names), names
        assert r.returncode == mr.tool_exit([files[n] for n in names]), names
        return r.returncode
    assert run("a-clean", "f-clean") == 0
    assert run("a-clean", "e-empty") == 1
    assert run("a-clean", "b-torn", "e-empty") == 3
    assert run("b-torn", "c-broken") == 2
    assert run("f-clean", "d-bad", "e-empty", "a-clean") == 2
    assert run(*files) == 2
    # an unreadable file is reported and the others are still scanned
    r = run_tool("--check-manifest", paths["a-clean"], str(tmp_path / "missing"), paths["f-clean"])
    assert r.returncode == 1 and "Failed to open" in r.stderr and "missing" in r.stderr
    assert r.stdout == mr.tool_line(paths["a-clean"], img) + mr.tool_line(paths["f-clean"], files["f-clean"])
