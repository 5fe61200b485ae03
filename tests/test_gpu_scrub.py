"""Page scrub on the GPU (pcs_pages_scrub_dev / _host, the C++ and CLI forms),
always against tests/scrub_ref.py: classes, type bytes, summary and the capped
ascending corrupt list, on every XXH3 page kernel family (fixed, split,
any-size stride, the unaligned run-time body), with outputs pre-filled with
garbage, repeated calls, two streams, a 256 MiB batch (XCD tile remap,
multi-block reduction) and the host pipeline across its 32 MiB chunk boundary.

Every batch mixes OK pages of all six type buckets, flipped pages, blank
pages (page 0, page n - 1, a whole 16-page tile), a zero header over a
non-zero body, a zero body under its correct header (OK) and near-blank pages
(one byte 0x01 at each of scrub_ref.near_blank_offsets: CORRUPT, never BLANK).
(65536, 37) cannot hold all of that at once: 16 + 1 blank, 17 near-blank, the
two special pages, a flip and five more OK buckets are 42 pages.  It runs as two
batches of that shape, each with every other ingredient and half of the
near-blank offsets."""
import os
import subprocess

import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
import scrub_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0x5A5A5A5A5A5A5A5A

# fixed; split (8, 16, 64 KiB); any-size stride; plus one multiple of 256 that is no compiled size
SHAPES = [(4096, 1003), (8192, 203), (16384, 101), (65536, 37), (249, 100), (1000, 517), (5000, 333), (2560, 77)]


def batches(P, n):
    """The batch(es) of one shape: [(pages, rows)], see the module docstring."""
    near = scrub_ref.near_blank_offsets(P)
    if n >= 64:
        return [scrub_ref.build_batch(P, n)]
    return [scrub_ref.build_batch(P, n, seed=1, near=near[:9]), scrub_ref.build_batch(P, n, seed=2, near=near[9:])]


def check_batch_on_cpu(pg, rows, P):
    """The test's own batch holds all three classes, all six buckets and its special pages."""
    cls, types, s, bad = scrub_ref.classify(pg, P)
    assert s["n_ok"] and s["n_corrupt"] and s["n_blank"] and all(s["ok_by_type"]), s
    assert (cls[rows["blank"]] == scrub_ref.BLANK).all()
    assert {0, len(pg) - 1} <= set(rows["blank"])
    assert cls[rows["zero_body_ok"]] == scrub_ref.OK
    assert cls[rows["zero_header"]] == scrub_ref.CORRUPT
    assert all(cls[r] == scrub_ref.CORRUPT for r in rows["near_blank"].values())
    assert (cls[rows["flipped"]] == scrub_ref.CORRUPT).all()
    return cls, types, s, bad


def to_dev(pg, offset=0):
    flat = torch.from_numpy(np.ascontiguousarray(pg).reshape(-1))
    buf = torch.empty(flat.numel() + 16, dtype=torch.uint8, device=DEV)
    view = buf[offset: offset + flat.numel()]
    view.copy_(flat)
    return view


def garbage(n, cap):
    return (torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device=DEV)[:n],
            torch.full((max(n, 1),), 0xDD, dtype=torch.uint8, device=DEV)[:n],
            torch.full((12,), 0x1234567, dtype=torch.int64, device=DEV),
            torch.from_numpy(np.full(max(cap, 1), SENTINEL, dtype=np.uint64).view(np.int64)).to(DEV))


def scrub_checked(dpages, P, n, want, cap=1024, reps=3, types=True):
    """reps calls into garbage-filled outputs, each compared with `want`."""
    wcls, wtypes, ws, wbad = want
    for _ in range(reps):
        cls, ty, summ, lst = garbage(n, cap)
        pcs.pages_scrub_async(dpages, P, n, cls, ty if types else False, summ, lst if cap else None, cap)
        torch.cuda.synchronize()
        got = pcs.summary_dict(summ.cpu().tolist())
        ws_cap = dict(ws, n_listed=min(ws["n_corrupt"], cap))
        assert got == ws_cap, (got, ws_cap)
        assert np.array_equal(cls.cpu().numpy(), wcls)
        if types:
            assert np.array_equal(ty.cpu().numpy(), wtypes)
        else:
            assert (ty.cpu().numpy() == 0xDD).all()  # a NULL type array leaves the caller's memory alone
        l = lst.cpu().numpy().view(np.uint64)
        k = got["n_listed"]
        assert np.array_equal(l[:k], wbad[:k])
        assert (l[k:] == SENTINEL).all()  # entries at n_listed and beyond are not written
    return cls


@pytest.mark.parametrize("P,n", SHAPES)
def test_scrub_matches_reference(P, n):
    for pg, rows in batches(P, n):
        want = check_batch_on_cpu(pg, rows, P)
        d = to_dev(pg)
        cls = scrub_checked(d, P, n, want)
        ok, _ = pcs.pages_validate(d, P, n)
        assert np.array_equal(cls.cpu().numpy() == pcs.PAGE_OK, ok.cpu().numpy() == 1)


def test_scrub_on_a_base_offset_by_8_bytes():
    P, n = 4096, 300
    pg, rows = scrub_ref.build_batch(P, n)
    want = check_batch_on_cpu(pg, rows, P)
    d = to_dev(pg, offset=8)
    assert d.data_ptr() % 16 == 8
    cls = scrub_checked(d, P, n, want)
    ok, _ = pcs.pages_validate(d, P, n)
    assert np.array_equal(cls.cpu().numpy() == pcs.PAGE_OK, ok.cpu().numpy() == 1)


def test_python_form_returns_listed_slice():
    P, n = 1000, 517
    pg, rows = scrub_ref.build_batch(P, n)
    wcls, wtypes, ws, wbad = scrub_ref.classify(pg, P, corrupt_cap=7)
    cls, types, s, bad = pcs.pages_scrub(to_dev(pg), P, n, corrupt_cap=7)
    assert s == ws and len(bad) == 7
    assert np.array_equal(bad.cpu().numpy().view(np.uint64), wbad)
    assert np.array_equal(cls.cpu().numpy(), wcls) and np.array_equal(types.cpu().numpy(), wtypes)


def test_corrupt_list_caps():
    P, n = 4096, 1003
    pg, rows = scrub_ref.build_batch(P, n, near=(), flips=12, zero_header=False)
    want = scrub_ref.classify(pg, P)
    assert want[2]["n_corrupt"] == 12
    d = to_dev(pg)
    scrub_checked(d, P, n, want, cap=5)    # the 5 smallest of 12, n_corrupt still 12
    scrub_checked(d, P, n, want, cap=40)   # cap above the count: the tail keeps its sentinel
    scrub_checked(d, P, n, want, cap=12)
    scrub_checked(d, P, n, want, cap=0)    # NULL list
    scrub_checked(d, P, n, want, cap=5, types=False)  # NULL type array: scratch is leased for it
    so = pcs.lib()
    summ = torch.zeros(12, dtype=torch.int64, device=DEV)
    cls = torch.zeros(n, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    assert so.pcs_pages_scrub_dev(d.data_ptr(), P, n, cls.data_ptr(), 0, summ.data_ptr(), 0, 5, s) == pcs.PCS_ERR_INVALID
    assert so.pcs_pages_scrub_dev(d.data_ptr(), 248, n, cls.data_ptr(), 0, summ.data_ptr(), 0, 0, s) == pcs.PCS_ERR_INVALID
    assert so.pcs_pages_scrub_dev(d.data_ptr(), 1 << 32, 1, cls.data_ptr(), 0, summ.data_ptr(), 0, 0, s) == pcs.PCS_ERR_INVALID
    assert so.pcs_pages_scrub_dev(d.data_ptr(), P, n, 0, 0, summ.data_ptr(), 0, 0, s) == pcs.PCS_ERR_INVALID
    assert so.pcs_pages_scrub_dev(d.data_ptr(), P, n, cls.data_ptr(), 0, 0, 0, 0, s) == pcs.PCS_ERR_INVALID
    torch.cuda.synchronize()


def test_empty_and_all_blank_batches():
    empty = torch.empty(16, dtype=torch.uint8, device=DEV)
    want = scrub_ref.classify(np.zeros(0, dtype=np.uint8), 4096)
    scrub_checked(empty, 4096, 0, want, cap=4)
    for P, n in ((4096, 100), (16384, 21), (1000, 50)):
        pg = np.zeros((n, P), dtype=np.uint8)
        want = scrub_ref.classify(pg, P)
        assert want[2]["n_blank"] == n and want[2]["first_corrupt"] == scrub_ref.NO_PAGE
        scrub_checked(to_dev(pg), P, n, want, cap=4)


def test_two_streams_interleaved():
    shapes = ((4096, 1003), (16384, 101))
    work = []
    for P, n in shapes:
        pg, rows = scrub_ref.build_batch(P, n, seed=7)
        work.append((P, n, to_dev(pg), scrub_ref.classify(pg, P, corrupt_cap=9)))
    streams = [torch.cuda.Stream(device=DEV) for _ in work]
    torch.cuda.synchronize()
    outs = [[garbage(n, 9) for _ in range(20)] for (P, n, d, w) in work]
    for rep in range(20):
        for k, (P, n, d, w) in enumerate(work):
            cls, ty, summ, lst = outs[k][rep]
            pcs.pages_scrub_async(d, P, n, cls, ty, summ, lst, 9, stream=streams[k])
    torch.cuda.synchronize()
    for k, (P, n, d, (wcls, wtypes, ws, wbad)) in enumerate(work):
        for cls, ty, summ, lst in outs[k]:
            assert pcs.summary_dict(summ.cpu().tolist()) == ws
            assert np.array_equal(cls.cpu().numpy(), wcls) and np.array_equal(ty.cpu().numpy(), wtypes)
            assert np.array_equal(lst.cpu().numpy().view(np.uint64)[:9], wbad)


def test_256_mib_batch_scattered_classes():
    """65,536 x 4 KiB: the grid covers every tile once (XCD tile remap) and
    the reduction runs over 16 spans."""
    P, n = 4096, 65536
    buf = torch.empty(n * P, dtype=torch.uint8, device=DEV)
    pcs.gen_pages(buf, P, n, 0x5C2B, 0)
    pv = buf.view(n, P)
    idx = torch.arange(n, device=DEV)
    pv[:, 8] = torch.tensor(scrub_ref.TYPE_BYTES, dtype=torch.uint8, device=DEV)[idx % 6]
    pcs.pages_stamp(buf, P, n)
    rng = np.random.default_rng(5)
    blank = np.unique(np.concatenate([rng.choice(n, 900, replace=False), np.arange(40000, 40500), [0, n - 1]]))
    bad = np.setdiff1d(rng.choice(n, 1500, replace=False), blank)
    pv[torch.from_numpy(blank).to(DEV)] = 0
    pv[torch.from_numpy(bad).to(DEV), 10] ^= 0xFF
    torch.cuda.synchronize()
    want = scrub_ref.classify(buf.cpu().numpy(), P, corrupt_cap=1024)
    assert want[2]["n_corrupt"] == len(bad) > 1024 and want[2]["n_blank"] == len(blank)
    cls = scrub_checked(buf, P, n, want, cap=1024, reps=1)
    scrub_checked(buf, P, n, scrub_ref.classify(buf.cpu().numpy(), P, corrupt_cap=4096), cap=4096, reps=1)
    ok, _ = pcs.pages_validate(buf, P, n)
    assert np.array_equal(cls.cpu().numpy() == pcs.PAGE_OK, ok.cpu().numpy() == 1)


def test_host_form_gathers_scattered_pages():
    P, n = 4096, 1200
    pg, rows = scrub_ref.build_batch(P, n, seed=3)
    wcls, wtypes, ws, wbad = scrub_ref.classify(pg, P, corrupt_cap=10)
    pages = [bytearray(pg[i].tobytes()) for i in range(n)]
    before = pcs.counter(pcs.COUNTER_GATHER_CHUNKS)
    cls, types, s, bad = pcs.scrub_pages_host(pages, P, corrupt_cap=10)
    assert pcs.counter(pcs.COUNTER_GATHER_CHUNKS) == before + 1
    assert s == ws and np.array_equal(bad, wbad)
    assert np.array_equal(cls, wcls) and np.array_equal(types, wtypes)
    cls, types, s, bad = pcs.scrub_ptrs(np.zeros(0, dtype=np.uint64), P, corrupt_cap=3)
    assert s["n_pages"] == 0 and s["first_corrupt"] == scrub_ref.NO_PAGE and len(bad) == 0


def test_host_form_direct_dma_across_the_chunk_boundary():
    """9,000 x 4 KiB contiguous pinned pages: two chunks (8,192 + 808) on the
    direct DMA path, corrupt pages in both; the list is global, ascending and
    capped across the boundary, the summary summed."""
    P, n = 4096, 9000
    dev = torch.empty(n * P, dtype=torch.uint8, device=DEV)
    pcs.gen_pages(dev, P, n, 0xD1EC7, 0)
    pv = dev.view(n, P)
    pv[:, 8] = torch.tensor(scrub_ref.TYPE_BYTES, dtype=torch.uint8, device=DEV)[torch.arange(n, device=DEV) % 6]
    pcs.pages_stamp(dev, P, n)
    bad = np.array([5, 100, 4000, 8190, 8191, 8192, 8193, 8500, 8999], dtype=np.int64)
    blank = np.concatenate([np.arange(8180, 8188), np.arange(8200, 8210), [0]])
    pv[torch.from_numpy(blank).to(DEV)] = 0
    pv[torch.from_numpy(bad).to(DEV), 10] ^= 0xFF
    pinned = torch.empty(n * P, dtype=torch.uint8, pin_memory=True)
    pinned.copy_(dev)
    torch.cuda.synchronize()
    ptrs = np.arange(n, dtype=np.uint64) * np.uint64(P) + np.uint64(pinned.data_ptr())
    for cap in (1024, 6, 4, 0):
        wcls, wtypes, ws, wbad = scrub_ref.classify(pinned.numpy(), P, corrupt_cap=cap)
        assert ws["n_corrupt"] == len(bad) and ws["n_blank"] == len(blank)
        before = pcs.counter(pcs.COUNTER_DIRECT_DMA_CHUNKS)
        cls, types, s, lst = pcs.scrub_ptrs(ptrs, P, corrupt_cap=cap)
        assert pcs.counter(pcs.COUNTER_DIRECT_DMA_CHUNKS) == before + 2
        assert s == ws, (cap, s, ws)
        assert np.array_equal(lst, wbad) and np.array_equal(lst, bad[:cap].astype(np.uint64))
        assert np.array_equal(cls, wcls) and np.array_equal(types, wtypes)


def test_cli_scrub_tells_blank_from_corrupted(tmp_path):
    f = tmp_path / "data.bin"
    tool = pcs.TOOL_PATH
    run = lambda *a: subprocess.run([tool, *a], capture_output=True, text=True)
    r = run("--gen", str(f), "64", "4096", "0x5EED0001")
    assert r.returncode == 0, r.stderr
    with open(f, "ab") as fh:
        fh.write(bytes(32 * 4096) + b"tail")  # the fallocated, never-written tail and a partial page
    r = run("--scrub", str(f))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith("Scrubbed 96 pages of 4096 bytes: 64 ok, 0 corrupted, 32 blank (")
    assert lines[0].endswith(" GiB/s incl. file I/O)")
    assert lines[1].startswith("ok by type: nonleaf_index=") and " other=" in lines[1] and len(lines) == 2
    assert sum(int(x.split("=")[1]) for x in lines[1].split()[3:]) == 64
    raw = np.fromfile(f, dtype=np.uint8)
    raw[5 * 4096 + 10] ^= 0xFF
    raw.tofile(f)
    r = run("--scrub", str(f), "4096")
    assert r.returncode == 2
    lines = r.stdout.splitlines()
    assert "63 ok, 1 corrupted, 32 blank" in lines[0] and lines[2:] == ["corrupted page at offset 20480"]
    # --scan is unchanged: it still calls the blank tail corrupted
    r = run("--scan", str(f))
    assert r.returncode == 2 and "96 pages of 4096 bytes: 33 corrupted, first at offset 20480" in r.stdout
    # more than 64 corrupted pages: 64 lines, ascending, then the remainder
    raw[np.arange(70) * 4096 + 10] ^= 0xFF   # pages 0..69 flipped (5 flipped back), 64..69 were blank
    raw.tofile(f)
    want = [i for i in range(70) if i != 5]
    r = run("--scrub", str(f))
    lines = r.stdout.splitlines()
    assert r.returncode == 2 and "1 ok, 69 corrupted, 26 blank" in lines[0]
    assert lines[2:66] == [f"corrupted page at offset {i * 4096}" for i in want[:64]]
    assert lines[66:] == ["... and 5 more corrupted pages"]


def test_cpp_try_scrub_pages():
    exe = os.path.join(HERE, "cpp", "scrub_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scrub_test ok" in r.stdout, r.stdout + r.stderr
