"""Page scrub on the GPU (pcs_pages_scrub_dev / _host, the C++ and CLI forms),
always against tests/scrub_ref.py: classes, type bytes, summary and the capped
ascending corrupt list, on every XXH3 page kernel family (fixed, split,
any-size stride, the unaligned run-time body), with outputs pre-filled with
garbage, repeated calls, two streams, a 256 MiB batch (XCD tile remap,
multi-block reduction) and the host pipeline across its 32 MiB chunk boundary,
at 4 KiB and at page sizes off the 256-byte grid (1000 gathered, 5000 direct
DMA; with the extents form).  The call helpers are in tests/scrub_gpu.py.

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
import extent_ref
import scrub_ref
from scrub_gpu import DEV, garbage, scrub_checked, to_dev

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

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
            assert np.array_equal(cls.cpu().numpy()[:n], wcls) and np.array_equal(ty.cpu().numpy()[:n], wtypes)
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


STAGE_BYTES = 32 << 20  # pcs_capi.cpp kStageBytes: a chunk of the staged pipeline holds STAGE_BYTES // P pages
EDGE_NEAR = (0, 8, 999, 500)


def offgrid_batch(P, seed):
    """STAGE_BYTES // P + 700 stamped pages of every type bucket with blank,
    near-blank (one byte 0x01 at each of EDGE_NEAR) and flipped pages just
    before and just after page e = STAGE_BYTES // P, the first page of the
    second chunk.  -> (pages, e, spare): page e itself is left to the caller,
    spare is a copy of its stamped content."""
    e = STAGE_BYTES // P
    n = e + 700
    rng = np.random.default_rng(seed)
    pg = rng.integers(0, 256, size=(n, P), dtype=np.uint8)
    pg[:, 8] = np.array(scrub_ref.TYPE_BYTES, dtype=np.uint8)[np.arange(n) % 6]
    scrub_ref.stamp(pg, np.arange(n))
    spare = pg[e].copy()
    for side in (e - 6, e + 3):
        for j, off in enumerate(EDGE_NEAR):
            pg[side + j] = 0
            pg[side + j, off] = 1
    pg[[0, e - 2, e + 1, n - 1]] = 0
    pg[[5, e - 1, e + 2, n - 2], 10] ^= 0xFF
    return pg, e, spare


def check_host_forms(ptrs, wcls, wtypes, P, counter, chunks):
    """pcs.scrub_ptrs and pcs.scrub_extents_ptrs against the reference classes
    of the same pages; each call moves `counter` by `chunks`."""
    for cap, run_cap in ((1024, 1024), (7, 5)):
        ws, wbad = scrub_ref.summarize(wcls, wtypes, cap)
        we, wruns = extent_ref.extents(wcls, run_cap=run_cap)
        before = pcs.counter(counter)
        cls, types, s, bad = pcs.scrub_ptrs(ptrs, P, corrupt_cap=cap)
        assert pcs.counter(counter) == before + chunks
        assert s == ws, (s, ws)
        assert np.array_equal(bad, wbad) and np.array_equal(cls, wcls) and np.array_equal(types, wtypes)
        before = pcs.counter(counter)
        s, bad, e, runs, cls, types = pcs.scrub_extents_ptrs(ptrs, P, run_cap=run_cap, corrupt_cap=cap, per_page=True)
        assert pcs.counter(counter) == before + chunks
        assert s == ws and np.array_equal(bad, wbad) and np.array_equal(cls, wcls) and np.array_equal(types, wtypes)
        assert e == we, (e, we)
        for f in ("first_page", "n_pages", "cls"):
            assert np.array_equal(runs[f], wruns[f]), f
    s, bad, e, runs = pcs.scrub_extents_ptrs(ptrs, P, run_cap=1024, corrupt_cap=1024)  # NULL cls / type
    assert s == scrub_ref.summarize(wcls, wtypes, 1024)[0] and e == extent_ref.extents(wcls, run_cap=1024)[0]


def edge_page_variants(pg, e, spare):
    """Page e blank, near-blank at its last byte, and flipped, in turn."""
    pg[e] = 0
    yield "blank"
    pg[e, -1] = 1
    yield "near-blank"
    pg[e] = spare
    pg[e, 10] ^= 0xFF
    yield "flipped"


def edge_reference(pg, P, e, what):
    """Reference classes and types; the batch holds what it should around page e."""
    wcls, wtypes, _, _ = scrub_ref.classify(pg, P)
    assert wcls[e] == (scrub_ref.BLANK if what == "blank" else scrub_ref.CORRUPT), what
    assert wcls[0] == wcls[e - 2] == wcls[e + 1] == wcls[-1] == scrub_ref.BLANK
    assert (wcls[[e - 6, e - 5, e - 4, e - 3, e - 1, e + 2, e + 3, e + 4, e + 5, e + 6]] == scrub_ref.CORRUPT).all()
    assert wcls[e - 7] == wcls[e + 7] == scrub_ref.OK
    return wcls, wtypes


def test_host_forms_gather_off_grid_pages_across_the_chunk_edge():
    """P = 1000 (the any-size body), 33,554 pages per chunk: scattered pages,
    two gathered chunks."""
    P = 1000
    pg, e, spare = offgrid_batch(P, 0x0FF1)
    n = len(pg)
    assert e == 33554 and n == 33554 + 700
    order = np.random.default_rng(7).permutation(n)
    store = np.empty((n, P), dtype=np.uint8)
    ptrs = np.uint64(store.ctypes.data) + order.astype(np.uint64) * np.uint64(P)  # page i lives in row order[i]
    for what in edge_page_variants(pg, e, spare):
        store[order] = pg
        check_host_forms(ptrs, *edge_reference(pg, P, e, what), P, pcs.COUNTER_GATHER_CHUNKS, 2)


def test_host_forms_direct_dma_off_grid_pages_across_the_chunk_edge():
    """P = 5000, 6,710 pages per chunk, one contiguous pinned buffer: two
    chunks on the direct DMA path."""
    P = 5000
    pg, e, spare = offgrid_batch(P, 0x0FF5)
    n = len(pg)
    assert e == 6710
    pinned = torch.empty(n * P, dtype=torch.uint8, pin_memory=True)
    view = pinned.numpy().reshape(n, P)
    ptrs = np.arange(n, dtype=np.uint64) * np.uint64(P) + np.uint64(pinned.data_ptr())
    for what in edge_page_variants(pg, e, spare):
        view[:] = pg
        check_host_forms(ptrs, *edge_reference(pg, P, e, what), P, pcs.COUNTER_DIRECT_DMA_CHUNKS, 2)


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
