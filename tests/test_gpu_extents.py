"""Scrub extents on the GPU: pcs_scrub_extents_dev over class arrays built on
the host (no page is hashed, so large n costs megabytes) at the lane, wave,
span and scan-round edges, at unaligned bases and on two streams; composed
with the scrub; the host form across its 32 MiB chunks; the C++ and CLI
layers.  The reference is tests/extent_ref.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
import extent_ref
import scrub_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0x5A5A5A5A5A5A5A5A
OK, BLANK, CORRUPT = extent_ref.OK, extent_ref.BLANK, extent_ref.CORRUPT
BASES = (0, 1, 3, 9)

SIZES = [0, 1, 15, 16, 17,                 # lane edge
         1023, 1024, 1025,                 # wave edge
         4095, 4096, 4097,                 # span edge
         1048575, 1048576, 1048577,        # round edge of the scan block (256 spans)
         2097153]                          # two rounds plus one


def run_words(runs) -> np.ndarray:
    """Reference runs as the (k, 3) u64 words the device writes."""
    w = np.zeros((len(runs), 3), dtype=np.uint64)
    w[:, 0], w[:, 1], w[:, 2] = runs["first_page"], runs["n_pages"], runs["cls"]
    return w


def upload(cls_np, base):
    """The class bytes at byte offset `base` of a larger tensor whose other
    bytes repeat the first / last class: a kernel that read a byte outside the
    range would merge it into a run."""
    n = cls_np.size
    buf = torch.empty(n + 32, dtype=torch.uint8, device=DEV)
    if n:
        buf[:base] = int(cls_np[0])
        buf[base + n:] = int(cls_np[-1])
        buf[base: base + n].copy_(torch.from_numpy(cls_np))
    return buf[base: base + n]


def outputs(cap):
    return (torch.full((12,), 0x1234567, dtype=torch.int64, device=DEV),
            torch.full((max(cap, 1), 3), SENTINEL, dtype=torch.int64, device=DEV))


def check_outputs(summ, runs, full, cap, n):
    """One call's device outputs against the reference at full cap."""
    fs, fruns = full
    want = dict(fs, n_listed=min(fs["n_runs"], cap))
    got = pcs.extent_dict(summ.cpu().tolist())
    assert got == want, (got, want)
    k = want["n_listed"]
    words = runs.cpu().numpy().view(np.uint64)
    assert np.array_equal(words[:k], run_words(fruns[:k]))
    assert (words[k:] == np.uint64(SENTINEL)).all()  # entries at n_listed and beyond are not written
    if k == fs["n_runs"]:
        assert int(words[:k, 1].sum()) == n  # nothing capped: the runs cover every page


def extents_checked(cls_np, cap, base=0, reps=3, full=None):
    """reps calls into garbage-filled outputs: the first compared with the
    reference, the others bit-identical to it."""
    n = cls_np.size
    full = full or extent_ref.extents(cls_np, run_cap=n + 8)
    d = upload(cls_np, base)
    first = None
    for _ in range(reps):
        summ, runs = outputs(cap)
        pcs.scrub_extents_async(d, n, summ, runs if cap else None, cap)
        torch.cuda.synchronize()
        if first is None:
            check_outputs(summ, runs, full, cap, n)
            first = (summ, runs)
        else:
            assert torch.equal(summ, first[0]) and torch.equal(runs, first[1])
    return full


def edge_starts(n, k):
    """Run starts exactly at, one before and one after every multiple of k that fits."""
    m = np.arange(k, n + 2, k, dtype=np.int64)
    b = np.unique(np.concatenate((m - 1, m, m + 1)))
    b = b[(b > 0) & (b < n)]
    step = np.zeros(n, dtype=np.int64)
    step[b] = 1
    return np.array([OK, BLANK, CORRUPT], dtype=np.uint8)[np.cumsum(step) % 3]


def patterns(n):
    """[(name, class array, caps)] for one size."""
    out = [("all_ok", np.full(n, OK, np.uint8), (1024,)),
           ("all_blank", np.full(n, BLANK, np.uint8), (1024,)),
           ("all_corrupt", np.full(n, CORRUPT, np.uint8), (1024,)),
           ("alternating", np.where(np.arange(n) % 2 == 0, OK, BLANK).astype(np.uint8), (0, 1, 7, n, n + 5))]
    for k in (16, 1024, 4096, 1048576):
        if k - 1 < n:
            out.append((f"starts_at_{k}", edge_starts(n, k), (None,)))  # None: every run and five more
    tail = np.full(n, OK, np.uint8)
    tail[n // 2 + 1:] = BLANK
    out.append(("ok_prefix_blank_tail", tail, (1024,)))
    if n >= 2:
        a = np.full(n, OK, np.uint8)
        a[0] = BLANK
        out.append(("hole_at_0", a, (1024,)))
    if n >= 3:
        a = np.full(n, OK, np.uint8)
        a[n - 2] = BLANK
        out.append(("hole_at_n-2", a, (1024,)))
    for edge in (16, 4096, 1048576):
        if n > edge + 6:
            a = np.full(n, OK, np.uint8)
            a[edge - 5: edge + 5] = BLANK  # a hole across a lane / span / round edge
            a[n - 1] = CORRUPT if n % 2 else OK
            out.append((f"hole_across_{edge}", a, (1024,)))
    a = np.full(n, OK, np.uint8)
    a[n // 3: n // 3 + max(1, min(n // 2, 5000))] = 7
    out.append(("foreign_byte_run", a, (1024,)))
    out.append(("geometric", extent_ref.geometric(n, 40.0 if n > 100000 else 5.0, seed=n + 11), (1024, n)))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_extents_match_reference(n):
    for i, (name, cls_np, caps) in enumerate(patterns(n)):
        full = extent_ref.extents(cls_np, run_cap=n + 8)
        if name == "alternating":
            assert full[0]["n_runs"] == n
        # every base at the small sizes and for the random runs; one base per pattern, in turn, at the large ones
        bases = BASES if n <= 4097 or name == "geometric" else (BASES[i % 4],)
        for j, cap in enumerate(caps):
            cap = full[0]["n_runs"] + 5 if cap is None else cap
            for base in (bases if j == 0 or n <= 4097 else bases[:1]):
                try:
                    extents_checked(cls_np, cap, base, reps=3, full=full)
                except AssertionError as e:
                    raise AssertionError(f"n={n} pattern={name} cap={cap} base={base}: {e}") from e


def test_null_run_list_and_python_form():
    cls_np = extent_ref.from_runs([(OK, 5000), (BLANK, 3), (OK, 10), (CORRUPT, 300), (OK, 7), (BLANK, 900)])
    d = upload(cls_np, 1)
    want, wruns = extent_ref.extents(cls_np, run_cap=4)
    s, runs = pcs.scrub_extents(d, run_cap=4)
    assert s == want and runs.dtype == pcs.EXTENT_DTYPE and np.array_equal(run_words(runs), run_words(wruns))
    assert (runs["reserved"] == 0).all()
    s, runs = pcs.scrub_extents(d, run_cap=0)  # NULL list: the emit pass is skipped
    assert s == dict(want, n_listed=0) and len(runs) == 0
    assert (s["written_pages"], s["n_holes"], s["n_hole_pages"], s["first_hole"]) == (5320, 1, 3, 5000)
    with pytest.raises(pcs.PcsError):
        pcs._call("pcs_scrub_extents_dev", d.data_ptr(), d.numel(), 0, 0, 0, 0)  # NULL summary
    with pytest.raises(pcs.PcsError):
        pcs._call("pcs_scrub_extents_dev", d.data_ptr(), d.numel(), torch.empty(12, dtype=torch.int64,
                                                                                 device=DEV).data_ptr(), 0, 4, 0)


def test_two_streams_interleaved():
    work = []
    for cls_np, cap in ((extent_ref.geometric(100003, 6.0, 5), 50000), (edge_starts(8193, 16), 9)):
        work.append((upload(cls_np, 3), cls_np.size, cap, extent_ref.extents(cls_np, run_cap=cls_np.size + 8)))
    streams = [torch.cuda.Stream(device=DEV) for _ in work]
    torch.cuda.synchronize()
    outs = [[outputs(cap) for _ in range(10)] for (d, n, cap, full) in work]
    for rep in range(10):
        for k, (d, n, cap, full) in enumerate(work):
            summ, runs = outs[k][rep]
            pcs.scrub_extents_async(d, n, summ, runs, cap, stream=streams[k])
    torch.cuda.synchronize()
    for k, (d, n, cap, full) in enumerate(work):
        for summ, runs in outs[k]:
            check_outputs(summ, runs, full, cap, n)


@pytest.mark.parametrize("P,n", [(4096, 1003), (65536, 37)])
def test_scrub_then_extents(P, n):
    pg, rows = scrub_ref.build_batch(P, n, near=scrub_ref.near_blank_offsets(P)[:9] if n < 64 else None)
    wcls = scrub_ref.classify(pg, P)[0]
    dpages = torch.from_numpy(pg.reshape(-1)).to(DEV)
    cls, types, s, bad = pcs.pages_scrub(dpages, P, n)
    assert np.array_equal(cls.cpu().numpy(), wcls)
    want, wruns = extent_ref.extents(wcls, run_cap=2048)
    got, runs = pcs.scrub_extents(cls, run_cap=2048)
    assert got == want and np.array_equal(run_words(runs), run_words(wruns))
    assert got["n_blank"] == s["n_blank"] and got["n_holes"] >= 1 and got["last_class"] == BLANK
    if n >= 900:  # one data file inside the batch: a sub-range of the class bytes
        want, wruns = extent_ref.extents(wcls[100:900], run_cap=2048)
        got, runs = pcs.scrub_extents(cls[100:900], run_cap=2048)
        assert got == want and np.array_equal(run_words(runs), run_words(wruns))


def test_host_form_gathers_scattered_pages():
    P, n = 4096, 1200
    pg, rows = scrub_ref.build_batch(P, n, seed=3)
    wcls, wtypes, ws, wbad = scrub_ref.classify(pg, P, corrupt_cap=10)
    pages = [bytearray(pg[i].tobytes()) for i in range(n)]
    for cap in (1024, 3, 0):
        we, wruns = extent_ref.extents(wcls, run_cap=cap)
        before = pcs.counter(pcs.COUNTER_GATHER_CHUNKS)
        s, bad, e, runs = pcs.scrub_extents_host(pages, P, run_cap=cap, corrupt_cap=10)  # NULL cls / type
        assert pcs.counter(pcs.COUNTER_GATHER_CHUNKS) == before + 1
        assert s == ws and np.array_equal(bad, wbad)
        assert e == we and np.array_equal(run_words(runs), run_words(wruns))
    s, bad, e, runs, cls, types = pcs.scrub_extents_host(pages, P, run_cap=5, corrupt_cap=10, per_page=True)
    assert s == ws and e == extent_ref.extents(wcls, run_cap=5)[0]
    assert np.array_equal(cls, wcls) and np.array_equal(types, wtypes)
    s, bad, e, runs = pcs.scrub_extents_ptrs(np.zeros(0, dtype=np.uint64), P, run_cap=3)
    assert s["n_pages"] == 0 and e == extent_ref.extents(np.zeros(0, np.uint8))[0] and len(runs) == 0
    # the scrub's own host form on the same pages is what it was
    cls, types, s, bad = pcs.scrub_pages_host(pages, P, corrupt_cap=10)
    assert s == ws and np.array_equal(bad, wbad) and np.array_equal(cls, wcls) and np.array_equal(types, wtypes)


def test_host_form_merges_across_the_chunk_boundaries():
    """2 x 8192 + 5 contiguous pinned 4 KiB pages: three chunks on the direct
    DMA path.  A corrupt run straddles the first chunk boundary, a blank run
    ends exactly at the second and the last pages are written, so the second
    chunk's blank tail is a hole of the batch."""
    P, n = 4096, 2 * 8192 + 5
    dev = torch.empty(n * P, dtype=torch.uint8, device=DEV)
    pcs.gen_pages(dev, P, n, 0xE87E, 0)
    pv = dev.view(n, P)
    wtypes = np.array(scrub_ref.TYPE_BYTES, dtype=np.uint8)[np.arange(n) % 6]
    pv[:, 8] = torch.from_numpy(wtypes).to(DEV)
    pcs.pages_stamp(dev, P, n)
    bad = np.concatenate([np.arange(8189, 8196), [12000]])
    blank = np.concatenate([[3], np.arange(8100, 8110), np.arange(16300, 16384)])
    pv[torch.from_numpy(blank).to(DEV)] = 0
    pv[torch.from_numpy(bad).to(DEV), 10] ^= 0xFF
    pinned = torch.empty(n * P, dtype=torch.uint8, pin_memory=True)
    pinned.copy_(dev)
    torch.cuda.synchronize()
    wcls = np.full(n, OK, np.uint8)
    wcls[blank], wcls[bad], wtypes[blank] = BLANK, CORRUPT, 0
    ws, wbad = scrub_ref.summarize(wcls, wtypes, corrupt_cap=5)
    ptrs = np.arange(n, dtype=np.uint64) * np.uint64(P) + np.uint64(pinned.data_ptr())
    for cap in (2, 4, 1024):
        we, wruns = extent_ref.extents(wcls, run_cap=cap)
        assert we["n_holes"] == 3 and we["n_hole_pages"] == len(blank) and we["written_pages"] == n
        before = pcs.counter(pcs.COUNTER_DIRECT_DMA_CHUNKS)
        s, lst, e, runs = pcs.scrub_extents_ptrs(ptrs, P, run_cap=cap, corrupt_cap=5)
        assert pcs.counter(pcs.COUNTER_DIRECT_DMA_CHUNKS) == before + 3
        assert s == ws and np.array_equal(lst, wbad)
        assert e == we, (cap, e, we)
        assert np.array_equal(run_words(runs), run_words(wruns))
    # cap 4 lists ok, blank, ok, blank; the corrupt run across the boundary is run 5 of the batch
    assert tuple(int(x) for x in extent_ref.extents(wcls, run_cap=1024)[1][5]) == (8189, 7, CORRUPT, 0)
    # the scrub's own host form on the same pages is what it was
    cls, types, s, lst = pcs.scrub_ptrs(ptrs, P, corrupt_cap=5)
    assert s == ws and np.array_equal(lst, wbad) and np.array_equal(cls, wcls) and np.array_equal(types, wtypes)


def test_cpp_try_scrub_extents():
    exe = os.path.join(HERE, "cpp", "extents_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "extents_test ok" in r.stdout, r.stdout + r.stderr


def test_cli_extents_tells_holes_from_the_tail(tmp_path):
    """300 pages: 280 written (one zeroed page inside them, two adjacent
    flipped pages across the tool's 1 MiB chunk edge) and a blank tail of 20."""
    f = tmp_path / "data.bin"
    env = dict(os.environ, PCS_SCAN_CHUNK_MIB="1")  # 256 pages per file chunk: the tool's own merge runs
    run = lambda *a: subprocess.run([pcs.TOOL_PATH, *a], capture_output=True, text=True, env=env)
    r = run("--gen", str(f), "280", "4096", "0x5EED0003")
    assert r.returncode == 0, r.stderr
    with open(f, "ab") as fh:
        fh.write(bytes(20 * 4096))
    P = 4096
    raw = np.fromfile(f, dtype=np.uint8)
    spare = raw[51 * P: 52 * P].copy()  # a stamped page
    raw[50 * P: 51 * P] = 0
    raw[255 * P + 10] ^= 0xFF
    raw[256 * P + 10] ^= 0xFF
    raw.tofile(f)
    r = run("--extents", str(f))
    assert r.returncode == 2, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith("Scrubbed 300 pages of 4096 bytes: 277 ok, 2 corrupted, 21 blank (")
    assert lines[1].startswith("ok by type: nonleaf_index=")
    assert lines[2:] == ["written extent: pages [0, 280) of 300, blank tail: 20 pages",
                         f"holes: 1 (1 pages), first at offset {50 * P}",
                         f"corrupted extent at offset {255 * P}: 2 pages"]
    # --scrub keeps its output shape and exit code
    r = run("--scrub", str(f))
    assert r.returncode == 2
    lines = r.stdout.splitlines()
    assert "277 ok, 2 corrupted, 21 blank" in lines[0]
    assert lines[2:] == [f"corrupted page at offset {255 * P}", f"corrupted page at offset {256 * P}"]
    # flipped pages repaired: only the hole is left
    raw[255 * P + 10] ^= 0xFF
    raw[256 * P + 10] ^= 0xFF
    raw.tofile(f)
    r = run("--extents", str(f), "4096")
    assert r.returncode == 3, r.stdout + r.stderr
    assert r.stdout.splitlines()[2:] == ["written extent: pages [0, 280) of 300, blank tail: 20 pages",
                                         f"holes: 1 (1 pages), first at offset {50 * P}"]
    # hole refilled with a stamped page: healthy and half-empty
    raw[50 * P: 51 * P] = spare
    raw.tofile(f)
    r = run("--extents", str(f))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert "280 ok, 0 corrupted, 20 blank" in lines[0]
    assert lines[2:] == ["written extent: pages [0, 280) of 300, blank tail: 20 pages", "holes: none"]
