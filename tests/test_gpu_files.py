"""Scrub files on the GPU: pcs_scrub_files_dev over class and type arrays
built on the host (no page is hashed, so large n costs megabytes) at the lane,
wave and span edges of the file lengths and boundaries, at the file counts
where the kernels change rounds, with partial covers, empty files, invalid
boundaries, unaligned bases and two streams; cross-checked against the scrub
and extent calls; the host form across its 32 MiB chunks; the C++ and CLI
layers.  The reference is tests/file_ref.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
import extent_ref
import file_ref
import scrub_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0x5A5A5A5A5A5A5A5A
OK, BLANK, CORRUPT = extent_ref.OK, extent_ref.BLANK, extent_ref.CORRUPT
NO = file_ref.NO_PAGE
BASES = (0, 1, 3, 9)

# Where the implementation changes path with the file count: k_files_reduce
# packs 4 files (one wave each) into a block; k_files_plan and k_files_summary
# give each thread of their single block 8 consecutive files, so a wave takes
# 512 files and a round 2048.
FILES_PER_REDUCE_BLOCK = 4
FILES_PER_THREAD = 8
FILES_PER_WAVE = 64 * FILES_PER_THREAD
FILES_PER_ROUND = 256 * FILES_PER_THREAD
FILE_COUNTS = [0, 1, FILES_PER_REDUCE_BLOCK - 1, FILES_PER_REDUCE_BLOCK, FILES_PER_REDUCE_BLOCK + 1,
               FILES_PER_THREAD - 1, FILES_PER_THREAD, FILES_PER_THREAD + 1, 255, 256, 257,
               FILES_PER_WAVE - 1, FILES_PER_WAVE, FILES_PER_WAVE + 1,
               FILES_PER_ROUND - 1, FILES_PER_ROUND, FILES_PER_ROUND + 1, 2 * FILES_PER_ROUND + 1]
EDGE_LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097]  # lane, wave and span edges


def types_for(n, seed=7):
    """Type bytes of every census bucket (and a few foreign ones), at random."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array(scrub_ref.TYPE_BYTES + (77,), dtype=np.uint8), size=n)


def upload(arr, base, pad):
    """arr at byte offset `base` of a larger tensor filled with `pad`: class
    bytes are padded with BLANK, so a kernel that read the byte before page 0
    as a predecessor would lose a blank-run start, and one that read past the
    end would count a blank page."""
    n = arr.size
    buf = torch.full((n + 32,), pad, dtype=torch.uint8, device=DEV)
    if n:
        buf[base: base + n].copy_(torch.from_numpy(arr))
    return buf[base: base + n]


def first_tensor(first):
    return torch.from_numpy(np.ascontiguousarray(first, dtype=np.uint64).view(np.int64).copy()).to(DEV)


def outputs(n_files, cap):
    return (torch.full((n_files + 2, 16), SENTINEL, dtype=torch.int64, device=DEV),
            torch.full((12,), 0x1234567, dtype=torch.int64, device=DEV),
            torch.full((cap + 2,), SENTINEL, dtype=torch.int64, device=DEV))


def check_outputs(out, want, n_files, cap):
    """One call's device outputs against the reference (taken at full cap)."""
    reports, summ, bad = out
    wreps, ws, wbad = want
    ws = dict(ws, n_listed=min(ws["n_bad_files"], cap))
    got = pcs.files_summary_dict(summ.cpu().tolist())
    assert got == ws, (got, ws)
    words = reports.cpu().numpy().view(np.uint64)
    k = ws["n_listed"]
    listed = bad.cpu().numpy().view(np.uint64)
    if ws["invalid_file"] != NO:  # no report and no list entry is written
        assert (words == np.uint64(SENTINEL)).all() and (listed == np.uint64(SENTINEL)).all()
        return
    want_words = file_ref.as_records(wreps).view(np.uint64).reshape(-1, 16)
    if not np.array_equal(words[:n_files], want_words):
        f = int(np.flatnonzero((words[:n_files] != want_words).any(axis=1))[0])
        raise AssertionError(f"file {f}: got {pcs.file_report_dict(words[f])}, want {wreps[f]}")
    assert (words[n_files:] == np.uint64(SENTINEL)).all()  # reports at n_files and beyond are not written
    assert np.array_equal(listed[:k], wbad[:k])
    assert (listed[k:] == np.uint64(SENTINEL)).all()       # entries at n_listed and beyond are not written


def files_checked(cls_np, types_np, first, caps=(1024,), bases=(0,), reps=3, want=None):
    """For every cap and base, `reps` calls into garbage-filled outputs: the
    first compared with the reference, the others bit-identical to it."""
    n, n_files = cls_np.size, len(first) - 1
    want = want or file_ref.files(cls_np, types_np, first, bad_cap=n_files + 8)
    dfirst = first_tensor(first)
    for base in bases:
        dc, dt = upload(cls_np, base, BLANK), upload(types_np, (base * 5 + 2) % 16, 1)
        for cap in caps:
            ref = None
            for _ in range(reps):
                out = outputs(n_files, cap)
                pcs.scrub_files_async(dc, dt, dfirst, n, n_files, out[0], out[1], out[2] if cap else None, cap)
                torch.cuda.synchronize()
                if ref is None:
                    try:
                        check_outputs(out, want, n_files, cap)
                    except AssertionError as e:
                        raise AssertionError(f"n={n} files={n_files} cap={cap} base={base}: {e}") from e
                    ref = out
                else:
                    assert all(torch.equal(a, b) for a, b in zip(out, ref))
    return want


def cut_of(lengths):
    return np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64)))).astype(np.uint64)


def test_file_lengths_at_the_lane_wave_and_span_edges():
    rng = np.random.default_rng(1)
    for k, mean in enumerate((1.5, 6.0, 300.0)):
        lengths = list(EDGE_LENGTHS) + list(rng.permutation(EDGE_LENGTHS))
        first = cut_of(lengths)
        n = int(first[-1])
        cls_np = extent_ref.geometric(n, mean, seed=k + 1)
        files_checked(cls_np, types_for(n, k), first, caps=(1024, 3), bases=BASES)
    for fill in (OK, BLANK, CORRUPT, 7):  # uniform bytes: all clean, all unwritten, all corrupt, a foreign class
        first = cut_of(EDGE_LENGTHS)
        n = int(first[-1])
        reps, s, bad = files_checked(np.full(n, fill, np.uint8), types_for(n), first, bases=(0, 3))
        assert s["n_unwritten_files"] == (len(EDGE_LENGTHS) if fill == BLANK else 1)  # the empty file
        assert s["n_bad_files"] == (len(EDGE_LENGTHS) - 1 if fill == CORRUPT else 0)
        assert s["n_ok"] + s["n_corrupt"] + s["n_blank"] == (0 if fill == 7 else n)  # bytes above 2 are counted nowhere


def test_boundaries_at_and_around_multiples_of_16_and_4096():
    n = 3 * 4096 + 40
    m = np.concatenate((np.arange(16, 200, 16), np.arange(4096, n, 4096)))
    b = np.unique(np.concatenate((m - 1, m, m + 1)))
    first = np.concatenate(([0], b[(b > 0) & (b < n)], [n])).astype(np.uint64)
    for k, mean in enumerate((1.3, 9.0, 700.0)):
        files_checked(extent_ref.geometric(n, mean, seed=40 + k), types_for(n, k), first, caps=(1024,), bases=BASES)
    # every page alternates, so every boundary has a blank page on one side of it
    alt = np.where(np.arange(n) % 2 == 0, BLANK, OK).astype(np.uint8)
    files_checked(alt, types_for(n), first, bases=(0, 9))


def test_runs_that_straddle_a_file_boundary_are_split():
    """A blank run and a corrupt run across a boundary: the blank pages that
    end file f are f's tail, those that start f + 1 are its hole."""
    n = 9000
    cls_np = np.full(n, OK, np.uint8)
    cls_np[95:105] = BLANK       # across 100
    cls_np[198:203] = CORRUPT    # across 200
    cls_np[4090:4100] = BLANK    # across 4096, a span edge inside file 3 only
    cls_np[8990:] = BLANK        # the last file's tail
    first = np.array([0, 100, 200, 300, n], dtype=np.uint64)
    reps, s, bad = files_checked(cls_np, types_for(n), first, caps=(1024, 0, 1), bases=BASES)
    assert (reps[0]["written_pages"], reps[0]["n_holes"], reps[0]["n_blank"]) == (95, 0, 5)
    assert (reps[1]["n_holes"], reps[1]["n_hole_pages"], reps[1]["first_hole"], reps[1]["first_corrupt"]) == (1, 5, 0, 98)
    assert (reps[2]["n_corrupt"], reps[2]["first_corrupt"], reps[2]["n_holes"]) == (3, 0, 0)
    assert (reps[3]["n_holes"], reps[3]["first_hole"], reps[3]["written_pages"]) == (1, 4090 - 300, 8990 - 300)
    assert bad.tolist() == [1, 2, 3] and s["n_corrupt_files"] == 2 and s["n_hole_files"] == 2
    # the same bytes cut one page later: every straddling run now has one page on the left
    files_checked(cls_np, types_for(n), np.array([0, 104, 199, 4097, n], dtype=np.uint64), bases=(0, 1))


@pytest.mark.parametrize("n_files", FILE_COUNTS)
def test_file_counts_at_the_block_and_round_edges(n_files):
    rng = np.random.default_rng(n_files)
    first = cut_of(rng.integers(0, 40, size=n_files))
    n = int(first[-1])
    cls_np = extent_ref.geometric(n, 4.0, seed=n_files + 3)
    want = files_checked(cls_np, types_for(n), first, caps=(0, 1, 1024), bases=(0, 3))
    assert n_files < 5 or want[1]["n_bad_files"] > 1
    if n_files == 0:  # no file: the whole summary is still written; pages in no file are in no report
        cls_np = extent_ref.geometric(5000, 4.0, seed=1)
        reps, s, bad = files_checked(cls_np, types_for(5000), np.array([0], dtype=np.uint64), caps=(0, 4))
        assert s == dict.fromkeys(file_ref.SUMMARY_FIELDS, 0) | {"first_bad_file": NO, "invalid_file": NO}


def test_five_thousand_one_page_files():
    n = 5000
    cls_np = extent_ref.geometric(n, 3.0, seed=5)
    reps, s, bad = files_checked(cls_np, types_for(n), np.arange(n + 1, dtype=np.uint64), caps=(8000, 10),
                                 bases=(0, 9))
    assert s["n_hole_files"] == 0 and s["n_unwritten_files"] == int((cls_np == BLANK).sum())
    assert np.array_equal(bad, np.flatnonzero(cls_np == CORRUPT))


def test_one_large_file_beside_one_page_files():
    big = 2 * 1024 * 1024 + 1
    first = np.array([0, 1, 2, 2 + big, 3 + big], dtype=np.uint64)
    n = int(first[-1])
    cls_np = extent_ref.geometric(n, 40.0, seed=2)
    cls_np[[0, 1, 2, n - 1]] = [BLANK, CORRUPT, BLANK, BLANK]  # the large file starts blank after a corrupt one-page file
    cls_np[2 + big - 4: 2 + big] = [OK, BLANK, BLANK, BLANK]   # and ends blank before a blank one-page file
    reps, s, bad = files_checked(cls_np, types_for(n), first, caps=(4,), bases=(0, 3), reps=2)
    assert reps[2]["n_pages"] == big and reps[2]["first_hole"] == 0 and reps[2]["written_pages"] == big - 3
    assert bad.tolist() == [1, 2] and s["n_unwritten_files"] == 2


def test_partial_cover_and_runs_of_empty_files():
    n = 20000
    cls_np = extent_ref.geometric(n, 7.0, seed=9)
    cls_np[:7] = CORRUPT   # in no file
    cls_np[n - 5:] = CORRUPT
    cls_np[7:12] = BLANK   # the first file starts with a hole whatever page 6 holds
    types_np = types_for(n)
    first = np.array([7, 7, 7, 7, 5000, 9000, 9000, 9000, 9000, 9000, 13000, n - 5, n - 5, n - 5], dtype=np.uint64)
    reps, s, bad = files_checked(cls_np, types_np, first, caps=(1024, 2), bases=BASES)
    assert s["n_pages"] == n - 12 and s["n_files"] == 13
    assert [r["n_pages"] for r in reps] == [0, 0, 0, 4993, 4000, 0, 0, 0, 0, 4000, n - 5 - 13000, 0, 0]
    assert reps[0]["first_corrupt"] == reps[0]["first_hole"] == NO and reps[3]["first_hole"] == 0
    assert s["n_corrupt"] == int((cls_np[7: n - 5] == CORRUPT).sum())
    # a gap between two files, and files that skip most of the batch
    files_checked(cls_np, types_np, np.array([100, 200], dtype=np.uint64), bases=(0, 1))
    reps, s, bad = files_checked(cls_np, types_np, np.array([n, n, n], dtype=np.uint64))
    assert s["n_pages"] == 0 and s["n_unwritten_files"] == 2


def test_invalid_boundaries_are_reported_and_nothing_else_is_written():
    n = 10000
    cls_np, types_np = extent_ref.geometric(n, 5.0, seed=4), types_for(n)
    huge = (1 << 63) + 12345
    for first, inv in (([0, 500, 400, n], 1),                 # a decreasing pair
                       ([0, 500, n + 1], 1),                  # an entry above n_pages
                       ([n + 1, n + 1], 0),
                       ([0, 100, huge, 300, 200, n], 1),      # garbage: the first invalid file is named
                       ([huge, 5, n], 0),
                       (list(range(0, 4400, 2)) + [3, n], 2199)):  # in the second round of the scan
        first = np.array(first, dtype=np.uint64)
        assert file_ref.invalid_file(first, n) == inv
        reps, s, bad = files_checked(cls_np, types_np, first, caps=(8, 0), bases=(0, 3))
        assert reps == [] and s == dict.fromkeys(file_ref.SUMMARY_FIELDS, 0) | {"n_files": len(first) - 1,
                                                                                  "invalid_file": inv}
    # the Python form hands back the summary and no reports
    recs, s, bad = pcs.scrub_files(upload(cls_np, 0, BLANK), upload(types_np, 0, 0), [0, 9, 3, n])
    assert len(recs) == 0 and len(bad) == 0 and s["invalid_file"] == 1
    # NULL arguments
    d, t, f = upload(cls_np, 0, BLANK), upload(types_np, 0, 0), first_tensor([0, n])
    rep, summ, lst = outputs(1, 4)
    for args in ((0, t.data_ptr(), n, f.data_ptr(), 1, rep.data_ptr(), summ.data_ptr(), lst.data_ptr(), 4, 0),
                 (d.data_ptr(), 0, n, f.data_ptr(), 1, rep.data_ptr(), summ.data_ptr(), lst.data_ptr(), 4, 0),
                 (d.data_ptr(), t.data_ptr(), n, 0, 1, rep.data_ptr(), summ.data_ptr(), lst.data_ptr(), 4, 0),
                 (d.data_ptr(), t.data_ptr(), n, f.data_ptr(), 1, 0, summ.data_ptr(), lst.data_ptr(), 4, 0),
                 (d.data_ptr(), t.data_ptr(), n, f.data_ptr(), 1, rep.data_ptr(), 0, lst.data_ptr(), 4, 0),
                 (d.data_ptr(), t.data_ptr(), n, f.data_ptr(), 1, rep.data_ptr(), summ.data_ptr(), 0, 4, 0)):
        with pytest.raises(pcs.PcsError):
            pcs._call("pcs_scrub_files_dev", *args)


def test_two_streams_interleaved():
    work = []
    for n, mean, first, cap in ((100003, 6.0, file_ref.even_cut(100003, 1024), 50), (8193, 2.0, file_ref.even_cut(8193, 16), 9)):
        cls_np, types_np = extent_ref.geometric(n, mean, 5), types_for(n, n)
        work.append((upload(cls_np, 3, BLANK), upload(types_np, 1, 0), first_tensor(first), n, len(first) - 1, cap,
                     file_ref.files(cls_np, types_np, first, bad_cap=len(first))))
    streams = [torch.cuda.Stream(device=DEV) for _ in work]
    torch.cuda.synchronize()
    outs = [[outputs(w[4], w[5]) for _ in range(10)] for w in work]
    for rep in range(10):
        for k, (dc, dt, df, n, n_files, cap, want) in enumerate(work):
            o = outs[k][rep]
            pcs.scrub_files_async(dc, dt, df, n, n_files, o[0], o[1], o[2], cap, stream=streams[k])
    torch.cuda.synchronize()
    for k, (dc, dt, df, n, n_files, cap, want) in enumerate(work):
        for o in outs[k]:
            check_outputs(o, want, n_files, cap)


def merged(s, e):
    """A file report's fields from a scrub summary and an extent summary of the same bytes."""
    return {"n_pages": s["n_pages"], "n_ok": s["n_ok"], "n_corrupt": s["n_corrupt"], "n_blank": s["n_blank"],
            "ok_by_type": s["ok_by_type"], "first_corrupt": s["first_corrupt"], "written_pages": e["written_pages"],
            "n_holes": e["n_holes"], "n_hole_pages": e["n_hole_pages"], "first_hole": e["first_hole"]}


@pytest.mark.parametrize("P,n", [(4096, 1003), (65536, 37)])
def test_reports_equal_the_scrub_and_extent_calls_on_each_sub_range(P, n):
    pg, rows = scrub_ref.build_batch(P, n, near=scrub_ref.near_blank_offsets(P)[:9] if n < 64 else None)
    dpages = torch.from_numpy(pg.reshape(-1)).to(DEV)
    cls, types, s, bad = pcs.pages_scrub(dpages, P, n)
    # one file that covers the batch: the two shipped reductions on the same bytes
    recs, fs, fbad = pcs.scrub_files(cls, types, [0, n])
    e, _ = pcs.scrub_extents(cls, run_cap=0)
    got = pcs.file_report_dict(recs[0])
    assert got == dict(merged(s, e), first_page=0)
    assert fs["n_corrupt"] == s["n_corrupt"] and fs["n_bad_files"] == 1 and fbad.tolist() == [0]
    # a cut of the batch: each file against the existing calls on its pages and class bytes
    first = [0, 0, 1, 17, 33, 48, 48, 100, 500, 900, n] if n > 900 else [0, 1, 16, 16, 20, 36, n]
    recs, fs, fbad = pcs.scrub_files(cls, types, first, bad_cap=3)
    assert recs.dtype == pcs.FILE_REPORT_DTYPE and len(recs) == len(first) - 1
    want = file_ref.files(scrub_ref.classify(pg, P)[0], pg[:, 8].copy(), first, bad_cap=3)
    assert [pcs.file_report_dict(r) for r in recs] == want[0] and fs == want[1] and np.array_equal(fbad, want[2])
    for f, (a, b) in enumerate(zip(first[:-1], first[1:])):
        _, _, s1, _ = pcs.pages_scrub(dpages[a * P: b * P], P, b - a, corrupt_cap=0)
        e1, _ = pcs.scrub_extents(cls[a:b], run_cap=0)
        assert pcs.file_report_dict(recs[f]) == dict(merged(s1, e1), first_page=a), f


def pinned_batch(n, P, blank, bad, seed):
    """n stamped pages in one pinned run with the given blank and flipped pages -> (tensor, ptrs, cls, types)."""
    assert blank.max() < n and bad.max() < n
    dev = torch.empty(n * P, dtype=torch.uint8, device=DEV)
    pcs.gen_pages(dev, P, n, seed, 0)
    pv = dev.view(n, P)
    wtypes = np.array(scrub_ref.TYPE_BYTES, dtype=np.uint8)[np.arange(n) % 6]
    pv[:, 8] = torch.from_numpy(wtypes).to(DEV)
    pcs.pages_stamp(dev, P, n)
    pv[torch.from_numpy(blank).to(DEV)] = 0
    pv[torch.from_numpy(bad).to(DEV), 10] ^= 0xFF
    pinned = torch.empty(n * P, dtype=torch.uint8, pin_memory=True)
    pinned.copy_(dev)
    torch.cuda.synchronize()
    wcls = np.full(n, OK, np.uint8)
    wcls[blank], wcls[bad], wtypes[blank] = BLANK, CORRUPT, 0
    ptrs = np.arange(n, dtype=np.uint64) * np.uint64(P) + np.uint64(pinned.data_ptr())
    return pinned, ptrs, wcls, wtypes


def host_checked(ptrs, P, wcls, wtypes, first, cap, counter, chunks):
    want = file_ref.files(wcls, wtypes, first, bad_cap=cap)
    before = pcs.counter(counter)
    recs, s, bad = pcs.scrub_files_ptrs(ptrs, P, first, bad_cap=cap)
    assert pcs.counter(counter) == before + chunks
    got = [pcs.file_report_dict(r) for r in recs]
    for f, (g, w) in enumerate(zip(got, want[0])):
        assert g == w, (f, g, w)
    assert len(got) == len(want[0]) and s == want[1] and np.array_equal(bad, want[2])
    return want


def test_host_form_merges_files_across_the_chunk_boundaries():
    """2 x 8192 + 5 contiguous pinned 4 KiB pages: three chunks on the direct
    DMA path.  One cut has a boundary exactly on the first chunk edge with empty
    files on it, a corrupt run across that edge, one-page files, and a file
    that straddles the second edge with a blank run across the joint; another
    is one file over all three chunks."""
    P, n = 4096, 2 * 8192 + 5
    bad = np.concatenate([np.arange(8189, 8196), [12000]])
    blank = np.concatenate([[3], np.arange(8100, 8110), np.arange(16378, 16388)])
    pinned, ptrs, wcls, wtypes = pinned_batch(n, P, blank, bad, 0xF11E)
    cut = np.array([0, 1, 2, 5000, 8192, 8192, 8192, 12000, n], dtype=np.uint64)
    reps, s, lst = host_checked(ptrs, P, wcls, wtypes, cut, 1024, pcs.COUNTER_DIRECT_DMA_CHUNKS, 3)
    assert (reps[3]["n_corrupt"], reps[3]["first_corrupt"]) == (3, 8189 - 5000)    # ends on the chunk edge
    assert (reps[6]["n_corrupt"], reps[6]["first_corrupt"]) == (4, 0)
    assert (reps[7]["n_holes"], reps[7]["n_hole_pages"], reps[7]["first_hole"]) == (1, 10, 16378 - 12000)  # one hole across the joint
    assert reps[7]["written_pages"] == n - 12000 and lst.tolist() == [2, 3, 6, 7]
    host_checked(ptrs, P, wcls, wtypes, cut, 2, pcs.COUNTER_DIRECT_DMA_CHUNKS, 3)
    host_checked(ptrs, P, wcls, wtypes, cut, 0, pcs.COUNTER_DIRECT_DMA_CHUNKS, 3)
    reps, s, lst = host_checked(ptrs, P, wcls, wtypes, np.array([0, n], dtype=np.uint64), 4,
                                pcs.COUNTER_DIRECT_DMA_CHUNKS, 3)                 # one file over three chunks
    assert (reps[0]["n_holes"], reps[0]["n_hole_pages"], reps[0]["first_hole"]) == (3, 21, 3)
    # the second chunk's blank tail stays a tail when the file ends with it
    host_checked(ptrs, P, wcls, wtypes, np.array([0, 16384, 16384, 16387, n], dtype=np.uint64), 4,
                 pcs.COUNTER_DIRECT_DMA_CHUNKS, 3)
    host_checked(ptrs, P, wcls, wtypes, file_ref.even_cut(n, 1000), 1024, pcs.COUNTER_DIRECT_DMA_CHUNKS, 3)
    # boundaries that do not cover the batch, or decrease, are refused on the host
    for first in ([1, n], [0, n - 1], [0, 9000, 8000, n], [0, n + 1]):
        with pytest.raises(pcs.PcsError) as ei:
            pcs.scrub_files_ptrs(ptrs, P, first)
        assert ei.value.code == pcs.PCS_ERR_INVALID
    # the scrub's own host form on the same pages is what it was
    cls, types, s, lst = pcs.scrub_ptrs(ptrs, P, corrupt_cap=5)
    assert np.array_equal(cls, wcls) and np.array_equal(types, wtypes) and s["n_corrupt"] == len(bad)


def test_host_form_gathers_scattered_pages():
    P, n = 4096, 1200
    pg, rows = scrub_ref.build_batch(P, n, seed=3)
    wcls, wtypes, ws, wbad = scrub_ref.classify(pg, P)
    pages = [bytearray(pg[i].tobytes()) for i in range(n)]
    arr, _keep = pcs._page_ptrs(pages)
    ptrs = np.array([arr[i] or 0 for i in range(n)], dtype=np.uint64)
    for first, cap in ((file_ref.even_cut(n, 100), 1024), ([0, 0, 1, 33, 40, 40, 47, 600, n, n], 2), ([0, n], 0)):
        host_checked(ptrs, P, wcls, wtypes, np.array(first, dtype=np.uint64), cap, pcs.COUNTER_GATHER_CHUNKS, 1)
    recs, s, bad = pcs.scrub_files_host(pages, P, [0, 600, n])
    assert s["n_corrupt"] == ws["n_corrupt"] and s["n_blank"] == ws["n_blank"] and s["n_files"] == 2
    # no page, files or not
    recs, s, bad = pcs.scrub_files_ptrs(np.zeros(0, dtype=np.uint64), P, [0, 0, 0])
    assert s["n_files"] == 2 and s["n_unwritten_files"] == 2 and s["n_pages"] == 0 and recs["first_hole"].tolist() == [NO, NO]
    recs, s, bad = pcs.scrub_files_ptrs(np.zeros(0, dtype=np.uint64), P, [0])
    assert len(recs) == 0 and s["n_files"] == 0 and s["first_bad_file"] == NO


def test_cpp_try_scrub_files():
    exe = os.path.join(HERE, "cpp", "files_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "files_test ok" in r.stdout, r.stdout + r.stderr


def test_cli_scrub_files_names_the_damaged_files(tmp_path):
    """Six files through 1 MiB tool chunks (256 pages): clean and full, a
    blank tail, a hole, two flipped pages across the tool's chunk edge, all
    blank, and one of 600 pages that spans three chunks."""
    P = 4096
    env = dict(os.environ, PCS_SCAN_CHUNK_MIB="1")
    run = lambda *a: subprocess.run([pcs.TOOL_PATH, *a], capture_output=True, text=True, env=env)
    names = ["clean", "tail", "hole", "flipped", "blank", "long"]
    sizes = [100, 100, 50, 60, 10, 600]
    paths = [str(tmp_path / f"{k}.bin") for k in names]
    for k, (p, sz) in enumerate(zip(paths, sizes)):
        r = run("--gen", p, str(sz), "4096", hex(0x5EED0100 + k))
        assert r.returncode == 0, r.stderr
    raw = {k: np.fromfile(p, dtype=np.uint8) for k, p in zip(names, paths)}
    raw["tail"][80 * P:] = 0
    spare = raw["hole"][21 * P: 22 * P].copy()
    raw["hole"][20 * P: 21 * P] = 0
    # files are packed back to back: "flipped" starts at batch page 250, so its pages 5 and 6 are 255 and 256
    assert sum(sizes[:3]) == 250
    raw["flipped"][5 * P + 10] ^= 0xFF
    raw["flipped"][6 * P + 10] ^= 0xFF
    raw["blank"][:] = 0
    raw["long"][590 * P:] = 0
    for k, p in zip(names, paths):
        raw[k].tofile(p)
    r = run("--scrub-files", "4096", *paths)
    assert r.returncode == 2, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[:-1] == [
        f"{paths[2]}: 50 pages, written [0, 50), 49 ok, 0 corrupted, 1 blank, 1 holes (1 pages), first hole at offset {20 * P}",
        f"{paths[3]}: 60 pages, written [0, 60), 58 ok, 2 corrupted, 0 blank, 0 holes (0 pages), first corrupted page at offset {5 * P}",
    ], r.stdout
    assert lines[-1].startswith("Scrubbed 6 files, 920 pages of 4096 bytes: 3 clean, 1 corrupted, 1 with holes, 1 unwritten (")
    assert "GiB/s incl. file I/O" in lines[-1]
    # flipped pages repaired: only the hole is left
    raw["flipped"][5 * P + 10] ^= 0xFF
    raw["flipped"][6 * P + 10] ^= 0xFF
    raw["flipped"].tofile(paths[3])
    r = run("--scrub-files", "4096", *paths)
    assert r.returncode == 3, r.stdout + r.stderr
    assert len(r.stdout.splitlines()) == 2 and r.stdout.startswith(paths[2] + ": 50 pages")
    # hole refilled with a stamped page: every file is healthy; a file with no whole page is skipped with a warning
    raw["hole"][20 * P: 21 * P] = spare
    raw["hole"].tofile(paths[2])
    small = tmp_path / "small.bin"
    small.write_bytes(b"\1" * 100)
    r = run("--scrub-files", "4096", *paths[:3], str(small), *paths[3:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "holds no whole page" in r.stderr and str(small) in r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith(
        "Scrubbed 6 files, 920 pages of 4096 bytes: 5 clean, 0 corrupted, 0 with holes, 1 unwritten, 1 skipped (")
    # --scrub on one of the files keeps its output shape
    r = run("--scrub", paths[1])
    assert r.returncode == 0 and "80 ok, 0 corrupted, 20 blank" in r.stdout.splitlines()[0]
