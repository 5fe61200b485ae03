"""The staged host pipeline (host_batch / host_scrub / pcs_batch in
eloqstore_amd/csrc/pcs_capi.cpp) where its slot ring wraps: calls of more than
three 32 MiB chunks in every mode, pages at and above the slot size, slot
capacities regrown on one thread, threads at once, uneven gather splits and
the asynchronous batch's one-shot staging.

Every page of every case has its own content (tests/host_ref.py), every call
goes through the C ABI, every output element is compared with the CPU oracle
(oracle.pages_digest, scrub_ref, extent_ref), every stamp is checked for its
footprint over the whole pool, and every call must move the counter of the
path it is meant to take by exactly its number of chunks.

Measured on an MI355X: the 48 tests take 20 s together, the slowest (a child
process per gather thread count) 2.6 s each.  The largest single host
allocation is a 336 MiB pool (5,374 x 64 KiB, beside its snapshot of the same
size); the four-thread case holds 4 x (96 + 96) MiB at once.
"""
import contextlib
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
import extent_ref
import scrub_ref
from host_ref import Source, assert_only_headers_changed, chunk_pages, n_chunks, snapshot
from scrub_gpu import tuning

pytestmark = pytest.mark.gpu

MiB = 1 << 20
ALGO_NAME = {pcs.XXH3_64: "xxh3", pcs.XXH64: "xxh64"}
PATH_COUNTERS = (pcs.COUNTER_ZERO_COPY_LAUNCHES, pcs.COUNTER_DIRECT_DMA_CHUNKS, pcs.COUNTER_GATHER_CHUNKS)
STAGED = {pcs.TUNE_ZERO_COPY: 0}  # registered pages take the staged (direct DMA) path, not zero-copy


@pytest.fixture(scope="module", autouse=True)
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert pcs.device_count() >= 1
    yield
    torch.cuda.synchronize()


@contextlib.contextmanager
def counted(counter: int, chunks: int):
    """The block moves `counter` by exactly `chunks` and no other path counter."""
    before = [pcs.counter(c) for c in PATH_COUNTERS]
    yield
    moved = {c: pcs.counter(c) - b for c, b in zip(PATH_COUNTERS, before)}
    assert moved == {c: (chunks if c == counter else 0) for c in PATH_COUNTERS}, (moved, counter, chunks)


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: first difference at index {i}: got {got[i]}, want {want[i]}; "
                             f"{int((got != want).sum())} of {want.size} differ")


def check_digest_stamp_validate(src: Source, algo: int) -> None:
    """digest, stamp (footprint over the whole pool) and validate of src's
    list, each on src's path in n_chunks chunks, all against the oracle."""
    P, n, k = src.P, src.n, n_chunks(src.P, src.n)
    want = src.digests(algo)
    with counted(src.counter, k):
        got = pcs.digest_ptrs(src.ptrs, P, algo)
    assert_same(got, want, "digest")
    before = snapshot(src.pages)
    with counted(src.counter, k):
        pcs.stamp_ptrs(src.ptrs, P, algo)
    assert_only_headers_changed(before, src.pages, src.rows, want)
    del before
    with counted(src.counter, k):
        ok, fb = pcs.validate_ptrs(src.ptrs, P, algo)
    assert_same(ok, np.ones(n, dtype=np.uint8), "validate after stamp")
    assert fb is None


# ---- 1. ring wrap, all modes ---------------------------------------------------

N_OF = {"3c": lambda c: 3 * c, "3c+1": lambda c: 3 * c + 1, "4c+1": lambda c: 4 * c + 1, "7c-1": lambda c: 7 * c - 1}
RING = [(P, nk, pcs.XXH3_64) for P in (4096, 5000, 65536) for nk in ("3c", "3c+1", "4c+1")] + \
       [(65536, "7c-1", pcs.XXH3_64)] + [(4096, nk, pcs.XXH64) for nk in ("3c", "3c+1", "4c+1")]


@pytest.mark.parametrize("kind", ["gather", "direct"])
@pytest.mark.parametrize("P,nk,algo", RING, ids=[f"{P}-{nk}-{ALGO_NAME[a]}" for P, nk, a in RING])
def test_ring_wrap_digest_stamp_validate(P, nk, algo, kind):
    """3, 4, 5 and 7 chunks through the three slots: the fourth chunk onwards
    reuses a slot that the in-loop drain has to empty first.  In the gather
    source every third pool page is left out of the (shuffled) list and must
    come through the stamp untouched."""
    n = N_OF[nk](chunk_pages(P, 1 << 40))
    assert n_chunks(P, n) == {"3c": 3, "3c+1": 4, "4c+1": 5, "7c-1": 7}[nk]
    with tuning(STAGED), Source(kind, P, n, seed=0x51C0 + P + n, hold_out=(kind == "gather")) as src:
        check_digest_stamp_validate(src, algo)


# ---- 2. first_bad over chunks --------------------------------------------------

@pytest.mark.parametrize("poll", [1, 0])
@pytest.mark.parametrize("kind", ["gather", "direct"])
def test_first_bad_over_five_chunks(kind, poll):
    """Verdicts are exact and first_bad is the smallest bad index wherever the
    bad pages sit: in the last (one-page) chunk, on the first page of a reused
    slot, on both sides of a chunk edge, in the first and the last chunk."""
    P = 4096
    c = chunk_pages(P, 1 << 40)
    n = 4 * c + 1
    with tuning({**STAGED, pcs.TUNE_ZC_POLL: poll}), Source(kind, P, n, seed=0xFB00 + poll) as src:
        src.stamp_by_oracle()
        k = n_chunks(P, n)
        with counted(src.counter, k):
            ok, fb = pcs.validate_ptrs(src.ptrs, P)
        assert_same(ok, np.ones(n, dtype=np.uint8), "validate of good pages")
        assert fb is None
        for j, bad in enumerate(([n - 1], [3 * c], [c - 1, c, 3 * c + 5], [0, n - 1])):
            rows = src.rows[bad]
            offs = [8, P - 1, 9 + j, P // 2][: len(bad)]
            src.pages[rows, offs] ^= 0x01
            want = np.ones(n, dtype=np.uint8)
            want[bad] = 0
            with counted(src.counter, k):
                ok, fb = pcs.validate_ptrs(src.ptrs, P)
            assert_same(ok, want, f"verdicts with bad pages {bad}")
            assert fb == min(bad), (fb, bad)
            src.pages[rows, offs] ^= 0x01


# ---- 3. pages at and above the slot size ----------------------------------------

BIG = [(16 * MiB + 256, pcs.XXH3_64), (32 * MiB, pcs.XXH3_64), (32 * MiB + 256, pcs.XXH3_64), (32 * MiB, pcs.XXH64)]


@pytest.mark.parametrize("kind", ["gather", "pinned"])
@pytest.mark.parametrize("P,algo", BIG, ids=[f"{P}-{ALGO_NAME[a]}" for P, a in BIG])
def test_pages_at_and_above_the_slot_size(P, algo, kind):
    """One page per chunk, four chunks: a page of 32 MiB fills the slot
    exactly, a larger one makes the slot grow past 32 MiB."""
    n = 4
    assert chunk_pages(P, n) == 1 and n_chunks(P, n) == 4
    with tuning(STAGED), Source(kind, P, n, seed=0xB16 + (P >> 8), hold_out=(kind == "gather")) as src:
        check_digest_stamp_validate(src, algo)
        src.pages[src.rows[2], P - 1] ^= 0x80
        with counted(src.counter, 4):
            ok, fb = pcs.validate_ptrs(src.ptrs, P, algo)
        assert_same(ok, np.array([1, 1, 0, 1], dtype=np.uint8), "verdicts with the last byte of page 2 flipped")
        assert fb == 2


# ---- 4. scrub and extents through five chunks ------------------------------------

SENTINEL = 0x5A5A5A5A5A5A5A5A
PAD = 16
CLS_FILL, TYPE_FILL = 0xEE, 0xDD


def scrub_raw(ptrs, P, cap, run_cap=None, per_page=True):
    """pcs_pages_scrub_host (run_cap None) or pcs_pages_scrub_extents_host into
    garbage-filled outputs with PAD sentinel elements past n, past the caps and
    so past n_listed; asserts the sentinels and returns
    (cls, types, summary, corrupt list[, extent summary, runs])."""
    ptrs = np.ascontiguousarray(ptrs, dtype=np.uint64)
    n = len(ptrs)
    cls = np.full(n + PAD, CLS_FILL, dtype=np.uint8)
    types = np.full(n + PAD, TYPE_FILL, dtype=np.uint8)
    summary = np.full(12, 0x1234567, dtype=np.uint64)
    corrupt = np.full(cap + PAD, SENTINEL, dtype=np.uint64)
    if run_cap is None:
        assert per_page
        pcs._call("pcs_pages_scrub_host", ptrs.ctypes.data, P, n, cls.ctypes.data, types.ctypes.data,
                  summary.ctypes.data, corrupt.ctypes.data, cap)
    else:
        ext = np.full(12, 0x7654321, dtype=np.uint64)
        runs = np.full((run_cap + PAD) * 3, SENTINEL, dtype=np.uint64)
        pcs._call("pcs_pages_scrub_extents_host", ptrs.ctypes.data, P, n, cls.ctypes.data if per_page else 0,
                  types.ctypes.data if per_page else 0, summary.ctypes.data, corrupt.ctypes.data, cap,
                  ext.ctypes.data, runs.ctypes.data, run_cap)
    s = pcs.summary_dict(summary)
    assert s["n_listed"] <= cap
    assert (corrupt[s["n_listed"]:] == SENTINEL).all(), "corrupt list written past n_listed"
    if per_page:
        assert (cls[n:] == CLS_FILL).all() and (types[n:] == TYPE_FILL).all()
    else:
        assert (cls == CLS_FILL).all() and (types == TYPE_FILL).all()
    out = (cls[:n], types[:n], s, corrupt[: s["n_listed"]])
    if run_cap is None:
        return out
    e = pcs.extent_dict(ext)
    assert e["n_listed"] <= run_cap
    assert (runs[3 * e["n_listed"]:] == SENTINEL).all(), "run list written past n_listed"
    return out + (e, runs[: 3 * e["n_listed"]].view(pcs.EXTENT_DTYPE))


def scrub_layout(layout, c, n):
    """(blank ranges, corrupt pages) by list position for n = 4c + 7 pages."""
    tail = (n - 3, n)
    if layout == "blank_span":
        # one blank run over all of chunks 1 and 2, one page into chunks 0 and 3
        blank = [(c - 1, 3 * c + 1), tail]
        corrupt = [3, c - 2, 3 * c + 1, 3 * c + 2, 3 * c + 9, 3 * c + c // 2, 4 * c - 1, 4 * c, 4 * c + 2]
    else:
        # corrupt pages in every chunk and on both sides of every chunk edge,
        # blank runs inside chunks 1 and 2
        blank = [(c + 2, 2 * c - 1), (2 * c + 1, 3 * c - 2), tail]
        corrupt = [5, c - 1, c, 2 * c - 1, 2 * c, 3 * c - 1, 3 * c, 3 * c + 1, 3 * c + 7, 3 * c + c // 2, 4 * c - 1,
                   4 * c, 4 * c + 2]
    return blank, corrupt


def assert_runs(runs, wruns):
    assert len(runs) == len(wruns)
    for f in ("first_page", "n_pages", "cls"):
        assert_same(runs[f], wruns[f], f"runs.{f}")


@pytest.mark.parametrize("layout", ["blank_span", "corrupt_edges"])
@pytest.mark.parametrize("kind,P", [("gather", 4096), ("direct", 5000)])
def test_scrub_and_extents_through_five_chunks(kind, P, layout):
    """ScrubMerge and ExtentMerge get a fourth and a fifth chunk: classes,
    types, summary, corrupt list, extent summary and runs against scrub_ref and
    extent_ref, with caps above the counts, truncating inside chunk 3's
    contribution, and 0; with and without the per-page arrays."""
    c = chunk_pages(P, 1 << 40)
    n = 4 * c + 7
    k = n_chunks(P, n)
    assert k == 5
    with tuning(STAGED), Source(kind, P, n, seed=0x5C2B + P) as src:
        pg, r = src.pages, src.rows
        pg[:, 8] = np.array(scrub_ref.TYPE_BYTES, dtype=np.uint8)[np.arange(pg.shape[0]) % 6]
        src.stamp_by_oracle()
        blank, corrupt = scrub_layout(layout, c, n)
        for a, b in blank:
            pg[r[a:b]] = 0
        for j, i in enumerate(corrupt):
            pg[r[i], (10, P - 1, 0, 8)[j % 4]] ^= 0xFF
        wcls, wtypes, ws_all, wbad_all = scrub_ref.classify(pg[r], P, corrupt_cap=n)
        assert_same(wbad_all, np.array(sorted(corrupt), dtype=np.uint64), "reference corrupt list")
        assert ws_all["n_blank"] == sum(b - a for a, b in blank)
        we_all, wruns_all = extent_ref.extents(wcls, run_cap=n)
        # caps that cut the lists inside what chunk 3 contributes
        cap_mid = int((wbad_all < 3 * c).sum()) + 2
        assert cap_mid < int((wbad_all < 4 * c).sum())
        run_mid = int((wruns_all["first_page"] < 3 * c).sum()) + 2
        assert run_mid < int((wruns_all["first_page"] < 4 * c).sum())
        for cap, run_cap in ((len(corrupt) + 5, we_all["n_runs"] + 5), (cap_mid, run_mid), (0, 0)):
            ws, wbad = scrub_ref.summarize(wcls, wtypes, cap)
            we, wruns = extent_ref.extents(wcls, run_cap=run_cap)
            with counted(src.counter, k):
                cls, types, s, bad = scrub_raw(src.ptrs, P, cap)
            assert s == ws, (s, ws)
            assert_same(bad, wbad, "corrupt list")
            assert_same(cls, wcls, "classes")
            assert_same(types, wtypes, "types")
            for per_page in (True, False):
                with counted(src.counter, k):
                    cls, types, s, bad, e, runs = scrub_raw(src.ptrs, P, cap, run_cap, per_page)
                assert s == ws and e == we, (s, ws, e, we)
                assert_same(bad, wbad, "corrupt list")
                assert_runs(runs, wruns)
                if per_page:
                    assert_same(cls, wcls, "classes")
                    assert_same(types, wtypes, "types")
            # the Python wrappers, as the other suites call them
            with counted(src.counter, k):
                cls, types, s, bad = pcs.scrub_ptrs(src.ptrs, P, corrupt_cap=cap)
            assert s == ws
            assert_same(bad, wbad, "corrupt list")
            assert_same(cls, wcls, "classes")
            assert_same(types, wtypes, "types")
            for per_page in (True, False):
                with counted(src.counter, k):
                    got = pcs.scrub_extents_ptrs(src.ptrs, P, run_cap=run_cap, corrupt_cap=cap, per_page=per_page)
                assert got[0] == ws and got[2] == we
                assert_same(got[1], wbad, "corrupt list")
                assert_runs(got[3], wruns)
                if per_page:
                    assert_same(got[4], wcls, "classes")
                    assert_same(got[5], wtypes, "types")


# ---- 5. capacity regrow on one thread --------------------------------------------

def check_scrub(src: Source, extents: bool) -> None:
    """A mixed batch (blank, corrupt and stamped pages of every type) through
    pcs.scrub_ptrs or pcs.scrub_extents_ptrs, everything compared."""
    P, n, k = src.P, src.n, n_chunks(src.P, src.n)
    pg, r = src.pages, src.rows
    pg[:, 8] = np.array(scrub_ref.TYPE_BYTES, dtype=np.uint8)[np.arange(pg.shape[0]) % 6]
    src.stamp_by_oracle()
    c = chunk_pages(P, n)
    blank = np.zeros(n, dtype=bool)
    blank[c - 2: c + 1] = True  # over the first chunk edge
    blank[n - 2:] = True
    pg[r[blank]] = 0
    bad = sorted({i for i in (1, c - 3, c + 1, n - 3) if i < n and not blank[i]})
    assert len(bad) >= 2
    pg[r[bad], 10] ^= 0xFF
    wcls, wtypes, ws, wbad = scrub_ref.classify(pg[r], P, corrupt_cap=3)
    assert wbad.tolist() == bad[:3]
    if not extents:
        with counted(src.counter, k):
            cls, types, s, lst = pcs.scrub_ptrs(src.ptrs, P, corrupt_cap=3)
    else:
        we, wruns = extent_ref.extents(wcls, run_cap=6)
        with counted(src.counter, k):
            s, lst, e, runs, cls, types = pcs.scrub_extents_ptrs(src.ptrs, P, run_cap=6, corrupt_cap=3, per_page=True)
        assert e == we, (e, we)
        assert_runs(runs, wruns)
    assert s == ws, (s, ws)
    assert_same(lst, wbad, "corrupt list")
    assert_same(cls, wcls, "classes")
    assert_same(types, wtypes, "types")


def regrow_sequence():
    big = 1 << 40
    steps = [
        ("batch", 65536, 600, "gather"),
        ("batch", 264, 2 * chunk_pages(264, big) + 3, "gather"),   # c = 127100: the result arrays (cap_n) grow
        ("batch", 4096, 3 * chunk_pages(4096, big) + 1, "direct"),  # only the device page buffers grow
        ("scrub", 5000, 2 * chunk_pages(5000, big) + 1, "direct"),
        ("extents", 1000, chunk_pages(1000, big) + 1, "gather"),
        ("batch", 8, 5000, "gather"),
        ("batch", 4096, 1, "gather"),
        ("batch", 65536, 600, "gather"),
    ]
    assert chunk_pages(264, big) == 127100
    for i, (what, P, n, kind) in enumerate(steps):
        with tuning(STAGED), Source(kind, P, n, seed=0x9E0 + i) as src:
            if what == "batch":
                check_digest_stamp_validate(src, pcs.XXH3_64)
                if P == 8:
                    check_digest_stamp_validate(src, pcs.XXH64)
            else:
                check_scrub(src, extents=(what == "extents"))


def run_in_threads(targets):
    """Run the callables in fresh threads at once; re-raise the first failure."""
    errors = [None] * len(targets)

    def body(i):
        try:
            targets[i]()
        except BaseException as e:  # noqa: BLE001 - reported in the caller
            errors[i] = e

    threads = [threading.Thread(target=body, args=(i,)) for i in range(len(targets))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i, e in enumerate(errors):
        if e is not None:
            raise AssertionError(f"thread {i} failed: {e!r}") from e


def test_slot_capacities_regrow_on_one_thread():
    """A fresh thread's staging context starts empty; the shapes come in an
    order in which the pinned page buffers, the device page buffers, the result
    arrays and the scrub / extent buffers each have to grow at a different
    step, on the gather and on the direct path, then small shapes reuse the
    large buffers.  Every result of every step is exact."""
    run_in_threads([regrow_sequence])


# ---- 6. threads at once ----------------------------------------------------------

def test_four_threads_at_once():
    """Four threads, each with its own staging context and its own content,
    stamp, validate and digest four-chunk gather batches at the same time."""
    P = 4096
    n = 3 * chunk_pages(P, 1 << 40) + 1
    k = n_chunks(P, n)
    T = 4
    srcs = [Source("gather", P, n, seed=0x7A00 + t) for t in range(T)]
    try:
        wants = [s.digests() for s in srcs]
        assert len({int(w[0]) for w in wants}) == T
        befores = [snapshot(s.pages) for s in srcs]
        barrier = threading.Barrier(T)
        got = [None] * T

        def work(t):
            s = srcs[t]
            barrier.wait()
            pcs.stamp_ptrs(s.ptrs, P)
            ok, fb = pcs.validate_ptrs(s.ptrs, P)
            got[t] = (ok, fb, pcs.digest_ptrs(s.ptrs, P))

        with tuning(STAGED), counted(pcs.COUNTER_GATHER_CHUNKS, 3 * k * T):
            run_in_threads([lambda t=t: work(t) for t in range(T)])
        for t in range(T):
            ok, fb, dig = got[t]
            assert_only_headers_changed(befores[t], srcs[t].pages, srcs[t].rows, wants[t])
            assert_same(ok, np.ones(n, dtype=np.uint8), f"thread {t} verdicts")
            assert fb is None
            assert_same(dig, wants[t], f"thread {t} digests")
    finally:
        for s in srcs:
            s.close()


# ---- 7. uneven gather splits -----------------------------------------------------

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_gather_child.py")


@pytest.mark.parametrize("threads", [1, 3, 7])
def test_uneven_gather_splits(threads):
    """PCS_GATHER_THREADS is read once per process, so a fresh child process
    gathers with 1, 3 and 7 threads: 6710 and 8176 pages per chunk do not
    divide by 3 (nor 6710 by 7), so the threads' ranges are uneven."""
    c5000, c4104 = chunk_pages(5000, 1 << 40), chunk_pages(4104, 1 << 40)
    assert (c5000, c4104) == (6710, 8176) and c5000 % 3 and c5000 % 7 and c4104 % 3
    env = dict(os.environ, PCS_GATHER_THREADS=str(threads))
    r = subprocess.run([sys.executable, CHILD, f"5000:{3 * c5000 + 1}", f"4104:{c4104 + 5}"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert f"gather threads {threads}" in r.stdout and r.stdout.count("ok ") == 2, r.stdout


# ---- 8. pcs_batch on its staged path ----------------------------------------------

def finish(batch: pcs.Batch, by_poll: bool) -> None:
    if by_poll:
        while not batch.poll():
            pass
    else:
        batch.wait()
        assert batch.poll()


def test_batch_staged_one_object_many_sizes():
    """One pcs_batch stages whole submissions in one shot: its buffers grow to
    40 MB, then serve smaller and differently shaped batches.  DIGEST, STAMP
    (footprint checked after completion) and VALIDATE with one corrupt page at
    every size, completion by poll and by wait in turn."""
    steps = [(4096, 10, "gather"), (5000, 8000, "gather"), (4096, 9000, "direct"), (65536, 3, "gather"),
             (1000, 1, "gather")]
    rnd = random.Random(0xBA7C4)
    b = pcs.Batch()
    turn = 0
    try:
        for i, (P, n, kind) in enumerate(steps):
            with tuning(STAGED), Source(kind, P, n, seed=0xBA00 + i, hold_out=(kind == "gather")) as src:
                for algo in (pcs.XXH3_64, pcs.XXH64):
                    want = src.digests(algo)
                    with counted(src.counter, 1):
                        b.submit_ptrs(b.DIGEST, src.ptrs, P, algo)
                        finish(b, turn % 2 == 0)
                    turn += 1
                    assert_same(np.array(b.result(), dtype=np.uint64), want, f"batch digest {P} x {n}")
                    before = snapshot(src.pages)
                    with counted(src.counter, 1):
                        b.submit_ptrs(b.STAMP, src.ptrs, P, algo)
                        finish(b, turn % 2 == 0)
                    turn += 1
                    assert_only_headers_changed(before, src.pages, src.rows, want)
                    assert_same(np.array(b.result(), dtype=np.uint64), want, f"batch stamp digests {P} x {n}")
                    bad = rnd.randrange(n)
                    src.pages[src.rows[bad], 8 + rnd.randrange(P - 8)] ^= 0x04
                    wok = np.ones(n, dtype=np.uint8)
                    wok[bad] = 0
                    with counted(src.counter, 1):
                        b.submit_ptrs(b.VALIDATE, src.ptrs, P, algo)
                        finish(b, turn % 2 == 0)
                    turn += 1
                    ok, fb = b.result()
                    assert_same(np.array(ok, dtype=np.uint8), wok, f"batch verdicts {P} x {n}")
                    assert fb == bad
    finally:
        b.close()
