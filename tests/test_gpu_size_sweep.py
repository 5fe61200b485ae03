"""Every page size through the fixed-stride kernels and the scrub.

data_page_size is any uint16_t, and the bodies that hash a page index it by
hand: xxh3_page_any derives NB, kmax, per-lane predicates, an 8-byte load of
the one piece that must not cross the page end, a separately loaded last
stripe and (scrub) an OR over every byte from P; xxh3_page_rt4 / _rt end in a
final block of 1-4 chunks; k_xxh64_stride unrolls 16 ways around a tail of
0-24 bytes; k_xxh64_lds walks 256-byte segments DEPTH at a time with a partial
last one.  A predicate wrong at one residue changes one digest for one family
of sizes, so the lists of tests/size_sweep.py hold every residue
(tests/test_size_sweep_cpu.py asserts what they reach) and each size gets the
same small set of checks, bit-exact against the CPU checker (the reference's
own xxHash where oracle/_ref is built, else the repo's oracle):

check_size        digest into a sentinel-padded output; stamp, the batch and
                  the 16 bytes on either side downloaded and compared with the
                  host image; validate (all 1, first_bad UINT64_MAX); validate
                  with one byte flipped on each of a few pages, at the
                  positions where the body changes what it does
                  (size_sweep.positions) and in the header.
check_scrub_size  a 17-page batch of blank pages, a zero body under its
                  header, one set bit at each such position, one header bit
                  and random stamped pages: classes, types, summary, corrupt
                  list and sentinels against tests/scrub_ref.py at two list
                  caps, then pages_validate against the classes.

A batch is a view at a chosen base alignment into one random pool that lives
on both sides: a stamp is checked by writing the checker's digests into the
host copy and comparing the download with it, so the two stay identical (the
device is repaired from the host when they differ).  A band loops over
its sizes inside one test and reports every failing (P, shift, step).  The
long lists run as several bands (size_sweep.A_BANDS and its kin, cut so that a
case takes no longer than the slowest case of the scrub walk); the CPU module
asserts that the bands, joined, are the lists.
"""
import contextlib

import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
import scrub_ref
import size_sweep as sw
from scrub_gpu import scrub_checked, tuning
from size_sweep import XXH3, XXH64
from test_gpu_batch_edges import (DEV, NONE, SENT64, SENT8, check_flags, check_words, cus, fb_value, flags,
                                  garbage_word, words)
from test_gpu_scrub_walk import COMPILED, body_of
from test_gpu_zero_copy import _zc_delta

pytestmark = pytest.mark.gpu

N = sw.N_PAGES
N64 = 69  # XXH64 and short pages: a 64-page tile of the quad kernels and 5 pages of the next


class Pool:
    """Random bytes on the host and the same bytes on the device."""

    def __init__(self, nbytes, seed=0x512E):
        self.host = sw.host_pool(nbytes, seed)
        self.dev = torch.from_numpy(self.host).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        self.stage = torch.empty(nbytes, dtype=torch.uint8).pin_memory()

    def download(self, a, b):
        """Device bytes [a, b) as a numpy view of the pinned staging buffer (valid until the next download)."""
        st = self.stage[:b - a]
        st.copy_(self.dev[a:b])
        return st.numpy()


@pytest.fixture(scope="module")
def pool():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    p = Pool(sw.POOL_BYTES)
    yield p
    del p
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def scrub_buf():
    """(device buffer the scrub batches are uploaded into, random rows)."""
    dev = torch.zeros(sw.POOL_BYTES, dtype=torch.uint8, device=DEV)
    assert dev.data_ptr() % 16 == 0
    rows = np.random.default_rng(0x5C2B).integers(0, 256, size=(5, 65535), dtype=np.uint8)
    yield dev, rows
    del dev
    torch.cuda.empty_cache()


class Band:
    """Collects the failing (P, shift, step) of a band; only assertion
    failures are collected, an error of the library ends the test at once."""

    def __init__(self):
        self.failed = []
        self.sizes = 0

    @contextlib.contextmanager
    def step(self, P, shift, name):
        try:
            yield
        except AssertionError as e:
            self.failed.append((P, shift, name, str(e)[:60]))

    def failed_at(self, P, shift, name):
        return any(f[:3] == (P, shift, name) for f in self.failed)

    def verdict(self, expect_sizes):
        assert self.sizes == expect_sizes, (self.sizes, expect_sizes)
        assert not self.failed, (f"{len(self.failed)} failing steps against the {sw.checker_name()}, (P, shift, step): "
                                 f"{[f[:3] for f in self.failed]}; first: {self.failed[0]}")


def header_words(rows):
    return np.ascontiguousarray(rows[:, :8]).view("<u8").ravel()


def check_size(band, pool, P, algo, shift, n=N):
    lo, hi = shift, shift + n * P
    a, b = max(0, lo - 16), hi + 16
    assert b <= pool.host.size and b + 48 <= pool.dev.numel()  # inside the pool, 64 bytes of slack behind the batch
    dv, hv = pool.dev[lo:hi], pool.host[lo:hi]
    assert dv.data_ptr() % 16 == shift
    band.sizes += 1
    want = sw.page_digests(hv, P, algo)

    with band.step(P, shift, "digest"):
        out = words(n)
        pcs.pages_digest(dv, P, n, algo, out=out)
        check_words(out, n, want, "digest")

    # the expected image is the host bytes with exactly the n headers replaced, so put them there on the host
    # and compare the batch and the 16 bytes on either side; both sides are identical again afterwards
    pcs.pages_stamp(dv, P, n, algo)
    got = pool.download(a, b)
    hv.reshape(n, P)[:, :8] = want.astype("<u8").view(np.uint8).reshape(n, 8)
    same = np.array_equal(got, pool.host[a:b])
    with band.step(P, shift, "stamp"):
        if not same:
            diff = np.flatnonzero(got != pool.host[a:b])
            assert False, ("stamp: bytes differ at (offset from the batch)", (diff[:8] - (lo - a)).tolist())
    if not same:  # the steps below need correct headers on the device too
        pool.dev[a:b].copy_(torch.from_numpy(pool.host[a:b]))

    def validate(bad, name):
        with band.step(P, shift, name):
            ok, fb = flags(n), garbage_word()
            pcs.pages_validate(dv, P, n, algo, ok=ok, first_bad=fb)
            wok = np.ones(n, dtype=np.uint8)
            wok[bad] = 0
            check_flags(ok, n, wok, name)
            assert fb_value(fb) == (min(bad) if bad else NONE), (name, "first_bad", fb_value(fb))

    validate([], "validate")

    # one structure position per page on pages 1, 2, 3, ..., and a header byte on the last page
    pos = sw.positions(P, algo)
    bad = list(range(1, len(pos) + 1)) + [n - 1]
    assert len(pos) + 1 < n - 1
    at = np.array([p * P + q for p, q in zip(bad, pos + [7])], dtype=np.int64)
    idx = torch.from_numpy(at).to(DEV)
    dv[idx] ^= 0x40
    hv[at] ^= 0x40
    rows = np.ascontiguousarray(hv.reshape(n, P)[bad])
    assert (sw.page_digests(rows, P, algo) != header_words(rows)).all(), (P, "the checker must see every flip")
    validate(bad, "validate flipped")
    dv[idx] ^= 0x40
    hv[at] ^= 0x40


def scrub_pages(P, rand_rows):
    """The 17-page scrub batch of a size and the classes it must get."""
    pg = np.zeros((N, P), dtype=np.uint8)
    pos = sw.xxh3_positions(P)
    walk = list(range(2, 2 + len(pos)))
    pg[walk, pos] = scrub_ref.walk_bit(pos)
    hdr = 2 + len(pos)
    bit = P % 64
    pg[hdr, bit // 8] = 1 << (bit % 8)
    rnd = list(range(hdr + 1, N - 1))
    assert len(rnd) >= 5
    pg[rnd] = np.resize(rand_rows[:, :P], (len(rnd), P))
    pg[rnd, 8] = np.array(scrub_ref.TYPE_BYTES, dtype=np.uint8)[(np.arange(len(rnd)) + P) % len(scrub_ref.TYPE_BYTES)]
    scrub_ref.stamp(pg, [1] + rnd)
    cls = np.full(N, scrub_ref.OK, dtype=np.uint8)
    cls[[0, N - 1]] = scrub_ref.BLANK
    cls[walk + [hdr]] = scrub_ref.CORRUPT
    return pg, cls


def check_scrub_size(band, scrub_buf, P, shift):
    dev, rand_rows = scrub_buf
    assert P >= 249 and shift + N * P + 64 <= dev.numel()
    pg, cls = scrub_pages(P, rand_rows)
    want = scrub_ref.classify(pg, P, corrupt_cap=N)
    assert np.array_equal(want[0], cls), (P, want[0], cls)  # an "always CORRUPT" or "always BLANK" kernel must fail
    d = dev[shift:shift + N * P]
    assert d.data_ptr() % 16 == shift
    d.copy_(torch.from_numpy(pg.reshape(-1)))
    with band.step(P, shift, "scrub cap 17"):
        scrub_checked(d, P, N, want, cap=N, reps=1)
    with band.step(P, shift, "scrub cap 3"):
        scrub_checked(d, P, N, want, cap=3, reps=1)
    with band.step(P, shift, "scrub against validate"):
        ok, _ = pcs.pages_validate(d, P, N)
        assert np.array_equal(ok.cpu().numpy() == 1, cls == pcs.PAGE_OK)


def any_body_band(band, pool, scrub_buf, sizes, scrub=True, n=N):
    for P in sizes:
        assert P % 256 != 0 and P >= 249  # what sends launch_xxh3_pages to body 2
        s = sw.shift(P)
        assert body_of(P, pool.dev.data_ptr() + s) == "any"
        check_size(band, pool, P, XXH3, s, n)
        if scrub:
            check_scrub_size(band, scrub_buf, P, s)


def assert_tuning(values):
    for k, v in values.items():
        assert pcs.get_tuning(k) == v, (k, v, pcs.get_tuning(k))


# ---- the any-size body ---------------------------------------------------------

@pytest.mark.parametrize("band_id", list(sw.A_BANDS))
def test_any_body_exhaustive(pool, scrub_buf, band_id):
    """All of A, NB by NB (size_sweep.A_BANDS: every NB in parts of consecutive sizes)."""
    sizes = sw.A_BANDS[band_id]
    assert {f"NB{sw.NB(P)}" for P in sizes} == {band_id.split("-")[0]}
    band = Band()
    any_body_band(band, pool, scrub_buf, sizes)
    band.verdict(len(sizes))


@pytest.mark.parametrize("band_id", list(sw.B_SPLIT_BANDS))
def test_any_body_deep(pool, scrub_buf, band_id):
    """All of B: the members with r % 8 == j (one NB each) in two parts, 65535 in the last."""
    sizes = sw.B_SPLIT_BANDS[band_id]
    j = int(band_id.split("-")[0])
    assert {sw.NB(P) for P in sizes if P != 65535} == {sw.B_NBS[j]} and (65535 in sizes) == (band_id == "7-1")
    band = Band()
    any_body_band(band, pool, scrub_buf, sizes)
    band.verdict(len(sizes))


NO_NT = {pcs.TUNE_NT_LOADS: 0}
ONE_PER_CU = {pcs.TUNE_XXH3_BLOCKS_PER_CU: 1}
TUNED = ([pytest.param(NO_NT, sizes, False, id=k) for k, sizes in sw.NO_NT_BANDS.items()]
         + [pytest.param(ONE_PER_CU, sizes, True, id=k) for k, sizes in sw.CAPPED_BANDS.items()])


@pytest.fixture(scope="module")
def big_pool():
    """The pool of the capped-grid bands: 16 * CUs + 17 pages of the largest size of A."""
    p = Pool(16 + (16 * cus() + 17) * max(sw.A) + 64, seed=0x512F)
    yield p
    del p
    torch.cuda.empty_cache()


def test_tuned_bands_hold_their_sizes():
    assert sum((p.values[1] for p in TUNED if p.values[2]), []) == sw.A[::7]
    assert sum((p.values[1] for p in TUNED if not p.values[2]), []) == sw.A_BY_NB[0] + sw.A_BY_NB[4]


@pytest.mark.parametrize("tune,sizes,capped", TUNED)
def test_any_body_tuned(pool, big_pool, scrub_buf, tune, sizes, capped):
    saved = {k: pcs.get_tuning(k) for k in tune}
    band = Band()
    with tuning(tune):
        assert_tuning(tune)
        if capped:
            n = 16 * cus() + 17
            assert (n + 15) // 16 > cus() * pcs.get_tuning(pcs.TUNE_XXH3_BLOCKS_PER_CU)  # the grid-stride loop iterates
            any_body_band(band, big_pool, scrub_buf, sizes, scrub=False, n=n)
        else:
            any_body_band(band, pool, scrub_buf, sizes)
    assert_tuning(saved)
    band.verdict(len(sizes))


def test_tuning_is_restored_on_an_exception():
    saved = {k: pcs.get_tuning(k) for k in {**NO_NT, **ONE_PER_CU}}
    with pytest.raises(RuntimeError):
        with tuning({**NO_NT, **ONE_PER_CU}):
            assert_tuning({**NO_NT, **ONE_PER_CU})
            raise RuntimeError("leaves the block early")
    assert_tuning(saved)


# ---- the chunk grid --------------------------------------------------------------

def chunk_body(variant, P):
    if variant == "base8":
        return "rt4"
    if P == 8192 and variant != "no_split":
        return "split"
    if P in COMPILED:
        return "fixed"
    return "rt" if variant == "rt_one_block" else "rt4"


CHUNK_VARIANTS = {"default": ({}, 0), "rt_one_block": ({pcs.TUNE_XXH3_RT_BATCH: 0}, 0),
                  "no_split": ({pcs.TUNE_XXH3_SPLIT_PAGES: 0}, 0), "base8": ({}, 8)}
CHUNK_DEFAULTS = {pcs.TUNE_XXH3_RT_BATCH: 1, pcs.TUNE_XXH3_SPLIT_PAGES: 8192, pcs.TUNE_NT_LOADS: 1,
                  pcs.TUNE_XXH3_BLOCKS_PER_CU: 0}


@pytest.mark.parametrize("variant", list(CHUNK_VARIANTS))
def test_chunk_grid(pool, scrub_buf, variant):
    tune, shift = CHUNK_VARIANTS[variant]
    band = Band()
    with tuning({**CHUNK_DEFAULTS, **tune}):
        assert_tuning({**CHUNK_DEFAULTS, **tune})
        bodies = set()
        for P in sw.C:
            body = body_of(P, pool.dev.data_ptr() + shift)
            assert body == chunk_body(variant, P), (P, body)
            bodies.add(body)
            check_size(band, pool, P, XXH3, shift)
            if P >= 249:
                check_scrub_size(band, scrub_buf, P, shift)
        assert bodies == {"default": {"fixed", "split", "rt4"}, "rt_one_block": {"fixed", "split", "rt"},
                          "no_split": {"fixed", "rt4"}, "base8": {"rt4"}}[variant]
    band.verdict(len(sw.C))


# ---- XXH64 -------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [0, 8])
def test_xxh64_quad(pool, shift):
    """k_xxh64_stride: ns % 16 around the 16-way unroll times the four tails."""
    sizes = [P for P in sw.S if not sw.x64_lds_takes(P, shift)]
    assert len(sizes) == (len(sw.S) if shift == 8 else len(sw.S) - 19)
    assert all(P % 8 == 0 and P >= 40 for P in sizes)  # pages_impl's own condition for the quad kernel
    band = Band()
    for P in sizes:
        check_size(band, pool, P, XXH64, shift, n=N64)
    band.verdict(len(sizes))


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_xxh64_lds(pool, waves):
    """k_xxh64_lds: K % 4 partial last segment times segs % DEPTH for depths 1-4."""
    band = Band()
    for layout in (2, 3, 5, 4):  # depths 1, 2, 3, 4
        tune = {pcs.TUNE_XXH64_WAVES: waves, pcs.TUNE_XXH64_LAYOUT: layout}
        with tuning(tune):
            assert_tuning(tune)
            for P in sw.L:
                assert sw.x64_lds_takes(P, 0)
                check_size(band, pool, P, XXH64, 0, n=N64)
    band.verdict(4 * len(sw.L))


# ---- the descriptor fallback behind the fixed-stride entry points --------------------

def test_short_list_holds_the_fallback_sizes():
    """What pages_impl hands to the descriptor path below 601 bytes is all in H
    (for XXH64 with the quad and LDS kernels' sizes between)."""
    assert set(range(8, 249)) <= set(sw.H[XXH3])
    assert {P for P in range(8, 601) if P < 40 or P % 8 != 0} <= set(sw.H[XXH64])


@pytest.mark.parametrize("algo,part", list(sw.H_BANDS), ids=[f"{('xxh3', 'xxh64')[a]}-{i}" for a, i in sw.H_BANDS])
def test_short_and_off_shape(pool, algo, part):
    sizes = sw.H_BANDS[(algo, part)]
    band = Band()
    for P in sizes:
        check_size(band, pool, P, algo, 0, n=N64)
    band.verdict(len(sizes))


# ---- every length in one descriptor batch ------------------------------------------

@pytest.fixture(scope="module")
def desc_image():
    offs, lens, total = sw.desc_layout()
    image = sw.host_pool(total + 64, seed=0xDE5C)
    edge = np.zeros(total + 65, dtype=np.int64)
    np.add.at(edge, offs.astype(np.int64), 1)
    np.add.at(edge, (offs + lens).astype(np.int64), -1)
    covered = np.cumsum(edge)[:total + 64]
    assert covered.max() == 1
    image[covered == 0] = 0x33  # the gaps, and the slack behind the last page
    return offs, lens, image


DESC_VARIANTS = [pytest.param(XXH3, {}, id="xxh3-default"),
                 pytest.param(XXH3, {pcs.TUNE_XXH3_RT_BATCH: 0}, id="xxh3-rt_one_block"),
                 pytest.param(XXH3, NO_NT, id="xxh3-no_nt"),
                 pytest.param(XXH64, {}, id="xxh64-default"),
                 pytest.param(XXH64, {pcs.TUNE_XXH64_LAYOUT: 5}, id="xxh64-depth3")]


@pytest.mark.parametrize("algo,tune", DESC_VARIANTS)
def test_desc_every_length(desc_image, algo, tune):
    offs, lens, image = desc_image
    n = len(offs)
    has_body = lens >= 8
    want = sw.desc_digests(image, offs, lens, algo)
    assert not want[~has_body].any() and int((~has_body).sum()) == 8
    base = torch.from_numpy(image).to(DEV)
    assert base.data_ptr() % 16 == 0
    d_off = torch.from_numpy(offs.view(np.int64)).to(DEV)
    d_len = torch.from_numpy(lens.view(np.int32)).to(DEV)
    with tuning(tune):
        assert_tuning(tune)
        out = words(n)
        pcs.desc_digest(base, d_off, d_len, n, algo, out=out)
        got = out.cpu().numpy().view(np.uint64)
        wrong = np.flatnonzero(got[:n] != want)
        assert wrong.size == 0, ("digest: (length, offset % 16)", [(int(lens[i]), int(offs[i]) % 16) for i in wrong[:40]])
        assert (got[n:] == SENT64).all()

        pcs.desc_stamp(base, d_off, d_len, n, algo)
        expect = image.copy()
        hb = np.flatnonzero(has_body)
        expect[(offs[hb].astype(np.int64)[:, None] + np.arange(8)).ravel()] = want[hb].astype("<u8").view(np.uint8)
        after = base.cpu().numpy()
        assert np.array_equal(after, expect), ("stamp: bytes differ at", np.flatnonzero(after != expect)[:8].tolist())

        ok, fb = flags(n), garbage_word()
        pcs.desc_validate(base, d_off, d_len, n, algo, ok=ok, first_bad=fb)
        hok = ok.cpu().numpy()
        wrong = np.flatnonzero(hok[:n] != has_body.astype(np.uint8))
        assert wrong.size == 0, ("validate: (length, offset % 16)", [(int(lens[i]), int(offs[i]) % 16) for i in wrong[:40]])
        assert (hok[n:] == SENT8).all()
        assert fb_value(fb) == int(np.flatnonzero(~has_body)[0])
    del base
    torch.cuda.empty_cache()


# ---- registered pages read in place ----------------------------------------------------

@pytest.mark.parametrize("algo", [XXH3, XXH64], ids=["xxh3", "xxh64"])
def test_zero_copy_every_size(algo):
    sizes = [P for P in sw.C if P <= 5120] if algo == XXH3 else sw.L
    assert len(sizes) == (20 if algo == XXH3 else 71)
    rng = np.random.default_rng(0x2C0 + algo)
    failed = []
    for P in sizes:
        with pcs.PagePool(64, P) as pp:
            pp.pages[:] = rng.integers(0, 256, size=(64, P), dtype=np.uint8)
            want = sw.page_digests(pp.pages, P, algo)
            idx = rng.permutation(64)[:40]
            ptrs = pp.ptr(idx)
            body = pp.pages[:, 8:].copy()
            untouched = np.setdiff1d(np.arange(64), idx)
            before = pp.pages[untouched].copy()

            def one_launch(fn, what):
                res, zc, gathered = _zc_delta(fn)
                if (zc, gathered) != (1, 0):
                    failed.append((P, what, "launches", zc, gathered))
                return res

            dig = one_launch(lambda: pcs.digest_ptrs(ptrs, P, algo), "digest")
            if not np.array_equal(dig, want[idx]):
                failed.append((P, "digest"))
            one_launch(lambda: pcs.stamp_ptrs(ptrs, P, algo), "stamp")
            if not (np.array_equal(header_words(pp.pages[idx]), want[idx]) and np.array_equal(pp.pages[:, 8:], body)
                    and np.array_equal(pp.pages[untouched], before)):
                failed.append((P, "stamp"))
                pp.pages[idx, :8] = want[idx].astype("<u8").view(np.uint8).reshape(-1, 8)
            ok, fb = one_launch(lambda: pcs.validate_ptrs(ptrs, P, algo), "validate")
            if not (ok.all() and fb is None):
                failed.append((P, "validate"))
            pos = sw.positions(P, algo)
            listed = np.arange(0, 40, 7)
            rows, cols = idx[listed], np.array([pos[j % len(pos)] for j in range(len(listed))])
            pp.pages[rows, cols] ^= 0x40
            assert (sw.page_digests(pp.pages[rows], P, algo) != header_words(pp.pages[rows])).all()
            ok, fb = one_launch(lambda: pcs.validate_ptrs(ptrs, P, algo), "validate flipped")
            if not (np.array_equal(np.flatnonzero(ok == 0), listed) and fb == 0):
                failed.append((P, "validate flipped"))
            del body, before
    assert not failed, failed
