"""Batch counts at the edges of the kernels' count-dependent control flow.

The parity suite covers page content (every XXH3 length class, odd sizes,
unaligned bases); this module covers how many pages or ranges a call carries:
the xcd_tile remap with a dispatch-order tail, every xcd_tile_eighths
remainder, capped grids whose grid-stride loops really loop, the zero-copy
list kernels looping, the scrub scan beyond one round of 256 spans, manifests
beyond one fold batch, raw ranges beyond one trip of the lane kernels, and the
verdict compare on all 64 header bits.

Every call goes through eloqstore_amd and the C ABI; the checker is the CPU
oracle (tests/scrub_ref.py for scrub).  Everything is bit-exact.  Every output
array is allocated PAD elements longer than the batch and pre-filled with a
sentinel, which must survive past element n; first_bad is pre-filled with
garbage.  Each test first asserts that its batch crosses the threshold it is
about on this device, so a part with more CUs makes the test larger, never
trivial.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
import oracle
import scrub_ref
from stream_ref import stream_fold
from workload import mixed_layout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TILE_PAGES = 16        # XXH3 page kernels: 256 threads, one 16-lane group per page (pcs_kernels.hip k_xxh3_fixed)
X64_TILE_PAGES = 64    # XXH64 page kernels: 256 threads, one quad per page (k_xxh64_lds with 4 waves, k_xxh64_stride)
REMAP_ROUND = 8 * 64   # xcd_tile<64>: 8 XCDs x chunks of 64 tiles; tiles past the last whole round keep their index
SCRUB_SPAN = 4096      # kScrubSpan: pages per k_scrub_count / k_scrub_list block
SCAN_ROUND = 256       # k_scrub_scan: spans scanned per round of its one 256-thread block
FOLD = 64              # k_manifest_fold: chunk digests folded per batch of one wave
BLOCKS_PER_CU = 8      # kBlocksPerCu and page_grid's automatic cap for pages above 16 KiB
MANIFEST_CHUNK = 1 << 20        # kManifestChunk (kCheckSumBatchSize)
SUMS16_TILES_PER_CHUNK = 16     # k_manifest_sums16 grid.x: 1024 blocks of 1 KiB / (16 groups x 4 blocks)
GENERIC_LANES_PER_CU = 256 * BLOCKS_PER_CU  # k_generic_desc: grid_for(n, 256, kBlocksPerCu), one lane per range

NONE = (1 << 64) - 1
SENT64 = 0x5A5A5A5A5A5A5A5A
SENT8 = 0xEE
PAD = 16
MiB = 1 << 20


def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- sentinel-padded outputs -------------------------------------------------

def words(n):
    return torch.full((n + PAD,), SENT64, dtype=torch.int64, device=DEV)


def flags(n, fill=SENT8):
    return torch.full((n + PAD,), fill, dtype=torch.uint8, device=DEV)


def garbage_word():
    return torch.full((1,), 0x1234, dtype=torch.int64, device=DEV)


def fb_value(fb):
    return int(fb.cpu().numpy().view(np.uint64)[0])


def check_words(out, n, want, what=""):
    got = out.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:n], want), (what, np.flatnonzero(got[:n] != want)[:8])
    assert (got[n:] == SENT64).all(), (what, "write past out[n]")


def check_flags(ok, n, want, what="", fill=SENT8):
    got = ok.cpu().numpy()
    assert np.array_equal(got[:n], want), (what, np.flatnonzero(got[:n] != want)[:8])
    assert (got[n:] == fill).all(), (what, "write past ok[n]")


@contextlib.contextmanager
def tuning(values):
    """pcs_set_tuning for the block, every key restored on every exit path."""
    saved = {k: pcs.get_tuning(k) for k in values}
    try:
        for k, v in values.items():
            pcs.set_tuning(k, v)
        yield
    finally:
        for k, v in saved.items():
            pcs.set_tuning(k, v)


# ---- batches -------------------------------------------------------------------

def fill(buf, P, n, seed):
    """Synthetic bytes from the device generator; a page size off the 8-byte
    grid is filled word by word (the bytes are arbitrary, only the oracle's
    view of them counts)."""
    if P % 8 == 0:
        pcs.gen_pages(buf, P, n, seed, 0)
    else:
        nb = n * P
        pcs.gen_pages(buf, 8, nb // 8, seed, 0)
        if nb % 8:
            buf[nb - nb % 8:nb] = 0xA7


def page_buffer(P, n, seed, shift=0):
    whole = torch.empty(shift + n * P + 32, dtype=torch.uint8, device=DEV)
    buf = whole[shift:shift + n * P]
    assert buf.data_ptr() % 16 == shift % 16
    fill(buf, P, n, seed)
    return buf


def headers(host, n, P):
    return np.ascontiguousarray(host.reshape(n, P)[:, :8]).view("<u8").ravel()


def seam_pages(n, ppb):
    """Page 0, page n - 1, and the first and last page of tiles 63, 64, 511,
    512 and the last tile (tiles of ppb pages), where they exist."""
    last = (n - 1) // ppb
    pages = {0, n - 1}
    for t in (63, 64, REMAP_ROUND - 1, REMAP_ROUND, last):
        if t * ppb < n:
            pages |= {t * ppb, min(t * ppb + ppb - 1, n - 1)}
    return sorted(pages)


def flip(buf, byte_pos):
    buf[torch.as_tensor(np.asarray(byte_pos, dtype=np.int64), device=DEV)] ^= 0x40


def oracle_says_bad(buf, offs, lens, algo):
    """The oracle's verdict on the listed (just corrupted) pages: all must fail."""
    for o, L in zip(offs, lens):
        page = buf[int(o):int(o) + int(L)].cpu().numpy()
        assert int(oracle.pages_digest(page, int(L), algo)[0]) != int(page[:8].copy().view("<u8")[0])


def validate_pages(buf, P, n, algo, bad, what):
    ok, fb = flags(n), garbage_word()
    pcs.pages_validate(buf, P, n, algo, ok=ok, first_bad=fb)
    want = np.ones(n, dtype=np.uint8)
    want[bad] = 0
    check_flags(ok, n, want, what)
    assert fb_value(fb) == (min(bad) if len(bad) else NONE), (what, fb_value(fb))


def check_pages(P, n, algo, ppb, seed, shift=0, kernel_stamp=True):
    """Digest, stamp (every header against the oracle), validate (all ok),
    validate with the seam pages corrupt (exactly those fail, first_bad 0) and
    with page n - 1 alone corrupt.  kernel_stamp=False writes the oracle's
    digests into the headers instead (digest and validate only)."""
    buf = page_buffer(P, n, seed, shift)
    host = buf.cpu().numpy().copy()
    want = oracle.pages_digest(host, P, algo)
    out = words(n)
    pcs.pages_digest(buf, P, n, algo, out=out)
    check_words(out, n, want, "digest")
    if kernel_stamp:
        pcs.pages_stamp(buf, P, n, algo)
        host.reshape(n, P)[:, :8] = want.astype("<u8").view(np.uint8).reshape(n, 8)
        after = buf.cpu().numpy()
        assert np.array_equal(headers(after, n, P), want), "stamp"
        assert np.array_equal(after, host), "stamp changed bytes past a header"
    else:
        assert P % 8 == 0 and shift % 8 == 0
        buf.view(torch.int64).view(n, P // 8)[:, 0] = torch.from_numpy(want.view(np.int64)).to(DEV)
    validate_pages(buf, P, n, algo, [], "validate")
    seams = seam_pages(n, ppb)
    pos = [p * P + 10 for p in seams]
    flip(buf, pos)
    oracle_says_bad(buf, [p * P for p in seams], [P] * len(seams), algo)
    validate_pages(buf, P, n, algo, seams, "seams")
    flip(buf, pos)
    flip(buf, [(n - 1) * P + 10])
    validate_pages(buf, P, n, algo, [n - 1], "last page")
    flip(buf, [(n - 1) * P + 10])
    return buf


def desc_buffer(offs, lens, seed):
    n = len(offs)
    total = int((offs + lens.astype(np.uint64)).max())
    base = torch.empty(total + 64, dtype=torch.uint8, device=DEV)
    base.fill_(0x33)  # gaps between pages
    d_off = torch.from_numpy(offs.view(np.int64)).to(DEV)
    d_len = torch.from_numpy(lens.view(np.int32)).to(DEV)
    pcs.gen_desc(base, d_off, d_len, n, seed, 0)
    return base, d_off, d_len


def validate_desc(base, d_off, d_len, n, algo, bad, what):
    ok, fb = flags(n), garbage_word()
    pcs.desc_validate(base, d_off, d_len, n, algo, ok=ok, first_bad=fb)
    want = np.ones(n, dtype=np.uint8)
    want[bad] = 0
    check_flags(ok, n, want, what)
    assert fb_value(fb) == (min(bad) if len(bad) else NONE), (what, fb_value(fb))


def check_desc(offs, lens, algo, ppb, seed):
    """check_pages on the descriptor entry points (every page >= 16 bytes)."""
    n = len(offs)
    assert int(lens.min()) >= 16
    base, d_off, d_len = desc_buffer(offs, lens, seed)
    host = base.cpu().numpy().copy()
    want = oracle.desc_digest(host, offs, lens, algo)
    out = words(n)
    pcs.desc_digest(base, d_off, d_len, n, algo, out=out)
    check_words(out, n, want, "digest")
    pcs.desc_stamp(base, d_off, d_len, n, algo)
    hdr = (offs.astype(np.int64)[:, None] + np.arange(8)).ravel()
    host[hdr] = want.astype("<u8").view(np.uint8)
    assert np.array_equal(base.cpu().numpy(), host), "stamp"
    validate_desc(base, d_off, d_len, n, algo, [], "validate")
    seams = seam_pages(n, ppb)
    pos = [int(offs[p]) + 10 for p in seams]
    flip(base, pos)
    oracle_says_bad(base, offs[seams], lens[seams], algo)
    validate_desc(base, d_off, d_len, n, algo, seams, "seams")
    flip(base, pos)
    flip(base, [int(offs[n - 1]) + 10])
    validate_desc(base, d_off, d_len, n, algo, [n - 1], "last page")


def uniform_desc(P, n, pitch=None):
    pitch = P if pitch is None else pitch
    return np.arange(n, dtype=np.uint64) * np.uint64(pitch), np.full(n, P, dtype=np.uint32)


# ---- scrub -----------------------------------------------------------------------

def scrub_batch(P, n, seed, blank, corrupt, shift=0):
    """n stamped pages on the device with type bytes cycling
    scrub_ref.TYPE_BYTES, the `blank` pages zeroed, then byte 10 of the
    `corrupt` pages flipped.  -> (device pages, reference classes, types)."""
    buf = page_buffer(P, n, seed, shift)
    cyc = torch.tensor(scrub_ref.TYPE_BYTES, dtype=torch.uint8, device=DEV)
    rows = buf.view(n, P)
    rows[:, 8] = cyc[torch.arange(n, device=DEV) % len(scrub_ref.TYPE_BYTES)]
    pcs.pages_stamp(buf, P, n)
    rows[torch.as_tensor(np.asarray(blank, dtype=np.int64), device=DEV)] = 0
    flip(buf, np.asarray(corrupt, dtype=np.int64) * P + 10)
    wcls, wtypes, _, _ = scrub_ref.classify(buf.cpu().numpy(), P)
    return buf, wcls, wtypes


def check_scrub(buf, P, n, wcls, wtypes, caps):
    """pcs_pages_scrub_dev on the first n pages of buf against the reference
    classes, for every list cap: classes, types, the whole summary, the list,
    and the sentinels past n / past n_listed."""
    wcls, wtypes = wcls[:n], wtypes[:n]
    for cap in caps:
        ws, wbad = scrub_ref.summarize(wcls, wtypes, cap)
        cls, ty = flags(n), flags(n, 0xDD)
        summ = torch.full((12,), 0x1234567, dtype=torch.int64, device=DEV)
        lst = words(cap)
        pcs.pages_scrub_async(buf, P, n, cls, ty, summ, lst, cap)
        torch.cuda.synchronize()
        assert pcs.summary_dict(summ.cpu().tolist()) == ws, (cap, pcs.summary_dict(summ.cpu().tolist()), ws)
        check_flags(cls, n, wcls, ("class", cap))
        check_flags(ty, n, wtypes, ("type", cap), fill=0xDD)
        got = lst.cpu().numpy().view(np.uint64)
        k = ws["n_listed"]
        assert np.array_equal(got[:k], wbad), (cap, np.flatnonzero(got[:k] != wbad)[:8])
        assert (got[k:] == SENT64).all(), (cap, "list written past n_listed")


# ---- 1. xcd_tile seams -----------------------------------------------------------

def remap_n(tiles, ppb):
    """A batch of `tiles` tiles whose last tile is partial (a single-page tile
    cannot be)."""
    n = tiles * ppb - 5 if ppb > 5 else tiles * ppb
    assert (n + ppb - 1) // ppb == tiles
    return n


def assert_remap_case(tiles):
    """511 is the last count without a remap, 512 the first (no tail), 513 and
    1101 have a dispatch-order tail."""
    assert tiles in (REMAP_ROUND - 1, REMAP_ROUND) or (tiles > REMAP_ROUND and tiles % REMAP_ROUND != 0)


@pytest.mark.parametrize("tiles", [511, 512, 513, 1101])
@pytest.mark.parametrize("P", [256, 4096])
def test_remap_fixed(P, tiles):
    assert_remap_case(tiles)
    check_pages(P, remap_n(tiles, TILE_PAGES), pcs.XXH3_64, TILE_PAGES, 0xE100 + P + tiles)


@pytest.mark.parametrize("tiles", [512, 1101])
@pytest.mark.parametrize("P,ppb", [(8192, 8), (16384, 4), (65536, 1)])
def test_remap_split(P, ppb, tiles):
    assert_remap_case(tiles)
    assert pcs.get_tuning(pcs.TUNE_XXH3_SPLIT_PAGES) == 8192  # these sizes take k_xxh3_split
    check_pages(P, remap_n(tiles, ppb), pcs.XXH3_64, ppb, 0xE200 + P + tiles)


# body 2 (any size), body 1 (4-block steps), body 0 (one block per step)
STRIDE_BODIES = [(249, None), (1000, None), (768, None), (768, {pcs.TUNE_XXH3_RT_BATCH: 0})]


@pytest.mark.parametrize("tiles", [512, 1101])
@pytest.mark.parametrize("P,tune", STRIDE_BODIES)
def test_remap_stride(P, tune, tiles):
    assert_remap_case(tiles)
    with tuning(tune or {}):
        check_pages(P, remap_n(tiles, TILE_PAGES), pcs.XXH3_64, TILE_PAGES, 0xE300 + P + tiles)


@pytest.mark.parametrize("tiles", [512, 1101])
@pytest.mark.parametrize("P", [256, 4096])
def test_remap_unaligned_base(P, tiles):
    """Fixed-size pages at base + 8: the unaligned chunked body of k_xxh3_stride."""
    assert_remap_case(tiles)
    check_pages(P, remap_n(tiles, TILE_PAGES), pcs.XXH3_64, TILE_PAGES, 0xE400 + P + tiles, shift=8)


@pytest.mark.parametrize("tiles", [512, 1101])
def test_remap_desc(tiles):
    """k_xxh3_desc over a mixed 4/8/16 KiB layout with off-grid (any-size
    body) and short (one lane) pages in the first tile, around the chunk seam,
    in the last whole round and in the tail."""
    assert_remap_case(tiles)
    n = remap_n(tiles, TILE_PAGES)
    offs, lens, _ = mixed_layout(0xE500 + tiles, 0, n)
    offs, lens = offs.copy(), lens.copy()
    odd = [1000, 100, 4088, 16, 249, 248]  # never longer than the 4 KiB slot they replace
    spots = [3, 63 * 16 + 15, 64 * 16, 511 * 16 + 7, n - 2]
    if tiles > REMAP_ROUND:
        spots += [512 * 16 + 1, 1100 * 16 + 2]
    for j, p in enumerate(spots):
        lens[p] = odd[j % len(odd)]
        lens[p + 1] = odd[(j + 3) % len(odd)]
    offs[spots[1]] += 8  # an 8-byte-aligned start inside its slot
    lens[spots[1]] = 1024
    check_desc(offs, lens, pcs.XXH3_64, TILE_PAGES, 0xE500 + tiles)


@pytest.mark.parametrize("nbytes", [4096 * 16 * 513 + 4096 * 3 + 48, 4096 * 16 * 1024])
def test_remap_stream_read(nbytes):
    npg = (nbytes - nbytes % 16 + 4095) // 4096
    tiles = (npg + 15) // 16
    # one whole round and a two-tile tail ending in a partial page; two whole rounds, no tail
    assert tiles in (REMAP_ROUND + 2, 2 * REMAP_ROUND)
    buf = torch.empty(nbytes + 16, dtype=torch.uint8, device=DEV)
    pcs.gen_pages(buf, 8, (nbytes + 16) // 8, 0xE600, 0)
    out = words(npg)
    pcs.stream_read(buf, nbytes, out)
    check_words(out, npg, stream_fold(buf.cpu().numpy()[:nbytes]), "stream_read")


# ---- 2. xcd_tile_eighths remainders ------------------------------------------------

EIGHTHS_TILES = list(range(1, 18)) + [8 * 200 + r for r in range(8)]


def test_eighths_tile_counts_cover_every_remainder():
    small = {t % 8 for t in EIGHTHS_TILES if t // 8 <= 2}
    large = {t % 8 for t in EIGHTHS_TILES if t // 8 == 200}
    assert small == set(range(8)) and large == set(range(8))


@pytest.mark.parametrize("tiles", EIGHTHS_TILES)
@pytest.mark.parametrize("P", [128, 1000])  # k_xxh64_lds, k_xxh64_stride
def test_eighths_pages(P, tiles):
    assert pcs.get_tuning(pcs.TUNE_XXH64_BLOCKS_PER_CU) == 0  # uncapped: grid == tiles, the remap runs
    n = X64_TILE_PAGES * tiles - 3
    assert (n + X64_TILE_PAGES - 1) // X64_TILE_PAGES == tiles
    check_pages(P, n, pcs.XXH64, X64_TILE_PAGES, 0xE700 + P + tiles)


@pytest.mark.parametrize("tiles", EIGHTHS_TILES)
@pytest.mark.parametrize("waves", [1, 2])
def test_eighths_lds_waves(waves, tiles):
    ppb = 16 * waves  # PCS_TUNE_XXH64_WAVES: a workgroup owns 16 pages per wave
    n = ppb * tiles - 3
    assert (n + ppb - 1) // ppb == tiles
    with tuning({pcs.TUNE_XXH64_WAVES: waves}):
        check_pages(128, n, pcs.XXH64, ppb, 0xE800 + waves + tiles)


@pytest.mark.parametrize("tiles", EIGHTHS_TILES)
def test_eighths_desc(tiles):
    n = X64_TILE_PAGES * tiles - 3
    assert (n + X64_TILE_PAGES - 1) // X64_TILE_PAGES == tiles
    offs, lens = uniform_desc(128, n)
    check_desc(offs, lens, pcs.XXH64, X64_TILE_PAGES, 0xE900 + tiles)


# ---- 3. capped grids that really loop ---------------------------------------------

def looping_n(ppb, blocks_per_cu=1):
    """Four trips of a grid capped at blocks_per_cu blocks per CU, the last
    one partial and ending in a partial tile (where a tile has several pages)."""
    cap = cus() * blocks_per_cu
    n = ppb * cap * 3 + ppb * 5 + 3
    ntiles = (n + ppb - 1) // ppb
    assert ntiles > 3 * cap and ntiles % cap != 0 and (ppb == 1 or n % ppb != 0)
    return n


ONE_BLOCK_PER_CU = {pcs.TUNE_XXH3_BLOCKS_PER_CU: 1, pcs.TUNE_XXH64_BLOCKS_PER_CU: 1}

# k_xxh3_fixed, k_xxh3_split (launched one block per tile whatever the knob says:
# at this count it runs its whole-grid form, remapped with a tail), k_xxh3_stride
# bodies 2, 1 and 0
CAPPED_XXH3 = [
    (256, TILE_PAGES, {}), (4096, TILE_PAGES, {}),
    (16384, 4, {}), (65536, 1, {}),
    (1000, TILE_PAGES, {}), (768, TILE_PAGES, {}), (768, TILE_PAGES, {pcs.TUNE_XXH3_RT_BATCH: 0}),
]
CAPPED_IDS = ["fixed256", "fixed4096", "split16k", "split64k", "any1000", "rt4_768", "rt_768"]


@pytest.mark.parametrize("P,ppb,tune", CAPPED_XXH3, ids=CAPPED_IDS)
def test_capped_xxh3_pages(P, ppb, tune):
    n = looping_n(ppb)
    with tuning({**ONE_BLOCK_PER_CU, **tune}):
        check_pages(P, n, pcs.XXH3_64, ppb, 0xEA00 + P)


@pytest.mark.parametrize("P,ppb,tune", CAPPED_XXH3, ids=CAPPED_IDS)
def test_capped_xxh3_scrub(P, ppb, tune):
    n = looping_n(ppb)
    trip = ppb * cus()  # pages per trip of the capped grid
    blank = [0, n - 1, trip - 1, trip, 2 * trip + 1, 3 * trip + 2]
    corrupt = [1, trip - 2, trip + 1, 2 * trip, 3 * trip, 3 * trip + ppb * 5, n - 2, trip]  # the last on a blank page
    with tuning({**ONE_BLOCK_PER_CU, **tune}):
        buf, wcls, wtypes = scrub_batch(P, n, 0xEB00 + P, blank, corrupt)
        assert (wcls[blank[:3]] == scrub_ref.BLANK).all() and (wcls[corrupt] == scrub_ref.CORRUPT).all()
        check_scrub(buf, P, n, wcls, wtypes, caps=[len(corrupt) + 3, 3])


@pytest.mark.parametrize("P", [128, 1000])  # k_xxh64_lds, k_xxh64_stride
def test_capped_xxh64_pages(P):
    n = looping_n(X64_TILE_PAGES)
    with tuning(ONE_BLOCK_PER_CU):
        check_pages(P, n, pcs.XXH64, X64_TILE_PAGES, 0xEC00 + P)


def test_default_cap_large_pages():
    """Default tuning: pages above 16 KiB cap the grid at 8 blocks per CU, so
    a batch of more than 16 * 8 * CUs such pages loops.  EloqStore's
    data_page_size is any uint16_t, e.g. 16,400 bytes (the any-size body)."""
    P = 16400
    assert P > 16384 and P % 256 != 0
    assert pcs.get_tuning(pcs.TUNE_XXH3_BLOCKS_PER_CU) == 0
    n = TILE_PAGES * BLOCKS_PER_CU * cus() + TILE_PAGES * 3 + 5
    assert (n + TILE_PAGES - 1) // TILE_PAGES > BLOCKS_PER_CU * cus()
    check_pages(P, n, pcs.XXH3_64, TILE_PAGES, 0xED00, kernel_stamp=False)
    torch.cuda.empty_cache()


# ---- 4. zero-copy list kernels looping ----------------------------------------------

@pytest.mark.parametrize("algo,P,ppb", [(pcs.XXH3_64, 256, TILE_PAGES), (pcs.XXH64, 128, X64_TILE_PAGES)])
def test_zero_copy_list_loops(algo, P, ppb):
    n = ppb * BLOCKS_PER_CU * cus() + 37
    assert (n + ppb - 1) // ppb > BLOCKS_PER_CU * cus()  # run_list's grid cap: the list kernels loop
    so = pcs.lib()
    zc = pcs.COUNTER_ZERO_COPY_LAUNCHES

    def call(fn, *args):
        before = pcs.counter(zc)
        rc = getattr(so, fn)(*args)
        assert rc == pcs.PCS_OK, so.pcs_last_error()
        assert pcs.counter(zc) == before + 1, fn  # one zero-copy launch served the whole batch

    with pcs.PagePool(n, P) as pool:
        pool.pages[:] = oracle.fill_pages(P, n, 0xEE00 + P).reshape(n, P)
        want = oracle.pages_digest(pool.pages, P, algo)
        idx = np.random.default_rng(P).permutation(n)
        ptrs = np.ascontiguousarray(pool.ptr(idx), dtype=np.uint64)
        body = pool.pages[:, 8:].copy()

        out = np.full(n + PAD, SENT64, dtype=np.uint64)
        call("pcs_pages_digest_host", ptrs.ctypes.data, P, n, algo, out.ctypes.data)
        assert np.array_equal(out[:n], want[idx]) and (out[n:] == SENT64).all()

        call("pcs_pages_stamp_host", ptrs.ctypes.data, P, n, algo)
        assert np.array_equal(headers(pool.pages, n, P), want)
        assert np.array_equal(pool.pages[:, 8:], body)

        def validate(bad_listed):
            ok = np.full(n + PAD, SENT8, dtype=np.uint8)
            fb = ctypes.c_uint64(0x1234)
            call("pcs_pages_validate_host_ex", ptrs.ctypes.data, P, n, algo, ok.ctypes.data, ctypes.byref(fb), 0)
            wok = np.ones(n, dtype=np.uint8)
            wok[bad_listed] = 0
            assert np.array_equal(ok[:n], wok) and (ok[n:] == SENT8).all()
            assert fb.value == (min(bad_listed) if bad_listed else NONE)

        validate([])
        for bad_listed in ([n - 1], [n // 2], [n // 2, n - 1]):  # positions in the list, not in the pool
            rows = idx[bad_listed]
            pool.pages[rows, 10] ^= 0x40
            assert (oracle.pages_digest(pool.pages[rows], P, algo) != headers(pool.pages[rows], len(rows), P)).all()
            validate(bad_listed)
            pool.pages[rows, 10] ^= 0x40


# ---- 5. scrub beyond one scan round -------------------------------------------------

SCRUB_P = 256
ROUND_PAGES = SCAN_ROUND * SCRUB_SPAN  # 2^20 pages: one round of k_scrub_scan


@pytest.fixture(scope="module")
def big_scrub():
    """2 rounds + 3 spans + 5 pages, built on the device; the reference classes
    are computed once and shared (the class of a page does not depend on n)."""
    n = 2 * ROUND_PAGES + 3 * SCRUB_SPAN + 5
    R = ROUND_PAGES
    blank = [0, n - 1, 4095, 4096, 4097, R - 2, R - 1, R, R + 1]  # span seam, round seam
    fixed = [4096, R - 1, R, 2 * R + 4095, n - 2]  # three of them in a blank run: near-blank pages are corrupt
    rng = np.random.default_rng(0xEF)
    rand = np.setdiff1d(rng.choice(n, size=3000, replace=False), np.array(blank + fixed))
    corrupt = np.concatenate([np.array(fixed), rand])
    buf, wcls, wtypes = scrub_batch(SCRUB_P, n, 0xEF00, blank, corrupt)
    assert (wcls[corrupt] == scrub_ref.CORRUPT).all()
    assert (wcls[[0, n - 1, 4095, 4097, R - 2, R + 1]] == scrub_ref.BLANK).all()
    yield buf, n, wcls, wtypes
    del buf
    torch.cuda.empty_cache()


def test_scrub_three_scan_rounds(big_scrub):
    buf, n, wcls, wtypes = big_scrub
    spans = (n + SCRUB_SPAN - 1) // SCRUB_SPAN
    assert spans > 2 * SCAN_ROUND and spans % SCAN_ROUND != 0 and n % SCRUB_SPAN != 0
    in_round_1 = int((wcls[:ROUND_PAGES] == scrub_ref.CORRUPT).sum())
    total = int((wcls == scrub_ref.CORRUPT).sum())
    assert 0 < in_round_1 and in_round_1 + 7 < total  # that cap ends inside round 2
    check_scrub(buf, SCRUB_P, n, wcls, wtypes, caps=[0, 5, in_round_1 + 7, total + 50])


def test_scrub_exactly_one_round(big_scrub):
    buf, _, wcls, wtypes = big_scrub
    n = ROUND_PAGES
    assert n == SCAN_ROUND * SCRUB_SPAN
    total = int((wcls[:n] == scrub_ref.CORRUPT).sum())
    check_scrub(buf, SCRUB_P, n, wcls, wtypes, caps=[total + 50, 5])


def test_scrub_one_page_into_round_two(big_scrub):
    buf, _, wcls, wtypes = big_scrub
    n = ROUND_PAGES + 1
    assert (n + SCRUB_SPAN - 1) // SCRUB_SPAN == SCAN_ROUND + 1
    assert wcls[n - 1] == scrub_ref.CORRUPT  # the one page of round 2 is corrupt
    total = int((wcls[:n] == scrub_ref.CORRUPT).sum())
    check_scrub(buf, SCRUB_P, n, wcls, wtypes, caps=[total + 50, total, total - 1])


# ---- 6. manifests beyond the small sizes -----------------------------------------------

MANIFEST_LENS = [31 * MiB + 5, 32 * MiB, 33 * MiB + 2049, 64 * MiB, 65 * MiB - 1, 129 * MiB + 777]


@pytest.fixture(scope="module")
def manifest_data():
    top = max(MANIFEST_LENS) + 16
    dbuf = torch.empty(top, dtype=torch.uint8, device=DEV)
    pcs.gen_pages(dbuf, 8, top // 8, 0xF000, 0)
    host = dbuf.cpu().numpy()
    want = {(shift, L): oracle.manifest_checksum(host[shift:shift + L]) for shift in (0, 8) for L in MANIFEST_LENS}
    want[(3, MANIFEST_LENS[2])] = oracle.manifest_checksum(host[3:3 + MANIFEST_LENS[2]])
    yield dbuf, host, want
    del dbuf
    torch.cuda.empty_cache()


def test_manifest_lengths_cross_their_thresholds():
    chunks = [(L + MANIFEST_CHUNK - 1) // MANIFEST_CHUNK for L in MANIFEST_LENS]
    assert chunks == [32, 32, 34, 64, 65, 130]
    # k_manifest_fold: exactly one batch, a batch and a remainder, two batches and a remainder
    assert FOLD in chunks and any(FOLD < c < 2 * FOLD for c in chunks) and any(c > 2 * FOLD and c % FOLD for c in chunks)
    # k_manifest_sums16: the first remapped tile count, and remapped counts with a tail
    tiles = [c * SUMS16_TILES_PER_CHUNK for c in chunks]
    assert REMAP_ROUND in tiles and any(t > REMAP_ROUND and t % REMAP_ROUND for t in tiles)


@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("shift", [0, 8])  # k_manifest_sums16 / k_manifest_sums when wide
def test_manifest_large(manifest_data, shift, wide):
    dbuf, _, want = manifest_data
    assert (dbuf.data_ptr() + shift) % 16 == shift
    with tuning({pcs.TUNE_MANIFEST_WIDE: wide}):
        for L in MANIFEST_LENS:
            d_out = words(1)
            pcs._call("pcs_manifest_checksum_dev", dbuf.data_ptr() + shift, L, d_out.data_ptr(), pcs._stream(None))
            check_words(d_out, 1, np.array([want[(shift, L)]], dtype=np.uint64), (wide, shift, L))


def test_manifest_large_unaligned(manifest_data):
    """Shift 3: one lane per chunk on the generic path (whatever
    TUNE_MANIFEST_WIDE says), so one size only."""
    dbuf, _, want = manifest_data
    L = MANIFEST_LENS[2]
    d_out = words(1)
    pcs._call("pcs_manifest_checksum_dev", dbuf.data_ptr() + 3, L, d_out.data_ptr(), pcs._stream(None))
    check_words(d_out, 1, np.array([want[(3, L)]], dtype=np.uint64), L)


def test_manifest_large_host(manifest_data):
    _, host, want = manifest_data
    L = 65 * MiB - 1
    assert (L + MANIFEST_CHUNK - 1) // MANIFEST_CHUNK > FOLD
    assert pcs.manifest_checksum_host(host[:L].tobytes()) == want[(0, L)]


# ---- 7. raw ranges looping ------------------------------------------------------------

def test_long_ranges_loop():
    n = BLOCKS_PER_CU * cus() + 37
    assert n > BLOCKS_PER_CU * cus()  # k_xxh3_long: grid_for(n, 1, 8), one workgroup per range
    rng = np.random.default_rng(0xF1)
    lens = rng.integers(2048, 6001, size=n).astype(np.uint32)
    lens[[0, 1, n - 1]] = [2048, 6000, 2049]
    pitch = (lens.astype(np.uint64) + np.uint64(7 + 8)) // np.uint64(8) * np.uint64(8)
    offs = np.zeros(n, dtype=np.uint64)
    np.cumsum(pitch[:-1], out=offs[1:])
    assert (offs % 8 == 0).all() and (offs % 16 == 8).any()
    total = int(offs[-1] + lens[-1])
    base = torch.empty(total + 16, dtype=torch.uint8, device=DEV)
    pcs.gen_pages(base, 8, (total + 16) // 8, 0xF100, 0)
    out = words(n)
    pcs.xxh3_64_ranges(base, torch.from_numpy(offs.view(np.int64)).to(DEV),
                       torch.from_numpy(lens.view(np.int32)).to(DEV), n, out=out)
    check_words(out, n, oracle.desc_raw_xxh3(base.cpu().numpy(), offs, lens), "long ranges")


@pytest.fixture(scope="module")
def short_ranges():
    n = GENERIC_LANES_PER_CU * cus() + 1000
    rng = np.random.default_rng(0xF2)
    lens = rng.integers(0, 65, size=n).astype(np.uint32)
    lens[[0, 1, n - 2, n - 1]] = [0, 64, 64, 0]
    offs = rng.integers(0, MiB - 64, size=n).astype(np.uint64)  # any alignment, overlapping
    base = torch.empty(MiB, dtype=torch.uint8, device=DEV)
    pcs.gen_pages(base, 8, MiB // 8, 0xF200, 0)
    return (n, base, base.cpu().numpy(), offs, lens, torch.from_numpy(offs.view(np.int64)).to(DEV),
            torch.from_numpy(lens.view(np.int32)).to(DEV))


def test_short_ranges_loop_xxh3(short_ranges):
    n, base, host, offs, lens, d_off, d_len = short_ranges
    assert n > GENERIC_LANES_PER_CU * cus()  # k_generic_desc: more than one trip
    out = words(n)
    pcs.xxh3_64_ranges(base, d_off, d_len, n, out=out)
    check_words(out, n, oracle.desc_raw_xxh3(host, offs, lens), "xxh3 ranges")


@pytest.mark.parametrize("seed", [0, 0x9E3779B97F4A7C15])
def test_short_ranges_loop_xxh64(short_ranges, seed):
    n, base, host, offs, lens, d_off, d_len = short_ranges
    assert n > GENERIC_LANES_PER_CU * cus()
    out = words(n)
    pcs.xxh64_ranges(base, d_off, d_len, n, seed, out=out)
    check_words(out, n, oracle.desc_raw_xxh64(host, offs, lens, seed), ("xxh64 ranges", seed))


# ---- 8. header-bit walk ---------------------------------------------------------------

WALK_N = 128
WALK_WANT = np.array([0] * 64 + [1] * 64, dtype=np.uint8)


def walk_positions(page_offsets):
    """Page i < 64: (byte position, mask) of header bit i."""
    return [(int(page_offsets[i]) + i // 8, 1 << (i % 8)) for i in range(64)]


def flip_header_bits(buf, page_offsets):
    pos = walk_positions(page_offsets)
    idx = torch.tensor([p for p, _ in pos], dtype=torch.int64, device=DEV)
    buf[idx] ^= torch.tensor([m for _, m in pos], dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("P,algo", [(4096, 0), (16384, 0), (1000, 0), (4096, 1), (1000, 1)],
                         ids=["fixed", "split", "stride", "x64_lds", "x64_stride"])
def test_header_bit_walk_pages(P, algo):
    n = WALK_N
    buf = page_buffer(P, n, 0xF300 + P + algo)
    pcs.pages_stamp(buf, P, n, algo)
    want_hdr = oracle.pages_digest(buf.cpu().numpy(), P, algo)
    flip_header_bits(buf, np.arange(n) * P)
    got_hdr = headers(buf.cpu().numpy(), n, P)
    assert np.array_equal(got_hdr[:64] ^ want_hdr[:64], np.uint64(1) << np.arange(64, dtype=np.uint64))
    assert np.array_equal(got_hdr[64:], want_hdr[64:])
    ok, fb = flags(n), garbage_word()
    pcs.pages_validate(buf, P, n, algo, ok=ok, first_bad=fb)
    check_flags(ok, n, WALK_WANT, (P, algo))
    assert fb_value(fb) == 0
    if algo == 0 and P == 4096:  # scrub: a page with one header bit off is CORRUPT, never BLANK or OK
        wcls, wtypes, _, _ = scrub_ref.classify(buf.cpu().numpy(), P)
        assert (wcls[:64] == scrub_ref.CORRUPT).all() and (wcls[64:] == scrub_ref.OK).all()
        check_scrub(buf, P, n, wcls, wtypes, caps=[100])


@pytest.mark.parametrize("P,pitch,algo", [(4096, 4096, 0), (1000, 1000, 0), (100, 104, 0), (4100, 4104, 1)],
                         ids=["xxh3_chunked", "xxh3_any", "xxh3_short", "x64_generic"])
def test_header_bit_walk_desc(P, pitch, algo):
    n = WALK_N
    offs, lens = uniform_desc(P, n, pitch)
    base, d_off, d_len = desc_buffer(offs, lens, 0xF400 + P)
    pcs.desc_stamp(base, d_off, d_len, n, algo)
    host = base.cpu().numpy()
    want_hdr = oracle.desc_digest(host, offs, lens, algo)
    assert np.array_equal(host[(offs.astype(np.int64)[:, None] + np.arange(8)).ravel()].view("<u8"), want_hdr)
    flip_header_bits(base, offs)
    ok, fb = flags(n), garbage_word()
    pcs.desc_validate(base, d_off, d_len, n, algo, ok=ok, first_bad=fb)
    check_flags(ok, n, WALK_WANT, (P, algo))
    assert fb_value(fb) == 0


def test_header_bit_walk_zero_copy():
    P, n = 4096, WALK_N
    with pcs.PagePool(n, P) as pool:
        pool.pages[:] = oracle.fill_pages(P, n, 0xF500).reshape(n, P)
        ptrs = pool.ptr(np.arange(n))
        pcs.stamp_ptrs(ptrs, P)
        assert np.array_equal(headers(pool.pages, n, P), oracle.pages_digest(pool.pages, P, 0))
        for i in range(64):
            pool.pages[i, i // 8] ^= 1 << (i % 8)
        before = pcs.counter(pcs.COUNTER_ZERO_COPY_LAUNCHES)
        ok, fb = pcs.validate_ptrs(ptrs, P)
        assert pcs.counter(pcs.COUNTER_ZERO_COPY_LAUNCHES) == before + 1
        assert np.array_equal(ok, WALK_WANT) and fb == 0
