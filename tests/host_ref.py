"""Helpers of the staged host pipeline tests (tests/test_gpu_host_pipeline.py,
tests/host_gather_child.py): the pipeline's chunk arithmetic restated, page
sources for each of its paths with distinct content in every page, and the
footprint check of a stamp (the listed pages' headers change, no other byte of
the pool does).

The arithmetic mirrors host_batch / host_scrub in eloqstore_amd/csrc/pcs_capi.cpp:
a call is cut into chunks of STAGE_BYTES // P pages (at least one page, at most
the whole call) which go through SLOTS staging slots in turn, so chunk k reuses
the slot of chunk k - SLOTS.
"""
import numpy as np

import oracle

STAGE_BYTES = 32 << 20  # kStageBytes
SLOTS = 3               # kSlots


def chunk_pages(P: int, n: int) -> int:
    """Pages per chunk of an n-page call at page size P."""
    return max(1, min(n, STAGE_BYTES // P))


def n_chunks(P: int, n: int) -> int:
    """Chunks an n-page call is cut into (0 for an empty call)."""
    return 0 if n == 0 else -(-n // chunk_pages(P, n))


def fill(pages: np.ndarray, seed: int, first_page: int = 0) -> None:
    """Fill a contiguous (N, P) uint8 array in place with oracle.fill_pages'
    generator: every 8-byte word depends on (seed, page, word), so no two pages
    and no two words of a page hold the same bytes."""
    N, P = pages.shape
    assert pages.flags.c_contiguous and pages.dtype == np.uint8 and P % 8 == 0
    oracle.lib().oracle_fill_pages(pages.ctypes.data, P, N, seed, first_page)


def headers(pages: np.ndarray) -> np.ndarray:
    """The N page headers (bytes [0, 8), little endian) of an (N, P) array, as a copy."""
    return np.ascontiguousarray(pages[:, :8]).view("<u8").reshape(-1)


def set_headers(pages: np.ndarray, rows, values) -> None:
    pages[np.asarray(rows, dtype=np.int64), :8] = \
        np.ascontiguousarray(values, dtype="<u8").view(np.uint8).reshape(-1, 8)


def pool_pages_with_holdout(n: int) -> int:
    """The smallest pool of which n pages remain once every third page
    (2, 5, 8, ...) is left out."""
    N = n + max(0, n - 1) // 2
    while N - N // 3 < n:
        N += 1
    return N


def listed_rows(n: int, N: int, seed: int) -> np.ndarray:
    """n distinct pool rows in a shuffled order: all of them when N == n, the
    rows r with r % 3 != 2 when N == pool_pages_with_holdout(n)."""
    rows = np.arange(N, dtype=np.int64)
    if N != n:
        rows = rows[rows % 3 != 2]
    assert rows.size == n
    return np.random.default_rng(seed).permutation(rows)


def snapshot(pages: np.ndarray) -> np.ndarray:
    """A copy of the whole pool, to compare with after a call."""
    return pages.copy()


def _words(a: np.ndarray) -> np.ndarray:
    flat = a.reshape(-1)
    return flat.view(np.uint64) if flat.size % 8 == 0 else flat


def first_difference(a: np.ndarray, b: np.ndarray):
    """Flat byte index of the first byte in which two equal-shaped contiguous
    uint8 arrays differ, or None."""
    assert a.shape == b.shape and a.flags.c_contiguous and b.flags.c_contiguous
    wa, wb = _words(a), _words(b)
    if np.array_equal(wa, wb):
        return None
    w = int(np.flatnonzero(wa != wb)[0])
    k = wa.itemsize
    fa, fb = a.reshape(-1), b.reshape(-1)
    return w * k + int(np.flatnonzero(fa[w * k:(w + 1) * k] != fb[w * k:(w + 1) * k])[0])


def assert_only_headers_changed(before: np.ndarray, after: np.ndarray, listed_idx, want) -> None:
    """before / after: the whole (N, P) pool around a stamp; listed_idx: the
    pool rows the call was given, in list order; want: their expected headers
    (u64) in the same order.  The listed rows' headers must equal want and
    every other byte of the pool must be what it was.  `before` is left
    unchanged."""
    N, P = after.shape
    listed_idx = np.asarray(listed_idx, dtype=np.int64)
    want = np.asarray(want, dtype=np.uint64)
    assert before.shape == after.shape and listed_idx.shape == want.shape
    got = headers(after)[listed_idx]
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"header of listed page {i} (pool row {int(listed_idx[i])}) is {int(got[i]):#018x}, "
                             f"want {int(want[i]):#018x}; {int((got != want).sum())} of {want.size} headers differ")
    expect = before.copy()
    set_headers(expect, listed_idx, want)
    at = first_difference(expect, after)
    if at is not None:
        row, off = divmod(at, P)
        where = "a listed page" if (listed_idx == row).any() else "a page outside the list"
        raise AssertionError(f"stray write: byte {off} of pool row {row} ({where}) changed from "
                             f"{int(before[row, off]):#04x} to {int(after[row, off]):#04x}")


class Source:
    """n pages of P bytes for one path of the host pipeline, each with its own content.

    kind "gather": an unregistered PagePool listed through shuffled pointers
    (with hold_out, every third pool page is left out of the list);
    "direct": a registered PagePool, contiguous and in order (the caller turns
    zero-copy off); "pinned": a torch pin_memory buffer, contiguous and in order.

    .pages is the (N, P) view of the whole pool, .rows the n listed pool rows
    in list order, .ptrs their addresses, .counter the pcs counter of the path.
    """

    def __init__(self, kind: str, P: int, n: int, seed: int, hold_out: bool = False):
        import eloqstore_amd as pcs
        self.kind, self.P, self.n = kind, P, n
        self.pool = self._pinned = None
        if kind == "gather":
            N = pool_pages_with_holdout(n) if hold_out else n
            self.pool = pcs.PagePool(N, P, register=False)
            self.pages, base = self.pool.pages, self.pool.base
            self.rows = listed_rows(n, N, seed)
            self.counter = pcs.COUNTER_GATHER_CHUNKS
        elif kind == "direct":
            self.pool = pcs.PagePool(n, P, register=True)
            self.pages, base = self.pool.pages, self.pool.base
            self.rows = np.arange(n, dtype=np.int64)
            self.counter = pcs.COUNTER_DIRECT_DMA_CHUNKS
        elif kind == "pinned":
            import torch
            self._pinned = torch.empty(n * P, dtype=torch.uint8, pin_memory=True)
            self.pages, base = self._pinned.numpy().reshape(n, P), self._pinned.data_ptr()
            self.rows = np.arange(n, dtype=np.int64)
            self.counter = pcs.COUNTER_DIRECT_DMA_CHUNKS
        else:
            raise ValueError(kind)
        self.ptrs = np.uint64(base) + self.rows.astype(np.uint64) * np.uint64(P)
        fill(self.pages, seed)

    def digests(self, algo: int = 0) -> np.ndarray:
        """The oracle's digests of the listed pages, in list order."""
        return oracle.pages_digest(self.pages, self.P, algo)[self.rows]

    def stamp_by_oracle(self, algo: int = 0) -> None:
        """Correct headers on every pool page, written by the oracle."""
        set_headers(self.pages, np.arange(self.pages.shape[0]), oracle.pages_digest(self.pages, self.P, algo))

    def close(self) -> None:
        self.pages = None
        if self.pool is not None:
            self.pool.close()
            self.pool = None
        self._pinned = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
