"""CPU checks of tests/host_ref.py: the staged pipeline's chunk arithmetic
against hand-worked values, the listed-rows builder, and the stamp footprint
checker on hand-made stray writes."""
import numpy as np
import pytest

import host_ref
import oracle
from host_ref import chunk_pages, n_chunks

MiB = 1 << 20


def test_stage_constants_match_the_library_source():
    import os
    src = open(os.path.join(os.path.dirname(__file__), "..", "eloqstore_amd", "csrc", "pcs_capi.cpp")).read()
    assert "constexpr size_t kStageBytes = 32u << 20;" in src and host_ref.STAGE_BYTES == 32 * MiB
    assert "constexpr int kSlots = 3;" in src and host_ref.SLOTS == 3


@pytest.mark.parametrize("P,per_chunk", [(4096, 8192), (5000, 6710), (1000, 33554), (65536, 512), (32 * MiB, 1),
                                         (32 * MiB + 256, 1), (16 * MiB + 256, 1), (264, 127100), (4104, 8176),
                                         (8, 4194304)])
def test_chunk_pages_hand_worked(P, per_chunk):
    assert chunk_pages(P, 10 ** 9) == per_chunk
    # a call smaller than a chunk is one chunk of its own size
    assert chunk_pages(P, 1) == 1 and n_chunks(P, 1) == 1
    if per_chunk > 1:
        assert chunk_pages(P, per_chunk - 1) == per_chunk - 1 and n_chunks(P, per_chunk - 1) == 1
    c = per_chunk
    assert [n_chunks(P, n) for n in (c, c + 1, 3 * c, 3 * c + 1, 4 * c + 1, 7 * c - 1, 4 * c + 7)] == \
        ([1, 2, 3, 4, 5, 7, 5] if c > 6 else [1, 2, 3, 4, 5, 6, 11])


def test_n_chunks_edges():
    assert n_chunks(4096, 0) == 0
    assert n_chunks(4096, 8192) == 1 and n_chunks(4096, 8193) == 2
    assert n_chunks(5000, 3 * 6710 + 1) == 4 and n_chunks(4104, 8176 + 5) == 2
    assert n_chunks(32 * MiB + 256, 4) == 4 and n_chunks(16 * MiB + 256, 4) == 4  # one page per chunk
    assert n_chunks(264, 2 * 127100 + 3) == 3


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 100, 24577, 3583])
def test_listed_rows_and_holdout(n):
    N = host_ref.pool_pages_with_holdout(n)
    rows = host_ref.listed_rows(n, N, seed=n)
    assert rows.size == n == np.unique(rows).size and not (rows % 3 == 2).any() and rows.max() < N
    # no smaller pool would do
    assert (N - 1) - (N - 1) // 3 < n
    if n > 4:
        assert not np.array_equal(rows, np.sort(rows))  # shuffled
    allrows = host_ref.listed_rows(n, n, seed=n)
    assert np.array_equal(np.sort(allrows), np.arange(n))


def test_fill_is_oracle_fill_pages_and_distinct():
    pg = np.zeros((37, 1000), dtype=np.uint8)
    host_ref.fill(pg, 0xABC)
    assert np.array_equal(pg.reshape(-1), oracle.fill_pages(1000, 37, 0xABC))
    assert np.unique(pg.reshape(-1).view(np.uint64)).size == 37 * 125  # every word of every page differs


def _pool(N=12, P=264, seed=5):
    pg = np.zeros((N, P), dtype=np.uint8)
    host_ref.fill(pg, seed)
    return pg


def test_footprint_checker_accepts_a_clean_stamp():
    before = _pool()
    kept = host_ref.snapshot(before)
    listed = np.array([7, 0, 4, 10], dtype=np.int64)
    want = oracle.pages_digest(before, 264)[listed]
    after = before.copy()
    host_ref.set_headers(after, listed, want)
    assert np.array_equal(host_ref.headers(after)[listed], want)
    host_ref.assert_only_headers_changed(before, after, listed, want)
    assert np.array_equal(before, kept)  # the snapshot is not touched
    # an empty list: nothing may change
    host_ref.assert_only_headers_changed(before, before.copy(), [], [])


@pytest.mark.parametrize("row,off,what", [
    (4, 8, "a listed page"),        # first body byte of a listed page (a 16-byte header copy lands here)
    (4, 263, "a listed page"),      # last byte of a listed page
    (5, 0, "a page outside the list"),   # header of a page that was not listed
    (11, 100, "a page outside the list"),
    (1, 263, "a page outside the list"),
])
def test_footprint_checker_sees_a_stray_write(row, off, what):
    before = _pool()
    listed = np.array([7, 0, 4, 10], dtype=np.int64)
    want = oracle.pages_digest(before, 264)[listed]
    after = before.copy()
    host_ref.set_headers(after, listed, want)
    after[row, off] ^= 0x10
    with pytest.raises(AssertionError, match=rf"stray write: byte {off} of pool row {row} \({what}\)"):
        host_ref.assert_only_headers_changed(before, after, listed, want)


def test_footprint_checker_sees_wrong_and_misplaced_headers():
    before = _pool()
    listed = np.array([7, 0, 4, 10], dtype=np.int64)
    want = oracle.pages_digest(before, 264)[listed]
    after = before.copy()
    host_ref.set_headers(after, listed, want[[1, 0, 2, 3]])  # two headers swapped
    with pytest.raises(AssertionError, match=r"header of listed page 0 \(pool row 7\)"):
        host_ref.assert_only_headers_changed(before, after, listed, want)
    after = before.copy()
    host_ref.set_headers(after, listed[:3], want[:3])  # the last listed page was not stamped
    with pytest.raises(AssertionError, match=r"header of listed page 3 \(pool row 10\)"):
        host_ref.assert_only_headers_changed(before, after, listed, want)
    after = before.copy()
    host_ref.set_headers(after, np.arange(4), want)  # scattered by list position, not by page
    with pytest.raises(AssertionError):
        host_ref.assert_only_headers_changed(before, after, listed, want)


def test_first_difference():
    a = np.arange(40, dtype=np.uint8).reshape(5, 8)
    assert host_ref.first_difference(a, a.copy()) is None
    for at in (0, 7, 8, 23, 39):
        b = a.copy()
        b.reshape(-1)[at] ^= 1
        b.reshape(-1)[39] ^= 2
        assert host_ref.first_difference(a, b) == at
    c = np.arange(15, dtype=np.uint8).reshape(3, 5)  # not a multiple of 8 bytes
    d = c.copy()
    d[2, 4] = 0
    assert host_ref.first_difference(c, d) == 14
