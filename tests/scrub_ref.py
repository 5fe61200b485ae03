"""Reference scrub classifier (numpy + the CPU oracle): what
pcs_pages_scrub_dev / _host must return for a batch of fixed-size pages.

Also the shared builders of the scrub tests' batches (hand-made pages of every
class), so the CPU and GPU tests check the same cases.
"""
import numpy as np

import oracle

CORRUPT, OK, BLANK = 0, 1, 2
NO_PAGE = (1 << 64) - 1
TYPE_BYTES = (0, 1, 2, 3, 255, 9)  # one type byte per census bucket, in bucket order


def bucket(t: int) -> int:
    return t if t < 4 else 4 if t == 255 else 5


BUCKET_OF = np.array([bucket(t) for t in range(256)], dtype=np.int64)  # type byte -> census bucket


def summarize(cls: np.ndarray, types: np.ndarray, corrupt_cap: int = 1024):
    """Summary dict and capped corrupt list of per-page classes and type bytes."""
    ok = cls == OK
    by_type = np.bincount(BUCKET_OF[types[ok]], minlength=6).tolist()
    bad = np.flatnonzero(cls == CORRUPT).astype(np.uint64)
    summary = {"n_pages": int(cls.size), "n_ok": int(ok.sum()), "n_corrupt": int(bad.size),
               "n_blank": int((cls == BLANK).sum()), "ok_by_type": by_type,
               "first_corrupt": int(bad[0]) if bad.size else NO_PAGE, "n_listed": int(min(bad.size, corrupt_cap))}
    return summary, bad[:corrupt_cap]


def classify(pages: np.ndarray, page_size: int, corrupt_cap: int = 1024):
    """pages: uint8 array of n * page_size bytes -> (cls, types, summary dict, corrupt list)."""
    P = page_size
    flat = np.ascontiguousarray(pages, dtype=np.uint8).reshape(-1)
    n = flat.size // P
    pg = flat[: n * P].reshape(n, P)
    if n == 0:
        empty = np.zeros(0, dtype=np.uint8)
        return empty, empty, {"n_pages": 0, "n_ok": 0, "n_corrupt": 0, "n_blank": 0, "ok_by_type": [0] * 6,
                              "first_corrupt": NO_PAGE, "n_listed": 0}, np.zeros(0, dtype=np.uint64)
    digest = oracle.pages_digest(pg, P, 0)
    stored = np.ascontiguousarray(pg[:, :8]).view("<u8").reshape(n)
    ok = stored == digest
    blank = ~pg.any(axis=1)
    assert not (ok & blank).any()  # XXH3 of a zero body is never 0 (tests/golden/scrub_blank.json)
    cls = np.where(ok, OK, np.where(blank, BLANK, CORRUPT)).astype(np.uint8)
    types = pg[:, 8].copy()
    summary, bad = summarize(cls, types, corrupt_cap)
    return cls, types, summary, bad


def stamp(pg: np.ndarray, rows) -> None:
    """Write the XXH3 digest of rows' bodies into their headers (SetChecksum)."""
    rows = np.asarray(rows, dtype=np.int64)
    if rows.size == 0:
        return
    P = pg.shape[1]
    sub = np.ascontiguousarray(pg[rows])
    pg[rows, :8] = oracle.pages_digest(sub, P, 0).astype("<u8").view(np.uint8).reshape(-1, 8)


NEAR_BLANK_OFFSETS = (0, 7, 8, 9, 15, 16, 255, 256, 1023, 1024, 1032)


def near_blank_offsets(P: int):
    offs = list(NEAR_BLANK_OFFSETS) + [P // 2, P - 65, P - 64, P - 9, P - 8, P - 1]
    return sorted({o for o in offs if 0 <= o < P})


WALK_FULL_MAX = 5120     # every byte of a page is walked up to this size
WALK_PIECE_MAX = 65536   # one byte per 16-byte piece up to this size, one per 64-byte stripe above
WALK_ENDS = 1100         # every byte of the first and the last WALK_ENDS bytes
WALK_EDGE = 24           # every byte within WALK_EDGE of a multiple of 4096 (slice and 4-block batch edges)
WALK_CONTROL_EVERY = 17  # rows 0, 17, 34, ... are control pages: 17 j % 16 = j % 16, every group slot of a tile
CONTROL_KINDS = ("blank", "zero_body_ok", "random_ok", "header_bit")


def walk_offsets(P: int) -> np.ndarray:
    """The byte offsets a walk batch visits, ascending (int64).

    P <= 5120: every byte.  Up to 64 KiB: one byte in every 16-byte piece k,
    16k + (5k + k // 16) % 16 (over 256 consecutive pieces that is every
    (lane, byte-in-piece) and every (chunk, byte-in-piece) pair), every byte of
    the first and last 1100, and every byte within 24 of a multiple of 4096.
    Above: one byte in every 64-byte stripe s, 64s + (13s + s // 16) % 64, and
    the two 1100-byte ends."""
    if P <= WALK_FULL_MAX:
        return np.arange(P, dtype=np.int64)
    ends = np.concatenate((np.arange(0, WALK_ENDS), np.arange(P - WALK_ENDS, P)))
    if P <= WALK_PIECE_MAX:
        k = np.arange((P + 15) // 16, dtype=np.int64)
        one = 16 * k + (5 * k + k // 16) % 16
        m = np.arange(0, P + 1, 4096, dtype=np.int64)
        edges = (m[:, None] + np.arange(-WALK_EDGE, WALK_EDGE + 1)).ravel()
        offs = np.concatenate((one, ends, edges))
    else:
        s = np.arange((P + 63) // 64, dtype=np.int64)
        one = 64 * s + (13 * s + s // 16) % 64
        offs = np.concatenate((one, ends))
    offs = np.minimum(offs, P - 1)
    return np.unique(offs[offs >= 0]).astype(np.int64)


def walk_bit(offs) -> np.ndarray:
    """The one set bit a walk page carries at offset o."""
    o = np.asarray(offs, dtype=np.int64)
    return (np.uint8(1) << ((o + o // 16) % 8).astype(np.uint8)).astype(np.uint8)


def build_walk_batch(P: int, seed: int = 1):
    """One walk page per offset of walk_offsets(P): all zero but for one byte
    holding the single bit walk_bit(o).  Rows 0, 17, 34, ... are control pages
    of the four CONTROL_KINDS in turn (control j is kind j % 4): blank; a zero
    body under its correct stamped header; a random stamped page with a type
    byte of TYPE_BYTES; a zero body under a header with the one bit j % 64 set.
    A blank control page is appended, so the first and the last page are blank.
    Returns (pages (n, P) uint8, rows): rows[kind] are the row indices of each
    control kind, rows["offsets"] / rows["walk_rows"] the offsets and the rows
    of their pages (aligned arrays), rows["walk"] the same as offset -> row."""
    offs = walk_offsets(P)
    nw = offs.size
    E = WALK_CONTROL_EVERY
    # walk page i sits at the i-th row that is not a multiple of 17
    walk_rows = np.arange(nw, dtype=np.int64) + np.arange(nw, dtype=np.int64) // (E - 1) + 1
    n = int(walk_rows[-1]) + 2
    pg = np.zeros((n, P), dtype=np.uint8)
    pg[walk_rows, offs] = walk_bit(offs)
    ctl = np.arange(0, n - 1, E, dtype=np.int64)  # the appended page n - 1 is not among them
    rows = {kind: ctl[i::4].tolist() for i, kind in enumerate(CONTROL_KINDS)}
    rows["blank"].append(n - 1)
    rng = np.random.default_rng(seed * 1000003 + P * 31)
    rnd = np.asarray(rows["random_ok"], dtype=np.int64)
    pg[rnd] = rng.integers(0, 256, size=(rnd.size, P), dtype=np.uint8)
    pg[rnd, 8] = np.array(TYPE_BYTES, dtype=np.uint8)[(rnd // E // 4) % len(TYPE_BYTES)]
    stamp(pg, rnd)
    stamp(pg, rows["zero_body_ok"])
    for r in rows["header_bit"]:
        bit = (r // E) % 64
        pg[r, bit // 8] = 1 << (bit % 8)
    rows["offsets"], rows["walk_rows"] = offs, walk_rows
    rows["walk"] = dict(zip(offs.tolist(), walk_rows.tolist()))
    return pg, rows


def build_batch(P: int, n: int, seed: int = 1, near=None, flips: int = 12, zero_header: bool = True):
    """A mixed batch of n pages: OK pages of all six type buckets (type byte
    set before stamping), `flips` pages corrupted by a flip at byte 10 (fewer
    when n is small, at least one), blank pages (page 0, page n - 1 and one
    whole 16-page tile: pages 32..47, or 0..15 when n < 64), a zero header
    over a non-zero body, a zero body under its correct header, and one
    near-blank page (zero but for one byte 0x01) per offset in `near`
    (default: near_blank_offsets(P)).  Returns (pages (n, P) uint8, rows)."""
    near = near_blank_offsets(P) if near is None else list(near)
    rng = np.random.default_rng(seed * 1000003 + P * 31 + n)
    pg = rng.integers(0, 256, size=(n, P), dtype=np.uint8)
    pg[:, 8] = np.array(TYPE_BYTES, dtype=np.uint8)[np.arange(n) % 6]
    stamp(pg, np.arange(n))
    rows = {}
    tile = list(range(32, 48)) if n >= 64 else list(range(0, 16))
    rows["blank"] = sorted(set([0, n - 1] + tile))
    free = [i for i in range(n) if i not in rows["blank"]]
    rng.shuffle(free)
    rows["ok_kept"] = [next(i for i in free if i % 6 == b) for b in range(6)]  # one untouched page per bucket
    free = [i for i in free if i not in rows["ok_kept"]]
    take = iter(free)
    pg[rows["blank"]] = 0
    rows["zero_body_ok"] = next(take)
    pg[rows["zero_body_ok"]] = 0
    stamp(pg, [rows["zero_body_ok"]])
    rows["zero_header"] = None
    if zero_header:
        rows["zero_header"] = next(take)
        pg[rows["zero_header"], :8] = 0
    rows["near_blank"] = {}
    for off in near:
        r = next(take)
        pg[r] = 0
        pg[r, off] = 1
        rows["near_blank"][off] = r
    left = len(free) - 1 - (1 if zero_header else 0) - len(near)
    assert left >= 1, "batch too small for its cases"
    rows["flipped"] = sorted(next(take) for _ in range(min(flips, left)))
    pg[rows["flipped"], 10] ^= 0xFF
    if left - len(rows["flipped"]) >= 3:  # room left: a few more blank pages at random places
        more = [next(take) for _ in range(3)]
        pg[more] = 0
        rows["blank"] = sorted(rows["blank"] + more)
    return pg, rows
