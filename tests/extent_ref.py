"""Reference scrub extents (numpy): what pcs_scrub_extents_dev /
pcs_pages_scrub_extents_host must return for an array of class bytes.

A run is a maximal range of equal bytes; only byte 2 is blank.  Run starts come
from np.diff, the summary fields are derived from the runs exactly as
include/eloqstore_pcs.h defines them.  Also the shared builders of the extent
tests' class arrays.
"""
import numpy as np

CORRUPT, OK, BLANK = 0, 1, 2
NO_PAGE = (1 << 64) - 1
RUN_DTYPE = np.dtype([("first_page", "<u8"), ("n_pages", "<u8"), ("cls", "<u4"), ("reserved", "<u4")])
FIELDS = ("n_pages", "n_runs", "n_listed", "written_pages", "n_blank", "n_blank_runs", "first_blank", "n_holes",
          "n_hole_pages", "first_hole", "first_class", "last_class")


def extents(cls, run_cap: int = 1024):
    """cls: uint8 array -> (summary dict, structured array of the first min(n_runs, run_cap) runs)."""
    cls = np.ascontiguousarray(cls, dtype=np.uint8).reshape(-1)
    n = int(cls.size)
    if n == 0:
        s = dict.fromkeys(FIELDS, 0)
        s.update(first_blank=NO_PAGE, first_hole=NO_PAGE, first_class=NO_PAGE, last_class=NO_PAGE)
        return s, np.zeros(0, dtype=RUN_DTYPE)
    starts = np.concatenate(([0], np.flatnonzero(np.diff(cls)) + 1)).astype(np.int64)
    lengths = np.diff(np.concatenate((starts, [n])))
    run_cls = cls[starts]
    written = np.flatnonzero(cls != BLANK)
    w = int(written[-1]) + 1 if written.size else 0
    blank_run = run_cls == BLANK
    hole = blank_run & (starts < w)
    s = {"n_pages": n, "n_runs": int(starts.size), "n_listed": int(min(starts.size, run_cap)), "written_pages": w,
         "n_blank": int((cls == BLANK).sum()), "n_blank_runs": int(blank_run.sum()),
         "first_blank": int(starts[blank_run][0]) if blank_run.any() else NO_PAGE,
         "n_holes": int(hole.sum()), "n_hole_pages": int(lengths[hole].sum()),
         "first_hole": int(starts[hole][0]) if hole.any() else NO_PAGE,
         "first_class": int(cls[0]), "last_class": int(cls[-1])}
    k = s["n_listed"]
    runs = np.zeros(k, dtype=RUN_DTYPE)
    runs["first_page"], runs["n_pages"], runs["cls"] = starts[:k], lengths[:k], run_cls[:k]
    return s, runs


def from_runs(pairs) -> np.ndarray:
    """[(class, length), ...] -> class array."""
    if not pairs:
        return np.zeros(0, dtype=np.uint8)
    return np.repeat(np.array([c for c, _ in pairs], dtype=np.uint8), [k for _, k in pairs])


def geometric(n: int, mean: float, seed: int, classes=(OK, OK, OK, BLANK, CORRUPT)) -> np.ndarray:
    """n class bytes in random runs of geometric length (adjacent runs may
    share a class and so form one run)."""
    rng = np.random.default_rng(seed)
    if n == 0:
        return np.zeros(0, dtype=np.uint8)
    lens = rng.geometric(1.0 / mean, size=max(4, int(2 * n / mean) + 16))
    while lens.sum() < n:
        lens = np.concatenate((lens, rng.geometric(1.0 / mean, size=lens.size)))
    c = rng.choice(np.array(classes, dtype=np.uint8), size=lens.size)
    return np.repeat(c, lens)[:n].copy()
