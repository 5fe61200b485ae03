"""Reference per-file scrub reports (numpy): what pcs_scrub_files_dev /
pcs_pages_scrub_files_host must return for a batch's class and type bytes cut
at file boundaries.

Nothing but slicing: a file's counting fields are scrub_ref.summarize on its
slice, its written extent and holes extent_ref.extents on the same slice, both
file-local; the totals are sums over the reports.
"""
import numpy as np

import extent_ref
import scrub_ref

NO_PAGE = (1 << 64) - 1
REPORT_FIELDS = ("first_page", "n_pages", "n_ok", "n_corrupt", "n_blank", "ok_by_type", "first_corrupt",
                 "written_pages", "n_holes", "n_hole_pages", "first_hole")
SUMMARY_FIELDS = ("n_files", "n_pages", "n_ok", "n_corrupt", "n_blank", "n_corrupt_files", "n_hole_files",
                  "n_bad_files", "n_unwritten_files", "first_bad_file", "n_listed", "invalid_file")
REPORT_DTYPE = np.dtype([("first_page", "<u8"), ("n_pages", "<u8"), ("n_ok", "<u8"), ("n_corrupt", "<u8"),
                         ("n_blank", "<u8"), ("ok_by_type", "<u8", (6,)), ("first_corrupt", "<u8"),
                         ("written_pages", "<u8"), ("n_holes", "<u8"), ("n_hole_pages", "<u8"), ("first_hole", "<u8")])


def report(cls, types, first_page: int, end_page: int) -> dict:
    """The report of the file that is pages [first_page, end_page) of the batch."""
    c, t = cls[first_page:end_page], types[first_page:end_page]
    s, _ = scrub_ref.summarize(c, t, corrupt_cap=0)
    e, _ = extent_ref.extents(c, run_cap=0)
    return {"first_page": int(first_page), "n_pages": int(end_page - first_page), "n_ok": s["n_ok"],
            "n_corrupt": s["n_corrupt"], "n_blank": s["n_blank"], "ok_by_type": s["ok_by_type"],
            "first_corrupt": s["first_corrupt"], "written_pages": e["written_pages"], "n_holes": e["n_holes"],
            "n_hole_pages": e["n_hole_pages"], "first_hole": e["first_hole"]}


def invalid_file(first, n_pages: int):
    """The first f with first[f] > first[f + 1] or first[f + 1] > n_pages, None when the boundaries are valid."""
    for f in range(len(first) - 1):
        if int(first[f]) > int(first[f + 1]) or int(first[f + 1]) > n_pages:
            return f
    return None


def files(cls, types, first, bad_cap: int = 1024):
    """cls, types: uint8 arrays; first: n_files + 1 page boundaries ->
    (list of report dicts, summary dict, uint64 array of the listed bad files).
    Invalid boundaries: no report, every summary word 0 but n_files and invalid_file."""
    cls = np.ascontiguousarray(cls, dtype=np.uint8).reshape(-1)
    types = np.ascontiguousarray(types, dtype=np.uint8).reshape(-1)
    n_files = len(first) - 1
    s = dict.fromkeys(SUMMARY_FIELDS, 0)
    s["n_files"] = n_files
    inv = invalid_file(first, int(cls.size))
    if inv is not None:
        s["invalid_file"] = inv
        return [], s, np.zeros(0, dtype=np.uint64)
    reps = [report(cls, types, int(first[f]), int(first[f + 1])) for f in range(n_files)]
    bad = [f for f, r in enumerate(reps) if r["n_corrupt"] or r["n_holes"]]
    for k in ("n_pages", "n_ok", "n_corrupt", "n_blank"):
        s[k] = sum(r[k] for r in reps)
    s.update(n_corrupt_files=sum(1 for r in reps if r["n_corrupt"]), n_hole_files=sum(1 for r in reps if r["n_holes"]),
             n_bad_files=len(bad), n_unwritten_files=sum(1 for r in reps if r["written_pages"] == 0),
             first_bad_file=bad[0] if bad else NO_PAGE, n_listed=min(len(bad), bad_cap), invalid_file=NO_PAGE)
    return reps, s, np.array(bad[:bad_cap], dtype=np.uint64)


def as_records(reps) -> np.ndarray:
    """Report dicts as the structured array the binding returns."""
    out = np.zeros(len(reps), dtype=REPORT_DTYPE)
    for i, r in enumerate(reps):
        for k in REPORT_FIELDS:
            out[i][k] = r[k]
    return out


def even_cut(n_pages: int, pages_per_file: int) -> np.ndarray:
    """Boundaries of equal-size files, the last one short."""
    return np.append(np.arange(0, n_pages, pages_per_file, dtype=np.uint64), np.uint64(n_pages))
