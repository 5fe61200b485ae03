"""Reference for the manifest scan: a pure-Python walker over manifest images
(the walk rule of include/eloqstore_pcs.h, after Replayer::ParseNextRecord,
src/replayer.cpp:74-140), records checked with oracle.manifest_checksum (the
reference's xxhash.c), a builder that writes images record by record the way
ManifestBuilder::Finalize does (header, payload, checksum, pad to align), and
the text of the reference's tools/manifest_check_tool.cpp."""
import struct

import numpy as np

import oracle

NO = (1 << 64) - 1
HEADER = 20
END_CLEAN, END_SHORT_HEADER, END_SHORT_PAYLOAD, END_SHORT_PADDING = range(4)
CLEAN, TORN_TAIL, BROKEN, BAD_SNAPSHOT, EMPTY = range(5)
VERDICT_NAMES = ("clean", "torn-tail", "broken", "bad-snapshot", "empty")

RECORD_DTYPE = np.dtype([("offset", "<u8"), ("stored", "<u8"), ("computed", "<u8"), ("payload_len", "<u4"),
                         ("root", "<u4"), ("ttl_root", "<u4"), ("ok", "<u4")])
REPORT_FIELDS = ("size", "n_records", "n_ok", "n_corrupt", "first_corrupt", "n_ok_after_corrupt",
                 "valid_prefix_bytes", "end_offset", "end_reason", "verdict", "first_record", "max_record_bytes")
REPORT_DTYPE = np.dtype([(k, "<u8") for k in REPORT_FIELDS])
SUMMARY_DTYPE = np.dtype([("n_images", "<u8"), ("n_records", "<u8"), ("n_ok", "<u8"), ("n_corrupt", "<u8"),
                          ("n_by_verdict", "<u8", (5,)), ("first_bad_image", "<u8"), ("n_listed", "<u8"),
                          ("invalid_image", "<u8")])


def round_up(v: int, align: int) -> int:
    return (v + align - 1) // align * align


# ---- builder -----------------------------------------------------------------
def record(payload: bytes, root: int = 0, ttl_root: int = 0) -> bytes:
    """One record, unpadded: checksum | root | ttl_root | len | payload."""
    body = struct.pack("<III", root, ttl_root, len(payload)) + bytes(payload)
    return struct.pack("<Q", oracle.manifest_checksum(body)) + body


def payload(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


class Builder:
    """Appends records at multiples of align; data() is the image so far."""

    def __init__(self, align: int = 4096):
        self.align = align
        self.buf = bytearray()
        self.offsets = []  # start of every record appended

    def add(self, payload_bytes: bytes, root: int = 0, ttl_root: int = 0) -> int:
        rec = record(payload_bytes, root, ttl_root)
        off = len(self.buf)
        self.offsets.append(off)
        self.buf += rec
        self.buf += b"\0" * (round_up(len(self.buf), self.align) - len(self.buf))
        return off

    def add_random(self, n: int, seed: int) -> int:
        return self.add(payload(n, seed), root=seed & 0xFFFFFFFF, ttl_root=(seed * 7 + 1) & 0xFFFFFFFF)

    def data(self) -> bytearray:
        return bytearray(self.buf)


def image(lens, seed: int = 1, align: int = 4096) -> bytearray:
    b = Builder(align)
    for k, n in enumerate(lens):
        b.add_random(n, seed * 1000 + k)
    return b.data()


# ---- walker --------------------------------------------------------------------
def walk(img, align: int = 4096):
    """-> (records: list of dicts, end_offset, end_reason)."""
    img = bytes(img)
    size, o, recs = len(img), 0, []
    while True:
        if o == size:
            return recs, o, END_CLEAN
        if size - o < HEADER:
            return recs, o, END_SHORT_HEADER
        stored, root, ttl, ln = struct.unpack_from("<QIII", img, o)
        e = o + HEADER + ln
        if e > size:
            return recs, o, END_SHORT_PAYLOAD
        computed = oracle.manifest_checksum(img[o + 8:e])
        recs.append({"offset": o, "stored": stored, "computed": computed, "payload_len": ln, "root": root,
                     "ttl_root": ttl, "ok": int(stored == computed)})
        o2 = round_up(e, align)
        if o2 > size:
            return recs, size, END_SHORT_PADDING
        o = o2


def verdict_of(flags) -> int:
    if not flags:
        return EMPTY
    if not flags[0]:
        return BAD_SNAPSHOT
    if all(flags):
        return CLEAN
    first = flags.index(0)
    return BROKEN if any(flags[first:]) else TORN_TAIL


def report(img, align: int = 4096, first_record: int = 0):
    recs, end_off, reason = walk(img, align)
    flags = [r["ok"] for r in recs]
    fc = flags.index(0) if 0 in flags else NO
    rep = {"size": len(img), "n_records": len(recs), "n_ok": sum(flags), "n_corrupt": len(flags) - sum(flags),
           "first_corrupt": fc, "n_ok_after_corrupt": 0 if fc == NO else sum(flags[fc:]),
           "valid_prefix_bytes": end_off if fc == NO else recs[fc]["offset"], "end_offset": end_off,
           "end_reason": reason, "verdict": verdict_of(flags), "first_record": first_record,
           "max_record_bytes": max((HEADER + r["payload_len"] for r in recs), default=0)}
    return rep, recs


def scan(images, align: int = 4096, record_cap: int = 1 << 30):
    """-> (reports, summary, records) as structured arrays, records capped."""
    reps, recs = [], []
    for img in images:
        rep, rs = report(img, align, len(recs))
        reps.append(rep)
        recs += rs
    s = np.zeros(1, SUMMARY_DTYPE)[0]
    s["n_images"] = len(images)
    s["n_records"] = len(recs)
    s["n_ok"] = sum(r["n_ok"] for r in reps)
    s["n_corrupt"] = sum(r["n_corrupt"] for r in reps)
    for r in reps:
        s["n_by_verdict"][r["verdict"]] += 1
    bad = [i for i, r in enumerate(reps) if r["verdict"] != CLEAN]
    s["first_bad_image"] = bad[0] if bad else NO
    s["n_listed"] = min(len(recs), record_cap)
    s["invalid_image"] = NO
    return as_reports(reps), s, as_records(recs[:record_cap])


def as_reports(reps) -> np.ndarray:
    out = np.zeros(len(reps), REPORT_DTYPE)
    for i, r in enumerate(reps):
        for k in REPORT_FIELDS:
            out[i][k] = r[k]
    return out


def as_records(recs) -> np.ndarray:
    out = np.zeros(len(recs), RECORD_DTYPE)
    for i, r in enumerate(recs):
        for k in RECORD_DTYPE.names:
            out[i][k] = r[k]
    return out


# ---- layout ----------------------------------------------------------------------
def pack(images, align: int = 4096):
    """Images back to back at multiples of align -> (uint8 array, offsets, sizes)."""
    offs, total = [], 0
    for img in images:
        offs.append(total)
        total += round_up(len(img), align)
    buf = np.zeros(max(total, 1), np.uint8)
    for o, img in zip(offs, images):
        buf[o:o + len(img)] = np.frombuffer(bytes(img), np.uint8)
    return buf[:total] if total else buf[:0], offs, [len(i) for i in images]


def invalid_image(offs, sizes, total: int, align: int):
    """First image that breaks a layout rule, or None."""
    for i, (o, s) in enumerate(zip(offs, sizes)):
        if o % align or o + s > total:
            return i
        if i and o < round_up(offs[i - 1] + sizes[i - 1], align):
            return i
    return None


# ---- tools/manifest_check_tool.cpp ---------------------------------------------------
def tool_text(path: str, img, align: int = 4096):
    """-> (stdout, stderr, exit code) of the reference tool on a file holding img."""
    img = bytes(img)
    recs, end_off, reason = walk(img, align)
    out = ""
    for k, r in enumerate(recs):
        out += f"Log #{k} at offset {r['offset']}\n  record size: {HEADER + r['payload_len']}\n"
        out += f"  root: {r['root']}\n  ttl_root: {r['ttl_root']}\n  payload_bytes: {r['payload_len']}\n"
        out += f"  checksum: {'OK' if r['ok'] else 'FAILED'}\n"
        if not r["ok"]:
            out += f"  payload_hex: {img[r['offset'] + HEADER:r['offset'] + HEADER + r['payload_len']].hex()}\n"
    if reason == END_SHORT_HEADER:
        return out, f"Manifest truncated while reading header at offset {end_off}\n", 1
    if reason == END_SHORT_PAYLOAD:
        return out, f"Manifest truncated while reading payload at offset {end_off + HEADER}\n", 1
    if not recs:
        return out, f"No manifest logs found in {path}\n", 1
    return out + f"Parsed {len(recs)} logs from {path}\n", "", 2 if any(not r["ok"] for r in recs) else 0


def tool_line(path: str, img, align: int = 4096) -> str:
    rep, _ = report(img, align)
    return (f"{path}: records {rep['n_records']} corrupt {rep['n_corrupt']} verdict {VERDICT_NAMES[rep['verdict']]} "
            f"valid_prefix_bytes {rep['valid_prefix_bytes']}\n")


def tool_exit(images, align: int = 4096, unreadable: bool = False) -> int:
    v = [report(i, align)[0]["verdict"] for i in images]
    if BROKEN in v or BAD_SNAPSHOT in v:
        return 2
    if TORN_TAIL in v:
        return 3
    return 1 if EMPTY in v or unreadable else 0
