"""Reference for the manifest replay and the liveness-aware scrub: a varint
encoder, builders of snapshot and log payloads on top of manifest_ref.Builder
(the layout ManifestBuilder writes, src/storage/root_meta.cpp:29-105), a
SEQUENTIAL decoder that follows the decode rules of include/eloqstore_pcs.h
byte by byte (after Replayer::Replay, src/replayer.cpp:27-72, 142-228, and
src/coding.cpp:141-201), and replay() / scrub_live() returning arrays in the
ABI's dtypes."""
import struct

import numpy as np

import manifest_ref as mref

NO = (1 << 64) - 1
M64 = (1 << 64) - 1
INVALID = 7  # MappingSnapshot::InvalidValue
NO_OWNER = 0xFFFFFFFF
OK, NOT_REPLAYABLE, MALFORMED, TABLE_CAP = range(4)

REPORT_FIELDS = ("status", "n_replayed", "malformed_record", "root", "ttl_root", "max_fp_id", "dict_bytes",
                 "snapshot_pages", "n_log_entries", "table_size", "table_first", "n_mapped", "min_fp", "max_fp",
                 "n_fp_beyond_max", "n_term_pairs")
REPORT_DTYPE = np.dtype([(k, "<u8") for k in REPORT_FIELDS])
SUMMARY_DTYPE = np.dtype([("n_images", "<u8"), ("n_by_status", "<u8", (4,)), ("n_rows", "<u8"),
                          ("n_rows_written", "<u8"), ("n_mapped", "<u8"), ("n_log_entries", "<u8"),
                          ("first_bad_image", "<u8"), ("invalid_image", "<u8"), ("reserved", "<u8")])
LIVE_PAGE_DTYPE = np.dtype([("index", "<u8"), ("page_id", "<u4"), ("cls", "<u4")])
LIVE_FIELDS = ("n_pages", "table_size", "n_mapped", "n_mapped_in_window", "n_duplicate", "live_ok", "live_blank",
               "live_corrupt", "dead_ok", "dead_blank", "dead_corrupt", "n_damaged", "first_damaged", "last_live",
               "n_listed", "reserved")
LIVE_SUMMARY_DTYPE = np.dtype([(k, "<u8") for k in LIVE_FIELDS])


class Malformed(Exception):
    pass


# ---- encoder -------------------------------------------------------------------
def varint(v: int, length: int | None = None, top: int = 0) -> bytes:
    """v in little-endian base 128.  length pads with zero groups up to that
    many bytes (a non-canonical but legal encoding); top is OR'ed into the last
    byte's payload bits (bits that wrap away in a 10- or 5-byte varint)."""
    out = []
    while True:
        b = v & 0x7F
        v >>= 7
        if v or (length is not None and len(out) + 1 < length):
            out.append(b | 0x80)
        else:
            out.append((b | top) & 0x7F)
            break
    return bytes(out)


def fp(file_page_id: int) -> int:
    """The mapping value of a file page."""
    return file_page_id << 3 | 1


def values_section(values) -> bytes:
    return b"".join(varint(v) for v in values)


def entries_section(entries) -> bytes:
    return b"".join(varint(p) + varint(v) for p, v in entries)


def term_section(pairs) -> bytes:
    return b"".join(varint(a) + varint(b) for a, b in pairs)


def snapshot_payload(max_fp_id: int, mapping: bytes, term: bytes = b"", dict_bytes: bytes = b"",
                     trailer: bytes = b"") -> bytes:
    return (varint(max_fp_id) + varint(len(dict_bytes)) + dict_bytes + struct.pack("<I", len(mapping)) + mapping +
            struct.pack("<I", len(term)) + term + trailer)


def log_payload(mapping: bytes, term: bytes = b"", trailer: bytes = b"") -> bytes:
    return struct.pack("<I", len(mapping)) + mapping + struct.pack("<I", len(term)) + term + trailer


def manifest(max_fp_id, values, logs=(), align: int = 4096, dict_bytes: bytes = b"", term=()) -> bytearray:
    """A healthy manifest: a snapshot of `values` and one log record per entry list."""
    b = mref.Builder(align)
    b.add(snapshot_payload(max_fp_id, values_section(values), term_section(term), dict_bytes), root=11, ttl_root=12)
    for k, entries in enumerate(logs):
        b.add(log_payload(entries_section(entries)), root=100 + k, ttl_root=200 + k)
    return b.data()


# ---- sequential decoder -----------------------------------------------------------
def read_varint(buf: bytes, pos: int, end: int, limit: int):
    """-> (value before any mod, next pos); Malformed when it does not end
    within `limit` bytes or before `end`."""
    v = 0
    for n in range(limit):
        if pos >= end:
            raise Malformed("varint leaves its section")
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << (7 * n)
        if b < 0x80:
            return v, pos
    raise Malformed("varint too long")


def read_section64(buf: bytes, pos: int, end: int):
    out = []
    while pos < end:
        v, pos = read_varint(buf, pos, end, 10)
        out.append(v & M64)
    return out


def read_term(buf: bytes, pos: int, end: int) -> int:
    vals = read_section64(buf, pos, end)
    if len(vals) % 2:
        raise Malformed("odd term count")
    return len(vals) // 2


def decode_snapshot(p: bytes):
    """-> (max_fp_id, dict_len, table values, term pairs)."""
    L = len(p)
    max_fp, pos = read_varint(p, 0, L, 10)
    max_fp &= M64
    dict_len, pos = read_varint(p, pos, L, 5)
    dict_len &= 0xFFFFFFFF
    if dict_len > L - pos:
        raise Malformed("dict_len")
    pos += dict_len
    rem = L - pos
    if rem < 8:
        raise Malformed("mapping_len")
    (mlen,) = struct.unpack_from("<I", p, pos)
    if mlen + 8 > rem:
        raise Malformed("mapping_len")
    values = read_section64(p, pos + 4, pos + 4 + mlen)
    (tlen,) = struct.unpack_from("<I", p, pos + 4 + mlen)
    if tlen > rem - mlen - 8:
        raise Malformed("term_len")
    pairs = read_term(p, pos + 8 + mlen, pos + 8 + mlen + tlen)
    return max_fp, dict_len, values, pairs


def decode_log(p: bytes):
    """-> (entries [(page_id, value)], term pairs)."""
    L = len(p)
    if L < 8:
        raise Malformed("short log")
    (mlen,) = struct.unpack_from("<I", p, 0)
    if mlen + 8 > L:
        raise Malformed("mapping_len")
    pos, end, entries = 4, 4 + mlen, []
    while pos < end:
        pid, pos = read_varint(p, pos, end, 5)
        if pos >= end:
            raise Malformed("odd count")
        v, pos = read_varint(p, pos, end, 10)
        entries.append((pid & 0xFFFFFFFF, v & M64))
    (tlen,) = struct.unpack_from("<I", p, 4 + mlen)
    if tlen > L - mlen - 8:
        raise Malformed("term_len")
    pairs = read_term(p, 8 + mlen, 8 + mlen + tlen)
    return entries, pairs


def replay_image(img, align: int = 4096):
    """-> (report dict without table_first, table list or None)."""
    img = bytes(img)
    rep, recs = mref.report(img, align)
    r = {k: 0 for k in REPORT_FIELDS}
    r["malformed_record"] = r["min_fp"] = r["max_fp"] = NO
    if rep["verdict"] not in (mref.CLEAN, mref.TORN_TAIL):
        r["status"] = NOT_REPLAYABLE
        return r, None
    n_rep = rep["n_records"] if rep["first_corrupt"] == NO else rep["first_corrupt"]
    r["n_replayed"] = n_rep
    payloads = [img[x["offset"] + mref.HEADER:x["offset"] + mref.HEADER + x["payload_len"]] for x in recs[:n_rep]]
    # every replayed record is decoded: malformed_record is the LOWEST record with a violation
    decoded, bad = [], None
    for k, p in enumerate(payloads):
        try:
            decoded.append(decode_snapshot(p) if k == 0 else decode_log(p))
        except Malformed:
            bad = k
            break
    if bad is not None:
        r["status"] = MALFORMED
        r["malformed_record"] = bad
        return r, None
    max_fp, dict_len, table, pairs = decoded[0]
    table = list(table)
    snap = len(table)
    n_entries = 0
    for entries, tp in decoded[1:]:
        pairs += tp
        for pid, v in entries:
            n_entries += 1
            if pid >= len(table):
                table += [INVALID] * (pid + 1 - len(table))
            table[pid] = v
            if v & 7 == 1:
                max_fp = max(max_fp, (v >> 3) + 1)
    r.update(root=recs[n_rep - 1]["root"], ttl_root=recs[n_rep - 1]["ttl_root"], max_fp_id=max_fp,
             dict_bytes=dict_len, snapshot_pages=snap, n_log_entries=n_entries, table_size=len(table),
             n_term_pairs=pairs)
    ids = [v >> 3 for v in table if v & 7 == 1]
    r["n_mapped"] = len(ids)
    if ids:
        r["min_fp"], r["max_fp"] = min(ids), max(ids)
    r["n_fp_beyond_max"] = sum(1 for i in ids if i >= max_fp)
    return r, table


def replay(images, align: int = 4096, table_cap: int = 1 << 40):
    """-> (reports, summary, table rows written) in the ABI's dtypes."""
    reps, rows, first = [], [], 0
    for img in images:
        r, table = replay_image(img, align)
        r["table_first"] = first
        if r["status"] == OK:
            if first + r["table_size"] > table_cap:
                r["status"] = TABLE_CAP
                r["n_mapped"], r["min_fp"], r["max_fp"], r["n_fp_beyond_max"] = 0, NO, NO, 0
            else:
                rows += table
            first += r["table_size"]
        reps.append(r)
    out = np.zeros(len(reps), REPORT_DTYPE)
    for i, r in enumerate(reps):
        for k in REPORT_FIELDS:
            out[i][k] = r[k]
    s = np.zeros(1, SUMMARY_DTYPE)[0]
    s["n_images"] = len(images)
    for r in reps:
        s["n_by_status"][r["status"]] += 1
    counted = [r for r in reps if r["status"] in (OK, TABLE_CAP)]
    s["n_rows"] = sum(r["table_size"] for r in counted)
    s["n_rows_written"] = len(rows)
    s["n_mapped"] = sum(r["n_mapped"] for r in reps)
    s["n_log_entries"] = sum(r["n_log_entries"] for r in counted)
    bad = [i for i, r in enumerate(reps) if r["status"] != OK]
    s["first_bad_image"] = bad[0] if bad else NO
    s["invalid_image"] = NO
    return out, s, np.array(rows, dtype=np.uint64)


# ---- scrub live ---------------------------------------------------------------------
def scrub_live(cls, fp_first: int, table, damaged_cap: int = 1 << 40):
    """-> (owner uint32 array, summary, damaged pages) in the ABI's dtypes."""
    cls = np.asarray(cls, dtype=np.uint8)
    table = np.asarray(table, dtype=np.uint64)
    n = cls.size
    owner = np.full(n, NO_OWNER, dtype=np.uint32)
    mapped = (table & np.uint64(7)) == 1
    ids = table >> np.uint64(3)
    inside = mapped & (ids >= np.uint64(fp_first)) & (ids < np.uint64(fp_first + n))
    rows = np.nonzero(inside)[0]
    # descending rows, so that the lowest row writes last
    for p in rows[::-1]:
        owner[int(ids[p]) - fp_first] = p
    live = owner != NO_OWNER
    s = np.zeros(1, LIVE_SUMMARY_DTYPE)[0]
    s["n_pages"], s["table_size"] = n, table.size
    s["n_mapped"], s["n_mapped_in_window"] = int(mapped.sum()), int(inside.sum())
    s["n_duplicate"] = int(inside.sum()) - int(live.sum())
    for name, c in (("ok", 1), ("blank", 2), ("corrupt", 0)):
        s["live_" + name] = int((live & (cls == c)).sum())
        s["dead_" + name] = int((~live & (cls == c)).sum())
    dam = np.nonzero(live & (cls != 1))[0]
    s["n_damaged"] = dam.size
    s["first_damaged"] = int(dam[0]) if dam.size else NO
    lv = np.nonzero(live)[0]
    s["last_live"] = int(lv[-1]) if lv.size else NO
    s["n_listed"] = min(dam.size, damaged_cap)
    pages = np.zeros(int(s["n_listed"]), LIVE_PAGE_DTYPE)
    for j, i in enumerate(dam[:damaged_cap]):
        pages[j] = (int(i), int(owner[i]), int(cls[i]))
    return owner, s, pages
