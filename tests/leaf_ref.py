"""CPU model of the leaf check (pcs_leaf_check_dev), written from the page
formats (data page: DataPageBuilder / DataPageIter; overflow page and
WriteOverflowValue's grouping) and from the walk's rules in
include/eloqstore_pcs.h:

  DataPageBuilder    a port of DataPageBuilder::Add / Finish (restart interval,
                     overflow, expire and compression bits, timestamps)
  overflow_page      the overflow-page constructor
  write_overflow_value   WriteOverflowValue's grouping for a given overflow_pointers
  iter_ref           DataPageIter::ParseNextKey step by step, sequentially
  decode_strict      the strict page rule, sequentially
  check              a plain walk -> leaves, summary, problems in the ABI's dtypes
  Forest             builds on tree_ref.Forest: data pages under a leaf-index root
  violations / control_pages   one page per rule of the strict rule, and its neighbour
  fuzz_page / fuzz_fold   the pages and the fold of tests/cpp/leaf_logic_test.cpp
  forests            the generated forests of tests/test_gpu_leaf_check.py
"""
import numpy as np

import tree_ref as tr
from tree_ref import M64, NO, NO64, GOLD, Rng, le16, le32, varint, fp

DATA, OVERFLOW = tr.DATA, tr.OVERFLOW
UNMAPPED, ABSENT, BLANK, CORRUPT, WRONG_TYPE, MALFORMED = (1 << k for k in range(6))
BAD_POINTER, BAD_CHAIN, SHARED = 64, 128, 256
SIX = 0x3F
HEADER = 19
MAX_POINTERS = 128
MAX_GROUPS = 4096
F_OVERFLOW, F_EXPIRE, F_COMPRESSION = 1, 2, 12

NODE_DTYPE = np.dtype([("owner", "<u4"), ("owner_entry", "<u2"), ("bits", "<u2"), ("a", "<u4"), ("b", "<u4")])
PROBLEM_DTYPE = np.dtype([("page_id", "<u4"), ("owner", "<u4"), ("bits", "<u4"), ("owner_entry", "<u4")])
SUMMARY_DTYPE = np.dtype([
    ("n_pages", "<u8"), ("table_size", "<u8"), ("n_data_pages", "<u8"), ("n_data_ok", "<u8"), ("n_entries", "<u8"),
    ("n_overflow_values", "<u8"), ("n_expiring", "<u8"), ("n_compressed", "<u8"), ("inline_value_bytes", "<u8"),
    ("overflow_value_bytes", "<u8"), ("n_refs", "<u8"), ("n_out_of_range_refs", "<u8"), ("n_extra_refs", "<u8"),
    ("n_refs_to_tree", "<u8"), ("n_misplaced_pointers", "<u8"), ("n_chain_capped", "<u8"), ("max_groups", "<u8"),
    ("n_overflow_pages", "<u8"), ("n_by_bit", "<u8", (9,)), ("n_problems", "<u8"), ("first_problem", "<u8"),
    ("n_listed", "<u8"), ("n_leaked_overflow", "<u8"), ("n_overflow_ok", "<u8")])


def zigzag(delta):
    return delta << 1 if delta >= 0 else ((-delta) << 1) | 1


def unzigzag(v):
    return -(v >> 1) if v & 1 else v >> 1


# ---- the builders -------------------------------------------------------------------------
class DataPageBuilder:
    """DataPageBuilder: add() returns False when the pair does not fit (the page is then unchanged)."""

    def __init__(self, P, interval=16):
        self.P, self.interval = P, interval
        self.buf = bytearray(HEADER)
        self.buf[8] = DATA
        self.restarts = [HEADER]
        self.counter = self.cnt = self.last_ts = 0
        self.last_key = b""

    def add(self, key, value, overflow=False, ts=0, expire_ts=0, compression=0):
        assert compression < 3
        stored = len(value) << 4 | int(overflow) | compression << 2 | (2 if expire_ts else 0)
        restart = self.counter >= self.interval
        shared = 0
        last_ts = 0 if restart else self.last_ts
        if not restart:
            m = min(len(self.last_key), len(key))
            while shared < m and self.last_key[shared] == key[shared]:
                shared += 1
        ts = min(ts, (1 << 63) - 1)
        entry = varint(shared) + varint(len(key) - shared) + varint(stored) + key[shared:] + bytes(value)
        if expire_ts:
            entry += varint(expire_ts)
        entry += varint(zigzag(ts - last_ts))
        if len(self.buf) + 2 * len(self.restarts) + 2 + (2 if restart else 0) + len(entry) > self.P:
            return False
        if restart:
            self.restarts.append(len(self.buf))
            self.counter = 0
        self.buf += entry
        self.last_key, self.last_ts = key, ts
        self.counter += 1
        self.cnt += 1
        return True

    def finish(self, prev=NO, nxt=NO, pad=0):
        buf = bytearray(self.buf)
        for r in self.restarts:
            buf += le16(r)
        buf += le16(len(self.restarts))
        buf[9:11] = le16(len(buf))
        buf[11:15], buf[15:19] = le32(prev), le32(nxt)
        assert len(buf) <= self.P
        return bytes(buf) + bytes([pad]) * (self.P - len(buf))


def build_data_page(P, items, interval=16, prev=NO, nxt=NO):
    """items: (key, value, overflow, ts, expire_ts, compression) -> (page, how many fitted)."""
    b = DataPageBuilder(P, interval)
    added = 0
    for it in items:
        if not b.add(*it):
            break
        added += 1
    return b.finish(prev, nxt), added


def overflow_page(P, value, pointers=(), filler=0):
    """OverflowPage(page_id, opts, val, pointers)."""
    n = len(pointers)
    assert 11 + len(value) + 4 * n + 1 <= P and n <= 255
    page = bytearray([filler]) * P
    page[0:8] = bytes(8)
    page[8] = OVERFLOW
    page[9:11] = le16(len(value))
    page[11:11 + len(value)] = value
    page[P - 1] = n
    page[P - 1 - 4 * n:P - 1] = b"".join(le32(p) for p in pointers)
    return bytes(page)


def write_overflow_value(P, value, overflow_pointers, alloc):
    """WriteOverflowValue: (the entry's encoded pointers, {page id: page}); alloc() gives the next page id."""
    page_cap = P - 11 - 1
    end_cap = page_cap - 4 * overflow_pointers
    assert end_cap > 0 and value
    head, pages, end_id, page_val = b"", {}, None, b""
    while value:
        size = min((len(value) + page_cap - 1) // page_cap, overflow_pointers)
        pointers = [alloc() for _ in range(size)]
        if end_id is None:
            head = b"".join(le32(p) for p in pointers)
        else:
            pages[end_id] = overflow_page(P, page_val, pointers)
        for i, pg in enumerate(pointers, 1):
            if i == overflow_pointers and len(value) > page_cap:
                end_id, page_val, value = pg, value[:end_cap], value[end_cap:]
                break
            page_val, value = value[:page_cap], value[page_cap:]
            pages[pg] = overflow_page(P, page_val)
    return head, pages


# ---- decoding ---------------------------------------------------------------------------
def _varint64(page, pos, limit):
    v = 0
    for i in range(10):
        if pos >= limit:
            return None
        b = page[pos]
        pos += 1
        v |= (b & 0x7F) << (7 * i)
        if b < 0x80:
            return v & M64, pos
    return None


def iter_ref(page, P):
    """What DataPageIter yields over a page whose content length and restart count are taken from the
    page: (key, value, overflow, expire_ts, timestamp, compression) per ParseNextKey until it invalidates itself."""
    C = int.from_bytes(page[9:11], "little")
    R = int.from_bytes(page[C - 2:C], "little")
    E = C - 2 * (1 + R)
    restart = [int.from_bytes(page[E + 2 * k:E + 2 * k + 2], "little") for k in range(R)]
    out = []
    cur, idx, key, ts = 0, 0, b"", 0
    while True:
        if cur >= E:
            return out
        if cur < HEADER:
            cur = HEADER
        is_restart = idx < R and cur == restart[idx]
        if E - cur < 3:
            return out
        a = tr._varint32(page, cur, E)
        b = tr._varint32(page, a[1], E) if a else None
        c = tr._varint32(page, b[1], E) if b else None
        if not c:
            return out
        shared, non_shared, stored, pos = a[0], b[0], c[0], c[1]
        assert (stored >> 2) & 3 != 3        # the reference CHECKs
        vlen = stored >> 4
        if E - pos < non_shared + vlen or len(key) < shared:
            return out
        key = key[:shared] + bytes(page[pos:pos + non_shared])
        pos += non_shared
        value = bytes(page[pos:pos + vlen])
        pos += vlen
        expire = 0
        if stored & 2:
            x = _varint64(page, pos, E)
            if not x:
                return out
            expire, pos = x
        t = _varint64(page, pos, E)
        if not t:
            return out
        ts = unzigzag(t[0]) if is_restart else ts + unzigzag(t[0])
        cur = t[1]
        out.append((key, value, bool(stored & 1), expire, ts, (stored >> 2) & 3))
        if idx + 1 < R and cur >= restart[idx + 1]:
            idx += 1


def decode_strict(page, P):
    """The strict rule: the list of entries as dicts (offset, shared, non_shared, flags, value_offset,
    value_len, expire_ts, ts_raw, key, value, timestamp), or None when the page is malformed."""
    assert len(page) == P
    if P < 21:
        return None
    C = int.from_bytes(page[9:11], "little")
    if C < 21 or C > P:
        return None
    R = int.from_bytes(page[C - 2:C], "little")
    E = C - 2 * (1 + R)
    if E < HEADER or (R == 0 and E != HEADER):
        return None
    o = [int.from_bytes(page[E + 2 * k:E + 2 * k + 2], "little") for k in range(R)] + [E]
    if R and o[0] != HEADER:
        return None
    out = []
    for k in range(R):
        lo, hi = o[k], o[k + 1]
        if not (R == 1 and E == HEADER) and not lo < hi <= E:
            return None
        pos, key, ts, first = lo, b"", 0, True
        while pos < hi:
            start = pos
            a = tr._varint32(page, pos, hi)
            b = tr._varint32(page, a[1], hi) if a else None
            c = tr._varint32(page, b[1], hi) if b else None
            if not c or a[0] > len(key):
                return None
            shared, non_shared, stored, pos = a[0], b[0], c[0], c[1]
            flags, vlen = stored & 15, stored >> 4
            if flags & 12 == 12 or non_shared + vlen > hi - pos:
                return None
            key = key[:shared] + bytes(page[pos:pos + non_shared])
            voff = pos + non_shared
            pos = voff + vlen
            if flags & 1 and (vlen % 4 or not 4 <= vlen <= 4 * MAX_POINTERS):
                return None
            expire = 0
            if flags & 2:
                x = _varint64(page, pos, hi)
                if not x:
                    return None
                expire, pos = x
            t = _varint64(page, pos, hi)
            if not t:
                return None
            pos = t[1]
            ts = unzigzag(t[0]) if first else ts + unzigzag(t[0])
            first = False
            out.append(dict(offset=start, shared=shared, non_shared=non_shared, flags=flags, value_offset=voff,
                            value_len=vlen, expire_ts=expire, ts_raw=t[0], key=key, value=bytes(page[voff:voff + vlen]),
                            timestamp=ts))
    return out


def as_iter(entries):
    """decode_strict's entries in iter_ref's form."""
    return [(e["key"], e["value"], bool(e["flags"] & 1), e["expire_ts"], e["timestamp"], (e["flags"] >> 2) & 3)
            for e in entries]


def overflow_rule(page, P):
    """The intrinsic rule of a type-3 page: (V, n) or None."""
    n, V = page[P - 1], int.from_bytes(page[9:11], "little")
    return (V, n) if n <= MAX_POINTERS and 11 + V + 4 * n + 1 <= P else None


# ---- the walk -----------------------------------------------------------------------------
def check(pages, P, fp_first, cls, table, tree_nodes, cap=None):
    """(leaves, summary, problems) as pcs_leaf_check_dev writes them; tree_nodes are tree_ref.check's."""
    pages = np.asarray(pages, dtype=np.uint8).reshape(-1)
    cls = np.asarray(cls, dtype=np.uint8)
    table = [int(v) for v in np.asarray(table, dtype=np.uint64)]
    rows, n_pages = len(table), cls.size
    leaves = np.zeros(rows, dtype=NODE_DTYPE)
    leaves["owner"] = NO
    s = np.zeros(1, dtype=SUMMARY_DTYPE)[0]
    reached = [int(x) != NO for x in tree_nodes["parent"]] if rows else []

    def page_of(row):
        v = table[row]
        if v & 7 != 1:
            return None
        i = (v >> 3) - fp_first
        return i if 0 <= i < n_pages else -1

    def body(i):
        return bytes(pages[i * P:(i + 1) * P])

    memo = {}

    def classify(c):
        """(bit, V, n, pointers of the page)"""
        if c not in memo:
            i = page_of(c)
            if i is None:
                r = (UNMAPPED, 0, 0, ())
            elif i < 0 or cls[i] > 2:
                r = (ABSENT, 0, 0, ())
            elif cls[i] == 2:
                r = (BLANK, 0, 0, ())
            elif cls[i] == 0:
                r = (CORRUPT, 0, 0, ())
            else:
                b = body(i)
                rule = overflow_rule(b, P) if b[8] == OVERFLOW else None
                if b[8] != OVERFLOW:
                    r = (WRONG_TYPE, 0, 0, ())
                elif rule is None:
                    r = (MALFORMED, 0, 0, ())
                else:
                    V, n = rule
                    r = (0, V, n, [int.from_bytes(b[P - 1 - 4 * n + 4 * j:P - 1 - 4 * n + 4 * j + 4], "little")
                                   for j in range(n)])
            memo[c] = r
        return memo[c]

    key, refs = {}, {}
    cnt = dict.fromkeys(("n_entries", "n_overflow_values", "n_expiring", "n_compressed", "inline_value_bytes", "n_refs",
                         "n_out_of_range_refs", "n_refs_to_tree", "n_misplaced_pointers", "n_chain_capped",
                         "max_groups"), 0)
    checked = []
    for p in range(rows):
        t = tree_nodes[p]
        if not (reached[p] and int(t["type"]) == DATA and not int(t["bits"]) & SIX):
            continue
        checked.append(p)
        entries = decode_strict(body(page_of(p)), P)
        dbits = a = b = 0
        if entries is None:
            dbits = MALFORMED
        else:
            a = len(entries)
            for e in entries:
                cnt["n_entries"] += 1
                cnt["n_expiring"] += bool(e["flags"] & F_EXPIRE)
                cnt["n_compressed"] += bool(e["flags"] & F_COMPRESSION)
                if not e["flags"] & F_OVERFLOW:
                    cnt["inline_value_bytes"] += e["value_len"]
                    continue
                b += 1
                ekey = p << 32 | e["offset"] << 16
                v = e["value"]
                ptrs = [int.from_bytes(v[4 * j:4 * j + 4], "little") for j in range(len(v) // 4)]
                groups = 0
                while True:
                    if groups == MAX_GROUPS:
                        cnt["n_chain_capped"] += 1
                        dbits |= BAD_CHAIN
                        break
                    groups += 1
                    nxt = None
                    for j, c in enumerate(ptrs):
                        cnt["n_refs"] += 1
                        if c >= rows:
                            cnt["n_out_of_range_refs"] += 1
                            dbits |= BAD_POINTER
                        elif reached[c]:
                            cnt["n_refs_to_tree"] += 1
                            dbits |= BAD_CHAIN
                        else:
                            key[c] = min(key.get(c, ekey), ekey)
                            refs[c] = refs.get(c, 0) + 1
                            cb, V, n, pp = classify(c)
                            if cb:
                                dbits |= BAD_CHAIN
                            elif n:
                                if j + 1 != len(ptrs):
                                    cnt["n_misplaced_pointers"] += 1
                                    dbits |= BAD_CHAIN
                                else:
                                    nxt = pp
                    if nxt is None:
                        break
                    ptrs = nxt
                cnt["max_groups"] = max(cnt["max_groups"], groups)
        leaves[p] = (p, 0, dbits, a, b)
    for c, k in key.items():
        cb, V, n, pp = classify(c)
        r = refs[c] & 0xFFFFFFFF
        leaves[c] = (k >> 32, (k >> 16) & 0xFFFF, cb | (SHARED if r > 1 else 0), r, V | n << 16)
    s["n_pages"], s["table_size"] = n_pages, rows
    for k, v in cnt.items():
        s[k] = v
    s["n_overflow_values"] = int(sum(int(leaves[p]["b"]) for p in checked))
    s["n_data_pages"] = len(checked)
    s["n_data_ok"] = sum(1 for p in checked if not int(leaves[p]["bits"]))
    s["n_overflow_pages"] = len(key)
    s["overflow_value_bytes"] = sum(int(leaves[c]["b"]) & 0xFFFF for c in key if not int(leaves[c]["bits"]) & SIX)
    s["n_overflow_ok"] = sum(1 for c in key if not int(leaves[c]["bits"]))
    s["n_extra_refs"] = cnt["n_refs"] - cnt["n_out_of_range_refs"] - cnt["n_refs_to_tree"] - len(key)
    mine = np.zeros(rows, dtype=bool)
    mine[checked] = True
    mine[list(key)] = True
    for k in range(9):
        s["n_by_bit"][k] = int((mine & ((leaves["bits"] >> k) & 1 == 1)).sum())
    bad = np.nonzero(mine & (leaves["bits"] != 0))[0]
    s["n_problems"] = bad.size
    s["first_problem"] = int(bad[0]) if bad.size else NO64
    listed = bad if cap is None else bad[:cap]
    s["n_listed"] = listed.size
    problems = np.zeros(listed.size, dtype=PROBLEM_DTYPE)
    problems["page_id"] = listed
    for k in ("owner", "bits", "owner_entry"):
        problems[k] = leaves[k][listed]
    for p in range(rows):
        if mine[p] or reached[p]:
            continue
        i = page_of(p)
        if i is not None and i >= 0 and cls[i] == 1 and int(pages[i * P + 8]) == OVERFLOW:
            s["n_leaked_overflow"] += 1
    return leaves, s, problems


def model(case, cap=None, tree_cap=None):
    """(tree outputs, leaf outputs) of a case."""
    t = tr.check(case["pages"], case["P"], case["fp_first"], case["cls"], case["table"], case["roots"], tree_cap)
    return t, check(case["pages"], case["P"], case["fp_first"], case["cls"], case["table"], t[0], cap)


# ---- table and window assembler -------------------------------------------------------------
class Forest(tr.Forest):
    """A leaf-index root (row 0) over data pages, and the overflow pages their values name."""

    def __init__(self, P, fp_first=0, overflow_base=1000):
        super().__init__(P, fp_first)
        self.next_overflow = overflow_base
        self.data = []                      # (page id, DataPageBuilder)

    def alloc(self):
        self.next_overflow += 1
        return self.next_overflow - 1

    def large(self, size, overflow_pointers, seed=1):
        """Writes a value of `size` bytes into overflow pages -> the entry's encoded pointers."""
        value = Rng(seed * 7919 + size).words((size + 7) // 8).astype("<u8").tobytes()[:size]
        head, pages = write_overflow_value(self.P, value, overflow_pointers, self.alloc)
        for pid, page in pages.items():
            self.put(pid, page)
        return head

    def page(self, page_id, interval=16):
        b = DataPageBuilder(self.P, interval)
        self.data.append((page_id, b))
        return b

    def finish(self, extra_children=(), rows=None, roots=None):
        """Links the data pages in order, puts them and the root, and returns the case."""
        ids = [p for p, _ in self.data]
        for k, (p, b) in enumerate(self.data):
            self.put(p, b.finish(ids[k - 1] if k else NO, ids[k + 1] if k + 1 < len(ids) else NO))
        kids = ids + list(extra_children)
        per = tr.fanout(self.P) if self.P > 64 else 3
        if len(kids) <= per:
            self.put(0, tr.index_page(self.P, True, kids))
        else:                               # a non-leaf root over leaf-index pages in rows 1 .. 8
            leaves = list(range(1, 1 + (len(kids) + per - 1) // per))
            assert leaves[-1] < min(ids) and len(leaves) <= per
            for k, leaf in enumerate(leaves):
                self.put(leaf, tr.index_page(self.P, True, kids[k * per:(k + 1) * per]))
            self.put(0, tr.index_page(self.P, False, leaves))
        self.roots = [0, NO]
        return self.case(rows, roots)


def ptrs(*ids):
    return b"".join(le32(i) for i in ids)


# ---- violations of the strict rule --------------------------------------------------------------
def _raw(P, C, tail, body=b""):
    """A data page from its parts: header, body from offset 19, `tail` ending at C."""
    page = bytearray(P)
    page[8] = DATA
    page[9:11] = le16(C)
    page[11:15], page[15:19] = le32(NO), le32(NO)
    page[19:19 + len(body)] = body
    if 0 <= C - len(tail) and C <= P:
        page[C - len(tail):C] = tail
    return bytes(page)


def _one_region(P, body):
    return _raw(P, 19 + len(body) + 4, le16(19) + le16(1), body)


def entry(shared, key, value=b"", flags=0, ts=0, expire=None):
    out = varint(shared) + varint(len(key)) + varint(len(value) << 4 | flags) + key + value
    if expire is not None:
        out += varint(expire)
    return out + varint(ts)


def violations(P):
    """name -> (a page of P bytes (P >= 64) that breaks exactly the named rule, its well-formed neighbour that
    differs in one byte)."""
    a = entry(0, b"ab", b"xyz", 0, 6)
    good = a + entry(1, b"c", b"", 0, 2)
    first = len(a)
    two = lambda o0, o1, body=good: _raw(P, 19 + len(body) + 6, le16(o0) + le16(o1) + le16(2), body)  # noqa: E731
    ok2 = two(19, 19 + first, a + entry(0, b"c", b"", 0, 2))

    def edit(page, pos, byte):
        out = bytearray(page)
        out[pos] = byte
        return bytes(out)

    one = _one_region(P, good)
    C1 = 19 + len(good) + 4
    b_off = 19 + first                              # the second entry of `one`
    ov = _one_region(P, a + entry(1, b"c", ptrs(7), F_OVERFLOW, 2))
    ov2 = _one_region(P, a + entry(1, b"c", ptrs(7, 8), F_OVERFLOW, 2))
    ex = _one_region(P, a + entry(1, b"c", b"", F_EXPIRE, 2, expire=5))
    big = 4 * (MAX_POINTERS + 1)
    top = _raw(P, P - 1, le16(19) + le16(1))          # one region of all-zero entries (0, 0, 0 | ts 0), C = P - 1
    assert (P - 1 - 23) % 4 == 0 and (P - 1) >> 8 == (P + 1) >> 8
    three = _raw(P, 19 + 3 * first + 8, le16(19) + le16(19 + first) + le16(19 + 2 * first) + le16(3), a + a + a)
    v5 = _one_region(P, a + b"\x80\x80\x80\x80\x00\x01\x00c\x02")          # shared = 0 in five bytes
    v10 = _one_region(P, a + b"\x01\x01\x00c" + b"\x80" * 9 + b"\x00")       # timestamp 0 in ten bytes
    if P > big + 64:
        too_long = _one_region(P, a + entry(1, b"c", bytes(big), F_OVERFLOW, 2))
        # with 512 the four bytes left over are one more entry: 0, 0, 0 | ts 2
        long_pair = (too_long, edit(too_long, b_off + 2, (4 * MAX_POINTERS << 4 | F_OVERFLOW) & 0x7F | 0x80))
    else:                                            # no room for 516 bytes: seven bytes where eight were
        long_pair = (edit(ov2, b_off + 2, 7 << 4 | F_OVERFLOW), ov2)
    v = {
        # header
        "C=20": (edit(_raw(P, 21, le16(0)), 9, 20), _raw(P, 21, le16(0))),
        "C=P+1": (edit(top, 9, (P + 1) & 0xFF), top),
        "E<19": (edit(_raw(P, 21, le16(0)), 19, 1), _raw(P, 21, le16(0))),
        "R=0,E!=19": (edit(_raw(P, 23, le16(19) + le16(1)), 21, 0), _raw(P, 23, le16(19) + le16(1))),
        "o[0]!=19": (edit(one, C1 - 4, 20), one),
        "restarts equal": (edit(ok2, 19 + len(good) + 2, 19), ok2),
        "restarts descending": (edit(three, 19 + 3 * first + 2, 19 + 2 * first + 1), three),
        "o[R-1]>=E": (edit(ok2, 19 + len(good) + 2, 19 + len(good)), ok2),
        # entries
        "entry crosses in shared": (edit(one, b_off, 0x81), one),
        "entry crosses in non_shared": (edit(ok2, 19 + len(good) + 2, 19 + first + 1), ok2),
        "entry crosses in stored_len": (edit(ok2, 19 + len(good) + 2, 19 + first + 2), ok2),
        "key and value do not fit": (edit(one, b_off + 2, 0x10), one),
        "entry crosses in timestamp": (edit(one, C1 - 5, 0x82), one),
        "entry crosses in expire": (edit(ex, 19 + first + 4, 0x85), ex),
        "shared!=0 at restart": (edit(ok2, 19 + first, 1), ok2),
        "shared>previous key": (edit(one, b_off, 3), one),
        "6-byte varint32": (edit(v5, b_off + 4, 0x80), v5),
        "11-byte varint64": (edit(v10, b_off + 4 + 9, 0x80), v10),
        "compression bits 3": (edit(one, b_off + 2, 12), one),
        "overflow value_len%4": (edit(ov, b_off + 2, 5 << 4 | F_OVERFLOW), ov),
        "overflow value_len=0": (edit(one, b_off + 2, F_OVERFLOW), one),
        "overflow value_len>512": long_pair,
    }
    return v


def control_pages(P):
    """Well-formed pages that stand next to the violations -> (page, the iterator's entries)."""
    a = entry(0, b"ab", b"xyz", 0, 6)
    out = {
        "empty": _raw(P, 23, le16(19) + le16(1)),
        "one region": _one_region(P, a + entry(1, b"c", b"", 0, 2)),
        "two regions": _raw(P, 19 + len(a) * 2 + 6, le16(19) + le16(19 + len(a)) + le16(2), a + a),
        "overflow 1": _one_region(P, a + entry(1, b"c", ptrs(7), F_OVERFLOW, 2)),
        "expire and compression": _one_region(P, a + entry(2, b"", b"q", F_EXPIRE | 8, 3, expire=1 << 40)),
        "10-byte varint64": _one_region(P, a + b"\x01\x01\x00c" + b"\x80" * 9 + b"\x01"),
        "5-byte varint32": _one_region(P, a + b"\x80\x80\x80\x80\x10\x01\x00c\x02"),
    }
    if P >= 1000:
        out["overflow 128"] = _one_region(P, a + entry(1, b"c", ptrs(*range(128)), F_OVERFLOW, 2))
    return out


# ---- the fuzz of tests/cpp/leaf_logic_test.cpp ----------------------------------------------------
FUZZ_SIZES = (32, 64, 1000, 4096)
FUZZ_SEED = 20250311


def fuzz_writer(P, rng):
    """A well-formed data page written straight in the format from rng's draws."""
    buf = bytearray(HEADER)
    buf[8] = DATA
    interval = 1 + rng.next() % 17
    want = rng.next() % 48
    restarts = [HEADER]
    counter = prev_len = 0
    for _ in range(want):
        a = rng.next()
        key_len = 1 + (a >> 8) % 200 if a & 15 == 0 else 1 + (a >> 8) % 12
        restart = counter >= interval
        b = rng.next()
        shared = 0 if restart else b % (min(prev_len, key_len - 1) + 1)
        non_shared = key_len - shared
        c = rng.next()
        flags = (1 if c & 7 == 0 else 0) | (2 if (c >> 3) & 1 else 0) | (((c >> 4) % 3) << 2)
        if flags & 1:
            vlen = 4 * (1 + (c >> 8) % 128) if (c >> 6) & 3 == 0 else 4 * (1 + (c >> 8) % 4)
        else:
            vlen = (c >> 8) % 40
        e = bytearray(varint(shared) + varint(non_shared) + varint(vlen << 4 | flags))
        for j in range(non_shared + vlen):
            if j % 8 == 0:
                d = rng.next()
            e.append((d >> (8 * (j % 8))) & 0xFF)
        if flags & 2:
            x = rng.next()
            e += varint(x >> (x & 63))
        t = rng.next()
        e += varint(t >> (t & 63))
        if len(buf) + len(e) + 2 * (len(restarts) + (1 if restart else 0)) + 2 > P:
            break
        if restart:
            restarts.append(len(buf))
            counter = 0
        buf += e
        prev_len = key_len
        counter += 1
    for r in restarts:
        buf += le16(r)
    buf += le16(len(restarts))
    buf[9:11] = le16(len(buf))
    return buf + bytes(P - len(buf))


def fuzz_page(t, seed=FUZZ_SEED):
    """Case t of the fuzz -> (P, page): random bytes when (t >> 2) & 3 == 0, else a well-formed page with
    zero to two random byte edits."""
    rng = Rng(((seed + t) * 0xD6E8FEB86659FD93) & M64)
    P = FUZZ_SIZES[t % 4]
    if (t >> 2) & 3 == 0:
        return P, rng.words((P + 7) // 8).astype("<u8").tobytes()[:P]
    page = fuzz_writer(P, rng)
    for _ in range(rng.next() % 3):
        pos = rng.next() % P
        page[pos] = rng.next() & 0xFF
    return P, bytes(page)


ENTRY_FIELDS = ("offset", "shared", "non_shared", "flags", "value_offset", "value_len", "expire_ts", "ts_raw")


def fold_page(fold, entries):
    """One page's verdict and entries into the running fold."""
    fold = (fold * GOLD + (0 if entries is None else 1 + len(entries))) & M64
    for e in entries or ():
        for k in ENTRY_FIELDS:
            fold = (fold * GOLD + e[k]) & M64
    return fold


def fuzz_fold(n, seed=FUZZ_SEED):
    """(fold, well-formed pages) over cases 0 .. n."""
    fold = ok = 0
    for t in range(n):
        P, page = fuzz_page(t, seed)
        entries = decode_strict(page, P)
        ok += entries is not None
        fold = fold_page(fold, entries)
    return fold, ok


# ---- the forests of the GPU tests -------------------------------------------------------------------
def key_of(i):
    return b"k%05d" % i


def plain(P, fp_first=0, n_pages=3, interval=16):
    """Data pages filled to the brim with small values, some expiring, some compressed; no overflow."""
    f = Forest(P, fp_first)
    i = 0
    for d in range(n_pages):
        b = f.page(10 + d, interval)
        while b.add(key_of(i), b"v" * (i % 23), False, 1000 + 7 * i, (i % 3 == 0) * (5000 + i), i % 3):
            i += 1
            if b.cnt >= 400:
                break
    return f.finish()


def regions(P, R, fp_first=0):
    """One data page with restart interval 1 and R entries, overflow entries in regions 0, 63, 64 and the last
    (those that exist), each a one-group chain of 1, 2 or 3 pages; a second page without values."""
    f = Forest(P, fp_first)
    b = f.page(10, 1)
    cap = P - 12
    for i in range(R):
        if i in (0, 63, 64, R - 1):
            ok = b.add(key_of(i), f.large(1 + (i % 3) * cap, 4, i), True, 50 + i)
        else:
            ok = b.add(key_of(i), b"v" * (i % 3), False, 50 + i, (i % 5 == 0) * 9)
        assert ok, (P, R, i)
    assert len(b.restarts) == R
    f.page(11).add(b"zz", b"tail")
    return f.finish()


def groups(P, n, fp_first=0):
    """One value whose single group has n pointers (overflow_pointers = 128), next to a small one."""
    f = Forest(P, fp_first)
    b = f.page(10)
    cap = P - 12
    assert b.add(b"a", f.large((n - 1) * cap + 1, 128), True, 1)
    assert b.add(b"b", f.large(5, 128, 2), True, 2, 77)
    return f.finish()


def chains(P, fp_first=0):
    """Values of 1, 2 and 3 groups with overflow_pointers = 2, and a last group exactly full with and
    without a successor (overflow_pointers = 4)."""
    f = Forest(P, fp_first)
    cap, end2, end4 = P - 12, P - 12 - 8, P - 12 - 16
    b = f.page(10, 2)
    # overflow_pointers 2: one group of two; a full group and one page more; two full groups and one page more.
    # overflow_pointers 4: a group exactly full and no successor; one byte more: a successor; a second group
    # exactly full
    sizes = [(cap + 3, 2), (2 * cap + 1, 2), (3 * cap + end2 + 1, 2), (4 * cap, 4), (4 * cap + 1, 4),
             (3 * cap + end4 + 4 * cap, 4)]
    for i, (size, op) in enumerate(sizes):
        head = f.large(size, op, i)
        if not b.add(key_of(i), head, True, i):
            b = f.page(10 + i, 2)
            assert b.add(key_of(i), head, True, i)
    return f.finish()


def every_bit(P=1000, fp_first=(1 << 40) + 12345):
    """Every bit, every kind of chain page, both cycles, both orders of a shared page, the bad pointers."""
    f = Forest(P, fp_first, overflow_base=300)
    ov = lambda value=b"v", pointers=(): overflow_page(P, value, pointers)  # noqa: E731
    # chain pages of the six kinds: rows 100 .. 106
    f.value(100, tr.INVALID)                             # UNMAPPED
    f.value(101, fp(fp_first + 100000))                  # ABSENT: above the window
    f.put(102, ov(), cls=tr.CLASS_ABSENT)                # ABSENT: not loaded
    f.put(103, ov(), cls=2)                              # BLANK
    f.put(104, ov(), cls=0)                              # CORRUPT
    f.put(105, tr.typed_page(P, 255))                    # WRONG_TYPE: a deleted page
    bad = bytearray(ov())
    bad[P - 1] = 129
    f.put(106, bytes(bad))                               # MALFORMED: n > 128
    bad = bytearray(ov())
    bad[9:11] = le16(P - 15)
    bad[P - 1] = 1
    f.put(107, bytes(bad))                               # MALFORMED: 11 + V + 4 + 1 = P + 1
    f.put(108, overflow_page(P, bytes(P - 16), [109]))   # the control: 11 + V + 4 + 1 = P, and a second group
    f.put(109, ov())
    # cycles
    f.put(110, ov(b"c", [110]))                          # a one-page cycle
    f.put(111, ov(b"c", [112]))
    f.put(112, ov(b"c", [111]))                          # a two-page cycle
    # a page shared by two values: 120 (owner: the smaller key comes first), 121 (comes second)
    f.put(120, ov(b"shared"))
    f.put(121, ov(b"shared"))
    f.put(122, ov(b"own"))
    f.put(123, ov(b"own"))
    # a misplaced pointer array: 130 is first of two and has a pointer
    f.put(130, ov(b"m", [131]))
    f.put(131, ov(b"m"))
    f.put(132, ov(b"m"))
    # a chain page that points beyond the table and into the tree
    f.put(140, ov(b"p", [5000, 11, 141]))
    f.put(141, ov(b"p"))
    # leaked: mapped overflow pages nobody names; 151 is named only by a malformed data page
    f.put(150, ov(b"leak"))
    f.put(151, ov(b"leak"))
    f.put(152, ov(b"leak"), cls=0)                       # corrupt: not counted as leaked
    b = f.page(10, 2)
    for i, c in enumerate(range(100, 109)):
        assert b.add(key_of(i), ptrs(c), True, i)
    b = f.page(11, 3)
    assert b.add(b"a", ptrs(110), True, 1)
    assert b.add(b"b", ptrs(111), True, 2)
    assert b.add(b"c", ptrs(121, 122), True, 3)          # 121: this key is the larger of its two bidders
    assert b.add(b"d", ptrs(120), True, 4, 99)
    assert b.add(b"e", b"inline", False, 5, 0, 1)
    b = f.page(12)
    assert b.add(b"a", ptrs(120, 123), True, 1)          # 120 again, from a larger page id
    assert b.add(b"b", ptrs(130, 132), True, 2)
    assert b.add(b"c", ptrs(4000), True, 3)              # beyond the table
    assert b.add(b"d", ptrs(0, 10, 132), True, 4)        # the index root and a data page
    assert b.add(b"e", ptrs(140), True, 5)
    b = f.page(9)                                        # later in the index order, smaller id: wins 121
    assert b.add(b"a", ptrs(121), True, 1)
    f.page(13).add(b"healthy", f.large(3 * (P - 12), 8), True, 1)
    f.data.append((14, DataPageBuilder(P)))              # the builder's empty page
    case = f.finish(rows=600)
    # row 15: a data page in the tree that is malformed and names 151
    bad, _ = build_data_page(P, [(b"a", ptrs(151), True, 1, 0, 0), (b"b", b"x", False, 2, 0, 0)])
    bad = bytearray(bad)
    bad[19 + 0] = 1                                      # shared != 0 in the first entry
    return case, bytes(bad)


def every_bit_case():
    case, bad = every_bit()
    P = case["P"]
    f_pages = bytearray(case["pages"].tobytes()) + bad
    cls = np.append(case["cls"], np.uint8(1))
    table = case["table"].copy()
    table[15] = fp(case["fp_first"] + cls.size - 1)
    # the root gains row 15 as a child: rebuild it in place
    root_slot = (int(table[0]) >> 3) - case["fp_first"]
    kids = tr.decode_strict(bytes(f_pages[root_slot * P:(root_slot + 1) * P]), P)
    f_pages[root_slot * P:(root_slot + 1) * P] = tr.index_page(P, True, kids + [15])
    return dict(case, pages=np.frombuffer(bytes(f_pages), dtype=np.uint8), cls=cls, table=table)


def fuzz_forest(P, count=120, seed=FUZZ_SEED):
    """The fuzz's pages of size P as data pages (type forced to 2) under one root; their pointers land anywhere."""
    f = Forest(P, 5, overflow_base=2000)
    t = FUZZ_SIZES.index(P)
    ids = list(range(10, 10 + count))
    for i in ids:
        page = bytearray(fuzz_page(t, seed)[1])
        page[8] = DATA
        f.put(i, bytes(page))
        t += 4
    per = tr.fanout(P)
    kids = []
    for k in range(0, count, per):
        f.put(5 + k // per, tr.index_page(P, True, ids[k:k + per]))
        kids.append(5 + k // per)
    f.put(0, tr.index_page(P, False, kids))
    for c in range(200, 260):                            # some rows for the random pointers to hit
        f.put(c, overflow_page(P, b"x" * (c % 7), [c + 1] if c % 4 == 0 else ()))
    f.roots = [0, NO]
    return f.case(rows=400)


def forests():
    """name -> case of every generated forest of the GPU tests."""
    out = {}
    for P in (64, 512, 1000, 4096, 16384):
        out[f"plain P {P}"] = plain(P, 0 if P != 1000 else (1 << 40) + 12345, 3, 16 if P != 512 else 1)
        out[f"chains P {P}"] = chains(P, 3)
    out["regions 1 P 64"] = regions(64, 1)
    out["regions 64 P 1000"] = regions(1000, 64)
    out["regions 65 P 1000"] = regions(1000, 65, 9)
    out["regions 129 P 4096"] = regions(4096, 129)
    out["regions 129 P 16384"] = regions(16384, 129)
    for n in (1, 64, 65, 128):
        out[f"group {n} P 1000"] = groups(1000, n)
    out["group 128 P 16384"] = groups(16384, 128, 1 << 41)
    out["every bit"] = every_bit_case()
    for P in (1000, 4096):
        out[f"fuzz pages P {P}"] = fuzz_forest(P)
    return out
