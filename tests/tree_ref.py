"""CPU model of the tree check (pcs_tree_check_dev), written from the page
formats (index page: IndexPageBuilder / IndexPageIter; data page header: prev
and next sibling) and from the walk's rules in include/eloqstore_pcs.h:

  build_index_page   a port of IndexPageBuilder (restart interval as a parameter,
                     varint shared / non_shared >= 128, negative deltas)
  data_page          header, sibling links and filler
  Forest             table and window assembler
  iter_ref           IndexPageIter::ParseNextKey step by step, sequentially; the
                     restart array only answers is_restart_pointer
  decode_strict      the strict page rule, sequentially
  check              a plain breadth-first walk -> nodes, summary, problems in
                     the ABI's dtypes
  violations         one page per rule of the strict rule that it breaks
  fuzz_page / fuzz_fold   the pages and the fold of tests/cpp/tree_logic_test.cpp
  forests            the generated forests of tests/test_gpu_tree_check.py
"""
import numpy as np

M64 = (1 << 64) - 1
NO = 0xFFFFFFFF
NO64 = M64
INT32_MAX = 0x7FFFFFFF
INVALID = 7                      # MappingSnapshot::InvalidValue
NONLEAF, LEAF, DATA, OVERFLOW = 0, 1, 2, 3
UNMAPPED, ABSENT, BLANK, CORRUPT, WRONG_TYPE, MALFORMED, BAD_CHILD, BAD_LINK = (1 << k for k in range(8))
SIX = 0x3F
MAX_DEPTH = 16
CLASS_ABSENT = 3
HEADER = 15

NODE_DTYPE = np.dtype([("parent", "<u4"), ("depth", "u1"), ("tree", "u1"), ("type", "u1"), ("bits", "u1"),
                       ("n_children", "<u4"), ("n_bad_children", "<u4")])
PROBLEM_DTYPE = np.dtype([("page_id", "<u4"), ("parent", "<u4"), ("bits", "<u4"), ("depth", "<u4")])
SUMMARY_DTYPE = np.dtype([
    ("n_pages", "<u8"), ("table_size", "<u8"), ("n_mapped", "<u8"), ("n_reached", "<u8"), ("n_nonleaf", "<u8"),
    ("n_leaf_index", "<u8"), ("n_data", "<u8"), ("n_refs", "<u8"), ("n_extra_refs", "<u8"),
    ("n_out_of_range_refs", "<u8"), ("max_depth", "<u8"), ("n_depth_capped", "<u8"), ("n_by_bit", "<u8", (8,)),
    ("n_problems", "<u8"), ("first_problem", "<u8"), ("n_listed", "<u8"), ("n_unreached_mapped", "<u8"),
    ("unreached_by_type", "<u8", (6,)), ("n_unreached_unread", "<u8"), ("n_chain_heads", "<u8")])


def fp(file_page):
    """The table value that maps a file page."""
    return (file_page << 3) | 1


# ---- encoding ---------------------------------------------------------------------------
def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def enc_delta(delta):
    return delta << 1 if delta >= 0 else ((-delta) << 1) | 1


def le16(v):
    return int(v).to_bytes(2, "little")


def le32(v):
    return int(v).to_bytes(4, "little")


def build_index_page(P, leaf, leftmost, entries, interval=16, pad=0):
    """IndexPageBuilder: Add(leftmost) then Add(key, id) for every entry, Finish.
    Returns (page bytes, number of entries that fitted)."""
    buf = bytearray(HEADER)
    buf[8] = LEAF if leaf else NONLEAF
    buf[11:15] = le32(leftmost)
    restarts = [HEADER]
    counter = added = last_id = 0
    last_key = b""
    for key, page_id in entries:
        assert key and 0 <= page_id <= INT32_MAX
        extra = shared = 0
        if counter < interval:
            m = min(len(last_key), len(key))
            while shared < m and last_key[shared] == key[shared]:
                shared += 1
        else:
            extra = 2
            last_id = 0
        non_shared = len(key) - shared
        entry = varint(shared) + varint(non_shared) + key[shared:] + varint(enc_delta(page_id - last_id))
        if len(buf) + 2 * len(restarts) + 2 + extra + len(entry) > P:
            break
        if counter >= interval:
            restarts.append(len(buf))
            counter = 0
        buf += entry
        last_key, last_id = key, page_id
        counter += 1
        added += 1
    if added == 0:
        restarts = []
    for r in restarts:
        buf += le16(r)
    buf += le16(len(restarts))
    buf[9:11] = le16(len(buf))
    assert len(buf) <= P
    return bytes(buf) + bytes([pad]) * (P - len(buf)), added


def index_page(P, leaf, children, interval=16):
    """An index page over `children` (the first is the leftmost pointer) with keys of its own making."""
    entries = [(b"k%07d" % i, c) for i, c in enumerate(children[1:])]
    page, added = build_index_page(P, leaf, children[0], entries, interval)
    assert added == len(entries), (P, len(children))
    return page


def data_page(P, prev=NO, nxt=NO, filler=0xAB):
    return bytes(8) + bytes([DATA]) + le16(19) + le32(prev) + le32(nxt) + bytes([filler]) * (P - 19)


def typed_page(P, type_byte, filler=0xCD):
    return bytes(8) + bytes([type_byte]) + bytes([filler]) * (P - 9)


# ---- decoding ---------------------------------------------------------------------------
def _varint32(page, pos, limit):
    """GetVarint32Ptr: (value, next pos) or None."""
    v = 0
    for i in range(5):
        if pos >= limit:
            return None
        b = page[pos]
        pos += 1
        v |= (b & 0x7F) << (7 * i)
        if b < 0x80:
            return v & 0xFFFFFFFF, pos
    return None


def iter_ref(page, P):
    """The children IndexPageIter yields over a page of P bytes whose content
    length and restart count are taken from the page (MemIndexPage), one
    ParseNextKey at a time until it invalidates itself."""
    C = int.from_bytes(page[9:11], "little")
    R = int.from_bytes(page[C - 2:C], "little")
    E = C - 2 * (1 + R)
    restart = [int.from_bytes(page[E + 2 * k:E + 2 * k + 2], "little") for k in range(R)]
    out = []
    cur, idx, key_len, page_id = 11, 0, 0, 0
    while True:
        if cur >= E:
            return out
        if cur < 15:
            out.append(int.from_bytes(page[11:15], "little"))
            cur, idx, key_len = 15, 0, 0
            page_id = out[-1]
            continue
        is_restart = idx < R and cur == restart[idx]
        if E - cur < 2:
            return out
        a = _varint32(page, cur, E)
        b = _varint32(page, a[1], E) if a else None
        if not b or key_len < a[0]:
            return out
        shared, non_shared, pos = a[0], b[0], b[1]
        pos += non_shared
        v = _varint32(page, pos, E) if pos <= E else None
        if not v:
            return out
        delta = -(v[0] >> 1) if v[0] & 1 else v[0] >> 1
        page_id = delta if is_restart else page_id + delta
        key_len = shared + non_shared
        cur = v[1]
        out.append(page_id & 0xFFFFFFFF)
        if idx + 1 < R and cur >= restart[idx + 1]:
            idx += 1


def decode_strict(page, P):
    """The strict rule: the list of children (leftmost first), or None when the page is malformed."""
    assert len(page) == P
    if P < 17:
        return None
    C = int.from_bytes(page[9:11], "little")
    if C < 17 or C > P:
        return None
    R = int.from_bytes(page[C - 2:C], "little")
    E = C - 2 * (1 + R)
    if E < HEADER or (R == 0 and E != HEADER):
        return None
    out = [int.from_bytes(page[11:15], "little")]
    o = [int.from_bytes(page[E + 2 * k:E + 2 * k + 2], "little") for k in range(R)] + [E]
    if R and o[0] != HEADER:
        return None
    for k in range(R):
        lo, hi = o[k], o[k + 1]
        if not lo < hi <= E:
            return None
        pos, key_len, page_id, first = lo, 0, 0, True
        while pos < hi:
            a = _varint32(page, pos, hi)
            b = _varint32(page, a[1], hi) if a else None
            if not b or a[0] > key_len:
                return None
            pos = b[1]
            if b[0] > hi - pos:
                return None
            pos += b[0]
            v = _varint32(page, pos, hi)
            if not v:
                return None
            delta = -(v[0] >> 1) if v[0] & 1 else v[0] >> 1
            page_id = delta if first else page_id + delta
            if not 0 <= page_id <= INT32_MAX:
                return None
            first, key_len, pos = False, a[0] + b[0], v[1]
            out.append(page_id)
    return out


# ---- the walk -----------------------------------------------------------------------------
def type_bucket(t):
    return t if t < 4 else 4 if t == 255 else 5


def check(pages, P, fp_first, cls, table, roots, cap=None):
    """(nodes, summary, problems) as pcs_tree_check_dev writes them."""
    pages = np.asarray(pages, dtype=np.uint8).reshape(-1)
    cls = np.asarray(cls, dtype=np.uint8)
    table = [int(v) for v in np.asarray(table, dtype=np.uint64)]
    rows, n_pages = len(table), cls.size
    nodes = np.zeros(rows, dtype=NODE_DTYPE)
    nodes["parent"], nodes["depth"], nodes["tree"], nodes["type"] = NO, 0xFF, 0xFF, 0xFF
    s = np.zeros(1, dtype=SUMMARY_DTYPE)[0]

    def page_of(row):
        v = table[row]
        if v & 7 != 1:
            return None
        i = (v >> 3) - fp_first
        return i if 0 <= i < n_pages else -1

    def body(i):
        return bytes(pages[i * P:(i + 1) * P])

    claimed, tree_of = {}, {}
    refs = oor = 0
    frontier = []
    for t, r in enumerate(int(x) for x in roots):
        if r >= NO:
            continue
        refs += 1
        if r >= rows:
            oor += 1
            continue
        if r not in claimed:
            claimed[r] = r
            tree_of[r] = t
            frontier.append(r)
    for d in range(MAX_DEPTH + 1):
        bids = {}
        for c in frontier:
            parent = claimed[c]
            tree = tree_of[c] if d == 0 else int(nodes[parent]["tree"])
            typ, bits, n_children, n_bad = 0xFF, 0, 0, 0
            i = page_of(c)
            if i is None:
                bits = UNMAPPED
            elif i < 0 or cls[i] > 2:
                bits = ABSENT
            elif cls[i] == 2:
                bits = BLANK
            elif cls[i] == 0:
                bits = CORRUPT
            else:
                typ = int(pages[i * P + 8])
                want = (NONLEAF, LEAF) if d == 0 or int(nodes[parent]["type"]) == NONLEAF else (DATA,)
                if typ not in want:
                    bits = WRONG_TYPE
                elif typ != DATA and d < MAX_DEPTH:
                    children = decode_strict(body(i), P)
                    if children is None:
                        bits = MALFORMED
                    else:
                        n_children = len(children)
                        for ch in children:
                            if ch >= rows:
                                n_bad += 1
                            elif ch not in claimed:
                                bids[ch] = min(bids.get(ch, c), c)
                        if n_bad:
                            bits |= BAD_CHILD
            nodes[c] = (parent, d, tree, typ, bits, n_children, n_bad)
            refs += n_children
            oor += n_bad
        frontier = sorted(bids)
        claimed.update(bids)
    reached = nodes["parent"] != NO

    def good_data(q):
        return q < rows and reached[q] and nodes[q]["type"] == DATA and not nodes[q]["bits"] & SIX

    links = {}
    for p in range(rows):
        if good_data(p):
            b = body(page_of(p))
            links[p] = (int.from_bytes(b[11:15], "little"), int.from_bytes(b[15:19], "little"))
    heads = 0
    for p, (prev, nxt) in links.items():
        heads += prev == NO
        ok = (nxt == NO or (nxt in links and links[nxt][0] == p)) and \
             (prev == NO or (prev in links and links[prev][1] == p))
        if not ok:
            nodes[p]["bits"] |= BAD_LINK
    s["n_pages"], s["table_size"] = n_pages, rows
    s["n_mapped"] = sum(1 for v in table if v & 7 == 1)
    s["n_reached"] = int(reached.sum())
    clean = reached & (nodes["bits"] == 0)
    for name, t in (("n_nonleaf", NONLEAF), ("n_leaf_index", LEAF), ("n_data", DATA)):
        s[name] = int((clean & (nodes["type"] == t)).sum())
    s["n_refs"], s["n_out_of_range_refs"] = refs, oor
    s["n_extra_refs"] = refs - oor - int(s["n_reached"])
    s["max_depth"] = int(nodes["depth"][reached].max()) if reached.any() else NO64
    s["n_depth_capped"] = int((clean & (nodes["type"] <= LEAF) & (nodes["depth"] == MAX_DEPTH)).sum())
    for k in range(8):
        s["n_by_bit"][k] = int((reached & ((nodes["bits"] >> k) & 1 == 1)).sum())
    bad = np.nonzero(reached & (nodes["bits"] != 0))[0]
    s["n_problems"] = bad.size
    s["first_problem"] = int(bad[0]) if bad.size else NO64
    listed = bad if cap is None else bad[:cap]
    s["n_listed"] = listed.size
    problems = np.zeros(listed.size, dtype=PROBLEM_DTYPE)
    problems["page_id"] = listed
    for k in ("parent", "bits", "depth"):
        problems[k] = nodes[k][listed]
    for p in range(rows):
        if reached[p] or table[p] & 7 != 1:
            continue
        i = page_of(p)
        if i >= 0 and cls[i] == 1:
            s["unreached_by_type"][type_bucket(int(pages[i * P + 8]))] += 1
        else:
            s["n_unreached_unread"] += 1
    s["n_unreached_mapped"] = int(s["unreached_by_type"].sum()) + int(s["n_unreached_unread"])
    s["n_chain_heads"] = heads
    return nodes, s, problems


# ---- table and window assembler -------------------------------------------------------------
class Forest:
    """Pages of one size in a window of file pages starting at fp_first, and the table that maps them."""

    def __init__(self, P, fp_first=0):
        self.P, self.fp_first = P, fp_first
        self.window, self.cls, self.table = [], [], {}
        self.roots = []

    def slot(self, page, cls=1):
        """Appends a page to the window -> its file page id."""
        assert len(page) == self.P
        self.window.append(bytes(page))
        self.cls.append(cls)
        return self.fp_first + len(self.window) - 1

    def put(self, page_id, page, cls=1):
        self.table[page_id] = fp(self.slot(page, cls))
        return page_id

    def value(self, page_id, v):
        self.table[page_id] = v

    def arrays(self, rows=None):
        rows = rows if rows is not None else (max(self.table) + 1 if self.table else 0)
        table = np.full(rows, INVALID, dtype=np.uint64)
        for k, v in self.table.items():
            if k < rows:
                table[k] = v
        pages = np.frombuffer(b"".join(self.window), dtype=np.uint8) if self.window else np.zeros(0, np.uint8)
        return pages, np.array(self.cls, dtype=np.uint8), table

    def case(self, rows=None, roots=None):
        pages, cls, table = self.arrays(rows)
        return dict(P=self.P, fp_first=self.fp_first, pages=pages, cls=cls, table=table,
                    roots=list(self.roots if roots is None else roots))


def chain(f, ids):
    """Healthy data pages with ids `ids`, linked in order."""
    for k, p in enumerate(ids):
        f.put(p, data_page(f.P, ids[k - 1] if k else NO, ids[k + 1] if k + 1 < len(ids) else NO))


# ---- violations of the strict rule --------------------------------------------------------------
def _raw(P, C, tail, body=b"", leaf=1, leftmost=5):
    """A page from its parts: header, body from offset 15, `tail` ending at C."""
    page = bytearray(P)
    page[8] = leaf
    page[9:11] = le16(C)
    page[11:15] = le32(leftmost)
    page[15:15 + len(body)] = body
    if 0 <= C - len(tail) and C <= P:
        page[C - len(tail):C] = tail
    return bytes(page)


def _one_region(P, body, leaf=1):
    """A page whose single region is `body`."""
    C = 15 + len(body) + 4
    return _raw(P, C, le16(15) + le16(1), body, leaf)


def violations(P):
    """name -> page of P bytes (P >= 64) that breaks exactly the named rule."""
    e = lambda shared, key, v: varint(shared) + varint(len(key)) + key + varint(v)  # noqa: E731
    good = e(0, b"ab", 20) + e(1, b"c", 2)
    two = lambda o0, o1, body=good: _raw(P, 15 + len(body) + 6, le16(o0) + le16(o1) + le16(2), body)  # noqa: E731
    first = len(e(0, b"ab", 20))
    v = {
        "C=16": _raw(P, 16, b""),
        "C=P+1": _raw(P, P + 1, b""),
        "E<15": _raw(P, 17, le16(1)),
        "R=0,E!=15": _raw(P, 19, le16(0)),
        "o[0]!=15": _raw(P, 15 + len(good) + 4, le16(16) + le16(1), good),
        "restarts equal": two(15, 15),
        "restarts descending": _raw(P, 15 + len(good) + 8, le16(15) + le16(15 + first + 1) + le16(15 + first) + le16(3),
                                    good),
        "o[R-1]>=E": two(15, 15 + len(good)),
        "entry crosses in shared": _one_region(P, e(0, b"ab", 20) + b"\x81"),
        "entry crosses in non_shared": _one_region(P, e(0, b"ab", 20) + b"\x01\x81"),
        "entry crosses in key": _one_region(P, e(0, b"ab", 20) + b"\x01\x05xy"),
        "entry crosses in child": _one_region(P, e(0, b"ab", 20) + b"\x01\x01x\x81"),
        "shared!=0 at restart": two(15, 15 + first, e(0, b"ab", 20) + e(1, b"c", 2)),
        "shared>previous key": _one_region(P, e(0, b"ab", 20) + e(3, b"c", 2)),
        "6-byte varint": _one_region(P, e(0, b"ab", 20) + b"\x01\x01x" + b"\x80\x80\x80\x80\x80\x01"),
        "id<0": _one_region(P, e(0, b"ab", 20) + e(1, b"c", enc_delta(-11))),
        "id>INT32_MAX": _one_region(P, e(0, b"ab", enc_delta(INT32_MAX)) + e(1, b"c", enc_delta(1))),
    }
    return v


def control_pages(P):
    """Well-formed neighbours of the violations: the same parts, no rule broken."""
    e = lambda shared, key, v: varint(shared) + varint(len(key)) + key + varint(v)  # noqa: E731
    a, b = e(0, b"ab", 20), e(0, b"c", 2)
    return {
        "one region": (_one_region(P, a + e(1, b"c", 2)), [5, 10, 11]),
        "two regions": (_raw(P, 15 + len(a + b) + 6, le16(15) + le16(15 + len(a)) + le16(2), a + b), [5, 10, 1]),
        "leftmost only": (_raw(P, 17, le16(0)), [5]),
        "id back to 0": (_one_region(P, a + e(1, b"c", enc_delta(-10))), [5, 10, 0]),
        "INT32_MAX": (_one_region(P, e(0, b"ab", enc_delta(INT32_MAX))), [5, INT32_MAX]),
    }


# ---- the fuzz of tests/cpp/tree_logic_test.cpp ----------------------------------------------------
GOLD = 0x9E3779B97F4A7C15
FUZZ_SIZES = (32, 64, 1000, 4096)
FUZZ_SEED = 20240607


class Rng:
    """splitmix64."""

    def __init__(self, seed):
        self.s = seed & M64

    def next(self):
        self.s = (self.s + GOLD) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def words(self, n):
        """The next n outputs as a numpy array."""
        with np.errstate(over="ignore"):
            z = np.uint64(self.s) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(GOLD)
            self.s = int(z[-1]) if n else self.s
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))


def fuzz_writer(P, rng):
    """A well-formed index page written straight in the format from rng's draws."""
    buf = bytearray(HEADER)
    buf[8] = rng.next() & 1
    buf[11:15] = le32(rng.next() % (1 << 31))
    interval = 1 + rng.next() % 17
    want = rng.next() % 48
    restarts = [HEADER]
    counter = prev_len = last_id = added = 0
    for _ in range(want):
        a = rng.next()
        key_len = 1 + (a >> 8) % 200 if a & 15 == 0 else 1 + (a >> 8) % 12
        restart = counter >= interval
        b = rng.next()
        shared = 0 if restart else b % (min(prev_len, key_len - 1) + 1)
        non_shared = key_len - shared
        page_id = rng.next() % (1 << 31)
        entry = bytearray(varint(shared) + varint(non_shared))
        for j in range(non_shared):
            if j % 8 == 0:
                c = rng.next()
            entry.append((c >> (8 * (j % 8))) & 0xFF)
        entry += varint(enc_delta(page_id - (0 if restart else last_id)))
        if len(buf) + len(entry) + 2 * (len(restarts) + (1 if restart else 0)) + 2 > P:
            break
        if restart:
            restarts.append(len(buf))
            counter = 0
        buf += entry
        prev_len, last_id = key_len, page_id
        counter += 1
        added += 1
    if added == 0:
        restarts = []
    for r in restarts:
        buf += le16(r)
    buf += le16(len(restarts))
    buf[9:11] = le16(len(buf))
    return buf + bytes(P - len(buf))


def fuzz_page(t, seed=FUZZ_SEED):
    """Case t of the fuzz -> (P, page): random bytes when (t >> 2) & 1 == 0, else a
    well-formed page with one to three random byte edits."""
    rng = Rng(((seed + t) * 0xD6E8FEB86659FD93) & M64)
    P = FUZZ_SIZES[t % 4]
    if (t >> 2) & 1 == 0:
        return P, rng.words((P + 7) // 8).astype("<u8").tobytes()[:P]
    page = fuzz_writer(P, rng)
    for _ in range(1 + rng.next() % 3):
        pos = rng.next() % P
        page[pos] = rng.next() & 0xFF
    return P, bytes(page)


def fold_page(fold, children):
    """One page's verdict and children into the running fold."""
    K = GOLD
    fold = (fold * K + (0 if children is None else 1 + len(children))) & M64
    for c in children or ():
        fold = (fold * K + c) & M64
    return fold


def fuzz_fold(n, seed=FUZZ_SEED):
    """(fold, well-formed pages) over cases 0 .. n."""
    fold = ok = 0
    for t in range(n):
        P, page = fuzz_page(t, seed)
        children = decode_strict(page, P)
        ok += children is not None
        fold = fold_page(fold, children)
    return fold, ok


# ---- the forests of the GPU tests -------------------------------------------------------------------
def fanout(P):
    """Children that surely fit one index page of P bytes built by index_page."""
    return max(1, (P - 64) // 12)


def wide(P, width, fp_first=0, interval=16):
    """A non-leaf root (row 0) over leaf-index pages over `width` chained data pages: one level of that width."""
    f = Forest(P, fp_first)
    per = fanout(P)
    data = list(range(1000, 1000 + width))
    leaves = list(range(1, 1 + (width + per - 1) // per))
    assert len(leaves) <= per
    f.put(0, index_page(P, False, leaves, interval))
    for k, leaf in enumerate(leaves):
        f.put(leaf, index_page(P, True, data[k * per:(k + 1) * per], interval))
    chain(f, data)
    f.roots = [0, NO]
    return f.case()


def fan_4097(P=32768):
    """A root with 4,097 children: rows 1 .. 4097 share eight data pages (duplicate owners are legal)."""
    f = Forest(P, 7)
    ids = list(range(1, 4098))
    entries = [(i.to_bytes(2, "big"), c) for i, c in enumerate(ids[1:])]
    page, added = build_index_page(P, True, ids[0], entries, 16)
    assert added == len(entries)
    f.put(0, page)
    shared = [f.slot(data_page(P)) for _ in range(8)]
    for i in ids:
        f.value(i, fp(shared[i % 8]))
    f.roots = [0]
    return f.case()


def three_levels(P, fp_first=0, fan=5):
    """root (non-leaf) -> fan leaf-index pages -> fan data pages each, one sibling chain; a ttl tree beside it."""
    f = Forest(P, fp_first)
    leaves = list(range(1, 1 + fan))
    data = list(range(100, 100 + fan * fan))
    f.put(0, index_page(P, False, leaves, 2))
    for k, leaf in enumerate(leaves):
        f.put(leaf, index_page(P, True, data[k * fan:(k + 1) * fan], 1))
    chain(f, data)
    f.put(50, index_page(P, True, [60, 61], 16))       # the ttl tree
    chain(f, [60, 61])
    f.put(70, typed_page(P, OVERFLOW))                  # reached by nobody: overflow pages never are
    f.put(71, data_page(P))                             # a leaked data page
    f.roots = [0, 50]
    return f.case()


def restart_every_entry(P=16384):
    """One 16 KiB leaf-index page with restart interval 1: more regions than lanes."""
    f = Forest(P, 3)
    n = 900
    ids = list(range(1, n + 1))
    f.put(0, index_page(P, True, ids, 1))
    shared = f.slot(data_page(P))
    for i in ids:
        f.value(i, fp(shared))
    f.roots = [0]
    return f.case()


def tie_breaks(P=512):
    f = Forest(P, 0)
    # two parents at one depth: rows 3 and 2 both point to 10; the lowest id (2) wins
    f.put(0, index_page(P, False, [3, 2, 4]))
    f.put(3, index_page(P, True, [10, 11]))
    f.put(2, index_page(P, True, [10, 12]))
    # two parents at different depths: 4 (depth 1, non-leaf) and 5 (depth 2) both point to 6
    f.put(4, index_page(P, False, [5, 6]))
    f.put(5, index_page(P, False, [6, 0, 4, 5]))        # and to the root, its parent and itself
    f.put(6, index_page(P, True, [13]))
    for d in (10, 11, 12, 13):
        f.put(d, data_page(P))
    # two equal roots, an empty tree, and a root beyond the table
    f.roots = [NO, 0, 0, 1 << 40, 20, 9999]
    f.put(20, index_page(P, True, [10]))                # another tree's pointer to a claimed page
    return f.case()


def every_bit(P=1000, fp_first=(1 << 40) + 12345):
    f = Forest(P, fp_first)
    kids = list(range(1, 13))
    f.put(0, index_page(P, False, kids + [500, 4000]))  # 4000: an entry child beyond the table
    f.put(12, violations(P)["shared>previous key"])      # MALFORMED
    f.value(1, INVALID)                                  # UNMAPPED: nobody wrote the row
    f.value(2, (fp_first << 3) | 2)                      # UNMAPPED: type bits 2
    f.value(3, fp(fp_first - 1))                         # ABSENT: below the window
    f.value(4, fp(fp_first + 10000))                     # ABSENT: above the window
    f.put(5, index_page(P, True, [30]), cls=CLASS_ABSENT)
    f.put(6, index_page(P, True, [31]), cls=2)           # BLANK
    f.put(7, index_page(P, True, [32]), cls=0)           # CORRUPT
    f.put(8, data_page(P))                               # WRONG_TYPE: a data page under a non-leaf
    f.put(9, index_page(P, True, [40, 41, 42]))
    f.put(40, index_page(P, True, [33]))                 # WRONG_TYPE: an index page under a leaf index
    f.put(41, typed_page(P, OVERFLOW))                   # WRONG_TYPE: an overflow page under a leaf index
    f.put(42, data_page(P))
    f.put(10, index_page(P, True, [3000, 42]))           # BAD_CHILD: the leftmost pointer beyond the table
    f.put(11, index_page(P, True, [43, 44, 45, 46, 47, 48]))
    # sibling links: 43 <-> 44 healthy; 45 -> 46 but 46's prev is wrong; 47's next is unreached, 48's next blank
    f.put(43, data_page(P, NO, 44))
    f.put(44, data_page(P, 43, NO))
    f.put(45, data_page(P, NO, 46))
    f.put(46, data_page(P, 44, NO))
    f.put(47, data_page(P, NO, 60))
    f.put(60, data_page(P, 47, NO))                      # healthy, but no index page points to it
    f.put(48, data_page(P, NO, 6))
    for d in (30, 31, 32, 33):
        f.put(d, data_page(P))                           # only the unread pages point to these
    f.put(500, index_page(P, True, [42]))
    f.put(49, data_page(P))
    f.roots = [0, 49]                                     # a data page as root
    return f.case(rows=600)


BATTERY_DATA = (5, 10, 11, 12)   # the rows a naive reader of the violation pages would follow


def battery(P=512):
    """Every violation as a child of one root; the data pages that only they name must stay unreached."""
    f = Forest(P, 11)
    v = violations(P)
    kids = list(range(101, 101 + len(v)))
    f.put(0, index_page(P, False, kids))
    for k, page in zip(kids, v.values()):
        f.put(k, page)
    for d in BATTERY_DATA:
        f.put(d, data_page(P))
    f.roots = [0]
    return f.case(rows=200)


def deep(levels, P=512):
    """A chain of `levels` single-pointer index pages (rows 0 ..) that ends in a data page."""
    f = Forest(P, 0)
    for k in range(levels):
        last = k == levels - 1
        f.put(k, index_page(P, last, [k + 1]))
    f.put(levels, data_page(P))
    f.roots = [0]
    return f.case()


def random_pages(P, count=300, seed=FUZZ_SEED):
    """The fuzz's pages of size P as index pages (type forced to 0, class 1) under at most eight roots."""
    f = Forest(P, 5)
    ids = list(range(1, count + 1))
    t = FUZZ_SIZES.index(P)
    for i in ids:
        page = bytearray(fuzz_page(t, seed)[1])
        page[8] = NONLEAF
        f.put(i, bytes(page))
        t += 4
    per = fanout(P)
    row = count + 1
    for k in range(0, count, per):
        f.put(row, index_page(P, False, ids[k:k + per]))
        f.roots.append(row)
        row += 1
    assert len(f.roots) <= 8
    return f.case(rows=row + 50)


def forests():
    """name -> case (P, fp_first, pages, cls, table, roots) of every generated forest of the GPU tests."""
    out = {}
    for width in (1, 63, 64, 65, 257):
        out[f"wide {width}"] = wide(512, width)
    out["wide 65 P 1000"] = wide(1000, 65, (1 << 40) + 12345)
    out["wide 40 P 4096"] = wide(4096, 40, 0, 3)
    out["wide 9 P 16384"] = wide(16384, 9)
    out["fan 4097"] = fan_4097()
    out["restart every entry"] = restart_every_entry()
    for P in (512, 1000, 4096, 16384):
        out[f"three levels P {P}"] = three_levels(P, 0 if P != 1000 else (1 << 40) + 12345)
    out["tie breaks"] = tie_breaks()
    out["every bit"] = every_bit()
    out["battery"] = battery()
    out["deep 16"] = deep(16)
    out["deep 17"] = deep(17)
    for P in (1000, 4096):
        out[f"random pages P {P}"] = random_pages(P)
    return out
