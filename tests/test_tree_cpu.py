"""The tree check without a GPU: the model of tests/tree_ref.py against the
reference's sequential iterator on every page the builder makes, hand-assembled
pages, one page per violation of the strict rule, the generated forests of the
GPU tests (so that none of them can pass vacuously), header / binding agreement,
and tests/cpp/tree_logic_test.cpp (csrc/tree_check.h under ASAN + UBSan, the
same functions the device kernel compiles) against the model's fold."""
import os
import re
import subprocess

import numpy as np
import pytest

import eloqstore_amd as pcs
import tree_ref as tr

HERE = os.path.dirname(os.path.abspath(__file__))
LOGIC = os.path.join(HERE, "cpp", "tree_logic_test_asan")


# ---- the builder's pages: the strict rule yields what the sequential iterator yields --------
def child_ids(kind, n, rng):
    if kind == "ascending":
        return [7 + 3 * i for i in range(n)]
    if kind == "descending":
        return [tr.INT32_MAX - 5 * i for i in range(n)]
    return [int(x) for x in rng.integers(0, tr.INT32_MAX + 1, n)]


def keys(n, rng, long_keys):
    out, prefix = [], b"p" * (150 if long_keys else 2)      # a shared prefix >= 128 needs a two-byte varint
    for i in range(n):
        tail = b"%06d" % i + (b"x" * 140 if long_keys and i % 5 == 0 else b"")
        out.append(prefix + tail)
    return out


@pytest.mark.parametrize("interval", [1, 2, 16, 17])
@pytest.mark.parametrize("kind", ["ascending", "descending", "random"])
def test_strict_rule_equals_the_iterator_on_builder_pages(interval, kind):
    rng = np.random.default_rng(interval * 7 + len(kind))
    seen_long = False
    for P in (512, 4096, 16384):
        for n in (0, 1, 15, 16, 17, 33, 100000):              # 100000: filled until Add refuses
            for long_keys in (False, True):
                m = min(n, 6000)
                ids = child_ids(kind, m + 1, rng)
                entries = list(zip(keys(m, rng, long_keys), ids[1:]))
                page, added = tr.build_index_page(P, interval % 2 == 0, ids[0], entries, interval)
                want = ids[:added + 1]
                assert tr.iter_ref(page, P) == want, (P, n, long_keys)
                assert tr.decode_strict(page, P) == want, (P, n, long_keys)
                if n == 100000:
                    # filled to P: not even the next entry fits
                    assert added < m and int.from_bytes(page[9:11], "little") > P - (320 if long_keys else 40)
                seen_long = seen_long or (long_keys and added > 1)
    assert seen_long


def test_builder_restart_layout():
    page, added = tr.build_index_page(512, True, 1, [(b"a%d" % i, i) for i in range(10)], 4)
    C = int.from_bytes(page[9:11], "little")
    assert added == 10 and int.from_bytes(page[C - 2:C], "little") == 3     # entries 0-3, 4-7, 8-9
    page, added = tr.build_index_page(512, True, 1, [], 4)
    assert page[9:11] == b"\x11\x00" and page[15:17] == b"\x00\x00"        # leftmost only: C = 17, R = 0


# ---- three pages assembled by hand from the format comment -------------------------------------
def hand(P, body):
    return bytes(body) + bytes(P - len(body))


HAND_PAGES = [
    # leftmost only: checksum 8 x 0 | type 1 | C = 17 | leftmost 9 | R = 0
    (hand(32, [0] * 8 + [1] + [17, 0] + [9, 0, 0, 0] + [0, 0]), [9]),
    # one region, two entries: "ab" -> 10 (v = 20), then shared 1 + "c" -> 10 - 3 = 7 (v = 3 << 1 | 1 = 7)
    (hand(64, [0] * 8 + [0] + [28, 0] + [5, 0, 0, 0]
          + [0, 2, 0x61, 0x62, 20] + [1, 1, 0x63, 7]
          + [15, 0] + [1, 0]), [5, 10, 7]),
    # two regions: [15, 20) "a" -> 300 (v = 600 = 0xD8 0x04), [20, 24) "b" -> 2 (v = 4): ids restart from 0
    (hand(64, [0] * 8 + [1] + [30, 0] + [0xFF, 0xFF, 0xFF, 0x7F]
          + [0, 1, 0x61, 0xD8, 0x04] + [0, 1, 0x62, 4]
          + [15, 0] + [20, 0] + [2, 0]), [tr.INT32_MAX, 300, 2]),
]


def test_hand_assembled_pages():
    for page, want in HAND_PAGES:
        assert tr.decode_strict(page, len(page)) == want
        assert tr.iter_ref(page, len(page)) == want


# ---- one page per violation ---------------------------------------------------------------------
@pytest.mark.parametrize("P", [64, 1000])
def test_every_violation_is_rejected(P):
    v = tr.violations(P)
    assert len(v) == 17
    for name, page in v.items():
        assert len(page) == P and tr.decode_strict(page, P) is None, name
    for name, (page, want) in tr.control_pages(P).items():
        assert tr.decode_strict(page, P) == want, name      # the same parts with no rule broken decode


# ---- the forests of the GPU tests ----------------------------------------------------------------
@pytest.fixture(scope="module")
def forests():
    out = {}
    for name, c in tr.forests().items():
        out[name] = (c, tr.check(c["pages"], c["P"], c["fp_first"], c["cls"], c["table"], c["roots"]))
    return out


def test_forests_cover_every_bit_and_tie_break(forests):
    bits = 0
    for name, (c, (nodes, s, problems)) in forests.items():
        assert int(s["n_reached"]) > 0, name
        for k in range(8):
            if int(s["n_by_bit"][k]):
                bits |= 1 << k
    assert bits == 0xFF
    nodes, s, problems = forests["every bit"][1]
    assert all(int(x) > 0 for x in s["n_by_bit"]), s["n_by_bit"]
    want = {1: tr.UNMAPPED, 2: tr.UNMAPPED, 3: tr.ABSENT, 4: tr.ABSENT, 5: tr.ABSENT, 6: tr.BLANK, 7: tr.CORRUPT,
            8: tr.WRONG_TYPE, 40: tr.WRONG_TYPE, 41: tr.WRONG_TYPE, 49: tr.WRONG_TYPE, 0: tr.BAD_CHILD,
            10: tr.BAD_CHILD, 12: tr.MALFORMED, 45: tr.BAD_LINK, 46: tr.BAD_LINK, 47: tr.BAD_LINK, 48: tr.BAD_LINK}
    got = {int(p["page_id"]): int(p["bits"]) for p in problems}
    assert got == want
    assert int(nodes[43]["bits"]) == 0 and int(nodes[44]["bits"]) == 0 and int(nodes[42]["bits"]) == 0
    for row in (30, 31, 32, 33, 60):                             # only unread pages point to these
        assert int(nodes[row]["parent"]) == tr.NO
    assert int(s["unreached_by_type"][tr.DATA]) == 5 and int(s["n_out_of_range_refs"]) == 2
    assert int(s["n_chain_heads"]) == 5                          # 42, 43, 45, 47, 48

    nodes, s, problems = forests["tie breaks"][1]
    assert int(nodes[10]["parent"]) == 20 and int(nodes[10]["depth"]) == 1 and int(nodes[10]["tree"]) == 4
    assert int(nodes[11]["parent"]) == 3 and int(nodes[12]["parent"]) == 2      # both parents were decoded
    assert int(nodes[6]["parent"]) == 4 and int(nodes[6]["depth"]) == 2          # the smaller depth wins
    assert int(nodes[0]["tree"]) == 1 and int(nodes[0]["parent"]) == 0           # of equal roots the lowest
    assert int(nodes[5]["n_children"]) == 4 and int(s["n_extra_refs"]) >= 5      # cycles: root, parent, self
    assert int(s["n_out_of_range_refs"]) == 1 and int(s["n_problems"]) == 0     # root 9999

    # same depth, two parents: a forest of its own, where no other tree interferes
    c = tr.tie_breaks()
    c["roots"] = [0]
    nodes, s, problems = tr.check(c["pages"], c["P"], c["fp_first"], c["cls"], c["table"], c["roots"])
    assert int(nodes[10]["parent"]) == 2 and int(nodes[10]["depth"]) == 2        # 2 < 3 at one depth

    assert int(forests["deep 16"][1][1]["n_depth_capped"]) == 0
    nodes, s, problems = forests["deep 16"][1]
    assert int(nodes[16]["depth"]) == 16 and int(nodes[16]["type"]) == tr.DATA and int(s["n_data"]) == 1
    nodes, s, problems = forests["deep 17"][1]
    assert int(s["n_depth_capped"]) == 1 and int(nodes[17]["parent"]) == tr.NO and int(s["max_depth"]) == 16

    nodes, s, problems = forests["battery"][1]
    assert int(s["n_by_bit"][5]) == 17 and int(s["n_reached"]) == 18
    for row in tr.BATTERY_DATA:
        assert int(nodes[row]["parent"]) == tr.NO
    assert int(s["unreached_by_type"][tr.DATA]) == len(tr.BATTERY_DATA)

    for name in ("random pages P 1000", "random pages P 4096"):
        nodes, s, problems = forests[name][1]
        assert int(s["n_by_bit"][5]) > 50 and int(s["n_refs"]) > 1000, name      # malformed and well-formed both
    nodes, s, problems = forests["fan 4097"][1]
    assert int(nodes[0]["n_children"]) == 4097 and int(s["n_reached"]) == 4098
    nodes, s, problems = forests["restart every entry"][1]
    assert int(nodes[0]["n_children"]) == 900
    for width in (1, 63, 64, 65, 257):
        assert int(forests[f"wide {width}"][1][1]["n_data"]) == width
    s = forests["three levels P 512"][1][1]
    assert (int(s["n_nonleaf"]), int(s["n_leaf_index"]), int(s["n_data"]), int(s["max_depth"])) == (1, 6, 27, 2)
    assert int(s["unreached_by_type"][tr.OVERFLOW]) == 1 and int(s["unreached_by_type"][tr.DATA]) == 1


# ---- header and binding --------------------------------------------------------------------------
def test_header_and_binding_agree():
    assert pcs.TREE_NODE_DTYPE.itemsize == 16 and pcs.TREE_PROBLEM_DTYPE.itemsize == 16
    assert pcs.TREE_SUMMARY_DTYPE.itemsize == 256
    assert pcs.TREE_NODE_DTYPE == tr.NODE_DTYPE and pcs.TREE_PROBLEM_DTYPE == tr.PROBLEM_DTYPE
    assert pcs.TREE_SUMMARY_DTYPE == tr.SUMMARY_DTYPE
    with open(pcs.HEADER_PATH) as f:
        text = f.read()
    for name in ("pcs_tree_node", "pcs_tree_problem", "pcs_tree_summary", "pcs_tree_bits", "pcs_tree_check_dev",
                 "pcs_tree_check_host"):
        assert name in text, name
    assert re.search(r"#define PCS_ABI_VERSION 7\b", text) and pcs.ABI_VERSION == 7
    assert re.search(r"#define PCS_TREE_MAX_DEPTH 16\b", text) and pcs.TREE_MAX_DEPTH == 16 == tr.MAX_DEPTH
    assert re.search(r"#define PCS_TREE_CLASS_ABSENT 3\b", text) and pcs.TREE_CLASS_ABSENT == 3
    enum = re.search(r"enum pcs_tree_bits \{(.*?)\};", text, re.S).group(1)
    values = {k: int(v) for k, v in re.findall(r"PCS_TREE_([A-Z_]+) = (\d+)", enum)}
    assert values == {"UNMAPPED": 1, "ABSENT": 2, "BLANK": 4, "CORRUPT": 8, "WRONG_TYPE": 16, "MALFORMED": 32,
                      "BAD_CHILD": 64, "BAD_LINK": 128}
    assert (pcs.TREE_UNMAPPED, pcs.TREE_ABSENT, pcs.TREE_BLANK, pcs.TREE_CORRUPT, pcs.TREE_WRONG_TYPE,
            pcs.TREE_MALFORMED, pcs.TREE_BAD_CHILD, pcs.TREE_BAD_LINK) == (1, 2, 4, 8, 16, 32, 64, 128)
    # the summary's fields in the header's order
    body = re.search(r"typedef struct pcs_tree_summary \{(.*?)\} pcs_tree_summary;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\[\d+\]", "", x.strip()) for decl in re.findall(r"uint64_t ([^;]+);", body)
              for x in decl.split(",")]
    assert fields == list(tr.SUMMARY_DTYPE.names)
    for fn in ("pcs_tree_check_dev", "pcs_tree_check_host"):
        assert fn in pcs._SIGS and fn in pcs.header_functions()


# ---- csrc/tree_check.h under ASAN + UBSan --------------------------------------------------------
def run_logic(*args):
    assert os.path.exists(LOGIC), "build() makes tests/cpp/tree_logic_test_asan"
    r = subprocess.run([LOGIC, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_logic_violation_battery_and_builder_pages(tmp_path):
    for P in (64, 1000):
        pages = list(tr.violations(P).values()) + [p for p, _ in tr.control_pages(P).values()]
        rng = np.random.default_rng(P)
        for interval in (1, 2, 16, 17):
            for n in (0, 1, 15, 16, 17, 33, 500):
                ids = child_ids("random", n + 1, rng)
                pages.append(tr.build_index_page(P, True, ids[0], list(zip(keys(n, rng, False), ids[1:])), interval)[0])
        path = tmp_path / f"pages_{P}"
        path.write_bytes(b"".join(pages))
        lines = run_logic("pages", str(path), str(P))
        assert len(lines) == len(pages) + 1
        fold = ok = 0
        for k, (line, page) in enumerate(zip(lines, pages)):
            want = tr.decode_strict(page, P)
            assert line == ("malformed" if want is None else " ".join(["ok"] + [str(c) for c in want])), k
            assert (want is None) == (k < 17), k
            fold = tr.fold_page(fold, want)
            ok += want is not None
        assert lines[-1] == f"fold {fold} ok {ok} pages {len(pages)}"
    for page, want in HAND_PAGES:
        path = tmp_path / "hand"
        path.write_bytes(page)
        assert run_logic("pages", str(path), str(len(page)))[0] == " ".join(["ok"] + [str(c) for c in want])


def test_logic_fuzz_fold_equals_the_model():
    n = 20000
    fold, ok = tr.fuzz_fold(n)
    assert 1000 < ok < n - 1000          # both verdicts occur often
    assert run_logic("fuzz", str(n)) == [f"fold {fold} ok {ok} pages {n}"]
