"""The leaf check without a GPU: the model of tests/leaf_ref.py against the
reference's sequential iterator on every page the builder makes, one page per
violation of the strict rule next to a control page that differs in one byte,
the generated forests of the GPU tests (so that none of them can pass
vacuously), header / binding agreement, and tests/cpp/leaf_logic_test.cpp
(csrc/leaf_check.h under ASAN + UBSan, the same functions the device kernel
compiles) against the model's fold."""
import os
import re
import subprocess

import numpy as np
import pytest

import eloqstore_amd as pcs
import leaf_ref as lr

HERE = os.path.dirname(os.path.abspath(__file__))
LOGIC = os.path.join(HERE, "cpp", "leaf_logic_test_asan")


# ---- the builder's pages: the strict rule yields what the sequential iterator yields --------
def items(n, expire, pointers, long_keys=False):
    """n pairs; every seventh value overflows with `pointers` pointers (0: none does)."""
    out, prefix = [], b"p" * (150 if long_keys else 2)       # a shared prefix >= 128 needs a two-byte varint
    ts = 1 << 40
    for i in range(n):
        key = prefix + b"%06d" % i + (b"x" * 140 if long_keys and i % 5 == 0 else b"")
        ts += (-1) ** i * (i * 1000003 % 7919)                # deltas of both signs
        exp = (ts + 3600 + i) if expire and i % 2 == 0 else 0
        if pointers and i % 7 == 3:
            out.append((key, lr.ptrs(*range(100 + i, 100 + i + pointers)), True, ts, exp, i % 3))
        else:
            out.append((key, b"v" * (i * 37 % 300 if i % 11 == 0 else i % 19), False, ts, exp, i % 3))
    return out


def want_of(its):
    return [(k, bytes(v), o, e, t, c) for k, v, o, t, e, c in its]


@pytest.mark.parametrize("interval", [1, 2, 16, 17])
@pytest.mark.parametrize("expire", [False, True])
def test_strict_rule_equals_the_iterator_on_builder_pages(interval, expire):
    seen = set()
    for P in (512, 4096, 16384):
        for pointers in (0, 1, 16, 128):
            for n in (0, 1, 15, 16, 17, 33, 100000):          # 100000: filled until Add refuses
                for long_keys in (False, True):
                    its = items(min(n, 3000), expire, pointers, long_keys)
                    page, added = lr.build_data_page(P, its, interval, 3, 4)
                    want = want_of(its[:added])
                    assert lr.iter_ref(page, P) == want, (P, n, pointers, long_keys)
                    got = lr.decode_strict(page, P)
                    assert got is not None and lr.as_iter(got) == want, (P, n, pointers, long_keys)
                    if n == 100000:
                        assert added < len(its)
                    if n == 0:                                  # the empty page: one restart, no entry
                        C = int.from_bytes(page[9:11], "little")
                        assert C == 23 and page[19:23] == b"\x13\x00\x01\x00" and got == []
                    seen |= {(pointers, e["value_len"] // 4) for e in got if e["flags"] & 1}
    assert {(1, 1), (16, 16), (128, 128)} <= seen              # each group size got onto some page


def test_builder_restart_layout():
    page, added = lr.build_data_page(512, [(b"a%d" % i, b"v", False, i, 0, 0) for i in range(10)], 4)
    C = int.from_bytes(page[9:11], "little")
    assert added == 10 and int.from_bytes(page[C - 2:C], "little") == 3     # entries 0-3, 4-7, 8-9
    assert page[8] == 2 and page[11:19] == b"\xff" * 8


def test_overflow_grouping():
    P = 64                                                     # page_cap 52, end cap 52 - 4 * overflow_pointers
    ids = iter(range(100, 200))
    head, pages = lr.write_overflow_value(P, bytes(range(201)), 2, lambda: next(ids))
    # groups: [100, 101] (52 + 44), [102, 103] (52 + 44), [104] (9)
    assert head == lr.ptrs(100, 101) and sorted(pages) == [100, 101, 102, 103, 104]
    rule = {p: lr.overflow_rule(pages[p], P) for p in pages}
    assert rule == {100: (52, 0), 101: (44, 2), 102: (52, 0), 103: (44, 1), 104: (9, 0)}
    assert pages[101][P - 9:P - 1] == lr.ptrs(102, 103) and pages[103][P - 5:P - 1] == lr.ptrs(104)
    value = b"".join(pages[p][11:11 + rule[p][0]] for p in sorted(pages))
    assert value == bytes(range(201))
    # a last group exactly full: no successor; one byte more: a successor
    head, pages = lr.write_overflow_value(P, bytes(2 * 52), 2, lambda: next(ids))
    assert len(pages) == 2 and all(lr.overflow_rule(p, P)[1] == 0 for p in pages.values())
    head, pages = lr.write_overflow_value(P, bytes(2 * 52 + 1), 2, lambda: next(ids))
    assert [lr.overflow_rule(pages[p], P) for p in sorted(pages)] == [(52, 0), (44, 1), (9, 0)]


# ---- one page per violation ---------------------------------------------------------------------
@pytest.mark.parametrize("P", [64, 1000])
def test_every_violation_is_rejected(P):
    v = lr.violations(P)
    assert len(v) == 22
    for name, (page, control) in v.items():
        assert len(page) == P and lr.decode_strict(page, P) is None, name
        # the neighbour differs in one byte and decodes
        assert len(control) == P and sum(a != b for a, b in zip(page, control)) == 1, name
        assert lr.decode_strict(control, P) is not None, name
    for name, page in lr.control_pages(P).items():
        got = lr.decode_strict(page, P)
        assert got is not None and lr.as_iter(got) == lr.iter_ref(page, P), name
    assert lr.decode_strict(lr.control_pages(P)["empty"], P) == []
    # the intrinsic overflow-page rule at its edge
    ok = lr.overflow_page(P, bytes(P - 16), [7])
    assert lr.overflow_rule(ok, P) == (P - 16, 1)
    bad = bytearray(ok)
    bad[9:11] = lr.le16(P - 15)
    assert lr.overflow_rule(bytes(bad), P) is None
    bad = bytearray(lr.overflow_page(P, b""))
    bad[P - 1] = 129
    assert lr.overflow_rule(bytes(bad), P) is None


# ---- the forests of the GPU tests ----------------------------------------------------------------
@pytest.fixture(scope="module")
def forests():
    return {name: (c, lr.model(c)) for name, c in lr.forests().items()}


def test_forests_cover_every_bit_and_every_summary_word(forests):
    bits = 0
    nonzero = set()
    for name, (c, (tree, (leaves, s, problems))) in forests.items():
        assert int(s["n_data_pages"]) > 0, name
        for k in range(9):
            if int(s["n_by_bit"][k]):
                bits |= 1 << k
        for k in lr.SUMMARY_DTYPE.names:
            if k not in ("n_by_bit", "first_problem") and int(s[k]):
                nonzero.add(k)
        if int(s["first_problem"]) != lr.NO64:
            nonzero.add("first_problem")
    assert bits == 0x1FF
    assert nonzero == set(lr.SUMMARY_DTYPE.names) - {"n_by_bit"}

    c, (tree, (leaves, s, problems)) = forests["every bit"]
    assert all(int(x) > 0 for x in s["n_by_bit"]), s["n_by_bit"]
    bits = {int(p["page_id"]): int(p["bits"]) for p in problems}
    for row, want in ((100, lr.UNMAPPED), (101, lr.ABSENT), (102, lr.ABSENT), (103, lr.BLANK), (104, lr.CORRUPT),
                      (105, lr.WRONG_TYPE), (106, lr.MALFORMED), (107, lr.MALFORMED), (15, lr.MALFORMED),
                      (120, lr.SHARED), (121, lr.SHARED), (132, lr.SHARED)):
        assert bits[row] == want, row
    assert bits[10] == lr.BAD_CHAIN and bits[11] == lr.BAD_CHAIN            # six kinds; both cycles
    assert bits[12] == lr.BAD_CHAIN | lr.BAD_POINTER
    for row in (108, 109, 122, 123, 131, 141, 13, 14, 9):
        assert row not in bits, row
    assert int(s["n_chain_capped"]) == 2 and int(s["max_groups"]) == lr.MAX_GROUPS
    assert int(leaves[110]["a"]) == lr.MAX_GROUPS and int(leaves[111]["a"]) == lr.MAX_GROUPS // 2
    # both orders of a shared page: the smaller key owns it, whether it bids first or second
    assert (int(leaves[120]["owner"]), int(leaves[120]["a"])) == (11, 2)
    assert (int(leaves[121]["owner"]), int(leaves[121]["a"])) == (9, 2)
    e11 = {e["key"]: e["offset"] for e in lr.decode_strict(bytes(c["pages"][
        ((int(c["table"][11]) >> 3) - c["fp_first"]) * c["P"]:][:c["P"]]), c["P"])}
    assert int(leaves[120]["owner_entry"]) == e11[b"d"] and int(leaves[110]["owner_entry"]) == e11[b"a"]
    assert int(s["n_misplaced_pointers"]) == 1 and int(s["n_refs_to_tree"]) == 3
    assert int(s["n_out_of_range_refs"]) == 2                              # 4000 in an entry, 5000 in a chain page
    # 150; 151 behind the malformed data page; 131 behind the misplaced pointers of 130, which nobody follows
    assert int(s["n_leaked_overflow"]) == 3 and int(leaves[131]["owner"]) == lr.NO
    assert int(leaves[151]["owner"]) == lr.NO and int(leaves[15]["a"]) == 0
    assert int(leaves[108]["b"]) == (c["P"] - 16) | 1 << 16 and int(leaves[14]["a"]) == 0
    assert (int(leaves[14]["owner"]), int(leaves[14]["bits"])) == (14, 0)  # the empty page is healthy

    for name, regions in (("regions 1 P 64", 1), ("regions 64 P 1000", 64), ("regions 65 P 1000", 65),
                          ("regions 129 P 4096", 129), ("regions 129 P 16384", 129)):
        c, (tree, (leaves, s, problems)) = forests[name]
        assert int(leaves[10]["a"]) == regions and int(s["n_problems"]) == 0, name
        assert int(leaves[10]["b"]) == len({0, 63, 64, regions - 1} & set(range(regions))), name
    for n in (1, 64, 65, 128):
        c, (tree, (leaves, s, problems)) = forests[f"group {n} P 1000"]
        assert int(s["n_overflow_pages"]) == n + 1 and int(s["n_problems"]) == 0 and int(s["max_groups"]) == 1
        assert int(s["overflow_value_bytes"]) == (n - 1) * 988 + 1 + 5
    for P in (64, 512, 1000, 4096, 16384):
        c, (tree, (leaves, s, problems)) = forests[f"chains P {P}"]
        assert int(s["n_overflow_values"]) == 6 and int(s["max_groups"]) == 3 and int(s["n_problems"]) == 0
        # pages per value: 2; 2 + 1; 2 + 2 + 1; 4 (exactly full, no successor); 4 + 1; 4 + 4 (the second full)
        assert int(s["n_overflow_ok"]) == int(s["n_overflow_pages"]) == int(s["n_refs"]) == 2 + 3 + 5 + 4 + 5 + 8
        c, (tree, (leaves, s, problems)) = forests[f"plain P {P}"]
        assert int(s["n_overflow_values"]) == 0 and int(s["n_expiring"]) > 0 and int(s["n_compressed"]) > 0
        assert int(s["n_data_ok"]) == int(s["n_data_pages"]) == 3 and int(s["inline_value_bytes"]) > 0
    for P in (1000, 4096):
        c, (tree, (leaves, s, problems)) = forests[f"fuzz pages P {P}"]
        assert int(s["n_by_bit"][5]) > 20 and int(s["n_data_ok"]) + int(s["n_by_bit"][6]) > 20   # both verdicts


# ---- header and binding --------------------------------------------------------------------------
def test_header_and_binding_agree():
    assert pcs.LEAF_NODE_DTYPE.itemsize == 16 and pcs.LEAF_PROBLEM_DTYPE.itemsize == 16
    assert pcs.LEAF_SUMMARY_DTYPE.itemsize == 256
    assert pcs.LEAF_NODE_DTYPE == lr.NODE_DTYPE and pcs.LEAF_PROBLEM_DTYPE == lr.PROBLEM_DTYPE
    assert pcs.LEAF_SUMMARY_DTYPE == lr.SUMMARY_DTYPE
    with open(pcs.HEADER_PATH) as f:
        text = f.read()
    for name in ("pcs_leaf_node", "pcs_leaf_problem", "pcs_leaf_summary", "pcs_leaf_bits", "pcs_leaf_check_dev",
                 "pcs_leaf_check_host"):
        assert name in text, name
    assert re.search(r"#define PCS_LEAF_MAX_GROUPS 4096\b", text) and pcs.LEAF_MAX_GROUPS == 4096 == lr.MAX_GROUPS
    enum = re.search(r"enum pcs_leaf_bits \{(.*?)\};", text, re.S).group(1)
    values = {k: int(v) for k, v in re.findall(r"PCS_LEAF_([A-Z_]+) = (\d+)", enum)}
    assert values == {"BAD_POINTER": 64, "BAD_CHAIN": 128, "SHARED": 256}
    assert (pcs.LEAF_BAD_POINTER, pcs.LEAF_BAD_CHAIN, pcs.LEAF_SHARED) == (lr.BAD_POINTER, lr.BAD_CHAIN, lr.SHARED)
    assert (lr.UNMAPPED, lr.ABSENT, lr.BLANK, lr.CORRUPT, lr.WRONG_TYPE, lr.MALFORMED) == (
        pcs.TREE_UNMAPPED, pcs.TREE_ABSENT, pcs.TREE_BLANK, pcs.TREE_CORRUPT, pcs.TREE_WRONG_TYPE, pcs.TREE_MALFORMED)
    # the structs' fields in the header's order
    for struct, dtype in (("pcs_leaf_summary", lr.SUMMARY_DTYPE), ("pcs_leaf_node", lr.NODE_DTYPE),
                          ("pcs_leaf_problem", lr.PROBLEM_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.sub(r"\[\d+\]", "", x.strip()) for decl in re.findall(r"uint(?:16|32|64)_t ([^;]+);", body)
                  for x in decl.split(",")]
        assert fields == list(dtype.names), struct
    for fn in ("pcs_leaf_check_dev", "pcs_leaf_check_host"):
        assert fn in pcs._SIGS and fn in pcs.header_functions()


# ---- csrc/leaf_check.h under ASAN + UBSan --------------------------------------------------------
def run_logic(*args):
    assert os.path.exists(LOGIC), "build() makes tests/cpp/leaf_logic_test_asan"
    r = subprocess.run([LOGIC, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_logic_violation_battery_and_builder_pages(tmp_path):
    for P in (64, 1000):
        v = lr.violations(P)
        pages = [p for p, _ in v.values()] + [c for _, c in v.values()]
        pages += list(lr.control_pages(P).values())
        for interval in (1, 2, 16, 17):
            for expire in (False, True):
                for pointers in (0, 1, 16, 128):
                    for n in (0, 1, 17, 500):
                        pages.append(lr.build_data_page(P, items(n, expire, pointers), interval)[0])
        path = tmp_path / f"pages_{P}"
        path.write_bytes(b"".join(pages))
        lines = run_logic("pages", str(path), str(P))
        assert len(lines) == len(pages) + 1
        fold = ok = 0
        for k, (line, page) in enumerate(zip(lines, pages)):
            want = lr.decode_strict(page, P)
            text = "malformed" if want is None else " ".join(
                ["ok"] + ["%d/%d/%d" % (e["offset"], e["flags"], e["value_len"]) for e in want])
            assert line == text, k
            assert (want is None) == (k < len(v)), k
            fold = lr.fold_page(fold, want)
            ok += want is not None
        assert lines[-1] == f"fold {fold} ok {ok} pages {len(pages)}"


def test_logic_fuzz_fold_equals_the_model():
    n = 20000
    fold, ok = lr.fuzz_fold(n)
    assert 1000 < ok < n - 1000          # both verdicts occur often
    assert run_logic("fuzz", str(n)) == [f"fold {fold} ok {ok} pages {n}"]
