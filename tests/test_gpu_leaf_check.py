"""Leaf check on the GPU: pcs_leaf_check_dev / _host, the C++ form and
page_checksum_tool --leaves against tests/leaf_ref.py.  The generated forests
are those tests/test_leaf_cpu.py checks against the model for coverage (every
bit, every summary word, both orders of a shared page), so none of the
comparisons here is vacuous.  Every device call runs with poisoned outputs and
guard words past every array, pages 8 bytes into an allocation, class bytes at
an odd address, and the inputs checked untouched."""
import os
import subprocess

import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
import leaf_ref as lr
import manifest_ref as mr
import replay_ref as rr
import tree_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0x5A5A5A5A5A5A5A5A
_MODEL = {}


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for k in want.dtype.names:
        assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist()[:12], want[k].tolist()[:12])


def model(name, case, cap=None):
    """(tree nodes, (leaves, summary, problems)) of the model, computed once per named case and cap."""
    key = (name, cap)
    if name is None or key not in _MODEL:
        tkey = (name, "tree")
        if name is None or tkey not in _MODEL:
            t = tr.check(case["pages"], case["P"], case["fp_first"], case["cls"], case["table"], case["roots"])[0]
            if name is not None:
                _MODEL[tkey] = t
        else:
            t = _MODEL[tkey]
        r = (t, lr.check(case["pages"], case["P"], case["fp_first"], case["cls"], case["table"], t, cap))
        if name is None:
            return r
        _MODEL[key] = r
    return _MODEL[key]


def leaf_dev(case, name=None, cap=None, leaves=True, stream=None, what=""):
    """The tree check and one leaf check on the device, the latter with poisoned outputs and guard words,
    checked against the model -> the raw output bytes."""
    P, fp_first = case["P"], case["fp_first"]
    pages, cls, table, roots = case["pages"], case["cls"], case["table"], case["roots"]
    n, rows = cls.size, table.size
    if cap is None:
        cap = int(model(name, case)[1][1]["n_problems"]) + 2
    wtree, (wleaves, ws, wprob) = model(name, case, cap)
    # the pages 8 bytes into an allocation and the class bytes at an odd address
    d_pages = torch.zeros(n * P + 16, dtype=torch.uint8, device=DEV)
    d_pages[8:8 + n * P] = torch.from_numpy(pages.copy()).to(DEV)
    d_cls = torch.zeros(n + 3, dtype=torch.uint8, device=DEV)
    d_cls[1:1 + n] = torch.from_numpy(cls.copy()).to(DEV)
    d_table = torch.from_numpy(table.view(np.int64).copy()).to(DEV) if rows else None
    d_roots = torch.from_numpy(np.array(roots, dtype=np.uint64).view(np.int64)).to(DEV)
    d_leaves = torch.full((rows + 2, 2), SENTINEL, dtype=torch.int64, device=DEV) if leaves else False
    d_sum = torch.full((34,), 0x1234567, dtype=torch.int64, device=DEV)
    d_list = torch.full((cap + 2, 2), SENTINEL, dtype=torch.int64, device=DEV)
    if stream is not None:   # the inputs and the poison were written on torch's current stream
        stream.wait_stream(torch.cuda.current_stream())
    d_tree, _, _ = pcs.tree_check_async(d_pages[8:], P, n, fp_first, d_cls[1:], d_table, d_roots, len(roots), rows,
                                        problem_cap=0, stream=stream)
    pcs.leaf_check_async(d_pages[8:], P, n, fp_first, d_cls[1:], d_table, d_tree, rows, d_leaves, d_sum,
                         d_list if cap else None, cap, stream)
    torch.cuda.synchronize()
    s = d_sum.cpu().numpy().view(np.uint64)
    assert (s[32:] == 0x1234567).all(), what
    same(s[:32].copy().view(lr.SUMMARY_DTYPE), np.array([ws]), what + " summary")
    out = [s[:32].tobytes()]
    if leaves:
        nd = d_leaves.cpu().numpy().view(np.uint64)
        same(np.ascontiguousarray(nd[:rows]).view(np.uint8).view(lr.NODE_DTYPE).reshape(-1), wleaves, what + " leaves")
        assert (nd[rows:] == SENTINEL).all(), what
        out.append(nd[:rows].tobytes())
    lst = d_list.cpu().numpy().view(np.uint64)
    listed = int(ws["n_listed"])
    same(np.ascontiguousarray(lst[:listed]).view(np.uint8).view(lr.PROBLEM_DTYPE).reshape(-1), wprob, what + " list")
    assert (lst[listed:] == SENTINEL).all(), what
    out.append(lst[:listed].tobytes())
    # the inputs are untouched, the tree's nodes among them
    assert np.array_equal(d_pages[8:8 + n * P].cpu().numpy(), pages) and np.array_equal(d_cls[1:1 + n].cpu().numpy(), cls)
    if rows:
        assert np.array_equal(d_table.cpu().numpy().view(np.uint64), table)
        got_tree = np.ascontiguousarray(d_tree[:rows].cpu().numpy()).view(np.uint8).view(tr.NODE_DTYPE).reshape(-1)
        same(got_tree, wtree, what + " tree nodes")
    return b"".join(out), (wleaves, ws, wprob)


FORESTS = lr.forests()


@pytest.mark.parametrize("name", list(FORESTS))
def test_forest_equals_the_model(name):
    leaf_dev(FORESTS[name], name, what=name)


def test_caps_nulls_and_empty_inputs():
    c = FORESTS["every bit"]
    n = int(model("every bit", c)[1][1]["n_problems"])
    assert n > 10
    for cap in (0, 1, n - 1, n):
        leaf_dev(c, "every bit", cap=cap, what=f"cap {cap}")
    leaf_dev(c, "every bit", leaves=False)
    leaf_dev(c, "every bit", leaves=False, cap=0)
    # n_pages == 0: the tree reads no page, so no data page is checked
    empty = dict(c, pages=np.zeros(0, np.uint8), cls=np.zeros(0, np.uint8))
    _, (leaves, s, problems) = leaf_dev(empty, what="n_pages 0")
    assert int(s["n_data_pages"]) == 0 and int(s["n_problems"]) == 0 and int(s["table_size"]) == c["table"].size
    # table_size == 0
    none = dict(c, table=np.zeros(0, np.uint64))
    _, (leaves, s, problems) = leaf_dev(none, what="table_size 0")
    assert int(s["n_data_pages"]) == 0 and int(s["first_problem"]) == lr.NO64 and int(s["n_pages"]) == c["cls"].size
    leaf_dev(dict(none, pages=np.zeros(0, np.uint8), cls=np.zeros(0, np.uint8)), cap=0, leaves=False)


def test_limits_are_checked_on_the_host():
    d = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    t = torch.zeros(8, dtype=torch.int64, device=DEV)
    nodes = torch.zeros((8, 2), dtype=torch.int64, device=DEV)
    s = torch.full((32,), 0x1234567, dtype=torch.int64, device=DEV)
    lv = torch.full((8, 2), SENTINEL, dtype=torch.int64, device=DEV)
    for P, rows, tree_nodes in ((31, 8, nodes), (65536, 8, nodes), (512, 1 << 32, nodes), (512, 8, None)):
        with pytest.raises(pcs.PcsError) as e:
            pcs.leaf_check_async(d, P, 1, 0, d, t, tree_nodes, rows, lv, s)
        assert e.value.code == pcs.PCS_ERR_INVALID
    with pytest.raises(pcs.PcsError) as e:                     # the window leaves the file page ids
        pcs.leaf_check_async(d, 512, 8, (1 << 61) - 4, d, t, nodes, 8, lv, s)
    assert e.value.code == pcs.PCS_ERR_INVALID
    with pytest.raises(pcs.PcsError) as e:                     # a misaligned leaf array
        pcs.leaf_check_async(d, 512, 8, 0, d, t, nodes, 8, d[4:], s)
    assert e.value.code == pcs.PCS_ERR_INVALID
    torch.cuda.synchronize()
    assert (s.cpu().numpy() == 0x1234567).all() and (lv.cpu().numpy().view(np.uint64) == SENTINEL).all()  # no launch
    leaf_dev(FORESTS["regions 1 P 64"], "regions 1 P 64")


def test_two_streams_give_identical_bytes():
    a, b = FORESTS["every bit"], FORESTS["chains P 512"]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got = {"a": [], "b": []}
    for _ in range(2):
        got["a"].append(leaf_dev(a, "every bit", stream=s1)[0])
        got["b"].append(leaf_dev(b, "chains P 512", stream=s2)[0])
    assert got["a"][0] == got["a"][1] and got["b"][0] == got["b"][1]
    # and really at the same time: both enqueued before either is waited for
    outs = []
    for c, s in ((a, s1), (b, s2), (a, s2), (b, s1)):
        n, rows = c["cls"].size, c["table"].size
        t = [torch.from_numpy(c["pages"].copy()).to(DEV), torch.from_numpy(c["cls"].copy()).to(DEV),
             torch.from_numpy(c["table"].view(np.int64).copy()).to(DEV),
             torch.from_numpy(np.array(c["roots"], dtype=np.uint64).view(np.int64)).to(DEV)]
        s.wait_stream(torch.cuda.current_stream())
        tree = pcs.tree_check_async(t[0], c["P"], n, c["fp_first"], t[1], t[2], t[3], len(c["roots"]), rows,
                                    problem_cap=0, stream=s)
        outs.append((t, tree, pcs.leaf_check_async(t[0], c["P"], n, c["fp_first"], t[1], t[2], tree[0], rows,
                                                   problem_cap=64, stream=s)))
    torch.cuda.synchronize()
    raw = [o[2][1].cpu().numpy().tobytes() + o[2][0].cpu().numpy().tobytes() for o in outs]
    assert raw[0] == raw[2] and raw[1] == raw[3]
    for r, g, c in ((raw[0], got["a"][0], a), (raw[1], got["b"][0], b)):   # summary and leaves of the checked calls
        assert r[:256] == g[:256]                                           # n_listed too: both caps exceed it
        assert r[256:] == g[256:256 + 16 * c["table"].size]


# ---- stamp -> scrub -> replay -> tree check -> leaf check, all on the device ---------------------------
SHIFT, FILE_ID = 6, 7


def chain_forest():
    P = 4096
    c = lr.chains(P, fp_first=FILE_ID << SHIFT)
    assert c["cls"].size <= 1 << SHIFT
    b = mr.Builder(4096)
    b.add(rr.snapshot_payload(c["fp_first"] + c["cls"].size, rr.values_section([int(v) for v in c["table"]])),
          root=c["roots"][0], ttl_root=c["roots"][1])
    return c, bytes(b.data())


def test_stamp_scrub_replay_tree_leaf_chain():
    c, img = chain_forest()
    P, n = c["P"], c["cls"].size
    pages = torch.from_numpy(c["pages"].copy()).to(DEV)
    pcs.pages_stamp(pages, P, n)
    cls, types, d, listed = pcs.pages_scrub(pages, P, n)
    assert int(d["n_ok"]) == n
    base = torch.from_numpy(np.frombuffer(img, np.uint8).copy()).to(DEV)
    off = torch.zeros(1, dtype=torch.int64, device=DEV)
    size = torch.full((1,), len(img), dtype=torch.int64, device=DEV)
    rows = c["table"].size
    _, reports, rsum, table = pcs.manifest_replay_async(base, off, size, 4096, rows)
    roots = reports.data_ptr() + 3 * 8           # root and ttl_root of the device report: no host round trip

    def run():
        tree = pcs.tree_check_async(pages, P, n, c["fp_first"], cls, table, roots, 2, rows, problem_cap=0)
        leaves, s, problems = pcs.leaf_check(pages, P, n, c["fp_first"], cls, table, tree[0])
        host_pages = pages.cpu().numpy()
        wt = tr.check(host_pages, P, c["fp_first"], cls.cpu().numpy(), c["table"], c["roots"])[0]
        want = lr.check(host_pages, P, c["fp_first"], cls.cpu().numpy(), c["table"], wt)
        same(leaves, want[0], "leaves")
        same(np.array([s]).view(lr.SUMMARY_DTYPE), np.array([want[1]]), "summary")
        same(problems, want[2][:1024], "problems")
        return leaves, s, problems

    leaves, s, problems = run()
    assert int(s["n_problems"]) == 0 and int(s["n_overflow_values"]) == 6 and int(s["n_overflow_pages"]) == 27
    assert int(s["n_leaked_overflow"]) == 0
    # zero the end page of the three-group value's first group and scrub again: the chain breaks there
    data = lr.decode_strict(bytes(c["pages"][((int(c["table"][10]) >> 3) - c["fp_first"]) * P:][:P]), P)
    end = int.from_bytes(data[2]["value"][4:8], "little")
    pages.view(n, P)[(int(c["table"][end]) >> 3) - c["fp_first"]].zero_()
    cls, types, d, listed = pcs.pages_scrub(pages, P, n)
    assert int(d["n_blank"]) == 1
    leaves, s, problems = run()
    assert int(s["n_by_bit"][2]) == 1 and int(s["n_by_bit"][7]) == 1 and int(s["n_problems"]) == 2
    assert int(s["n_leaked_overflow"]) == 3      # the two groups behind the blank page


# ---- host form --------------------------------------------------------------------------------------
def test_host_form_equals_the_device_form():
    for name in ("every bit", "chains P 4096", "regions 65 P 1000"):
        c = FORESTS[name]
        wtree, want = model(name, c, 100)
        tnodes, tsum, leaves, s, problems = pcs.leaf_check_host(c["pages"], c["P"], c["fp_first"], c["cls"], c["table"],
                                                                c["roots"], 100)
        same(tnodes, wtree, name)
        same(leaves, want[0], name)
        same(np.array([s]).view(lr.SUMMARY_DTYPE), np.array([want[1]]), name)
        same(problems, want[2], name)
        assert int(tsum["n_reached"]) == int((wtree["parent"] != tr.NO).sum())
    tnodes, tsum, leaves, s, problems = pcs.leaf_check_host(c["pages"], c["P"], c["fp_first"], c["cls"], c["table"],
                                                            c["roots"], 0, want_nodes=False)
    assert tnodes is None and leaves is None and problems.size == 0 and int(s["n_entries"]) == int(want[1]["n_entries"])
    # without class bytes the call scrubs: stamped pages are OK, a flipped overflow page is corrupt
    c, img = chain_forest()
    pages = torch.from_numpy(c["pages"].copy()).to(DEV)
    pcs.pages_stamp(pages, c["P"], c["cls"].size)
    host = pages.cpu().numpy().copy()
    ov = (int(c["table"][1003]) >> 3) - c["fp_first"]
    host[ov * c["P"] + 200] ^= 0x40
    cls = np.ones(c["cls"].size, np.uint8)
    cls[ov] = 0
    wt = tr.check(host, c["P"], c["fp_first"], cls, c["table"], c["roots"])[0]
    want = lr.check(host, c["P"], c["fp_first"], cls, c["table"], wt)
    tnodes, tsum, leaves, s, problems = pcs.leaf_check_host(host, c["P"], c["fp_first"], None, c["table"], c["roots"])
    same(leaves, want[0], "scrubbed")
    same(np.array([s]).view(lr.SUMMARY_DTYPE), np.array([want[1]]), "scrubbed")
    same(problems, want[2], "scrubbed")
    assert int(s["n_by_bit"][3]) == 1
    pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 1)
    try:
        with pytest.raises(pcs.PcsError) as e:
            pcs.leaf_check_host(host, c["P"], c["fp_first"], None, c["table"], c["roots"])
        assert e.value.code == pcs.PCS_ERR_HIP
    finally:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 0)
    tnodes, tsum, leaves, s, problems = pcs.leaf_check_host(host, c["P"], c["fp_first"], None, c["table"], c["roots"])
    same(leaves, want[0], "after the injected failure")


# ---- C++ form ---------------------------------------------------------------------------------------
def test_cpp_form(tmp_path):
    exe = os.path.join(HERE, "cpp", "leaf_test")
    assert os.path.exists(exe), "build() makes tests/cpp/leaf_test"
    c = FORESTS["every bit"]
    (tmp_path / "pages").write_bytes(c["pages"].tobytes())
    (tmp_path / "table").write_bytes(c["table"].tobytes())
    (tmp_path / "classes").write_bytes(c["cls"].tobytes())
    r = subprocess.run([exe, str(tmp_path / "pages"), str(c["P"]), str(c["fp_first"]), str(tmp_path / "table"),
                        ",".join(str(x) for x in c["roots"]), str(tmp_path / "classes"), "6"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    wtree, (wleaves, ws, wprob) = model("every bit", c, 6)
    got, problems, tree_problems = {}, [], []
    for line in r.stdout.splitlines():
        k, *v = line.split()
        if k == "problem":
            problems.append(tuple(int(x) for x in v))
        elif k == "tree_problem":
            tree_problems.append(tuple(int(x) for x in v))
        else:
            got[k] = int(v[0])
    for k in lr.SUMMARY_DTYPE.names:
        if k == "n_listed":
            continue
        if k == "n_by_bit":
            for j, x in enumerate(ws[k].tolist()):
                assert got[f"{k}_{j}"] == x, (k, j)
        else:
            assert got[k] == int(ws[k]), k
    assert problems == [tuple(int(x) for x in p) for p in wprob.tolist()] and len(problems) == 6
    fold = 0
    for w0, w1 in wleaves.view(np.uint64).reshape(-1, 2).tolist():
        fold = ((fold * tr.GOLD + w0) * tr.GOLD + w1) & tr.M64
    assert got["leaf_fold"] == fold
    fold = 0
    for w0, w1 in wtree.view(np.uint64).reshape(-1, 2).tolist():
        fold = ((fold * tr.GOLD + w0) * tr.GOLD + w1) & tr.M64
    assert got["node_fold"] == fold
    bad = np.nonzero((wtree["parent"] != tr.NO) & (wtree["bits"] != 0))[0]
    assert tree_problems == [(int(p), int(wtree[p]["parent"]), int(wtree[p]["bits"]), int(wtree[p]["depth"])) for p in bad]
    assert got["tree_n_problems"] == bad.size and got["tree_n_reached"] == int((wtree["parent"] != tr.NO).sum())


# ---- CLI ---------------------------------------------------------------------------------------------
def run_tool(*args):
    return subprocess.run([pcs.TOOL_PATH, *args], capture_output=True, text=True, timeout=120)


def test_cli_leaves(tmp_path):
    c, img = chain_forest()
    P, n = c["P"], c["cls"].size
    pages = torch.from_numpy(c["pages"].copy()).to(DEV)
    pcs.pages_stamp(pages, P, n)
    good = pages.cpu().numpy().copy()
    manifest = tmp_path / "manifest_3"
    manifest.write_bytes(img)
    data = tmp_path / f"data_{FILE_ID}_3"

    def run(host, *more, flag="--leaves"):
        data.write_bytes(host.tobytes())
        return run_tool(flag, str(manifest), str(P), str(SHIFT), str(data), *more)

    def slot(row):
        return (int(c["table"][row]) >> 3) - c["fp_first"]

    r = run(good)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[:-2] == run(good, flag="--tree").stdout.splitlines()      # the --tree report comes first
    wt, (wl, ws, wp) = lr.model(c)
    assert lines[-2] == ("leaves data_pages %d ok %d entries 6 overflow_values 6 expiring 0 compressed 0 inline_bytes 0"
                         % (int(ws["n_data_pages"]), int(ws["n_data_ok"])))
    assert lines[-1] == ("overflow pages 27 ok 27 value_bytes %d refs 27 extra 0 out_of_range 0 to_tree 0 misplaced 0 "
                         "capped 0 max_groups 3 leaked 0" % int(ws["overflow_value_bytes"]))
    # a blank chain page: exit 3, the page printed with its owner; the pages behind it are leaked
    bad = good.copy()
    bad[slot(1003) * P:(slot(1003) + 1) * P] = 0
    r = run(bad)
    assert r.returncode == 3, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    owner = int(lr.model(dict(c, cls=np.where(np.arange(n) == slot(1003), 2, 1).astype(np.uint8)))[1][0][1003]["owner"])
    assert any(x.startswith(f"  leaf problem: page_id 1003 owner {owner} entry ") and x.endswith(" blank") for x in lines)
    assert any(x.startswith(f"  leaf problem: page_id {owner} owner {owner} entry 0 bad-chain") for x in lines)
    # a corrupt chain page beats a blank one: exit 2
    bad[slot(1000) * P + 300] ^= 1
    r = run(bad)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert any(x.endswith(" corrupt") and x.startswith("  leaf problem: page_id 1000 ") for x in r.stdout.splitlines())
    # a malformed data page: exit 2 (the page is stamped again so that its checksum holds)
    bad = torch.from_numpy(good.copy()).to(DEV)
    bad.view(n, P)[slot(10), 19] = 1                      # shared != 0 in the first entry
    pcs.pages_stamp(bad, P, n)
    r = run(bad.cpu().numpy())
    assert r.returncode == 2 and "  leaf problem: page_id 10 owner 10 entry 0 malformed" in r.stdout.splitlines()
    # the exit code --tree would give passes through: a blank data page is the tree's finding
    bad = good.copy()
    bad[slot(10) * P:(slot(10) + 1) * P] = 0
    r = run(bad)
    assert r.returncode == 3 == run(bad, flag="--tree").returncode
    assert "leaf problem" not in r.stdout and " leaked " in r.stdout.splitlines()[-1]
    # chain pages in a file that is not given are absent, which never fails the run
    table = c["table"].copy()
    table[1003] = tr.fp((FILE_ID + 1) << SHIFT)
    b = mr.Builder(4096)
    b.add(rr.snapshot_payload((FILE_ID + 2) << SHIFT, rr.values_section([int(v) for v in table])), root=0,
          ttl_root=tr.NO)
    manifest.write_bytes(bytes(b.data()))
    r = run(good)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert any(x.startswith("  leaf problem: page_id 1003 ") and x.endswith(" absent") for x in r.stdout.splitlines())
    # a manifest that cannot be replayed: one line, exit 2, as --tree
    broken = bytearray(img)
    broken[30] ^= 1
    (tmp_path / "manifest_9").write_bytes(bytes(broken))
    r = run_tool("--leaves", str(tmp_path / "manifest_9"), str(P), str(SHIFT), str(data))
    assert r.returncode == 2 and r.stdout == f"{tmp_path / 'manifest_9'}: manifest cannot be replayed: not-replayable\n"
    r = run_tool("--leaves", str(manifest), str(P), str(SHIFT))
    assert r.returncode == 1 and "--leaves" in r.stderr
