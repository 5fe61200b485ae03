"""Tree check on the GPU: pcs_tree_check_dev / _host, the C++ form and
page_checksum_tool --tree against tests/tree_ref.py.  The generated forests are
those tests/test_tree_cpu.py checks against the model for coverage (every bit,
both tie-breaks, the depth cap), so none of the comparisons here is vacuous.
Every device call runs with poisoned outputs and guard words past every array."""
import os
import subprocess

import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
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
    key = (name, cap)
    if name is None or key not in _MODEL:
        r = tr.check(case["pages"], case["P"], case["fp_first"], case["cls"], case["table"], case["roots"], cap)
        if name is None:
            return r
        _MODEL[key] = r
    return _MODEL[key]


def tree_dev(case, name=None, cap=None, nodes=True, stream=None, what=""):
    """One device call with poisoned outputs and guard words, checked against the model -> the raw output bytes."""
    P, fp_first = case["P"], case["fp_first"]
    pages, cls, table, roots = case["pages"], case["cls"], case["table"], case["roots"]
    n, rows = cls.size, table.size
    if cap is None:
        cap = int(model(name, case)[1]["n_problems"]) + 2
    wnodes, ws, wprob = model(name, case, cap)
    # the pages 8 bytes into an allocation and the class bytes at an odd address
    d_pages = torch.zeros(n * P + 16, dtype=torch.uint8, device=DEV)
    d_pages[8:8 + n * P] = torch.from_numpy(pages.copy()).to(DEV)
    d_cls = torch.zeros(n + 3, dtype=torch.uint8, device=DEV)
    d_cls[1:1 + n] = torch.from_numpy(cls.copy()).to(DEV)
    d_table = torch.from_numpy(table.view(np.int64).copy()).to(DEV) if rows else None
    d_roots = torch.from_numpy(np.array(roots, dtype=np.uint64).view(np.int64)).to(DEV)
    d_nodes = torch.full((rows + 2, 2), SENTINEL, dtype=torch.int64, device=DEV) if nodes else False
    d_sum = torch.full((34,), 0x1234567, dtype=torch.int64, device=DEV)
    d_list = torch.full((cap + 2, 2), SENTINEL, dtype=torch.int64, device=DEV)
    if stream is not None:   # the inputs and the poison were written on torch's current stream
        stream.wait_stream(torch.cuda.current_stream())
    pcs.tree_check_async(d_pages[8:], P, n, fp_first, d_cls[1:], d_table, d_roots, len(roots), rows, d_nodes, d_sum,
                         d_list if cap else None, cap, stream)
    torch.cuda.synchronize()
    s = d_sum.cpu().numpy().view(np.uint64)
    assert (s[32:] == 0x1234567).all(), what
    same(s[:32].copy().view(tr.SUMMARY_DTYPE), np.array([ws]), what + " summary")
    out = [s[:32].tobytes()]
    if nodes:
        nd = d_nodes.cpu().numpy().view(np.uint64)
        same(np.ascontiguousarray(nd[:rows]).view(np.uint8).view(tr.NODE_DTYPE).reshape(-1), wnodes, what + " nodes")
        assert (nd[rows:] == SENTINEL).all(), what
        out.append(nd[:rows].tobytes())
    lst = d_list.cpu().numpy().view(np.uint64)
    listed = int(ws["n_listed"])
    same(np.ascontiguousarray(lst[:listed]).view(np.uint8).view(tr.PROBLEM_DTYPE).reshape(-1), wprob, what + " list")
    assert (lst[listed:] == SENTINEL).all(), what
    out.append(lst[:listed].tobytes())
    # the inputs are untouched
    assert np.array_equal(d_pages[8:8 + n * P].cpu().numpy(), pages) and np.array_equal(d_cls[1:1 + n].cpu().numpy(), cls)
    return b"".join(out), (wnodes, ws, wprob)


FORESTS = tr.forests()


@pytest.mark.parametrize("name", list(FORESTS))
def test_forest_equals_the_model(name):
    tree_dev(FORESTS[name], name, what=name)


def test_two_parents_at_one_depth_lowest_id_wins():
    c = dict(tr.tie_breaks(), roots=[0])
    _, (nodes, s, problems) = tree_dev(c, "tie breaks, one root")
    assert int(nodes[10]["parent"]) == 2 and int(nodes[10]["depth"]) == 2


def test_roots_empty_beyond_the_table_and_a_data_page():
    c = tr.three_levels(512)
    rows = c["table"].size
    # only empty trees; a root beyond the table is counted in n_refs and n_out_of_range_refs and reaches nothing
    for roots in ([tr.NO], [tr.NO, 1 << 63], [rows], [rows + 5, tr.NO - 1, tr.NO]):
        _, (nodes, s, problems) = tree_dev(dict(c, roots=roots), what=str(roots))
        assert int(s["n_reached"]) == 0 and int(s["max_depth"]) == tr.NO64 and int(s["n_problems"]) == 0
        assert int(s["n_out_of_range_refs"]) == int(s["n_refs"]) == sum(1 for r in roots if r < tr.NO)
        assert int(s["n_unreached_mapped"]) == int(s["n_mapped"])
    _, (nodes, s, problems) = tree_dev(dict(c, roots=[100] * 8))      # a data page as every root
    assert problems.tolist() == [(100, 100, tr.WRONG_TYPE, 0)] and int(s["n_extra_refs"]) == 7


def test_caps_nulls_and_empty_inputs():
    c = FORESTS["every bit"]
    n = int(model("every bit", c)[1]["n_problems"])
    assert n > 10
    for cap in (0, n - 1, n, 1):
        tree_dev(c, "every bit", cap=cap, what=f"cap {cap}")
    tree_dev(c, "every bit", nodes=False)
    tree_dev(c, "every bit", nodes=False, cap=0)
    # n_pages == 0: whatever the tree points to is absent
    empty = dict(c, pages=np.zeros(0, np.uint8), cls=np.zeros(0, np.uint8))
    _, (nodes, s, problems) = tree_dev(empty, what="n_pages 0")
    assert int(s["n_by_bit"][1]) > 0 and int(s["n_unreached_unread"]) > 0
    # table_size == 0: every root lies beyond it
    none = dict(c, table=np.zeros(0, np.uint64))
    _, (nodes, s, problems) = tree_dev(none, what="table_size 0")
    assert int(s["n_out_of_range_refs"]) == 2 and int(s["n_reached"]) == 0
    tree_dev(dict(none, pages=np.zeros(0, np.uint8), cls=np.zeros(0, np.uint8)), cap=0, nodes=False)


def test_limits_are_checked_on_the_host():
    c = FORESTS["wide 1"]
    d = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    t = torch.zeros(8, dtype=torch.int64, device=DEV)
    for P, n_roots in ((31, 1), (65536, 1), (512, 0), (512, 9)):
        with pytest.raises(pcs.PcsError) as e:
            pcs.tree_check_async(d, P, 1, 0, d, t, t, n_roots)
        assert e.value.code == pcs.PCS_ERR_INVALID
    with pytest.raises(pcs.PcsError) as e:
        pcs.tree_check_async(d, 512, 1, 0, d, t, t, 1, table_size=1 << 32)
    assert e.value.code == pcs.PCS_ERR_INVALID
    tree_dev(c, "wide 1")


def test_two_streams_give_identical_bytes():
    a, b = FORESTS["random pages P 1000"], FORESTS["tie breaks"]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got = {"a": [], "b": []}
    for _ in range(2):
        got["a"].append(tree_dev(a, "random pages P 1000", stream=s1)[0])
        got["b"].append(tree_dev(b, "tie breaks", stream=s2)[0])
    assert got["a"][0] == got["a"][1] and got["b"][0] == got["b"][1]
    # and really at the same time: both enqueued before either is waited for
    outs = []
    for c, s in ((a, s1), (b, s2), (a, s2), (b, s1)):
        n, rows = c["cls"].size, c["table"].size
        t = [torch.from_numpy(c["pages"].copy()).to(DEV), torch.from_numpy(c["cls"].copy()).to(DEV),
             torch.from_numpy(c["table"].view(np.int64).copy()).to(DEV),
             torch.from_numpy(np.array(c["roots"], dtype=np.uint64).view(np.int64)).to(DEV)]
        s.wait_stream(torch.cuda.current_stream())
        outs.append((t, pcs.tree_check_async(t[0], c["P"], n, c["fp_first"], t[1], t[2], t[3], len(c["roots"]), rows,
                                             problem_cap=64, stream=s)))
    torch.cuda.synchronize()
    raw = [o[1][0].cpu().numpy().tobytes() + o[1][1].cpu().numpy().tobytes() for o in outs]
    assert raw[0] == raw[2] and raw[1] == raw[3]
    for r, g, c in ((raw[0], got["a"][0], a), (raw[1], got["b"][0], b)):   # the nodes of the checked calls above
        assert r[:-256] == g[256:256 + 16 * c["table"].size]


# ---- stamp -> scrub -> replay -> tree check, all on the device --------------------------------------
def chain_forest():
    P = 4096
    c = tr.three_levels(P, fp_first=7 << 6)
    b = mr.Builder(4096)
    b.add(rr.snapshot_payload(c["fp_first"] + c["cls"].size, rr.values_section([int(v) for v in c["table"]])),
          root=c["roots"][0], ttl_root=c["roots"][1])
    return c, bytes(b.data())


def test_stamp_scrub_replay_tree_check_chain():
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
    # root and ttl_root are words 3 and 4 of the device report: no host round trip
    roots = reports.data_ptr() + 3 * 8

    def run():
        nodes, s, problems = pcs.tree_check(pages, P, n, c["fp_first"], cls, table, roots, 2)
        host_pages = pages.cpu().numpy()
        want = tr.check(host_pages, P, c["fp_first"], cls.cpu().numpy(), c["table"], c["roots"])
        same(nodes, want[0], "nodes")
        same(np.array([s]).view(tr.SUMMARY_DTYPE), np.array([want[1]]), "summary")
        same(problems, want[2][:1024], "problems")
        return s

    s = run()
    assert int(s["n_problems"]) == 0 and (int(s["n_nonleaf"]), int(s["n_leaf_index"]), int(s["n_data"])) == (1, 6, 27)
    assert s["unreached_by_type"].tolist() == [0, 0, 1, 1, 0, 0]
    # zero one reached leaf-index page and scrub again: its subtree is lost
    leaf_fp = int(c["table"][2]) >> 3
    pages.view(n, P)[leaf_fp - c["fp_first"]].zero_()
    cls, types, d, listed = pcs.pages_scrub(pages, P, n)
    assert int(d["n_blank"]) == 1
    s = run()
    assert int(s["n_by_bit"][2]) == 1 and int(s["first_problem"]) == 2
    assert s["unreached_by_type"].tolist() == [0, 0, 1 + 5, 1, 0, 0] and int(s["n_data"]) == 20
    assert int(s["n_by_bit"][7]) == 2         # the chain is cut on both sides of the lost pages


# ---- host form --------------------------------------------------------------------------------------
def test_host_form_equals_the_device_form():
    for name in ("every bit", "three levels P 4096", "tie breaks"):
        c = FORESTS[name]
        want = model(name, c, 100)
        nodes, s, problems = pcs.tree_check_host(c["pages"], c["P"], c["fp_first"], c["cls"], c["table"], c["roots"], 100)
        same(nodes, want[0], name)
        same(np.array([s]).view(tr.SUMMARY_DTYPE), np.array([want[1]]), name)
        same(problems, want[2], name)
    nodes, s, problems = pcs.tree_check_host(c["pages"], c["P"], c["fp_first"], c["cls"], c["table"], c["roots"], 0,
                                             want_nodes=False)
    assert nodes is None and problems.size == 0 and int(s["n_reached"]) == int(model("tie breaks", c)[1]["n_reached"])
    # without class bytes the call scrubs: stamped pages are OK, a flipped one is corrupt
    c, img = chain_forest()
    pages = torch.from_numpy(c["pages"].copy()).to(DEV)
    pcs.pages_stamp(pages, c["P"], c["cls"].size)
    host = pages.cpu().numpy().copy()
    leaf = (int(c["table"][3]) >> 3) - c["fp_first"]
    host[leaf * c["P"] + 200] ^= 0x40
    cls = np.ones(c["cls"].size, np.uint8)
    cls[leaf] = 0
    want = tr.check(host, c["P"], c["fp_first"], cls, c["table"], c["roots"])
    nodes, s, problems = pcs.tree_check_host(host, c["P"], c["fp_first"], None, c["table"], c["roots"])
    same(nodes, want[0], "scrubbed")
    same(np.array([s]).view(tr.SUMMARY_DTYPE), np.array([want[1]]), "scrubbed")
    same(problems, want[2], "scrubbed")
    assert int(s["n_by_bit"][3]) == 1
    pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 1)
    try:
        with pytest.raises(pcs.PcsError) as e:
            pcs.tree_check_host(host, c["P"], c["fp_first"], None, c["table"], c["roots"])
        assert e.value.code == pcs.PCS_ERR_HIP
    finally:
        pcs.set_tuning(pcs.TUNE_FAIL_INJECT, 0)
    nodes, s, problems = pcs.tree_check_host(host, c["P"], c["fp_first"], None, c["table"], c["roots"])
    same(nodes, want[0], "after the injected failure")


# ---- C++ form ---------------------------------------------------------------------------------------
def test_cpp_form(tmp_path):
    exe = os.path.join(HERE, "cpp", "tree_test")
    assert os.path.exists(exe), "build() makes tests/cpp/tree_test"
    c = FORESTS["every bit"]
    (tmp_path / "pages").write_bytes(c["pages"].tobytes())
    (tmp_path / "table").write_bytes(c["table"].tobytes())
    (tmp_path / "classes").write_bytes(c["cls"].tobytes())
    r = subprocess.run([exe, str(tmp_path / "pages"), str(c["P"]), str(c["fp_first"]), str(tmp_path / "table"),
                        ",".join(str(x) for x in c["roots"]), str(tmp_path / "classes"), "6"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    wnodes, ws, wprob = model("every bit", c, 6)
    got, problems = {}, []
    for line in r.stdout.splitlines():
        k, *v = line.split()
        if k == "problem":
            problems.append(tuple(int(x) for x in v))
        else:
            got[k] = int(v[0])
    for k in tr.SUMMARY_DTYPE.names:
        if k == "n_listed":
            continue
        if k in ("n_by_bit", "unreached_by_type"):
            for j, x in enumerate(ws[k].tolist()):
                assert got[f"{k}_{j}"] == x, (k, j)
        else:
            assert got[k] == int(ws[k]), k
    assert problems == [tuple(int(x) for x in p) for p in wprob.tolist()] and len(problems) == 6
    fold = 0
    for w0, w1 in wnodes.view(np.uint64).reshape(-1, 2).tolist():
        fold = ((fold * tr.GOLD + w0) * tr.GOLD + w1) & tr.M64
    assert got["node_fold"] == fold


# ---- CLI ---------------------------------------------------------------------------------------------
SHIFT, FILE_ID = 6, 7


def run_tool(*args):
    return subprocess.run([pcs.TOOL_PATH, *args], capture_output=True, text=True, timeout=120)


def test_cli_tree(tmp_path):
    c, img = chain_forest()
    P, n = c["P"], c["cls"].size
    assert n <= 1 << SHIFT and c["fp_first"] == FILE_ID << SHIFT
    pages = torch.from_numpy(c["pages"].copy()).to(DEV)
    pcs.pages_stamp(pages, P, n)
    good = pages.cpu().numpy().copy()
    manifest = tmp_path / "manifest_3"
    manifest.write_bytes(img)
    data = tmp_path / f"data_{FILE_ID}_3"

    def run(host, *more):
        data.write_bytes(host.tobytes())
        return run_tool("--tree", str(manifest), str(P), str(SHIFT), str(data), *more)

    def slot(row):
        return (int(c["table"][row]) >> 3) - c["fp_first"]

    r = run(good)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == "tree root 0 reached 31 nonleaf 1 leaf_index 5 data 25 problems 0 max_depth 2"
    assert lines[1] == "tree ttl_root 50 reached 3 nonleaf 0 leaf_index 1 data 2 problems 0 max_depth 1"
    assert lines[2] == "unreached mapped 2 nonleaf 0 leaf_index 0 data 1 overflow 1 deleted 0 other 0 unread 0"
    assert len(lines) == 3
    # a blank leaf-index page: exit 3, the page printed with its parent
    bad = good.copy()
    bad[slot(2) * P:(slot(2) + 1) * P] = 0
    r = run(bad)
    assert r.returncode == 3, (r.stdout, r.stderr)
    assert "  problem: page_id 2 parent 0 depth 1 blank" in r.stdout.splitlines()
    assert r.stdout.splitlines()[-1].startswith("unreached mapped 7 nonleaf 0 leaf_index 0 data 6 overflow 1 ")
    # a corrupt page beats a blank one: exit 2
    bad[slot(3) * P + 300] ^= 1
    r = run(bad)
    assert r.returncode == 2, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert "  problem: page_id 2 parent 0 depth 1 blank" in lines
    assert "  problem: page_id 3 parent 0 depth 1 corrupt" in lines
    assert any(x.endswith(" bad-link") for x in lines)
    # a file of another id that is not given: its pages are absent, which never fails the run
    c2 = tr.three_levels(P, fp_first=FILE_ID << SHIFT)
    table = c2["table"].copy()
    table[60] = tr.fp((FILE_ID + 1) << SHIFT)           # a data page of the ttl tree lives in file 8
    b = mr.Builder(4096)
    b.add(rr.snapshot_payload((FILE_ID + 2) << SHIFT, rr.values_section([int(v) for v in table])), root=0, ttl_root=50)
    manifest.write_bytes(bytes(b.data()))
    r = run(good)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert "  problem: page_id 60 parent 50 depth 1 absent" in lines
    assert "  problem: page_id 61 parent 50 depth 1 bad-link" in lines
    # with file 8 given the window spans both files
    other = tmp_path / f"data_{FILE_ID + 1}_3"
    page = torch.from_numpy(np.frombuffer(tr.data_page(P, tr.NO, 61), np.uint8).copy()).to(DEV)
    pcs.pages_stamp(page, P, 1)
    other.write_bytes(page.cpu().numpy().tobytes())
    r = run(good, str(other))
    assert r.returncode == 0 and "problem:" not in r.stdout, (r.stdout, r.stderr)
    # a span that cannot be resident: exit 1 with a message
    far = tmp_path / "data_4000000000_3"
    far.write_bytes(good.tobytes())
    r = run(good, str(far))
    assert r.returncode == 1 and "does not fit in device memory" in r.stderr
    # a manifest that cannot be replayed: one line, exit 2
    broken = bytearray(img)
    broken[30] ^= 1
    (tmp_path / "manifest_9").write_bytes(bytes(broken))
    r = run_tool("--tree", str(tmp_path / "manifest_9"), str(P), str(SHIFT), str(data))
    assert r.returncode == 2 and r.stdout == f"{tmp_path / 'manifest_9'}: manifest cannot be replayed: not-replayable\n"
    r = run_tool("--tree", str(manifest), str(P), str(SHIFT), str(tmp_path / "data_7"))
    assert r.returncode == 1 and "Not a data file name" in r.stderr
