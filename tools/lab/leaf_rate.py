#!/usr/bin/env python3
"""Tree check and leaf check against what they replace.

Device-resident inputs, 4 KiB pages, a three-level tree (a non-leaf root over
990 leaf-index pages of 990 children each: what 4 KiB index pages hold with
four-byte keys), data pages made by the builder port of tests/leaf_ref.py and
replicated on the device with their sibling links and pointers patched in:

  plain      980,100 data pages of small inline values
  overflow   15,000 data pages of 64 entries, one value in sixteen overflowing
             into one group of 16 pointers: 960,000 overflow pages

Timed in one process with device events around each whole call (medians and
minima over --rounds, after a warm-up call of each):

  tree call  pcs_tree_check_dev
  leaf call  pcs_leaf_check_dev over the tree call's nodes
  cpu loops  the pages, class bytes and table copied to the host (timed) and the
             same rules as one-core C++ loops (tools/lab/leaf_cpu_loop.cpp,
             compiled from csrc/tree_check.h and csrc/leaf_check.h); their
             counts are compared with the device's summaries

  make -C tools/lab "$PWD/tools/lab/libleaf_cpu_loop.so"
  python tools/lab/leaf_rate.py [--rounds R] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import struct
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eloqstore_amd as pcs  # noqa: E402
import leaf_ref as lr  # noqa: E402
import tree_ref as tr  # noqa: E402

DEV = "cuda:0"
P = 4096
FAN = 990
FP_FIRST = 1 << 20
DATA0 = 1000                     # the first data row; rows 1 .. FAN are the leaf-index pages


def index_pages(n_data):
    """The root and the leaf-index pages over data rows DATA0 .. DATA0 + n_data."""
    leaves = (n_data + FAN - 1) // FAN
    assert leaves <= FAN
    out = []
    for k in range(leaves):
        ids = list(range(DATA0 + k * FAN, DATA0 + min(n_data, (k + 1) * FAN)))
        page, added = tr.build_index_page(P, True, ids[0], [(struct.pack(">I", i), i) for i in ids[1:]], 64)
        assert added == len(ids) - 1
        out.append(page)
    rows = list(range(1, 1 + leaves))
    root, added = tr.build_index_page(P, False, rows[0], [(struct.pack(">I", i), i) for i in rows[1:]], 64)
    assert added == leaves - 1
    return root, out


def le32_bytes(ids):
    """An int64 device tensor of ids < 2^32 as (n, 4) little-endian bytes."""
    return ids.to(torch.int32).contiguous().view(torch.uint8).reshape(-1, 4)


def build(n_data, overflow):
    """-> (pages, cls, table, roots) on the device and the number of file pages."""
    templates, offsets = [], None
    for t in range(16):
        b = lr.DataPageBuilder(P, 16)
        i = 0
        while True:
            key = b"key-%02d-%06d" % (t, i)
            if overflow and i % 16 == 7:
                ok = b.add(key, bytes(64), True, 1000 + i)
            else:
                ok = b.add(key, bytes([65 + (i + t) % 26]) * (20 + (i * 7) % 13), False, 1000 + i, (i % 4 == 0) * 99)
            if not ok or (overflow and b.cnt == 64):
                break
            i += 1
        page = b.finish()
        off = [e["value_offset"] for e in lr.decode_strict(page, P) if e["flags"] & 1]
        assert offsets is None or off == offsets          # one layout, so one patch serves every page
        offsets = off
        templates.append(np.frombuffer(page, np.uint8))
    per_page = len(offsets) * 16                           # overflow pages per data page
    n_over = n_data * per_page
    root, leaves = index_pages(n_data)
    n_index = 1 + len(leaves)
    n_pages = n_index + n_data + n_over
    pages = torch.empty((n_pages, P), dtype=torch.uint8, device=DEV)
    pages[:n_index] = torch.from_numpy(np.frombuffer(root + b"".join(leaves), np.uint8).reshape(-1, P).copy()).to(DEV)
    data = pages[n_index:n_index + n_data]
    idx = torch.arange(n_data, device=DEV)
    data.copy_(torch.from_numpy(np.stack(templates)).to(DEV)[idx % 16])
    rows = DATA0 + idx
    prev, nxt = rows - 1, rows + 1
    prev[0] = nxt[-1] = tr.NO
    data[:, 11:15] = le32_bytes(prev)
    data[:, 15:19] = le32_bytes(nxt)
    over0 = DATA0 + n_data                                 # the first overflow row
    for s, off in enumerate(offsets):
        ids = over0 + (idx[:, None] * len(offsets) + s) * 16 + torch.arange(16, device=DEV)[None, :]
        data[:, off:off + 64] = le32_bytes(ids.reshape(-1)).reshape(n_data, 64)
    if n_over:
        ov = np.frombuffer(lr.overflow_page(P, bytes(range(256)) * 15 + bytes(P - 12 - 3840)), np.uint8)
        pages[n_index + n_data:] = torch.from_numpy(ov.copy()).to(DEV)
    table = np.full(over0 + n_over, tr.INVALID, dtype=np.uint64)
    table[0] = tr.fp(FP_FIRST)
    table[1:n_index] = (np.arange(FP_FIRST + 1, FP_FIRST + n_index, dtype=np.uint64) << np.uint64(3)) | np.uint64(1)
    table[DATA0:] = (np.arange(FP_FIRST + n_index, FP_FIRST + n_pages, dtype=np.uint64) << np.uint64(3)) | np.uint64(1)
    cls = torch.ones(n_pages, dtype=torch.uint8, device=DEV)
    d_table = torch.from_numpy(table.view(np.int64)).to(DEV)
    roots = torch.from_numpy(np.array([0, tr.NO], dtype=np.uint64).view(np.int64)).to(DEV)
    return pages.reshape(-1), cls, d_table, roots, n_pages


def timed(fn, rounds):
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def case(name, n_data, overflow, rounds, lib, say):
    pages, cls, table, roots, n_pages = build(n_data, overflow)
    rows = table.numel()
    nodes = torch.empty((rows, 2), dtype=torch.int64, device=DEV)
    tsum = torch.empty(32, dtype=torch.int64, device=DEV)
    leaves = torch.empty((rows, 2), dtype=torch.int64, device=DEV)
    lsum = torch.empty(32, dtype=torch.int64, device=DEV)
    plist = torch.empty((1024, 2), dtype=torch.int64, device=DEV)

    def tree():
        pcs.tree_check_async(pages, P, n_pages, FP_FIRST, cls, table, roots, 2, rows, nodes, tsum, plist, 1024)

    def leaf():
        pcs.leaf_check_async(pages, P, n_pages, FP_FIRST, cls, table, nodes, rows, leaves, lsum, plist, 1024)

    tree()
    leaf()
    torch.cuda.synchronize()
    ts = tsum.cpu().numpy().view(np.uint64).view(pcs.TREE_SUMMARY_DTYPE)[0]
    ls = lsum.cpu().numpy().view(np.uint64).view(pcs.LEAF_SUMMARY_DTYPE)[0]
    t_med, t_min = timed(tree, rounds)
    l_med, l_min = timed(leaf, rounds)
    # the yardstick: the bytes to the host, then one core
    t0 = time.perf_counter()
    h_pages, h_cls, h_table = pages.cpu().numpy(), cls.cpu().numpy(), table.cpu().numpy().view(np.uint64)
    copy_s = time.perf_counter() - t0
    h_roots = np.array([0, tr.NO], dtype=np.uint64)
    state = np.zeros(rows, dtype=np.uint8)
    out_t, out_l = np.zeros(4, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    vp = ctypes.c_void_p
    t0 = time.perf_counter()
    lib.tree_cpu_loop(vp(h_pages.ctypes.data), P, n_pages, FP_FIRST, vp(h_cls.ctypes.data), vp(h_table.ctypes.data), rows,
                      vp(h_roots.ctypes.data), 2, vp(state.ctypes.data), vp(out_t.ctypes.data))
    tree_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    lib.leaf_cpu_loop(vp(h_pages.ctypes.data), P, n_pages, FP_FIRST, vp(h_cls.ctypes.data), vp(h_table.ctypes.data), rows,
                      vp(state.ctypes.data), vp(out_l.ctypes.data))
    leaf_s = time.perf_counter() - t0
    assert [int(x) for x in out_t] == [int(ts["n_reached"]), int(ts["n_data"]), int(ts["n_problems"]), int(ts["n_refs"])], \
        (out_t, ts)
    assert [int(x) for x in out_l] == [int(ls[k]) for k in (
        "n_entries", "n_overflow_values", "n_refs", "n_overflow_pages", "n_problems", "n_leaked_overflow",
        "overflow_value_bytes", "inline_value_bytes")], (out_l, ls)
    gib = n_pages * P / 2 ** 30
    say(f"{name}: {n_pages} file pages ({gib:.2f} GiB), {rows} table rows, {int(ts['n_reached'])} reached, "
        f"{int(ls['n_data_pages'])} data pages, {int(ls['n_entries'])} entries, {int(ls['n_overflow_values'])} overflow "
        f"values, {int(ls['n_overflow_pages'])} overflow pages, {int(ts['n_problems'])} + {int(ls['n_problems'])} problems")
    say(f"  tree call   median {t_med:9.3f} ms  min {t_min:9.3f} ms   ({rounds} rounds)")
    say(f"  leaf call   median {l_med:9.3f} ms  min {l_min:9.3f} ms")
    say(f"  D2H copy    {copy_s * 1e3:9.1f} ms (pageable host memory, once)")
    say(f"  tree cpu    {tree_s * 1e3:9.1f} ms one core; with the copy {(copy_s + tree_s) * 1e3:9.1f} ms = "
        f"{(copy_s + tree_s) * 1e3 / t_med:7.0f} x the tree call")
    say(f"  leaf cpu    {leaf_s * 1e3:9.1f} ms one core; with the copy {(copy_s + leaf_s) * 1e3:9.1f} ms = "
        f"{(copy_s + leaf_s) * 1e3 / l_med:7.0f} x the leaf call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scale", type=int, default=1, help="divide the page counts by this (a quick look)")
    a = ap.parse_args()
    lib = ctypes.CDLL(os.path.join(HERE, "libleaf_cpu_loop.so"))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.tree_cpu_loop.argtypes = [vp, u64, u64, u64, vp, vp, u64, vp, ctypes.c_uint32, vp, vp]
    lib.leaf_cpu_loop.argtypes = [vp, u64, u64, u64, vp, vp, u64, vp, vp]
    lib.tree_cpu_loop.restype = lib.leaf_cpu_loop.restype = None
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"leaf_rate: {torch.cuda.get_device_name(0)}, {pcs.version()}, page size {P}, device events around each call")
    case("plain", FAN * FAN // a.scale, False, a.rounds, lib, say)
    case("overflow", 15000 // a.scale, True, a.rounds, lib, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
