#!/usr/bin/env python3
"""Manifest replay and scrub live against what they replace.

Device-resident inputs, records stamped with the engine's own manifest checksum:

  a  one image: an 8 MiB snapshot plus 100 log records of 100 entries
  b  1,024 images of 64 KiB (a snapshot of about 40 KiB and five logs each)
  c  1 M class bytes and a mapping table of 1 M rows

Timed in one process, the variants interleaved round by round (medians and
minima), device events around each variant:

  replay call   pcs_manifest_replay_dev, one call for the whole batch, at each
                decode tile of --tiles (PCS_TUNE_REPLAY_TILE); it includes the scan
  scan call     pcs_manifest_scan_dev alone over the same batch
  cpu loop      the parent's way: the images copied to the host and a plain
                one-core C++ loop of the same rules (tools/lab/replay_cpu_loop.cpp,
                which takes no checksum: the scan call has done that)
  live call     pcs_scrub_live_dev
  live cpu      the class bytes and the table copied to the host, one core

  make -C tools/lab libreplay_cpu_loop.so
  python tools/lab/replay_rate.py [--rounds R] [--tiles 256,1024,4096] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import struct
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import eloqstore_amd as pcs  # noqa: E402

DEV = "cuda:0"
ALIGN = 4096
MIB = 1 << 20


def varints(values: np.ndarray) -> bytes:
    """The concatenated varints of a uint64 array (vectorised: one pass per byte position)."""
    v = values.astype(np.uint64)
    n_bytes = np.ones(v.size, dtype=np.int64)
    t = v >> np.uint64(7)
    while t.any():
        n_bytes += t != 0
        t >>= np.uint64(7)
    ends = np.cumsum(n_bytes)
    out = np.zeros(int(ends[-1]) if v.size else 0, dtype=np.uint8)
    starts = ends - n_bytes
    for k in range(10):
        live = n_bytes > k
        if not live.any():
            break
        b = ((v[live] >> np.uint64(7 * k)) & np.uint64(0x7F)).astype(np.uint8)
        b |= (n_bytes[live] > k + 1).astype(np.uint8) << 7
        out[starts[live] + k] = b
    return out.tobytes()


def record(payload: bytes, root: int) -> bytes:
    body = struct.pack("<III", root, root + 1, len(payload)) + payload
    rec = struct.pack("<Q", pcs.manifest_checksum_host(body)) + body
    return rec + bytes(-len(rec) % ALIGN)


def manifest(rng, mapping_bytes: int, logs: int, entries: int) -> bytes:
    pages = mapping_bytes * 10 // 45  # values of 4 and 5 bytes
    values = rng.integers(0, 1 << 28, pages, dtype=np.uint64) << np.uint64(3) | np.uint64(1)
    sec = varints(values)
    img = record(varints(np.array([1 << 28], dtype=np.uint64)) + b"\0" + struct.pack("<I", len(sec)) + sec +
                 struct.pack("<I", 0), 1)
    for j in range(logs):
        pair = np.empty(2 * entries, dtype=np.uint64)
        pair[0::2] = rng.integers(0, pages + 50, entries, dtype=np.uint64)
        pair[1::2] = rng.integers(0, 1 << 28, entries, dtype=np.uint64) << np.uint64(3) | np.uint64(1)
        sec = varints(pair)
        img += record(struct.pack("<I", len(sec)) + sec + struct.pack("<I", 0), 2 + j)
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--tiles", default="256,1024,4096")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("replay_rate needs a GPU")
    cpu = ctypes.CDLL(os.path.join(HERE, "libreplay_cpu_loop.so"))
    tiles = [int(t) for t in a.tiles.split(",")]
    default_tile = pcs.get_tuning(pcs.TUNE_REPLAY_TILE)
    rng = np.random.default_rng(1)
    distinct = [manifest(rng, 40 << 10, 5, 100) for _ in range(16)]
    batches = (("a 8 MiB + 100 logs", [manifest(rng, 8 * MIB, 100, 100)]),
               ("b 1024 x 64 KiB", [distinct[i % 16] + bytes(65536 - len(distinct[i % 16])) for i in range(1024)]))

    variants, checks = [], []
    for label, images in batches:
        offs, total = [], 0
        for img in images:
            offs.append(total)
            total += len(img)
        base = torch.from_numpy(np.frombuffer(b"".join(images), dtype=np.uint8).copy()).to(DEV)
        off = torch.tensor(offs, dtype=torch.int64, device=DEV)
        size = torch.tensor([len(i) for i in images], dtype=torch.int64, device=DEV)
        n = len(images)
        want = []
        for img in images[:16]:
            out = (ctypes.c_uint64 * 4)()
            assert cpu.replay_cpu(img, ctypes.c_uint64(len(img)), ALIGN, out) == 0
            want.append(list(out))
        cap = sum(want[i % len(want)][1] for i in range(n))
        srep = torch.empty((n, 12), dtype=torch.int64, device=DEV)
        rep = torch.empty((n, 16), dtype=torch.int64, device=DEV)
        summ = torch.empty(12, dtype=torch.int64, device=DEV)
        ssum = torch.empty(12, dtype=torch.int64, device=DEV)
        table = torch.empty(cap, dtype=torch.int64, device=DEV)
        n_rec = total // ALIGN + n
        recs = torch.empty((n_rec, 5), dtype=torch.int64, device=DEV)

        def replay_call(tile, base=base, off=off, size=size, total=total, n=n, srep=srep, rep=rep, summ=summ,
                        table=table, cap=cap):
            pcs.set_tuning(pcs.TUNE_REPLAY_TILE, tile)
            pcs.manifest_replay_async(base, off, size, ALIGN, cap, total, n, srep, rep, summ, table)

        def scan_call(base=base, off=off, size=size, total=total, n=n, srep=srep, ssum=ssum, recs=recs, n_rec=n_rec):
            pcs.manifest_scan_async(base, off, size, ALIGN, total, n, srep, ssum, recs, n_rec)

        def cpu_loop(base=base, offs=offs, images=images):
            host = base.cpu().numpy()
            out = (ctypes.c_uint64 * 4)()
            for o, img in zip(offs, images):
                rc = cpu.replay_cpu(ctypes.c_void_p(host.ctypes.data + o), ctypes.c_uint64(len(img)), ALIGN, out)
                assert rc == 0

        for t in tiles:
            variants.append((f"replay call tile {t:<5} {label}", lambda t=t, f=replay_call: f(t), a.rounds))
        variants.append((f"scan call              {label}", scan_call, a.rounds))
        variants.append((f"cpu loop               {label}", cpu_loop, max(3, a.rounds // 4)))
        checks.append((lambda f=replay_call: f(default_tile), summ, rep, n, cap, want))

    # c: scrub live
    n_pages = rows = 1 << 20
    cls = torch.from_numpy(rng.choice(np.array([0, 1, 1, 1, 1, 1, 1, 2], dtype=np.uint8), n_pages)).to(DEV)
    ids = rng.integers(0, 2 * n_pages, rows, dtype=np.uint64)
    ltable = torch.from_numpy((ids << np.uint64(3) | np.uint64(1)).view(np.int64)).to(DEV)
    owner = torch.empty(n_pages, dtype=torch.int32, device=DEV)
    lsum = torch.empty(16, dtype=torch.int64, device=DEV)
    damaged = torch.empty((4096, 2), dtype=torch.int64, device=DEV)

    def live_call():
        pcs.scrub_live_async(cls, n_pages, 0, ltable, rows, owner, lsum, damaged, 4096)

    live_out = (ctypes.c_uint64 * 8)()

    def live_cpu():
        c, t = cls.cpu().numpy(), ltable.cpu().numpy()
        own = np.empty(n_pages, dtype=np.uint32)
        cpu.live_cpu(ctypes.c_void_p(c.ctypes.data), ctypes.c_uint64(n_pages), ctypes.c_uint64(0),
                     ctypes.c_void_p(t.ctypes.data), ctypes.c_uint64(rows), ctypes.c_void_p(own.ctypes.data), live_out)

    variants.append(("live call              c 1 M pages, 1 M rows", live_call, a.rounds))
    variants.append(("live cpu               c 1 M pages, 1 M rows", live_cpu, max(3, a.rounds // 4)))

    for _, f, _ in variants:  # warm every shape
        f()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for r in range(a.rounds):
        for k, (_, f, todo) in enumerate(variants):
            if r >= todo:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    pcs.set_tuning(pcs.TUNE_REPLAY_TILE, default_tile)
    for f, summ, rep, n, cap, want in checks:  # sanity: the timed calls computed what the cpu loop computes
        f()
        s = summ.cpu().numpy().view(np.uint64).tolist()
        assert s[0] == n and s[1] == n and s[5] == cap and s[6] == cap and s[10] == (1 << 64) - 1, s
        r = rep.cpu().numpy().view(np.uint64)
        for i in range(min(n, 16)):
            assert [int(r[i][9]), int(r[i][5]), int(r[i][11])] == want[i][1:], (i, r[i].tolist(), want[i])
    live_call()
    live_cpu()
    ls = lsum.cpu().numpy().view(np.uint64).tolist()
    assert [ls[2], ls[3], ls[5], ls[6], ls[7], ls[8], ls[9], ls[10]] == list(live_out), (ls, list(live_out))

    lines = [f"replay_rate: device-resident inputs at align {ALIGN}, up to {a.rounds} interleaved rounds, device events "
             f"around each variant ({pcs.version()}); default tile {default_tile}",
             f"{'variant':<46} {'rounds':>6} {'median us':>12} {'min us':>12}"]
    for (name, _, _), t in zip(variants, times):
        lines.append(f"{name:<46} {len(t):6d} {statistics.median(t):12.1f} {min(t):12.1f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
