#!/usr/bin/env python3
"""Manifest scan against what it replaces.

Three device-resident batches, records stamped with the engine's own manifest
checksum:

  a  one 8 MiB image of one-slot records (2,048 records)
  b  1,024 images of 64 KiB (16 one-slot records each)
  c  one image: a 64 MiB snapshot plus 100 log records

Timed in one process, the variants interleaved round by round (medians and
minima over the rounds), device events around each variant:

  scan call       pcs_manifest_scan_dev, one call for the whole batch, at each
                  walk tile of --tiles (PCS_TUNE_MANIFEST_WALK_TILE)
  record loop     the parent's way: the images copied to the host, a host walk
                  over the headers there, then pcs_manifest_checksum_dev once
                  per record and one copy of the digests back

A loop is as long as its host-side launches take, so it runs fewer rounds
(--loop-calls bounds the calls per variant).  Only the serial LDS walk exists:
pointer doubling was not built, so there is no second walk variant to time.

  python tools/lab/manifest_scan_rate.py [--rounds R] [--tiles 256,1024,2048,4096] [--loop-calls C] [--out FILE]
"""
import argparse
import os
import statistics
import struct
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import eloqstore_amd as pcs  # noqa: E402

DEV = "cuda:0"
ALIGN = 4096
MIB = 1 << 20


def record(payload: bytes, root: int) -> bytes:
    body = struct.pack("<III", root, root + 1, len(payload)) + payload
    rec = struct.pack("<Q", pcs.manifest_checksum_host(body)) + body
    return rec + bytes(-len(rec) % ALIGN)


def small_records(k: int) -> list:
    rng = np.random.default_rng(k)
    return [record(rng.integers(0, 256, 40 + 229 * j % 3000, dtype=np.uint8).tobytes(), j) for j in range(k)]


def batches():
    recs = small_records(16)
    a = b"".join(recs[j % 16] for j in range(8 * MIB // ALIGN))
    b = [b"".join(recs[(i + j) % 16] for j in range(16)) for i in range(1024)]
    snap = record(np.random.default_rng(7).integers(0, 256, 64 * MIB - 20, dtype=np.uint8).tobytes(), 9)
    c = snap + b"".join(recs[j % 16] for j in range(100))
    return (("a 1 x 8 MiB", [a]), ("b 1024 x 64 KiB", b), ("c 64 MiB + 100", [c]))


def host_walk(img: bytes):
    """(offset, content length) of every record, by the walk rule."""
    out, o, size = [], 0, len(img)
    while size - o >= 20:
        ln = struct.unpack_from("<I", img, o + 16)[0]
        if o + 20 + ln > size:
            break
        out.append((o, 12 + ln))
        o = (o + 20 + ln + ALIGN - 1) // ALIGN * ALIGN
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--tiles", default="256,1024,2048,4096")
    ap.add_argument("--loop-calls", type=int, default=40000, help="most per-record calls one loop variant makes over all its rounds")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("manifest_scan_rate needs a GPU")
    tiles = [int(t) for t in a.tiles.split(",")]
    default_tile = pcs.get_tuning(pcs.TUNE_MANIFEST_WALK_TILE)

    variants, checks = [], []
    for label, images in batches():
        offs, total = [], 0
        for img in images:
            offs.append(total)
            total += len(img)  # every image here is a multiple of ALIGN
        base = torch.from_numpy(np.frombuffer(b"".join(images), dtype=np.uint8).copy()).to(DEV)
        off = torch.tensor(offs, dtype=torch.int64, device=DEV)
        size = torch.tensor([len(i) for i in images], dtype=torch.int64, device=DEV)
        n = len(images)
        n_records = sum(len(host_walk(i)) for i in images)
        reports = torch.empty((n, 12), dtype=torch.int64, device=DEV)
        summ = torch.empty(12, dtype=torch.int64, device=DEV)
        recs = torch.empty((n_records, 5), dtype=torch.int64, device=DEV)
        digests = torch.empty(n_records, dtype=torch.int64, device=DEV)

        def scan_call(tile, base=base, off=off, size=size, total=total, n=n, reports=reports, summ=summ, recs=recs,
                      n_records=n_records):
            pcs.set_tuning(pcs.TUNE_MANIFEST_WALK_TILE, tile)
            pcs.manifest_scan_async(base, off, size, ALIGN, total, n, reports, summ, recs, n_records)

        def record_loop(base=base, offs=offs, images=images, digests=digests):
            host = base.cpu().numpy().tobytes()  # the parent has no header gather: the images come back whole
            k, stored = 0, []
            for o, img in zip(offs, images):
                for ro, content in host_walk(host[o:o + len(img)]):
                    pcs._call("pcs_manifest_checksum_dev", base.data_ptr() + o + ro + 8, content,
                              digests.data_ptr() + 8 * k, pcs._stream(None))
                    stored.append(struct.unpack_from("<Q", host, o + ro)[0])
                    k += 1
            got = digests.cpu().numpy().view(np.uint64)
            assert (got == np.array(stored, dtype=np.uint64)).all()

        for t in tiles:
            variants.append((f"scan call tile {t:<5} {label}", lambda t=t, f=scan_call: f(t), a.rounds))
        variants.append((f"record loop          {label}", record_loop, max(2, min(a.rounds, a.loop_calls // n_records))))
        checks.append((lambda f=scan_call: f(default_tile), summ, n, n_records))

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
    pcs.set_tuning(pcs.TUNE_MANIFEST_WALK_TILE, default_tile)
    for f, summ, n, n_records in checks:  # sanity: the timed calls computed what they should
        f()
        s = summ.cpu().numpy().view(np.uint64).tolist()
        assert s[:4] == [n, n_records, n_records, 0] and s[4] == n and s[11] == (1 << 64) - 1, s

    lines = [f"manifest_scan_rate: device-resident images at align {ALIGN}, up to {a.rounds} interleaved rounds, "
             f"device events around each variant ({pcs.version()}); default tile {default_tile}; serial LDS walk only",
             f"{'variant':<40} {'rounds':>6} {'median us':>12} {'min us':>12}"]
    for (name, _, _), t in zip(variants, times):
        lines.append(f"{name:<40} {len(t):6d} {statistics.median(t):12.1f} {min(t):12.1f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
