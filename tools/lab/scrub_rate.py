#!/usr/bin/env python3
"""Scrub against validate on device-resident pages.

Times pcs_pages_validate_dev and pcs_pages_scrub_dev with device events, the
variants interleaved round by round in one process (medians and minima over
the rounds), on 1 M x 4 KiB pages by default:

  validate            this build's validate kernel (the baseline)
  validate (parent)   the same call in another build of the library
                      (--parent-lib: libeloqstore_pcs.so of the commit before
                      the scrub), when given
  scrub valid         every page valid
  scrub half blank    the second half of the batch all zero (a fallocated tail)
  scrub 1/1000 bad    one page in 1000 flipped

and validate / scrub valid once on the 16 KiB shape (the split kernel).  The
scrub call is the hash pass plus the three reduction launches; their split
comes from a kernel trace of this script (--trace-rounds keeps that run
short), see profiles/scrub/scrub_rate.txt.

  python tools/lab/scrub_rate.py [--pages N] [--rounds R] [--parent-lib SO] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import eloqstore_amd as pcs  # noqa: E402

DEV = "cuda:0"


def parent_validate(path):
    so = ctypes.CDLL(path)
    f = so.pcs_pages_validate_dev
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int] + [ctypes.c_void_p] * 3
    f.restype = ctypes.c_int
    so.pcs_abi_version.restype = ctypes.c_int
    return f, so.pcs_abi_version()


def make_pages(P, n, seed):
    buf = torch.empty(n * P, dtype=torch.uint8, device=DEV)
    pcs.gen_pages(buf, P, n, seed, 0)
    buf.view(n, P)[:, 8] = (torch.arange(n, device=DEV) % 4).to(torch.uint8)
    pcs.pages_stamp(buf, P, n)
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--trace-rounds", type=int, default=0, help="short run for a kernel trace: this many rounds, no report file")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scrub_rate needs a GPU")
    rounds = a.trace_rounds or a.rounds
    P, n = 4096, a.pages
    n16 = max(16, n // 4)
    stream = torch.cuda.current_stream().cuda_stream

    valid = make_pages(P, n, 0x5C2B01)
    half = valid.clone()
    half.view(n, P)[n // 2:] = 0
    sparse = valid.clone()
    pcs.flip_byte(sparse, P, n, every=1000, byte_offset=10)
    valid16 = make_pages(16384, n16, 0x5C2B02)

    ok = torch.empty(n, dtype=torch.uint8, device=DEV)
    fb = torch.empty(1, dtype=torch.int64, device=DEV)
    cls = torch.empty(n, dtype=torch.uint8, device=DEV)
    ty = torch.empty(n, dtype=torch.uint8, device=DEV)
    summ = torch.empty(12, dtype=torch.int64, device=DEV)
    lst = torch.empty(1024, dtype=torch.int64, device=DEV)

    def validate(buf, psize, cnt):
        return lambda: pcs.pages_validate(buf, psize, cnt, ok=ok, first_bad=fb)

    def scrub(buf, psize, cnt):
        return lambda: pcs.pages_scrub_async(buf, psize, cnt, cls, ty, summ, lst, 1024)

    variants = [("validate              4 KiB", validate(valid, P, n), n * P),
                ("scrub valid           4 KiB", scrub(valid, P, n), n * P),
                ("scrub half blank      4 KiB", scrub(half, P, n), n * P),
                ("scrub 1/1000 bad      4 KiB", scrub(sparse, P, n), n * P),
                ("validate             16 KiB", validate(valid16, 16384, n16), n16 * 16384),
                ("scrub valid          16 KiB", scrub(valid16, 16384, n16), n16 * 16384)]
    if a.parent_lib:
        pv, abi = parent_validate(a.parent_lib)

        def parent(buf, psize, cnt):
            def run():
                rc = pv(buf.data_ptr(), psize, cnt, 0, ok.data_ptr(), fb.data_ptr(), stream)
                assert rc == 0, rc
            return run
        variants.insert(1, (f"validate (parent, ABI {abi}) 4 KiB", parent(valid, P, n), n * P))
        variants.append((f"validate (parent, ABI {abi}) 16 KiB", parent(valid16, 16384, n16), n16 * 16384))

    for _, f, _ in variants:  # warm every shape
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(rounds):
        for k, (_, f, _) in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    # sanity: the timed calls computed what they should
    d = pcs.summary_dict(summ.cpu().tolist())
    assert d["n_pages"] == n16 and d["n_ok"] == n16, d
    pcs.pages_scrub_async(sparse, P, n, cls, ty, summ, lst, 1024)
    d = pcs.summary_dict(summ.cpu().tolist())
    assert d["n_corrupt"] == (n + 999) // 1000 and d["n_blank"] == 0, d
    pcs.pages_scrub_async(half, P, n, cls, ty, summ, lst, 1024)
    d = pcs.summary_dict(summ.cpu().tolist())
    assert d["n_blank"] == n - n // 2 and d["n_corrupt"] == 0, d

    lines = [f"scrub_rate: {n} x 4 KiB and {n16} x 16 KiB device-resident pages, {rounds} interleaved rounds, "
             f"device events around each call ({pcs.version()})",
             f"{'variant':<36} {'median us':>10} {'min us':>10} {'TB/s (median)':>14}  vs validate"]
    base = {}
    for (name, _, nbytes), t in zip(variants, times):
        med, mn = statistics.median(t), min(t)
        shape = name.split()[-2] + " " + name.split()[-1]
        if name.startswith("validate  "):
            base[shape] = med
        rel = f"{med / base[shape] - 1:+.1%}" if shape in base else ""
        lines.append(f"{name:<36} {med:10.1f} {mn:10.1f} {nbytes / med / 1e6:14.3f}  {rel}")
    text = "\n".join(lines)
    print(text)
    if a.out and not a.trace_rounds:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
