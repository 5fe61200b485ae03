#!/usr/bin/env python3
"""Scrub extents against what they replace.

Class bytes come from real scrubs of 1 M and 8 M device-resident pages (256 B
pages: the extents read one class byte per page whatever the page size): all
valid, the second half blank (a fallocated tail), one corrupt page in 1000.
Timed in one process, the variants interleaved round by round (medians and
minima over the rounds):

  extents cap 0       pcs_scrub_extents_dev, summary only (two launches)
  extents cap 1024    summary and the first 1024 runs (three launches)
  scrub call          pcs_pages_scrub_dev on the same pages, for scale: its hash
                      pass plus its own three-launch reduction
  D2H + numpy         the alternative: the class bytes copied to pinned host
                      memory and run-scanned on one core (np.diff), wall clock

The device variants are timed with device events around each call, the host
alternative with the wall clock around copy, wait and scan.  The split between
the scrub's reduction kernels and the extent kernels comes from a kernel trace
of this script (--trace-rounds keeps that run short), see
profiles/extents/extent_rate.txt.

  python tools/lab/extent_rate.py [--rounds R] [--trace-rounds T] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import eloqstore_amd as pcs  # noqa: E402

DEV = "cuda:0"
P = 256


def make_pages(n, seed):
    buf = torch.empty(n * P, dtype=torch.uint8, device=DEV)
    pcs.gen_pages(buf, P, n, seed, 0)
    pcs.pages_stamp(buf, P, n)
    return buf


def host_run_scan(cls: np.ndarray):
    """The single-core alternative: runs and the written extent from the bytes."""
    starts = np.flatnonzero(np.diff(cls)) + 1
    written = np.flatnonzero(cls != pcs.PAGE_BLANK)
    return starts.size + 1, int(written[-1]) + 1 if written.size else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--trace-rounds", type=int, default=0, help="short run for a kernel trace: this many rounds, 1 M pages only, no report file")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("extent_rate needs a GPU")
    rounds = a.trace_rounds or a.rounds
    sizes = (1 << 20,) if a.trace_rounds else (1 << 20, 8 << 20)

    variants, checks = [], []
    for n in sizes:
        valid = make_pages(n, 0xE87E01 + n)
        half = valid.clone()
        half.view(n, P)[n // 2:] = 0
        sparse = valid.clone()
        pcs.flip_byte(sparse, P, n, every=1000, byte_offset=10)
        label = f"{n >> 20} M"
        for kind, pages in (("valid", valid), ("half blank", half), ("1/1000 bad", sparse)):
            cls, ty, summ, lst = pcs.pages_scrub_async(pages, P, n)
            torch.cuda.synchronize()
            ext = torch.empty(12, dtype=torch.int64, device=DEV)
            runs = torch.empty((1024, 3), dtype=torch.int64, device=DEV)
            pinned = torch.empty(n, dtype=torch.uint8, pin_memory=True)

            def ext_call(cap, cls=cls, ext=ext, runs=runs, n=n):
                return lambda: pcs.scrub_extents_async(cls, n, ext, runs if cap else None, cap)

            def host_call(cls=cls, pinned=pinned):
                def run():
                    pinned.copy_(cls, non_blocking=True)
                    torch.cuda.synchronize()
                    return host_run_scan(pinned.numpy())
                return run

            variants.append((f"extents cap 0      {label} {kind}", ext_call(0), "dev"))
            variants.append((f"extents cap 1024   {label} {kind}", ext_call(1024), "dev"))
            if kind == "valid":
                variants.append((f"scrub call (256 B) {label} {kind}",
                                 lambda pages=pages, n=n, cls=cls, ty=ty, summ=summ, lst=lst:
                                 pcs.pages_scrub_async(pages, P, n, cls, ty, summ, lst, 1024), "dev"))
            variants.append((f"D2H + numpy        {label} {kind}", host_call(), "host"))
            # what the timed calls must compute
            want_runs, want_written = host_run_scan(cls.cpu().numpy())
            checks.append((ext_call(1024), ext, want_runs, want_written, n))
        del valid

    for _, f, _ in variants:  # warm every shape
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(rounds):
        for k, (_, f, how) in enumerate(variants):
            if how == "dev":
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
            else:
                t0 = time.perf_counter()
                f()
                times[k].append((time.perf_counter() - t0) * 1e6)
    for f, ext, want_runs, want_written, n in checks:  # sanity: the timed calls computed what they should
        f()
        d = pcs.extent_dict(ext.cpu().tolist())
        assert (d["n_pages"], d["n_runs"], d["written_pages"]) == (n, want_runs, want_written), d

    lines = [f"extent_rate: class bytes of real scrubs ({P} B pages), {rounds} interleaved rounds, device events around "
             f"each device call, wall clock around the host alternative ({pcs.version()})",
             f"{'variant':<40} {'median us':>10} {'min us':>10}"]
    for (name, _, _), t in zip(variants, times):
        lines.append(f"{name:<40} {statistics.median(t):10.1f} {min(t):10.1f}")
    text = "\n".join(lines)
    print(text)
    if a.out and not a.trace_rounds:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
