#!/usr/bin/env python3
"""Scrub files against what they replace.

Class and type bytes come from one real scrub of 1 M device-resident 4 KiB
pages (one corrupt page in 1000, one zeroed page inside the written pages, the
last quarter blank), cut four ways: 1024 files of 1024 pages, 4 files of
262,144 pages, 1 file of 1 M pages and 65,536 files of 16 pages.  Timed in one
process, the variants interleaved round by round (medians and minima over the
rounds), device events around each variant:

  files call      pcs_scrub_files_dev, one call for the whole cut (four launches)
  extents loop    the parent's first way: pcs_scrub_extents_dev (cap 0) once per
                  file on the file's slice of the class bytes; gives the written
                  extent and the holes, no census
  scrub loop      the parent's second way: pcs_pages_scrub_dev once per file on
                  the file's pages (hashes them again); gives the census, no holes

A loop is as long as its host-side launches take, so the loops over many files
run fewer rounds (--loop-calls bounds the calls per variant).  For the one-file
cut the yardstick is the kernel time of the two existing reductions, k_scrub_*
plus k_extent_*, against k_files_*: take it from a kernel trace of this script
(--trace-rounds keeps that run short and leaves the loops out), see
profiles/files/files_rate.txt.

  python tools/lab/files_rate.py [--rounds R] [--trace-rounds T] [--only-cut K] [--loop-calls C] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import eloqstore_amd as pcs  # noqa: E402

DEV = "cuda:0"
P = 4096
N = 1 << 20
CUTS = ((1024, "1024 x 1024"), (262144, "4 x 262144"), (N, "1 x 1 M"), (16, "65536 x 16"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--trace-rounds", type=int, default=0, help="short run for a kernel trace: this many rounds, no loops, no report file")
    ap.add_argument("--loop-calls", type=int, default=200000, help="most per-file calls one loop variant makes over all its rounds")
    ap.add_argument("--only-cut", type=int, default=-1, help="time one cut only (0-3), e.g. for a kernel trace of that cut")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("files_rate needs a GPU")
    rounds = a.trace_rounds or a.rounds

    pages = torch.empty(N * P, dtype=torch.uint8, device=DEV)
    pcs.gen_pages(pages, P, N, 0xF11E01, 0)
    pcs.pages_stamp(pages, P, N)
    pcs.flip_byte(pages, P, N, every=1000, byte_offset=10)
    pages.view(N, P)[3 * N // 4:] = 0
    pages.view(N, P)[5001] = 0
    cls, types, summ, lst = pcs.pages_scrub_async(pages, P, N)
    torch.cuda.synchronize()
    cls_h = cls.cpu().numpy()

    variants, checks = [], []
    for index, (per_file, label) in enumerate(CUTS):
        if a.only_cut not in (-1, index):
            continue
        n_files = N // per_file
        first = torch.arange(0, N + 1, per_file, dtype=torch.int64, device=DEV)
        reports = torch.empty((n_files, 16), dtype=torch.int64, device=DEV)
        fsum = torch.empty(12, dtype=torch.int64, device=DEV)
        bad = torch.empty(1024, dtype=torch.int64, device=DEV)
        ext = torch.empty(12, dtype=torch.int64, device=DEV)

        def files_call(first=first, n_files=n_files, reports=reports, fsum=fsum, bad=bad):
            pcs.scrub_files_async(cls, types, first, N, n_files, reports, fsum, bad, 1024)

        def extents_loop(per_file=per_file, n_files=n_files, ext=ext):
            for f in range(n_files):
                pcs.scrub_extents_async(cls[f * per_file: (f + 1) * per_file], per_file, ext, None, 0)

        def scrub_loop(per_file=per_file, n_files=n_files):
            for f in range(n_files):
                a0, a1 = f * per_file, (f + 1) * per_file
                pcs.pages_scrub_async(pages[a0 * P: a1 * P], P, per_file, cls[a0:a1], types[a0:a1], summ, lst, 0)

        variants.append((f"files call     {label}", files_call, rounds))
        if a.trace_rounds:
            if n_files == 1:  # the two existing reductions on the same bytes, for the kernel trace
                variants.append((f"extents cap 0  {label}", extents_loop, rounds))
                variants.append((f"scrub call     {label}", scrub_loop, rounds))
        else:
            loop_rounds = max(2, min(rounds, a.loop_calls // n_files))
            variants.append((f"extents loop   {label}", extents_loop, loop_rounds))
            variants.append((f"scrub loop     {label}", scrub_loop, loop_rounds))
        # what the timed call must compute: the holes and the corrupt files, from the class bytes on the host
        per = cls_h.reshape(n_files, per_file)
        checks.append((files_call, fsum, n_files, int((per == pcs.PAGE_CORRUPT).any(axis=1).sum()),
                       int((cls_h == pcs.PAGE_BLANK).sum())))

    for _, f, _ in variants:  # warm every shape
        f()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for r in range(rounds):
        for k, (_, f, todo) in enumerate(variants):
            if r >= todo:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    for f, fsum, n_files, want_corrupt_files, want_blank in checks:  # sanity: the timed calls computed what they should
        f()
        d = pcs.files_summary_dict(fsum.cpu().tolist())
        assert (d["n_files"], d["n_pages"], d["n_corrupt_files"], d["n_blank"], d["invalid_file"]) == \
            (n_files, N, want_corrupt_files, want_blank, pcs.NO_PAGE), d
        assert d["n_hole_files"] == 1

    lines = [f"files_rate: class and type bytes of one real scrub of {N} x {P} B pages, up to {rounds} interleaved rounds, "
             f"device events around each variant ({pcs.version()})",
             f"{'variant':<32} {'rounds':>6} {'median us':>12} {'min us':>12}"]
    for (name, _, _), t in zip(variants, times):
        lines.append(f"{name:<32} {len(t):6d} {statistics.median(t):12.1f} {min(t):12.1f}")
    text = "\n".join(lines)
    print(text)
    if a.out and not a.trace_rounds:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
