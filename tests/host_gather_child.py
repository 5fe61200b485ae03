"""Child process of tests/test_gpu_host_pipeline.py::test_uneven_gather_splits.

    python host_gather_child.py P:n [P:n ...]

The gather thread count (PCS_GATHER_THREADS) is read once per process, so the
test starts this script afresh for each count.  For every shape it lists n
pages of an unregistered pool through shuffled pointers (every third pool page
left out) and checks the digests, the stamp's footprint over the whole pool and
the verdicts against the CPU oracle.  Exit status 0 when everything is exact;
1 with the first differing index on stdout otherwise.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import eloqstore_amd as pcs  # noqa: E402
import host_ref  # noqa: E402


def first_diff(got, want):
    d = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return int(d[0]) if d.size else None


def run(P: int, n: int) -> None:
    k = host_ref.n_chunks(P, n)
    with host_ref.Source("gather", P, n, seed=0xC41D + P, hold_out=True) as src:
        want = src.digests()
        calls = 0
        before_chunks = pcs.counter(pcs.COUNTER_GATHER_CHUNKS)
        got = pcs.digest_ptrs(src.ptrs, P)
        calls += 1
        i = first_diff(got, want)
        if i is not None:
            sys.exit(f"P={P} n={n}: digest differs first at index {i}: {int(got[i]):#x} != {int(want[i]):#x}")
        before = host_ref.snapshot(src.pages)
        pcs.stamp_ptrs(src.ptrs, P)
        calls += 1
        host_ref.assert_only_headers_changed(before, src.pages, src.rows, want)
        ok, fb = pcs.validate_ptrs(src.ptrs, P)
        calls += 1
        i = first_diff(ok, np.ones(n, dtype=np.uint8))
        if i is not None or fb is not None:
            sys.exit(f"P={P} n={n}: verdict differs first at index {i} (first_bad {fb})")
        moved = pcs.counter(pcs.COUNTER_GATHER_CHUNKS) - before_chunks
        if moved != calls * k:
            sys.exit(f"P={P} n={n}: {moved} gather chunks, want {calls} x {k}")
    print(f"ok P={P} n={n} chunks={k}")


def main(argv) -> int:
    print(f"gather threads {os.environ.get('PCS_GATHER_THREADS', 'default')}")
    try:
        for arg in argv:
            P, n = (int(x) for x in arg.split(":"))
            run(P, n)
    except AssertionError as e:
        print(f"FAILED: {e}")
        return 1
    except SystemExit as e:
        print(f"FAILED: {e.code}")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
