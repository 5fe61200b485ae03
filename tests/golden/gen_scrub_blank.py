#!/usr/bin/env python3
"""Generate tests/golden/scrub_blank.json from the REFERENCE's own xxHash.

A never-written page is all zero: stored digest 0 over a body of P - 8 zero
bytes.  The fixture records XXH3_64bits of that body for the page sizes the
scrub tests use, computed by oracle/_ref/libxxhash_ref.so (the reference's
vendored external/xxhash.c compiled unmodified by `make -C oracle ref`, as in
gen_golden.py).  Every value is non-zero, which is why a plain validate calls
a blank page corrupted and why "blank" has to be a class of its own.

Run from the repo root:  python tests/golden/gen_scrub_blank.py
"""
import json
import os

from gen_golden import ROOT, load_ref

PAGE_SIZES = (249, 256, 1000, 4096, 5000, 8192, 16384, 32768, 65536)


def main():
    ref = load_ref()
    rows = []
    for P in PAGE_SIZES:
        body = bytes(P - 8)
        h = int(ref.XXH3_64bits(body, len(body)))
        assert h != 0, P
        rows.append([P, f"{h:016x}"])
    fx = {
        "generator": "tests/golden/gen_scrub_blank.py",
        "source": "reference external/xxhash.c compiled by oracle/Makefile (oracle/_ref)",
        "xxh_version_number": int(ref.XXH_versionNumber()),
        "columns": ["page_size", "xxh3_64_of_zero_body"],
        "rows": rows,
    }
    out = os.path.join(ROOT, "tests", "golden", "scrub_blank.json")
    with open(out, "w") as f:
        json.dump(fx, f, indent=0, separators=(",", ":"))
    print("wrote", out, rows)


if __name__ == "__main__":
    main()
