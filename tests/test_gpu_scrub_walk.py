"""One set bit walked through every page body and launch variant of the scrub.

A page is BLANK when every byte is zero.  The kernels decide that from an OR
over the words each lane loaded, kept by hand in five page bodies
(xxh3_page_fixed, _rt, _rt4, _any in csrc/xxh3_page.h, xxh3_split_tile in
pcs_kernels.hip); a term dropped from that OR changes no digest, so only a
non-zero byte at the dropped position shows it.  scrub_ref.build_walk_batch
puts one bit at every byte (up to 5 KiB; above, one byte per 16-byte piece or
64-byte stripe, every byte near the ends and near the multiples of 4096), each
on a page of its own, with control pages (blank, zero body under its correct
header, random stamped, one header bit) on every group slot of a tile.

Every case asserts what decides the dispatch of launch_xxh3_pages (page size,
base alignment, the tuning values read back), scrubs into garbage-filled
outputs with sentinels past n and past n_listed, and compares classes, type
bytes, the whole summary and the corrupt list with tests/scrub_ref.py, bit
for bit.  A batch and its reference are built once per page size and shared
by the tuning variants (cases are ordered by page size; one batch is held at
a time)."""
import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
import scrub_ref
from scrub_gpu import DEV, scrub_checked, tuning

pytestmark = pytest.mark.gpu

COMPILED = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536)  # k_xxh3_fixed / k_xxh3_split sizes
DEFAULTS = {pcs.TUNE_XXH3_BLOCKS_PER_CU: 0, pcs.TUNE_NT_LOADS: 1, pcs.TUNE_XXH3_RT_BATCH: 1,
            pcs.TUNE_XXH3_SPLIT_PAGES: 8192}
NO_SPLIT = {pcs.TUNE_XXH3_SPLIT_PAGES: 0}
SPLIT_16K = {pcs.TUNE_XXH3_SPLIT_PAGES: 16384}
RT_ONE = {pcs.TUNE_XXH3_RT_BATCH: 0}
NO_NT = {pcs.TUNE_NT_LOADS: 0}
ONE_PER_CU = {pcs.TUNE_XXH3_BLOCKS_PER_CU: 1}


def body_of(P, ptr):
    """The page body launch_xxh3_pages runs for this page size, base address
    and the tuning in force (read back from the library)."""
    split = pcs.get_tuning(pcs.TUNE_XXH3_SPLIT_PAGES)
    if P % 256 != 0:
        return "any"
    if ptr % 16 != 0:
        return "rt4"
    if split > 0 and P >= split and 8192 <= P <= 65536 and P & (P - 1) == 0:
        return "split"
    if P in COMPILED:
        return "fixed"
    return "rt4" if pcs.get_tuning(pcs.TUNE_XXH3_RT_BATCH) != 0 else "rt"


def case(body, P, shift=0, tune=None, name="default", whole_list=False):
    return pytest.param(body, P, shift, tune or {}, whole_list, id=f"{P}-{body}-{name}" + (f"-base{shift}" if shift else ""))


CASES = (
    [case("fixed", P, whole_list=P == 4096) for P in (256, 512, 1024, 2048, 4096)]
    + [case("fixed", P, tune=NO_SPLIT, name="no_split", whole_list=P == 8192) for P in (8192, 16384, 32768, 65536)]
    + [case("split", P, whole_list=P == 16384) for P in (8192, 16384, 32768, 65536)]
    + [case("fixed", 8192, tune=SPLIT_16K, name="split_16k"), case("split", 16384, tune=SPLIT_16K, name="split_16k")]
    + [case("rt4", P, whole_list=P == 5120) for P in (768, 1280, 2560, 3072, 4352, 5120, 9216, 20480, 131328)]
    + [case("rt4", 4096, shift=8), case("rt4", 16384, shift=8)]
    + [case("rt", P, tune=RT_ONE, name="rt_one_block", whole_list=P == 5120)
       for P in (768, 1280, 3072, 4352, 5120, 9216, 131328)]
    + [case("any", P, whole_list=P == 5000)
       for P in (249, 250, 255, 257, 264, 1000, 1032, 1033, 1039, 1040, 1096, 2047, 2049, 4095, 4097, 4104, 4160,
                 5000, 8000, 12345, 65535, 135176)]
    + [case("any", P, shift=s) for P in (1000, 4097, 65535) for s in (3, 8)]
    # non-temporal loads off: one size of every row above
    + [case("fixed", 4096, tune=NO_NT, name="no_nt"),
       case("fixed", 65536, tune={**NO_SPLIT, **NO_NT}, name="no_split_no_nt"),
       case("split", 65536, tune=NO_NT, name="no_nt"),
       case("split", 16384, tune={**SPLIT_16K, **NO_NT}, name="split_16k_no_nt"),
       case("rt4", 5120, tune=NO_NT, name="no_nt"),
       case("rt", 5120, tune={**RT_ONE, **NO_NT}, name="rt_one_block_no_nt"),
       case("any", 5000, tune=NO_NT, name="no_nt")]
    # the grid capped at one block per CU (the batch-edge module covers n far above the cap)
    + [case("fixed", 4096, tune=ONE_PER_CU, name="grid_stride"),
       case("split", 16384, tune=ONE_PER_CU, name="grid_stride"),
       case("any", 1000, tune=ONE_PER_CU, name="grid_stride")]
)
CASES.sort(key=lambda c: (c.values[1], c.values[2]))  # one batch in memory at a time

_held = {}  # the batch of the page size in hand: host pages, reference, and its upload at one base shift


@pytest.fixture(scope="module", autouse=True)
def release_the_held_batch():
    yield
    _held.clear()
    torch.cuda.empty_cache()


def walk_batch(P):
    """(pages, rows, reference at cap 1024, reference list at cap n), built once per page size."""
    if _held.get("P") != P:
        _held.clear()
        torch.cuda.empty_cache()
        pg, rows = scrub_ref.build_walk_batch(P, seed=1)
        n = len(pg)
        wcls, wtypes, ws, wbad = scrub_ref.classify(pg, P, corrupt_cap=n)
        # an "always CORRUPT" or "always BLANK" kernel must fail on the controls
        loud = np.concatenate((rows["walk_rows"], rows["header_bit"]))
        assert (wcls[loud] == scrub_ref.CORRUPT).all()
        assert (wcls[rows["blank"]] == scrub_ref.BLANK).all() and {0, n - 1} <= set(rows["blank"])
        assert (wcls[rows["zero_body_ok"]] == scrub_ref.OK).all() and (wcls[rows["random_ok"]] == scrub_ref.OK).all()
        assert ws["n_corrupt"] == loud.size and ws["n_blank"] == len(rows["blank"]) and ws["n_ok"] >= 2
        assert wbad.size == loud.size
        _held.update(P=P, pg=pg, n=n, want=(wcls, wtypes, ws, wbad))
    return _held


def uploaded(P, shift):
    held = walk_batch(P)
    if held.get("shift") != shift:
        held.pop("dev", None)
        flat = torch.from_numpy(held["pg"].reshape(-1))
        whole = torch.empty(shift + flat.numel() + 32, dtype=torch.uint8, device=DEV)
        view = whole[shift: shift + flat.numel()]
        view.copy_(flat)
        torch.cuda.synchronize()
        held.update(shift=shift, dev=view)
    return held["dev"]


@pytest.mark.parametrize("body,P,shift,tune,whole_list", CASES)
def test_walk(body, P, shift, tune, whole_list):
    held = walk_batch(P)
    n, want = held["n"], held["want"]
    d = uploaded(P, shift)
    with tuning({**DEFAULTS, **tune}):
        # what decides the dispatch
        assert d.data_ptr() % 16 == shift % 16
        for k, v in {**DEFAULTS, **tune}.items():
            assert pcs.get_tuning(k) == v, (k, v)
        assert body_of(P, d.data_ptr()) == body
        cls = scrub_checked(d, P, n, want, cap=1024, reps=2)
        if whole_list:
            scrub_checked(d, P, n, want, cap=n, reps=1)
        ok, _ = pcs.pages_validate(d, P, n)
        assert np.array_equal(cls.cpu().numpy() == pcs.PAGE_OK, ok.cpu().numpy() == 1)


def test_matrix_reaches_every_final_block_shape():
    """The sizes on the 256-byte grid end in a final block of 1, 2, 3 and 4
    chunks, with no full block, within one 4-block batch and beyond it, the
    last batch a single chunk (4352) and a full one (5120); the sizes off it
    include P % 64 == 8 (the last stripe starts where the ordinary ones end),
    9 (one more ordinary stripe) and the sizes around them."""
    grid = sorted({c.values[1] for c in CASES if c.values[1] % 256 == 0})
    nb = lambda P: (P - 9) // 1024
    assert {P // 256 - 4 * nb(P) for P in grid} == {1, 2, 3, 4}
    for body in ("fixed", "rt4", "rt", "any"):
        sizes = [c.values[1] for c in CASES if c.values[0] == body]
        assert any(nb(P) == 0 for P in sizes) and any(nb(P) >= 4 for P in sizes), body
        if body != "fixed":
            assert any(nb(P) >= 8 for P in sizes), body  # three batches
    assert {4352, 5120} <= set(grid)
    odd = {c.values[1] for c in CASES if c.values[0] == "any"}
    assert {1032, 1033, 1039, 1040} <= odd  # around the first full block (P - 9 = 1024) and the next piece
    assert {P % 64 for P in odd} >= {8, 9, 63, 0, 1}
