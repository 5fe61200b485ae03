"""The size sweep reaches what it claims: every count below is asserted for
exactly the lists tests/test_gpu_size_sweep.py iterates (both import them from
tests/size_sweep.py), so a size dropped there fails here."""
import numpy as np
import pytest

import oracle
import size_sweep as sw
from size_sweep import NB, block_residue, kidx, r64, shift

OFF_GRID = {247, 503, 759, 1015}  # (P - 9) % 1024 of the multiples of 256, which the stride path sends elsewhere


def test_list_sizes():
    assert len(sw.A) == 5880 and {NB(P) for P in sw.A} == set(range(6))
    assert len(sw.B) == 1021 and max(sw.B) == 65535 and len(set(sw.B)) == 1021
    assert sw.C == [256 * k for k in range(1, 41)]
    assert len(sw.S) == 163 and max((P - 8) // 32 for P in sw.S) == 41
    assert len(sw.L) == 71 and {(P + 255) // 256 for P in sw.L} == set(range(1, 19))
    assert sw.H[sw.XXH3] == list(range(8, 249))
    assert sw.H[sw.XXH64] == list(range(8, 249)) + [P for P in range(249, 601) if P % 8]
    assert sorted(sum(sw.A_BY_NB.values(), [])) == sw.A
    assert sorted(sum(sw.B_BANDS, [])) == sorted(sw.B) and 65535 in sw.B_BANDS[7]
    assert all(P % 256 != 0 for P in sw.A + sw.B)  # what sends launch_xxh3_pages to the any-size body
    assert all(249 <= P <= 65535 for P in sw.A + sw.B + sw.C[1:])
    assert sw.POOL_BYTES >= 16 + sw.N_PAGES * max(sw.B) + 64


def test_bands_are_the_lists():
    """The parametrised bands of the GPU tests, joined, are the lists: no size is dropped or run twice."""
    flat = lambda bands: sum(bands.values(), [])
    assert flat(sw.A_BANDS) == sw.A
    for nb in range(6):
        assert flat({k: v for k, v in sw.A_BANDS.items() if k.startswith(f"NB{nb}-")}) == sw.A_BY_NB[nb]
    for j in range(8):
        assert flat({k: v for k, v in sw.B_SPLIT_BANDS.items() if k.startswith(f"{j}-")}) == sw.B_BANDS[j]
    assert sorted(flat(sw.B_SPLIT_BANDS)) == sorted(sw.B)
    assert flat(sw.NO_NT_BANDS) == sw.A_BY_NB[0] + sw.A_BY_NB[4]
    assert flat(sw.CAPPED_BANDS) == sw.A[::7] and len(sw.A[::7]) == 840
    for algo in (sw.XXH3, sw.XXH64):
        assert flat({k: v for k, v in sw.H_BANDS.items() if k[0] == algo}) == sw.H[algo]
    for bands, per in ((sw.A_BANDS, sw.PER_BAND), (sw.B_SPLIT_BANDS, sw.PER_BAND_DEEP), (sw.NO_NT_BANDS, sw.PER_BAND),
                       (sw.H_BANDS, sw.PER_BAND_SHORT)):
        assert all(0 < len(v) <= per for v in bands.values())
    assert all(0 < sum(v) <= sw.CAPPED_BAND_BYTES for v in sw.CAPPED_BANDS.values())


def test_a_reaches_every_block_residue():
    for nb in range(1, 6):
        got = {block_residue(P) for P in sw.A_BY_NB[nb]}
        assert got == set(range(1024)) - OFF_GRID and len(got) == 1020, nb
    got = {block_residue(P) for P in sw.A_BY_NB[0]}
    assert got == set(range(240, 1024)) - OFF_GRID and len(got) == 780
    # with them every kmax, every r64, every P % 16
    assert {kidx(P) for P in sw.A} == set(range(16))
    assert {r64(P) for P in sw.A} == set(range(64))
    assert {P % 16 for P in sw.A} == set(range(16))


def test_a_alignment_coverage():
    r64_align, kidx_align, r64_shift = set(), set(), set()
    for P in sw.A:
        s = shift(P)
        assert 0 <= s < 16
        r64_shift.add((r64(P), s))
        for i in range(sw.N_PAGES):
            a = (s + i * P) % 16
            r64_align.add((r64(P), a))
            kidx_align.add((kidx(P), a))
    assert r64_align == {(r, a) for r in range(64) for a in range(16)}
    assert kidx_align == {(k, a) for k in range(16) for a in range(16)}
    assert r64_shift == {(r, a) for r in range(64) for a in range(16)}


def test_b_residues_and_batches():
    formula = [P for _, P in sw.B_FORMULA]
    res = [block_residue(P) for P in formula]
    assert len(res) == 1020 and set(res) == set(range(1024)) - OFF_GRID  # each reachable residue once
    assert sw.B == formula + [65535]
    assert {NB(P) % 4 for P in sw.B} == {0, 1, 2, 3}
    assert all(P % 256 != 0 for P in sw.B)
    assert min(NB(P) for P in sw.B) == 6 and max(NB(P) for P in formula) == 62
    # trips of xxh3_page_any's four-block loop over NB + 1 blocks: two at the least, three and more from NB 8 on
    trips = {nb: (nb + 1 + 3) // 4 for nb in sw.B_NBS}
    assert trips == {6: 2, 7: 2, 8: 3, 9: 3, 13: 4, 18: 5, 31: 8, 62: 16}
    assert (NB(65535) + 1 + 3) // 4 == 16
    for j, band in enumerate(sw.B_BANDS):
        assert {NB(P) for P in band if P != 65535} == {sw.B_NBS[j]}


def test_c_final_blocks():
    combos = {(P // 256 - 4 * NB(P), NB(P) % 4) for P in sw.C}
    assert combos == {(c, m) for c in (1, 2, 3, 4) for m in range(4)}
    assert max(NB(P) for P in sw.C) == 9


def test_s_unroll_and_tails():
    ns = lambda P: (P - 8) // 32
    assert {ns(P) % 16 for P in sw.S} == set(range(16))
    # below one trip of the 16-way unroll: every stripe count the kernel accepts (P >= 40 is one stripe)
    assert {ns(P) for P in sw.S if ns(P) < 16} == set(range(1, 16))
    assert {ns(P) % 16 for P in sw.S if ns(P) >= 16} == set(range(16))
    assert {ns(P) for P in sw.S if ns(P) >= 32} >= {32, 33, 41}  # two trips and a remainder
    for rem in range(16):
        assert {(P - 8) % 32 for P in sw.S if ns(P) % 16 == rem and ns(P) > 0} == {0, 8, 16, 24}, rem


def test_l_segments():
    assert {(P // 64) % 4 for P in sw.L} == {0, 1, 2, 3}
    segs = [(P + 255) // 256 for P in sw.L]
    assert {s % 12 for s in segs} == set(range(12))
    for depth in (1, 2, 3, 4):
        assert {s % depth for s in segs} == set(range(depth))
        # every (partial last segment, remainder of the segment loop) pair
        assert {((P // 64) % 4, s % depth) for P, s in zip(sw.L, segs)} == {(k, d) for k in range(4) for d in range(depth)}
    assert all(sw.x64_lds_takes(P, 0) and not sw.x64_lds_takes(P, 8) for P in sw.L)


def test_positions_are_inside_the_page():
    for algo, sizes in ((sw.XXH3, sw.A + sw.B + sw.C + sw.H[sw.XXH3]), (sw.XXH64, sw.S + sw.L + sw.H[sw.XXH64])):
        for P in sizes:
            pos = sw.positions(P, algo)
            assert all(8 <= p < P for p in pos) and len(pos) == len(set(pos)) <= 8
            assert (P > 8) == (len(pos) > 0)
    assert sw.xxh3_positions(1000) == [8, 967, 968, 935, 936, 999]
    assert sw.xxh3_positions(5000) == [8, 4103, 4104, 4935, 4936, 4999]
    assert sw.xxh3_positions(1100) == [8, 1031, 1032, 1095, 1096, 1035, 1036, 1099]
    assert sw.xxh64_positions(1000) == [8, 999, 975, 976, 991, 992]
    assert sw.xxh64_positions(100) == [8, 71, 72, 75, 76, 91, 92, 99]


def test_desc_layout():
    offs, lens, total = sw.desc_layout()
    assert sorted(lens.tolist()) == sorted(list(range(6153)) + sw.B)
    want = np.array([shift(n) if n >= 249 else 0 for n in lens.tolist()])
    assert np.array_equal(offs % 16, want)
    end = offs + lens
    assert (offs[1:] >= end[:-1]).all() and (offs[1:] - end[:-1] < 16).all() and int(end[-1]) == total
    # the four block residues the stride path cannot give the any-size body, at an unaligned offset
    seen = {block_residue(int(n)) for n, o in zip(lens, offs) if n >= 249 and n % 256 == 0 and o % 16 != 0}
    assert seen == OFF_GRID


def test_checker_agreement():
    """The repo's oracle and the reference's own xxHash agree on 17 random
    pages of every size of the sweep, both algorithms."""
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref is not built")
    pool = sw.host_pool()
    sizes = sorted(set(sw.A + sw.B + sw.C + sw.S + sw.L + sw.H[sw.XXH3] + sw.H[sw.XXH64]))
    bad = []
    for P in sizes:
        s = shift(P) if P >= 249 else 0
        pages = pool[s:s + sw.N_PAGES * P]
        for algo in (sw.XXH3, sw.XXH64):
            if not np.array_equal(oracle.pages_digest(pages, P, algo), oracle.ref_pages_digest(pages, P, algo)):
                bad.append((P, algo))
    assert not bad, bad[:20]
