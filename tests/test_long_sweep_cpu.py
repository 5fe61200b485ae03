"""The long-range sweep reaches what it claims: every count below is asserted
for exactly the lists tests/test_gpu_long_sweep.py iterates (both import them
from tests/long_sweep.py), so a length dropped there fails here.  The checkers
are checked too: the reference's xxHash against the repo's oracle on every raw
range, and the folded chunk digests against the oracle's manifest checksum."""
import numpy as np
import pytest

import oracle
import long_sweep as ls
from long_sweep import CHUNK, HALF, MiB, nb, nst, r

ALL_R = set(range(1024))
ALL_NST = set(range(16))


def test_r_is_exhaustive():
    assert ls.R == list(range(6153))
    for n in range(1, 6):  # the lane kernel below 2048, the long kernel from nb == 1, r == 1023
        assert {r(L) for L in ls.R if nb(L) == n} == ALL_R, n
    assert {r(L) for L in ls.R if nb(L) == 1 and L >= ls.LONG_MIN} == {1023}
    assert {r(L) for L in ls.R if nb(L) == 6} == set(range(8))
    assert ls.LONG_MIN - 1 in ls.R and ls.LONG_MIN in ls.R
    # every XXH3 short class: 0, 1-3, 4-8, 9-16, 17-128, 129-240, 241-...
    assert set(range(0, 242)) <= set(ls.R)


def test_rd_residues_and_block_counts():
    assert len(ls.RD_FORMULA) == 1024 and ls.RD == ls.RD_FORMULA + [MiB - 1, MiB]
    assert sorted(r(L) for L in ls.RD_FORMULA) == list(range(1024))  # every residue, once
    assert {nb(L) for L in ls.RD_FORMULA} == set(ls.RD_NBS)
    for n in ls.RD_NBS:
        assert {nst(L) for L in ls.RD_FORMULA if nb(L) == n} == ALL_NST, n
    for edge in (16, 64, 64 + 16, 128):
        assert {edge - 1, edge, edge + 1} <= set(ls.RD_NBS), edge
    # k_xxh3_long: the last window holds 1..64 blocks, dealt 16 at a time; each edge of the deal is reached
    last = {ls.windows(L)[-1] for L in ls.RD_FORMULA}
    assert {15, 16, 17, 63, 64, 1, 7} <= last
    assert {len(ls.windows(L)) for L in ls.RD_FORMULA} == {1, 2, 3}
    assert (nb(MiB - 1), nst(MiB - 1), nb(MiB), nst(MiB)) == (1023, 15, 1023, 15)
    assert min(ls.RD) > max(ls.R)  # a length is in R or in RD, never both
    assert sum(ls.RD) < 80 * MiB


def test_m_residues_block_counts_and_halves():
    assert len(ls.M_FORMULA) == 1024 and ls.M == ls.M_FORMULA + [2048, MiB] + list(range(1, 2048))
    assert len(set(ls.M)) == len(ls.M)
    assert sorted(r(L) for L in ls.M_FORMULA) == list(range(1024))
    assert {nb(L) for L in ls.M_FORMULA} == set(ls.M_NBS)
    for n in ls.M_NBS:
        assert {nst(L) for L in ls.M_FORMULA if nb(L) == n} == ALL_NST, n
    assert all(ls.LONG_MIN <= L <= CHUNK for L in ls.M_FORMULA + [2048, MiB])
    assert all(1 <= L < ls.LONG_MIN for L in ls.M_SHORT)
    assert {nb(L) % 4 for L in ls.M_FORMULA} == {0, 1, 2, 3}  # k_manifest_sums16: four blocks to a group
    # k_manifest_chain: the eight-ahead loop's remainder over both halves
    first = {ls.halves(L)[0] for L in ls.M_FORMULA}
    second = {ls.halves(L)[1] for L in ls.M_FORMULA if len(ls.halves(L)) == 2}
    assert {h % 8 for h in first | second} == set(range(8))
    assert {h % 8 for h in first} == set(range(8)) and HALF in first
    assert second == {1, 8, 510, 511}
    assert ls.halves(1 + 1024 * 512) == [512] and ls.halves(1 + 1024 * 513) == [512, 1]
    assert nb(2048) == 1 and nb(MiB) == 1023
    assert sum(ls.M) < 330 * MiB


def test_m2_and_host_members():
    assert ls.M2_TAILS == ls.M[::16] and len(ls.M2_TAILS) == 193
    formula = [L for L in ls.M2_TAILS if L in set(ls.M_FORMULA)]
    assert len(formula) == 64 and {nb(L) for L in formula} == set(ls.M_NBS)
    assert any(L < ls.LONG_MIN for L in ls.M2_TAILS)
    assert ls.M2_HEAD == 2 * CHUNK
    assert len(ls.M_HOST) == 32 and {nb(L) for L in ls.M_HOST} == set(ls.M_NBS)


@pytest.mark.parametrize("mode", ls.RAW_MODES)
def test_raw_layout(mode):
    offs, lens, total = ls.raw_layout(mode)
    deep = ls.RD if mode != "odd" else [L for L in ls.RD if nb(L) <= 17]
    assert sorted(lens.tolist()) == sorted(ls.R + deep)
    if mode == "odd":
        assert {nb(L) for L in deep} == {7, 15, 16, 17} and len(deep) == 4 * 79  # k % 13 in 0..3, k < 1024
        assert {int(o) % 8 for o in offs} == set(range(1, 8))
        # each residue of the address meets each length class below 241 bytes and long ranges of every nb
        assert {(int(o) % 8, nb(int(n))) for o, n in zip(offs, lens)} >= {(a, n) for a in range(1, 8) for n in range(6)}
    else:
        assert set((offs % 16).tolist()) == {0 if mode == "a0" else 8}
    end = offs + lens
    assert int(offs[0]) >= 8 and (offs[1:] >= end[:-1]).all() and (offs[1:] - end[:-1] < 16).all()
    assert int(end[-1]) == total and total + ls.RAW_SLACK <= ls.raw_source_bytes()
    # neighbours differ in length: the order is shuffled, not sorted
    assert np.count_nonzero(np.diff(lens.astype(np.int64)) > 0) > lens.size // 3


def test_raw_image_poisons_exactly_the_gaps():
    offs, lens, total = ls.raw_layout("odd")
    source = np.zeros(total + ls.RAW_SLACK, dtype=np.uint8)
    image = ls.raw_image(source, offs, lens, total)
    covered = np.zeros(total + ls.RAW_SLACK, dtype=bool)
    for o, n in zip(offs.tolist(), lens.tolist()):
        assert not covered[o:o + n].any()
        covered[o:o + n] = True
    assert np.array_equal(image == ls.POISON, ~covered)
    assert not source.any()  # the source is left as it was


def test_manifest_calls_never_repeat_a_start():
    total_calls = 0
    for form, (wide, align) in ls.FORMS.items():
        calls = ls.manifest_calls(align)
        starts = [c[2] for c in calls]
        assert all(b - a == 16 for a, b in zip(starts, starts[1:])) and len(set(starts)) == len(starts)
        assert all(s >= 8 and s % 16 == align for s in starts)
        assert max(s + t for _, _, s, t in calls) + 64 <= ls.MANIFEST_POOL_BYTES
        m = [c[1] for c in calls if c[0] == "M"]
        m2 = [c[1] for c in calls if c[0] == "M2"]
        assert all(c[3] == c[1] for c in calls if c[0] == "M")
        assert all(c[3] == 2 * CHUNK + c[1] for c in calls if c[0] == "M2")
        if align % 8 == 0:
            assert m == ls.M and m2 == ls.M2_TAILS
        else:
            assert m == [L for L in ls.M if ls.lanes_ok(L)] and m2 == [L for L in ls.M2_TAILS if ls.lanes_ok(L)]
            assert set(ls.M_SHORT) <= set(m) and {nb(L) for L in m if L >= ls.LONG_MIN} == {1, 2, 3, 4, 5, 6, 8, 9}
            assert sorted(r(L) for L in m if L in set(ls.M_FORMULA)) == [k for k in range(1024) if k % 13 < 7]
        total_calls += len(calls)
    assert ls.FORMS == {"wide16": (1, 0), "wide8": (1, 8), "narrow8": (0, 8), "lanes3": (1, 3)}
    host = ls.host_calls()
    assert [c[1] for c in host] == ls.M_HOST and len({c[2] for c in host}) == len(host)


def test_fold_against_the_oracle():
    """The per-chunk checker plus the Python fold is the oracle's manifest checksum."""
    pool = ls.manifest_pool()
    calls = [c for c in ls.manifest_calls(3) if c[0] == "M"][::97] + ls.manifest_calls(8)[-3:] + ls.manifest_calls(0)[500:503]
    assert any(c[3] > 2 * CHUNK for c in calls) and any(c[3] < ls.LONG_MIN for c in calls)
    starts, totals = [c[2] for c in calls], [c[3] for c in calls]
    want = [oracle.manifest_checksum(pool[s:s + t]) for s, t in zip(starts, totals)]
    assert ls.manifest_expected(pool, starts, totals, xxh3=oracle.desc_raw_xxh3).tolist() == want
    assert ls.manifest_expected(pool, starts, totals).tolist() == want
    assert ls.fold([]) == 0 and ls.fold([1]) == ls.FOLD_MUL


def test_checker_agreement():
    """The repo's oracle and the reference's own xxHash agree on every raw
    range of R + RD at all three alignments, XXH3 and seeded XXH64."""
    if not ls.has_ref():
        pytest.skip("oracle/_ref is not built")
    source = np.random.default_rng(0xA6E).integers(0, 256, size=ls.raw_source_bytes(), dtype=np.uint8)
    bad = []
    for mode in ls.RAW_MODES:
        offs, lens, total = ls.raw_layout(mode)
        image = ls.raw_image(source, offs, lens, total)
        a, b = oracle.desc_raw_xxh3(image, offs, lens), ls.ref_raw_xxh3(image, offs, lens)
        bad += [(mode, "xxh3", int(lens[i])) for i in np.flatnonzero(a != b)]
        short = np.flatnonzero(lens <= max(ls.R))
        assert short.size == len(ls.R)
        for seed in (0, ls.SEED2):
            a = oracle.desc_raw_xxh64(image, offs[short], lens[short], seed)
            b = ls.ref_raw_xxh64(image, offs[short], lens[short], seed)
            bad += [(mode, "xxh64", seed, int(lens[short][i])) for i in np.flatnonzero(a != b)]
    assert not bad, bad[:20]


def test_checker_sees_a_flip_at_every_edge():
    """A checker that ignored the tail block or the last stripe would let the
    same mistake in a kernel through: one flipped byte at the first byte, both
    sides of the end of the full blocks, both sides of the end of the ordinary
    stripes, the start of the last stripe and the last byte changes the digest."""
    rng = np.random.default_rng(0xF11)
    for L in (2048, 2049, 3072, 3073, 6152, ls.RD_FORMULA[3], ls.RD_FORMULA[1000]):
        buf = rng.integers(0, 256, size=L + 16, dtype=np.uint8)
        off, ln = np.array([8], dtype=np.uint64), np.array([L], dtype=np.uint32)
        want = int(ls.raw_xxh3(buf, off, ln)[0])
        e = 1024 * nb(L) + 64 * nst(L)
        for pos in {0, 1024 * nb(L) - 1, 1024 * nb(L), e - 1, min(e, L - 1), L - 64, L - 1}:
            buf[8 + pos] ^= 0x40
            assert int(ls.raw_xxh3(buf, off, ln)[0]) != want, (L, pos)
            buf[8 + pos] ^= 0x40
        for pos in (7, 8 + L):  # outside the range
            buf[pos] ^= 0x40
            assert int(ls.raw_xxh3(buf, off, ln)[0]) == want, (L, pos)
            buf[pos] ^= 0x40
