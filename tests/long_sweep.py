"""Lengths for the long-range sweep (tests/test_long_sweep_cpu.py asserts what
the lists reach, tests/test_gpu_long_sweep.py runs them), the layouts both
modules share and the CPU checkers.

A raw XXH3 range of L >= 2048 bytes at 8-byte alignment is hashed as
nb(L) = (L - 1) // 1024 full 1 KiB blocks, a tail block of
nst(L) = ((L - 1) % 1024) // 64 ordinary stripes and the last stripe at L - 64
(csrc/pcs_kernels.hip: k_xxh3_long, k_manifest_sums16 / k_manifest_sums and
k_manifest_chain).  Around that: k_xxh3_long runs windows of 64 blocks dealt
16 at a time to its groups, k_manifest_sums16 gives four blocks to a group,
k_manifest_chain takes the sums in halves of 512 blocks and scrambles eight
ahead.  Shorter and unaligned ranges run on one lane (k_generic_desc).
"""
import ctypes

import numpy as np

import oracle

MiB = 1 << 20
CHUNK = MiB          # kManifestChunk
LONG_MIN = 2048      # kLongMin
WIN = 64             # kLongWin
HALF = 512           # k_manifest_chain's LDS half
SEED2 = 0x9E3779B97F4A7C15
FOLD_MUL = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1
POISON = 0x33


def r(L):
    return (L - 1) % 1024


def nb(L):
    """Full 1 KiB blocks of a long range."""
    return (L - 1) // 1024


def nst(L):
    """Ordinary 64-byte stripes of the tail block."""
    return ((L - 1) % 1024) // 64


# R: every short class, the 2047/2048 hand-over and nb 1..6 at every residue
R = list(range(0, 6153))

# RD: every residue once more at block counts around the group deal (16), the
# window (64), a window and a deal (64 + 16) and two windows (128)
RD_NBS = [7, 15, 16, 17, 63, 64, 65, 79, 80, 81, 127, 128, 129]
RD_FORMULA = [1 + 1024 * RD_NBS[k % 13] + k for k in range(1024)]
RD = RD_FORMULA + [MiB - 1, MiB]

# M: one manifest chunk
M_NBS = [2, 3, 4, 5, 6, 8, 9, 511, 512, 513, 520, 1022, 1023]
M_FORMULA = [1 + 1024 * M_NBS[k % 13] + k for k in range(1024)]
M_SHORT = list(range(1, 2048))  # the xxh3_any branch of the chain kernel
M = M_FORMULA + [2048, MiB] + M_SHORT

# M2: every 16th member of M as the last chunk behind two full ones
M2_TAILS = M[::16]
M2_HEAD = 2 * CHUNK

# the host form: 32 members of M, every block count of M_NBS
M_HOST = M_FORMULA[::32]


def halves(L):
    """Block counts k_manifest_chain stages in LDS, half by half."""
    n = nb(L)
    return [min(HALF, n - h0) for h0 in range(0, n, HALF)]


def windows(L):
    """Block counts of k_xxh3_long's windows."""
    n = nb(L)
    return [min(WIN, n - w0) for w0 in range(0, n, WIN)]


# ---- checkers ------------------------------------------------------------------

def checker_name():
    return "reference" if has_ref() else "oracle"


def has_ref():
    ref = oracle.ref_lib()
    return ref is not None and hasattr(ref, "ref_desc_digest")


def ref_raw_xxh3(base, offs, lens):
    """The reference's XXH3_64bits over [off, off + len): a "page" that starts
    8 bytes earlier has exactly that body.  Every offset must be >= 8."""
    offs = np.asarray(offs, dtype=np.uint64)
    lens = np.asarray(lens, dtype=np.uint32)
    assert offs.size == 0 or int(offs.min()) >= 8
    return oracle.ref_desc_digest(base, offs - np.uint64(8), lens + np.uint32(8), 0)


def ref_raw_xxh64(base, offs, lens, seed):
    ref = oracle.ref_lib()
    assert base.dtype == np.uint8 and base.flags.c_contiguous
    p = base.ctypes.data
    assert int((np.asarray(offs, dtype=np.uint64) + np.asarray(lens, dtype=np.uint64)).max()) <= base.size
    return np.array([ref.XXH64(p + int(o), int(n), ctypes.c_uint64(seed)) for o, n in zip(offs, lens)], dtype=np.uint64)


def raw_xxh3(base, offs, lens):
    """The checker: the reference's own xxHash where oracle/_ref is built,
    else the repo's restatement."""
    return ref_raw_xxh3(base, offs, lens) if has_ref() else oracle.desc_raw_xxh3(base, offs, lens)


def raw_xxh64(base, offs, lens, seed):
    return ref_raw_xxh64(base, offs, lens, seed) if has_ref() else oracle.desc_raw_xxh64(base, offs, lens, seed)


def fold(digests):
    """ManifestBuilder::CalcChecksum's aggregate of the chunk digests."""
    agg = 0
    for h in digests:
        agg = (((agg << 1) | (agg >> 63)) & MASK) ^ int(h)
        agg = (agg * FOLD_MUL) & MASK
    return agg


def manifest_expected(base, starts, totals, xxh3=None):
    """Manifest checksums of base[start:start + total] for every call: one
    pass of the checker over all 1 MiB chunks, folded per call."""
    xxh3 = xxh3 or raw_xxh3
    offs, lens, first = [], [], [0]
    for s, t in zip(starts, totals):
        for c in range(0, t, CHUNK):
            offs.append(s + c)
            lens.append(min(CHUNK, t - c))
        first.append(len(offs))
    dig = xxh3(base, np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32))
    return np.array([fold(dig[a:b]) for a, b in zip(first[:-1], first[1:])], dtype=np.uint64)


# ---- raw ranges ------------------------------------------------------------------

RAW_MODES = ("a0", "a8", "odd")


def raw_lengths(mode, seed=0x10A6):
    """R + RD in a fixed shuffled order; the one-lane run keeps RD up to 17 blocks."""
    deep = RD if mode != "odd" else [L for L in RD if nb(L) <= 17]
    lens = np.array(R + deep, dtype=np.uint32)
    np.random.default_rng(seed).shuffle(lens)
    return lens


def raw_layout(mode):
    """Each length at the next offset >= 8 with offset % 16 == 0 ("a0"),
    offset % 16 == 8 ("a8") or offset % 8 == 1..7 in rotation ("odd").
    -> (offs uint64, lens uint32, total bytes)."""
    lens = raw_lengths(mode)
    offs = np.empty(lens.size, dtype=np.uint64)
    cur = 8
    for i, n in enumerate(lens.tolist()):
        if mode == "odd":
            cur += (1 + i % 7 - cur) % 8
        else:
            cur += ((0 if mode == "a0" else 8) - cur) % 16
        offs[i] = cur
        cur += n
    return offs, lens, cur


RAW_SLACK = 64


def raw_source_bytes():
    return max(raw_layout(m)[2] for m in RAW_MODES) + RAW_SLACK


def raw_image(source, offs, lens, total):
    """The first total + 64 bytes of source with every byte outside the ranges poisoned."""
    image = source[:total + RAW_SLACK].copy()
    o, e = offs.astype(np.int64), offs.astype(np.int64) + lens.astype(np.int64)
    image[:o[0]] = POISON
    image[e[-1]:] = POISON
    for k in range(16):  # a gap is shorter than 16 bytes
        at = e[:-1] + k
        image[at[at < o[1:]]] = POISON
    return image


# ---- manifests ---------------------------------------------------------------------

# form -> (PCS_TUNE_MANIFEST_WIDE, content address % 16)
FORMS = {"wide16": (1, 0), "wide8": (1, 8), "narrow8": (0, 8), "lanes3": (1, 3)}


def lanes_ok(ell):
    """What the unaligned form runs: one lane per chunk is slow."""
    return ell < LONG_MIN or nb(ell) <= 9


def manifest_calls(align):
    """The calls of one content alignment, M then M2: (list name, swept
    length, content start in the pool, content length).  Call i starts at
    16 * (i + 1) + align, so no two calls hash the same bytes at the same
    block index and stale scratch can never hold the right value."""
    tails = [("M", ell, ell) for ell in M] + [("M2", ell, M2_HEAD + ell) for ell in M2_TAILS]
    if align % 8 != 0:
        tails = [t for t in tails if lanes_ok(t[1])]
    return [(name, ell, 16 * (i + 1) + align, total) for i, (name, ell, total) in enumerate(tails)]


def host_calls():
    return [("host", ell, 16 * (i + 1), ell) for i, ell in enumerate(M_HOST)]


MANIFEST_POOL_BYTES = 16 * (len(M) + len(M2_TAILS) + 1) + 16 + M2_HEAD + CHUNK + 64


def manifest_pool(seed=0x3A9F):
    return np.random.default_rng(seed).integers(0, 256, size=MANIFEST_POOL_BYTES, dtype=np.uint8)
