"""Page sizes for the size sweep (tests/test_size_sweep_cpu.py asserts what
the lists reach, tests/test_gpu_size_sweep.py runs them), the positions inside
a page where a body changes what it does, and the helpers both modules share.

An XXH3 page of P >= 249 bytes is hashed as NB(P) full 1 KiB blocks, a final
block of kidx(P) ordinary 64-byte stripes and r64(P) bytes past them, and the
last stripe at P - 64 (csrc/xxh3_page.h, xxh3_page_any).  An XXH64 page is
(P - 8) // 32 stripes of 32 bytes and a tail of (P - 8) % 32 bytes.
"""
import numpy as np

import oracle

XXH3, XXH64 = 0, 1
N_PAGES = 17                 # pages per size: 17 * P mod 16 = P mod 16, so the page alignment rotates through a batch
POOL_BYTES = 16 + N_PAGES * 65535 + 64


def NB(P):
    """Full 1 KiB blocks of an XXH3 page."""
    return (P - 9) // 1024


def kidx(P):
    """Ordinary 64-byte stripes of the final block (kmax / 4 in xxh3_page_any)."""
    return ((P - 9) % 1024) // 64


def r64(P):
    return (P - 9) % 64


def block_residue(P):
    return (P - 9) % 1024


def shift(P):
    """Base alignment of a size's batch in lists A and B."""
    return (kidx(P) + 5 * NB(P)) % 16


# A: the any-size body, exhaustive: every size off the 256-byte grid with up to five full blocks
A = [P for P in range(249, 6153) if P % 256 != 0]

# B: the any-size body, deep: every block residue once more at 6-62 full blocks
# (two to sixteen trips of the four-block loop), and the largest uint16_t
B_NBS = [6, 7, 8, 9, 13, 18, 31, 62]
B_FORMULA = [(r, 9 + 1024 * B_NBS[r % 8] + r) for r in range(1024) if r % 256 != 247]
B = [P for _, P in B_FORMULA] + [65535]
B_BANDS = [[P for r, P in B_FORMULA if r % 8 == j] for j in range(8)]
B_BANDS[7].append(65535)

# C: the chunk grid (k_xxh3_fixed / k_xxh3_split / xxh3_page_rt4 / xxh3_page_rt)
C = [256 * k for k in range(1, 41)]

# S: the XXH64 quad kernel (k_xxh64_stride)
S = list(range(40, 1337, 8))

# L: the XXH64 LDS kernel
L = [64 * k for k in range(2, 73)]

# H: short and off-shape sizes, served by the descriptor fallback
H_BOTH = list(range(8, 249))
H_XXH64_ONLY = [P for P in range(249, 601) if P % 8 != 0]
H = {XXH3: H_BOTH, XXH64: H_BOTH + H_XXH64_ONLY}

A_BY_NB = {nb: [P for P in A if NB(P) == nb] for nb in range(6)}


def split(sizes, per):
    """sizes as consecutive bands of at most `per`, of near-equal length."""
    k = -(-len(sizes) // per)
    return [sizes[i * len(sizes) // k:(i + 1) * len(sizes) // k] for i in range(k)]


def split_weight(sizes, budget):
    """sizes as consecutive bands whose sizes sum to at most `budget` bytes."""
    bands = [[]]
    for P in sizes:
        if bands[-1] and sum(bands[-1]) + P > budget:
            bands.append([])
        bands[-1].append(P)
    return bands


# The bands the GPU tests run, one parametrised case each: {id: sizes}.  They
# are cut so that a case stays below the slowest case of the scrub walk
# (measured per size: about 0.8 ms with 17 pages and the scrub batch, twice
# that at the deep sizes; the capped grid's 16 * CUs + 17 pages cost by the
# byte, so those bands are cut by the sum of their page sizes).
PER_BAND, PER_BAND_DEEP, CAPPED_BAND_BYTES, PER_BAND_SHORT = 128, 64, 50000, 300
A_BANDS = {f"NB{nb}-{i}": part for nb in range(6) for i, part in enumerate(split(A_BY_NB[nb], PER_BAND))}
B_SPLIT_BANDS = {f"{j}-{i}": part for j in range(8) for i, part in enumerate(split(B_BANDS[j], PER_BAND_DEEP))}
NO_NT_BANDS = {f"no_nt-NB{nb}-{i}": part for nb in (0, 4) for i, part in enumerate(split(A_BY_NB[nb], PER_BAND))}
CAPPED = A[::7]  # every 7th size of A
CAPPED_BANDS = {f"one_block_per_cu-{i}": part for i, part in enumerate(split_weight(CAPPED, CAPPED_BAND_BYTES))}
H_BANDS = {(algo, i): part for algo in (0, 1) for i, part in enumerate(split(H[algo], PER_BAND_SHORT))}


def x64_lds_takes(P, base_shift):
    """pages_impl sends these XXH64 sizes to k_xxh64_lds, the rest of S to k_xxh64_stride."""
    return base_shift % 16 == 0 and P % 64 == 0 and P >= 128


def _kept(pos, P):
    out = []
    for p in pos:
        if 8 <= p < P and p not in out:
            out.append(p)
    return out


def xxh3_positions(P):
    """First body byte, both sides of the end of the full blocks, both sides
    of the end E of the ordinary stripes, both sides of the start of the last
    stripe, and the last byte."""
    nb = NB(P)
    E = 8 + 1024 * nb + 64 * ((P - 9 - 1024 * nb) // 64)
    return _kept([8, 8 + 1024 * nb - 1, 8 + 1024 * nb, E - 1, E, P - 65, P - 64, P - 1], P)


def xxh64_positions(P):
    """First body byte, both sides of the end of the 32-byte stripes, both
    sides of the second and of the last tail word, and the last byte."""
    e = 8 + 32 * ((P - 8) // 32)
    return _kept([8, e - 1, e, P - 25, P - 24, P - 9, P - 8, P - 1], P)


def positions(P, algo):
    return xxh3_positions(P) if algo == XXH3 else xxh64_positions(P)


def checker_name():
    return "reference" if oracle.ref_lib() is not None else "oracle"


def page_digests(pages, P, algo):
    """The checker: the reference's own xxHash where oracle/_ref is built,
    else the repo's restatement."""
    fn = oracle.ref_pages_digest if oracle.ref_lib() is not None else oracle.pages_digest
    return fn(pages, P, algo)


def desc_digests(base, offs, lens, algo):
    """The checker on a descriptor batch; a page shorter than its 8-byte
    header has no body to hash and digests to 0 (include/eloqstore_pcs.h)."""
    ref = oracle.ref_lib()
    fn = oracle.ref_desc_digest if ref is not None and hasattr(ref, "ref_desc_digest") else oracle.desc_digest
    out = np.zeros(len(offs), dtype=np.uint64)
    has_body = np.flatnonzero(np.asarray(lens) >= 8)
    out[has_body] = fn(base, np.asarray(offs)[has_body], np.asarray(lens)[has_body], algo)
    return out


def host_pool(nbytes=POOL_BYTES, seed=0x512E):
    return np.random.default_rng(seed).integers(0, 256, size=nbytes, dtype=np.uint8)


def desc_layout(seed=0x0DE5C):
    """Every length 0..6152 once plus all of B in a fixed random order, each
    at the next offset with offset % 16 == shift(length) (0 below 249).
    -> (offs uint64, lens uint32, total bytes)."""
    lens = np.array(list(range(0, 6153)) + B, dtype=np.uint32)
    np.random.default_rng(seed).shuffle(lens)
    offs = np.empty(lens.size, dtype=np.uint64)
    cur = 0
    for i, n in enumerate(lens.tolist()):
        want = shift(n) if n >= 249 else 0
        cur += (want - cur) % 16
        offs[i] = cur
        cur += n
    return offs, lens, cur
