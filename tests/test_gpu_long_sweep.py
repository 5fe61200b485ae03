"""The raw-range and manifest XXH3 kernels by tail shape and window, and the
scratch pool under two streams.

k_xxh3_long, k_manifest_sums16 / k_manifest_sums / k_manifest_chain and the
one-lane xxh3_any index a range by hand from nb = (L - 1) / 1024,
nst = ((L - 1) % 1024) / 64 and a last stripe at L - 64, inside loops with
edges of their own (64-block windows dealt 16 blocks at a time, four blocks to
a group, LDS halves of 512 blocks scrambled eight ahead).  A predicate wrong
at one residue or one block count changes one digest for one family of
lengths, so the lists of tests/long_sweep.py hold every residue at every such
block count (tests/test_long_sweep_cpu.py asserts what they reach), and every
comparison is bit-exact against the CPU checker (the reference's own xxHash
where oracle/_ref is built, else the repo's oracle).

test_raw_ranges   R + RD as one descriptor batch in a poisoned image at three
                  alignments: pcs_xxh3_64_ranges_dev, and pcs_xxh64_ranges_dev
                  on R at two seeds, into sentinel-padded outputs.
test_manifest     M and M2 through pcs_manifest_checksum_dev in its four forms,
                  each call into a garbage-filled word.  Call i reads its
                  content from pool[16 * (i + 1) + align:], so a block sum or
                  chunk digest left in the pooled scratch by an earlier call
                  is never the right one.
test_two_streams  the five users of the scratch pool that had no two-stream
                  test, ten interleaved repetitions each, one synchronise.
test_scratch_outlives_its_stream
                  a scratch buffer last used on a stream that no longer exists
                  is passed over by the pool, not an error of the next call
                  (what test_manifest met in the whole suite).

A case collects every failing (length, alignment, form) and reports them all.

Measured on an MI355X, per case, the checker's share included: test_raw_ranges
0.2-0.44 s at offset % 16 == 0 (it draws the 86 MiB of random bytes the three
share), 0.08 s at 8 and 0.06 s on the lanes; test_manifest 0.07-0.09 s for M
in every form (3,073 calls and 318 MiB hashed in the aligned ones; the expected values of an
alignment are computed in its first case), 0.01-0.02 s for M2 and 0.53 s for
M2 on the lanes (two full chunks on one lane each per call); the host form
0.03 s; test_two_streams_stamp 0.08-0.24 s, the other two-stream cases and
test_scratch_outlives_its_stream 0.01-0.05 s.
No case comes near the slowest case of the size sweep, so no list is cut into
bands: a case is a whole list in one form.
"""
import ctypes

import numpy as np
import pytest
import torch

import eloqstore_amd as pcs
import long_sweep as ls
import size_sweep as sw
from long_sweep import MiB
from size_sweep import XXH3, XXH64
from test_gpu_batch_edges import DEV, PAD, SENT64, SENT8, check_flags, check_words, fb_value, tuning, words

pytestmark = pytest.mark.gpu

GARBAGE = 0x1234
REPS = 10


class Cases:
    """The Band of the size sweep for lengths: collects the failing
    (length, alignment, form) of a case instead of stopping at the first."""

    def __init__(self):
        self.failed = []
        self.checked = 0

    def compare(self, got, want, lengths, aligns, form):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape == (len(lengths),)
        self.checked += got.size
        for i in np.flatnonzero(got != want):
            self.failed.append((int(lengths[i]), int(aligns[i]), form))

    def verdict(self, expect_checked):
        assert self.checked == expect_checked, (self.checked, expect_checked)
        assert not self.failed, (f"{len(self.failed)} wrong digests against the {ls.checker_name()}, "
                                 f"(length, alignment, form): {self.failed[:60]}")


def to_dev(host):
    d = torch.from_numpy(host).to(DEV)
    assert d.data_ptr() % 16 == 0
    return d


def dev_i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)


def got_words(out, n, what):
    got = out.cpu().numpy().view(np.uint64)
    assert (got[n:] == SENT64).all(), (what, "write past out[n]")
    return got[:n]


# ---- raw ranges --------------------------------------------------------------------

@pytest.fixture(scope="module")
def raw_source():
    return np.random.default_rng(0x10A7).integers(0, 256, size=ls.raw_source_bytes(), dtype=np.uint8)


@pytest.mark.parametrize("mode", ls.RAW_MODES)
def test_raw_ranges(raw_source, mode):
    offs, lens, total = ls.raw_layout(mode)
    n = len(offs)
    image = ls.raw_image(raw_source, offs, lens, total)
    assert int(offs.min()) >= 8 and int((offs + lens).max()) + ls.RAW_SLACK <= image.size
    base = to_dev(image)
    aligns = (offs % 16).astype(np.int64)
    if mode == "odd":
        assert (aligns % 8 != 0).all()  # every range on one lane of k_generic_desc
    else:
        assert (aligns == (0 if mode == "a0" else 8)).all()  # k_xxh3_long takes every range of 2048 bytes and more
    cases = Cases()

    out = words(n)
    pcs.xxh3_64_ranges(base, dev_i64(offs), dev_i32(lens), n, out=out)
    cases.compare(got_words(out, n, "xxh3"), ls.raw_xxh3(image, offs, lens), lens, aligns, "xxh3")

    short = np.flatnonzero(lens <= max(ls.R))
    assert short.size == len(ls.R)
    s_off, s_len = offs[short], lens[short]
    d_off, d_len = dev_i64(s_off), dev_i32(s_len)
    for seed in (0, ls.SEED2):
        out = words(short.size)
        pcs.xxh64_ranges(base, d_off, d_len, short.size, seed, out=out)
        cases.compare(got_words(out, short.size, "xxh64"), ls.raw_xxh64(image, s_off, s_len, seed), s_len,
                      aligns[short], f"xxh64 seed {seed:#x}")
    cases.verdict(n + 2 * len(ls.R))
    del base
    torch.cuda.empty_cache()


# ---- manifests -----------------------------------------------------------------------

class ManifestPool:
    def __init__(self):
        self.host = ls.manifest_pool()
        self.dev = to_dev(self.host)
        self._want = {}

    def want(self, align):
        """Expected checksum of every call of an alignment, computed once: {(list, length): checksum}."""
        if align not in self._want:
            calls = ls.manifest_calls(align)
            sums = ls.manifest_expected(self.host, [c[2] for c in calls], [c[3] for c in calls])
            self._want[align] = {c[:2]: int(h) for c, h in zip(calls, sums)}
            assert len(self._want[align]) == len(calls)
        return self._want[align]


@pytest.fixture(scope="module")
def mpool():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    p = ManifestPool()
    yield p
    del p
    torch.cuda.empty_cache()


def run_manifests(dev, calls, stream=None):
    """pcs_manifest_checksum_dev for every call, each into its own
    garbage-filled word of one sentinel-padded array.  -> the words."""
    n = len(calls)
    out = torch.full((n + PAD,), GARBAGE, dtype=torch.int64, device=DEV)
    out[n:] = SENT64
    s = pcs._stream(stream)
    prev = None
    for j, (_, _, start, total) in enumerate(calls):
        assert start != prev and start + total + 64 <= dev.numel()  # consecutive calls never share a start
        prev = start
        pcs._call("pcs_manifest_checksum_dev", dev.data_ptr() + start, total, out.data_ptr() + 8 * j, s)
        if j % 32 == 31:  # bounds the scratch buffers in flight, and hands the same ones out again
            torch.cuda.synchronize()
    return got_words(out, n, "manifest")


@pytest.mark.parametrize("name", ["M", "M2"])
@pytest.mark.parametrize("form", list(ls.FORMS))
def test_manifest(mpool, form, name):
    wide, align = ls.FORMS[form]
    calls = [c for c in ls.manifest_calls(align) if c[0] == name]
    if align % 8 == 0:
        assert [c[1] for c in calls] == (ls.M if name == "M" else ls.M2_TAILS)
    assert all((mpool.dev.data_ptr() + c[2]) % 16 == align for c in calls)
    want = mpool.want(align)
    cases = Cases()
    with tuning({pcs.TUNE_MANIFEST_WIDE: wide}):
        assert pcs.get_tuning(pcs.TUNE_MANIFEST_WIDE) == wide
        got = run_manifests(mpool.dev, calls)
    cases.compare(got, np.array([want[c[:2]] for c in calls], dtype=np.uint64), [c[1] for c in calls],
                  [align] * len(calls), f"{form} {name}")
    cases.verdict(len(calls))


def test_manifest_host_form(mpool):
    calls = ls.host_calls()
    want = ls.manifest_expected(mpool.host, [c[2] for c in calls], [c[3] for c in calls])
    cases = Cases()
    got = [pcs.manifest_checksum_host(mpool.host[s:s + t].tobytes()) for _, _, s, t in calls]
    cases.compare(np.array(got, dtype=np.uint64), want, [c[1] for c in calls], [0] * len(calls), "host")
    cases.verdict(len(ls.M_HOST))


# ---- two streams -----------------------------------------------------------------------
# Each user of the scratch pool on two streams with different inputs, ten
# interleaved repetitions, every output pre-filled with a sentinel, one
# synchronise at the end, every repetition compared with the checker.

def two_streams():
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    torch.cuda.synchronize()  # inputs and sentinels are in place before either stream starts
    return streams


def random_pages(P, n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n * P, dtype=np.uint8)


def test_two_streams_stamp():
    """The two-pass XXH3 stamp keeps its digests in scratch.  Every repetition
    stamps its own copy of the batch inside a sentinel-filled arena, and the
    whole arena is compared: the headers and the bytes around them."""
    work = []
    for k, (P, n) in enumerate(((4096, 1003), (1000, 2011))):
        pages = random_pages(P, n, 0x57A0 + k)
        want = sw.page_digests(pages, P, XXH3)
        slot = 16 + (n * P + 15) // 16 * 16 + 16
        arena = np.full(REPS * slot + 16, 0xC3, dtype=np.uint8)
        expect = arena.copy()
        stamped = pages.copy()
        stamped.reshape(n, P)[:, :8] = want.astype("<u8").view(np.uint8).reshape(n, 8)
        for rep in range(REPS):
            at = rep * slot + 16
            arena[at:at + n * P] = pages
            expect[at:at + n * P] = stamped
        assert not np.array_equal(arena, expect)
        work.append((P, n, slot, to_dev(arena), expect))
    streams = two_streams()
    for rep in range(REPS):
        for k, (P, n, slot, d, _) in enumerate(work):
            at = rep * slot + 16
            pcs.pages_stamp(d[at:at + n * P], P, n, XXH3, stream=streams[k])
    torch.cuda.synchronize()
    for P, n, slot, d, expect in work:
        after = d.cpu().numpy()
        diff = np.flatnonzero(after != expect)
        assert diff.size == 0, (P, "stamp: bytes differ at (repetition, page, byte)",
                                [((int(x) - 16) // slot, ((int(x) - 16) % slot) // P, ((int(x) - 16) % slot) % P)
                                 for x in diff[:8]])


def test_two_streams_fallback():
    """The odd-shape fallback of the fixed-stride entry points keeps the
    descriptors it builds in scratch: an XXH64 digest of 1000-byte pages at a
    base off the 8-byte grid on one stream, an XXH3 validate of 200-byte pages
    on the other."""
    Pa, na, Pb, nb = 1000, 3001, 200, 5003
    whole = torch.empty(4 + na * Pa + 32, dtype=torch.uint8, device=DEV)
    a_host = random_pages(Pa, na, 0xFA11)
    a = whole[4:4 + na * Pa]
    a.copy_(torch.from_numpy(a_host))
    assert a.data_ptr() % 8 == 4  # what sends XXH64 pages of a multiple of 8 bytes to the fallback
    want_a = sw.page_digests(a_host, Pa, XXH64)

    assert Pb < 249  # XXH3 below the long path: the fallback
    b_host = random_pages(Pb, nb, 0xFA12)
    b_host.reshape(nb, Pb)[:, :8] = sw.page_digests(b_host, Pb, XXH3).astype("<u8").view(np.uint8).reshape(nb, 8)
    bad = [7, 100, 2500, nb - 1]
    b_host.reshape(nb, Pb)[bad, 10] ^= 0x40
    want_ok = np.ones(nb, dtype=np.uint8)
    want_ok[bad] = 0
    rows = np.ascontiguousarray(b_host.reshape(nb, Pb)[bad])
    assert (sw.page_digests(rows, Pb, XXH3) != np.ascontiguousarray(rows[:, :8]).view("<u8").ravel()).all()
    b = to_dev(b_host)

    outs = [words(na) for _ in range(REPS)]
    oks = [torch.full((nb + PAD,), SENT8, dtype=torch.uint8, device=DEV) for _ in range(REPS)]
    fbs = [torch.full((1,), GARBAGE, dtype=torch.int64, device=DEV) for _ in range(REPS)]
    streams = two_streams()
    for rep in range(REPS):
        pcs.pages_digest(a, Pa, na, XXH64, out=outs[rep], stream=streams[0])
        pcs.pages_validate(b, Pb, nb, XXH3, ok=oks[rep], first_bad=fbs[rep], stream=streams[1])
    torch.cuda.synchronize()
    for rep in range(REPS):
        check_words(outs[rep], na, want_a, ("fallback digest", rep))
        check_flags(oks[rep], nb, want_ok, ("fallback validate", rep))
        assert fb_value(fbs[rep]) == bad[0], (rep, fb_value(fbs[rep]))


def test_two_streams_xxh64_flag_word():
    """The XXH64 descriptor path keeps a flag word in scratch: the fast kernel
    sets it when it leaves an off-shape page to the generic pass.  One
    stream's batch holds such pages and the other's none, so a word shared by
    the two would skip the pass (sentinels stay in out) or run it for nothing."""
    rng = np.random.default_rng(0xF1A6)
    work = []
    for k, n in enumerate((2000, 1500)):
        offs = np.arange(n, dtype=np.uint64) * np.uint64(4096)
        lens = np.full(n, 4096, dtype=np.uint32)
        if k == 0:
            odd = rng.choice(n, size=40, replace=False)
            lens[odd] = np.resize(np.array([1000, 4088, 100, 4032], dtype=np.uint32), odd.size)
            offs[odd[lens[odd] == 4032]] += np.uint64(8)  # a line shape at an address off the 16-byte grid
        off_shape = (lens % 64 != 0) | (lens < 128) | (offs % 16 != 0)
        assert int(off_shape.sum()) == (40 if k == 0 else 0)
        image = rng.integers(0, 256, size=n * 4096 + 64, dtype=np.uint8)
        want = sw.desc_digests(image, offs, lens, XXH64)
        work.append((n, to_dev(image), dev_i64(offs), dev_i32(lens), want, [words(n) for _ in range(REPS)]))
    streams = two_streams()
    for rep in range(REPS):
        for k, (n, base, d_off, d_len, _, outs) in enumerate(work):
            pcs.desc_digest(base, d_off, d_len, n, XXH64, out=outs[rep], stream=streams[k])
    torch.cuda.synchronize()
    for k, (n, _, _, _, want, outs) in enumerate(work):
        for rep in range(REPS):
            check_words(outs[rep], n, want, ("xxh64 desc_digest, stream", k, "repetition", rep))


def hip_runtime():
    """The HIP runtime the library itself runs on, for raw stream handles."""
    pcs.lib()
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths.pop())
    vp = ctypes.c_void_p
    for name, args in (("hipStreamCreate", [ctypes.POINTER(vp)]), ("hipStreamSynchronize", [vp]),
                       ("hipStreamDestroy", [vp]), ("hipStreamBeginCapture", [vp, ctypes.c_int]),
                       ("hipStreamEndCapture", [vp, ctypes.POINTER(vp)]), ("hipGraphDestroy", [vp]),
                       ("hipGetLastError", [])):
        getattr(hip, name).argtypes, getattr(hip, name).restype = args, ctypes.c_int
    return hip


def test_scratch_outlives_its_stream():
    """A scratch buffer is fenced by an event recorded on its last caller's
    stream, and the pool queries that event on every later lease.  The runtime
    keeps the address of the stream in the event and reads the stream's capture
    state from there when the event is queried, whether the stream still exists
    or not: after the stream is destroyed the query can answer
    hipErrorCapturedEvent (in the whole suite it did, on test_manifest, with no
    capture anywhere in the process).  Such a buffer must be passed over, not
    fail the next caller.  Here the first caller's stream is destroyed and new
    streams, one of which usually takes its address, begin an empty capture
    that is never replayed; the next call must succeed and be right.  (When no
    new stream lands on the address the calls are merely two more manifests.)"""
    hip = hip_runtime()
    relaxed = 2  # hipStreamCaptureModeRelaxed: other streams of this thread may allocate and launch
    total = MiB + 2049
    host = np.random.default_rng(0x57E4).integers(0, 256, size=total + 64, dtype=np.uint8)
    dev = to_dev(host)
    want = ls.manifest_expected(host, [16, 32], [total, total])
    out = torch.full((2 + PAD,), GARBAGE, dtype=torch.int64, device=DEV)
    out[2:] = SENT64
    torch.cuda.synchronize()  # every scratch buffer is idle: the next lease takes the first that fits
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    try:
        pcs._call("pcs_manifest_checksum_dev", dev.data_ptr() + 16, total, out.data_ptr(), s.value)
        assert hip.hipStreamSynchronize(s) == 0
    finally:
        assert hip.hipStreamDestroy(s) == 0
    fresh = []
    try:
        for _ in range(8):
            t = ctypes.c_void_p()
            assert hip.hipStreamCreate(ctypes.byref(t)) == 0
            fresh.append(t)
        for t in fresh:
            assert hip.hipStreamBeginCapture(t, relaxed) == 0
        pcs._call("pcs_manifest_checksum_dev", dev.data_ptr() + 32, total, out.data_ptr() + 8, pcs._stream(None))
    finally:
        for t in fresh:
            g = ctypes.c_void_p()
            hip.hipStreamEndCapture(t, ctypes.byref(g))  # the runtime may have invalidated the capture at the address
            if g.value:
                hip.hipGraphDestroy(g)
            hip.hipStreamDestroy(t)
        hip.hipGetLastError()  # whatever that left behind is not the next launch's error
    torch.cuda.synchronize()
    check_words(out, 2, want, "manifest after its scratch's stream is gone")


@pytest.mark.parametrize("wide", [1, 0], ids=["wide", "narrow"])
def test_two_streams_manifest(wide):
    """The manifest keeps block sums and chunk digests (wide form) or chunk
    descriptors and digests (narrow form) in scratch.  Two contents of
    different lengths; a repetition moves its content start by 16 bytes, as in
    test_manifest."""
    totals = (3 * MiB + 777, 1 * MiB + 2049)
    region = (3 * MiB + 777 + 16 * (REPS + 2) + 64) // 16 * 16
    host = np.random.default_rng(0x2A9F).integers(0, 256, size=2 * region, dtype=np.uint8)
    dev = to_dev(host)
    starts = [[k * region + 16 * (rep + 1) for rep in range(REPS)] for k in range(2)]
    assert all(s % 16 == 0 and s >= 8 for s in starts[0] + starts[1])  # k_manifest_sums16 / k_xxh3_long, not the lanes
    want = [ls.manifest_expected(host, starts[k], [totals[k]] * REPS) for k in range(2)]
    assert len(set(want[0].tolist()) | set(want[1].tolist())) == 2 * REPS
    outs = [torch.full((REPS + PAD,), GARBAGE, dtype=torch.int64, device=DEV) for _ in range(2)]
    for o in outs:
        o[REPS:] = SENT64
    with tuning({pcs.TUNE_MANIFEST_WIDE: wide}):
        streams = two_streams()
        for rep in range(REPS):
            for k in range(2):
                assert starts[k][rep] + totals[k] <= (k + 1) * region
                pcs._call("pcs_manifest_checksum_dev", dev.data_ptr() + starts[k][rep], totals[k],
                          outs[k].data_ptr() + 8 * rep, pcs._stream(streams[k]))
        torch.cuda.synchronize()
    for k in range(2):
        check_words(outs[k], REPS, want[k], ("manifest", "wide" if wide else "narrow", "stream", k))
