// pcs_kernels.hip — hand-written CDNA4 (gfx950) kernels for EloqStore's page
// checksum path: XXH3_64bits(page + 8, P - 8) / XXH64(page + 8, P - 8, 0) over
// many independent pages per launch (reference call sites:
// src/storage/page.cpp:18-31, src/async_io_manager.cpp:239-244 / 353-366,
// src/tasks/write_task.cpp:58-79).
//
// Work decomposition:
//
//   XXH3 long path — one 16-lane DPP row ("group") per page, 4 pages per wave.
//     Chunk c of a 1 KiB input block is 256 page bytes; lane g of the group
//     loads page bytes [blk*1024 + 256c + 16g, +16) with one global_load_dwordx4,
//     so a wave-instruction reads four fully-used 256 B segments.  Inside an
//     XXH3 block the accumulator updates are pure mod-2^64 sums (xxhash.h:5778-
//     5817), so each lane folds its words into four partial sums and a block
//     needs one cross-lane reduction: a DPP row_ror:15 exchange (page words sit
//     one u64 ahead of the 8-byte-offset hashed stripes) plus row_ror 4/8 folds.
//     The per-block scramble (xxhash.h:5827-5856) runs redundantly on every lane
//     for the accumulator pair (2p, 2p+1), p = g & 3; the merge (xxhash.h:6029-
//     6062) folds the four pairs with row_ror 1/2.
//   XXH64 — one quad per page (lane a owns accumulator a), 16 pages per wave;
//     the serial round chain of each accumulator stays in one lane.
//   Generic — one lane per input range, any length (all XXH3 length classes,
//     xxhash.h:4641-4856), for odd-sized descriptors and raw ranges.
#include "xxh3_page.h"
#include "eloqstore_pcs_internal.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <atomic>
#include <mutex>
#include <vector>

namespace pcs {

// Block tile = 16 consecutive pages (one per group).  The loop runs over
// tiles, so its trip count is uniform across the block and the barriers below
// cannot diverge.  Digest / verdict mode stages the tile's 16 results in LDS
// and writes them as one coalesced non-temporal store (128 B of digests or
// 16 B of verdicts) instead of 16 scattered 8-byte stores.
//
// When the grid covers every tile once, tiles are renumbered so that each
// XCD streams chunks of 64 consecutive tiles, the eight XCDs on adjacent
// chunks (xcd_tile, xxh3_page.h): +7.5 % on config 2 against dispatch order,
// and free of the placement dependence of one contiguous eighth per XCD.
//
// Digest and validate only: a stamp (SetChecksum) is this kernel's digest
// pass followed by k_scatter_stamp (pages_impl), because header writes
// interleaved with the read stream cost 20 % at every rewrite width
// (the in-place forms were retired in round 2).
//
// Scrub mode (kScrub, all three families): `ok` receives the page class and
// the digest slot `out` carries the type-byte array instead (scrub_types);
// no digest leaves the kernel.  A tile's class and type bytes are staged in
// tile_h (class | type << 8) and leave as two coalesced 16-byte nt stores.
__device__ __forceinline__ uint8_t* scrub_types(uint64_t* out) { return reinterpret_cast<uint8_t*>(out); }

template <int P, int MODE, bool NT>
__global__ __launch_bounds__(256) void k_xxh3_fixed(const uint8_t* __restrict__ pages, uint64_t n,
                                                   uint64_t* __restrict__ out, uint8_t* __restrict__ ok,
                                                   unsigned long long* first_bad) {
    static_assert(MODE != kStamp, "stamps run as digest + k_scatter_stamp");
    __shared__ uint64_t tile_h[16];
    __shared__ uint8_t tile_ok[16];
    const Xxh3Lane L = make_xxh3_lane(threadIdx.x & 15);
    const int grp = threadIdx.x >> 4;
    const uint64_t ntiles = (n + 15) / 16;
    const bool remap = gridDim.x == ntiles;
    for (uint64_t t0 = blockIdx.x; t0 < ntiles; t0 += gridDim.x) {
        const uint64_t t = remap ? xcd_tile(t0, ntiles) : t0;
        const uint64_t pg = t * 16 + grp;
        if (pg < n) {
            const uint8_t* page = pages + pg * (uint64_t)P;
            uint64_t stored = 0;
            u32x4 first;
            if constexpr (MODE == kScrub) {
                ScrubProbe sp;
                const uint64_t h = xxh3_page_fixed<P, NT, true>(page, L, stored, first, &sp);
                const uint8_t cls = scrub_class(sp, h == stored);
                if (L.g == 0) tile_h[grp] = (uint64_t)cls | ((uint64_t)sp.type << 8);
            } else {
                const uint64_t h = xxh3_page_fixed<P, NT>(page, L, stored, first);
                if (L.g == 0) {
                    tile_h[grp] = h;
                    tile_ok[grp] = (h == stored) ? 1 : 0;
                }
            }
        }
        __syncthreads();
        const uint64_t i = t * 16 + threadIdx.x;
        if (threadIdx.x < 16 && i < n) {
            if constexpr (MODE == kScrub) {
                const uint64_t ct = tile_h[threadIdx.x];
                st_nt(ok + i, (uint8_t)ct);
                st_nt(scrub_types(out) + i, (uint8_t)(ct >> 8));
            } else {
                if (MODE == kDigest || out) st_nt(out + i, tile_h[threadIdx.x]);
                if (MODE == kValidate) st_nt(ok + i, tile_ok[threadIdx.x]);
            }
        }
        if (MODE == kValidate && first_bad && threadIdx.x == 0) {
            // one note per tile: its smallest failing page
            for (int k = 0; k < 16 && t * 16 + k < n; ++k)
                if (!tile_ok[k]) {
                    note_bad(first_bad, t * 16 + k);
                    break;
                }
        }
        __syncthreads();
    }
}

// Split pages (P = 8, 16, 32 or 64 KiB): G = P / 4096 groups share a page,
// group j loading its 4 KiB slice (blocks 4j .. 4j+3) at once, so a
// workgroup streams 64 KiB of contiguous page bytes instead of 16 separate
// pages.  XXH3's long loop is acc <- scramble(acc + S_b) over block sums S_b
// that depend on the data only (xxhash.h:5988-6017), so the groups compute
// their S_b in parallel into LDS and one group per page then runs the short
// serial chain (the long-range kernel's scheme, k_xxh3_long).  A slice's last
// block needs the next slice's first word (its carry); it is left out of the
// group's sum and added by the chain from the word the next group publishes.
// One tile of the split scheme: PPB = 16 / G pages, group grp = (page slot ps,
// slice j).  page_at(ps) gives the page's address (nullptr: no page in that
// slot).  S holds PPB * P/1024 block-sum records of 4 pairs x 2 u64 (512 u64),
// C the 16 slice carry words.  On return (after one block barrier) the page
// digests and verdicts are in tile_h / tile_ok[ps]; the caller must barrier
// before reading them.
// SCRUB: tile_h[ps] receives class | type << 8 instead of the digest.  A
// slice whose first word is non-zero is not blank; the other slices OR their
// words (the gate is uniform over the group), and every group publishes
// "my slice is all zero" in Z[grp] for the chain group to combine.
template <int P, bool NT, typename PageAt, bool SCRUB = false>
__device__ __forceinline__ void xxh3_split_tile(const Xxh3Lane& L, PageAt page_at, uint64_t* S, uint64_t* C,
                                                uint64_t* tile_h, uint8_t* tile_ok, uint8_t* Z = nullptr) {
    static_assert(P % 4096 == 0 && P >= 8192 && P <= 65536, "split pages are 8..64 KiB");
    constexpr int G = P / 4096;       // groups per page
    constexpr int NB = P / 1024 - 1;  // full blocks (xxhash.h:5996); block NB is the final one, 4 chunks
    constexpr int NB1 = NB + 1;
    const int grp = threadIdx.x >> 4, ps = grp / G, j = grp % G, p = L.g & 3;
    const uint8_t* page = page_at(ps);
    uint64_t stored = 0;
    [[maybe_unused]] uint32_t ptype = 0;  // SCRUB: page byte 8 (lane 0 of slice 0)
    if (page) {
        const u32x4* base = reinterpret_cast<const u32x4*>(page + 4096u * j) + L.g;
        u32x4 d[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) d[i][c] = ld16<NT>(base + i * 64 + c * 16);
        stored = lo64(d[0][0]);
        if (L.g == 0) C[ps * G + j] = lo64(d[0][0]);
        if constexpr (SCRUB) {
            ScrubProbe sp;
            scrub_probe_init(sp, L.g, d[0][0]);
            ptype = sp.type;
            if (sp.gate) {
                uint32_t o = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < 4; ++c) o |= or16(d[i][c]);
                sp.orw = o;
            }
            const bool zero = sp.gate && row_or32(sp.gate ? sp.orw : 1u) == 0;
            if (L.g == 0) Z[grp] = zero ? 1 : 0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint64_t Te, To;
            if (i < 3) xxh3_block_terms<false>(L, d[i], lo64(d[i + 1][0]), 4, Te, To);
            else if (j < G - 1) xxh3_block_terms<false, true>(L, d[i], 0, 4, Te, To);
            else xxh3_block_terms<true>(L, d[i], 0, 4, Te, To);
            if (L.g < 4) {
                uint64_t* r = S + ((ps * NB1 + 4 * j + i) * 4 + p) * 2;
                r[0] = Te;
                r[1] = To;
            }
        }
    }
    __syncthreads();
    if (j == 0 && page) {
        const uint64_t k22 = c_keys.acc[22];  // key of a block's last input word (stripe 15, lane 7)
        const uint64_t* Sp = S + (ps * NB1 * 4 + p) * 2;
        uint64_t Ae = L.init_e, Ao = L.init_o;
#pragma unroll 4
        for (int b = 0; b < NB; ++b) {
            uint64_t Te = Sp[b * 8], To = Sp[b * 8 + 1];
            if ((b & 3) == 3 && p == 3) {  // slice boundary: add the carry word's terms
                const uint64_t cw = C[ps * G + ((b + 1) >> 2)];
                Te += cw;
                To += mul32x32(cw ^ k22);
            }
            Ae = xxh3_scramble(Ae + Te, L.ks_e);
            Ao = xxh3_scramble(Ao + To, L.ks_o);
        }
        const uint64_t h = xxh3_merge(L, Ae + Sp[NB * 8], Ao + Sp[NB * 8 + 1], (uint64_t)(P - 8));
        if constexpr (SCRUB) {
            if (L.g == 0) {
                bool blank = true;
#pragma unroll
                for (int jj = 0; jj < G; ++jj) blank = blank && Z[ps * G + jj] != 0;
                const uint8_t cls = (h == stored) ? kClassOk : blank ? kClassBlank : kClassCorrupt;
                tile_h[ps] = (uint64_t)cls | ((uint64_t)ptype << 8);
            }
        } else if (L.g == 0) {
            tile_h[ps] = h;
            tile_ok[ps] = (h == stored) ? 1 : 0;
        }
    }
}

template <int P, int MODE, bool NT>
__global__ __launch_bounds__(256) void k_xxh3_split(const uint8_t* __restrict__ pages, uint64_t n,
                                                   uint64_t* __restrict__ out, uint8_t* __restrict__ ok,
                                                   unsigned long long* first_bad) {
    constexpr int PPB = 16 / (P / 4096);  // pages per 256-thread block
    __shared__ uint64_t S[64 * 8];        // block sums per accumulator pair (even, odd)
    __shared__ uint64_t C[16];            // first input word of each slice (the previous block's carry)
    __shared__ uint64_t tile_h[16];
    __shared__ uint8_t tile_ok[16];
    __shared__ uint8_t Z[MODE == kScrub ? 16 : 1];  // scrub: slice g is all zero
    const Xxh3Lane L = make_xxh3_lane(threadIdx.x & 15);
    const uint64_t ntiles = (n + PPB - 1) / PPB;
    const bool remap = gridDim.x == ntiles;
    for (uint64_t t0 = blockIdx.x; t0 < ntiles; t0 += gridDim.x) {
        const uint64_t t = remap ? xcd_tile(t0, ntiles) : t0;
        auto page_at = [&](int ps) -> const uint8_t* {
            const uint64_t pg = t * PPB + ps;
            return pg < n ? pages + pg * (uint64_t)P : nullptr;
        };
        if constexpr (MODE == kScrub)
            xxh3_split_tile<P, NT, decltype(page_at), true>(L, page_at, S, C, tile_h, tile_ok, Z);
        else
            xxh3_split_tile<P, NT>(L, page_at, S, C, tile_h, tile_ok);
        __syncthreads();
        const uint64_t i0 = t * PPB;
        if (threadIdx.x < PPB && i0 + threadIdx.x < n) {
            if constexpr (MODE == kScrub) {
                const uint64_t ct = tile_h[threadIdx.x];
                st_nt(ok + i0 + threadIdx.x, (uint8_t)ct);
                st_nt(scrub_types(out) + i0 + threadIdx.x, (uint8_t)(ct >> 8));
            } else {
                if (MODE == kDigest || out) st_nt(out + i0 + threadIdx.x, tile_h[threadIdx.x]);
                if (MODE == kValidate) st_nt(ok + i0 + threadIdx.x, tile_ok[threadIdx.x]);
            }
        }
        if (MODE == kValidate && first_bad && threadIdx.x == 0) {
            for (int k = 0; k < PPB && i0 + k < n; ++k)
                if (!tile_ok[k]) {
                    note_bad(first_bad, i0 + k);
                    break;
                }
        }
        // the next tile's writes to S / tile_h wait for everyone's reads here
        __syncthreads();
    }
}

// Fixed stride, run-time page size.  BODY 0 / 1: the chunked body one block
// or four blocks per step (P % 256 == 0, 16-byte-aligned pages); BODY 2: the
// any-size body (any P >= 249, any alignment).
template <int MODE, bool NT, int BODY>
__global__ __launch_bounds__(256) void k_xxh3_stride(const uint8_t* __restrict__ pages, uint32_t P, uint64_t n,
                                                    uint64_t* __restrict__ out, uint8_t* __restrict__ ok,
                                                    unsigned long long* first_bad) {
    const Xxh3Lane L = make_xxh3_lane(threadIdx.x & 15);
    const uint64_t ntiles = (n + 15) / 16;
    const bool remap = gridDim.x == ntiles;
    for (uint64_t t0 = blockIdx.x; t0 < ntiles; t0 += gridDim.x) {
        const uint64_t pg = (remap ? xcd_tile(t0, ntiles) : t0) * 16 + (threadIdx.x >> 4);
        if (pg >= n) continue;
        const uint8_t* page = pages + pg * (uint64_t)P;
        uint64_t stored = 0;
        if constexpr (MODE == kScrub) {
            ScrubProbe sp;
            const uint64_t h = BODY == 2   ? xxh3_page_any<NT, true>(page, P, L, stored, &sp)
                               : BODY == 1 ? xxh3_page_rt4<NT, true>(page, P, L, stored, &sp)
                                           : xxh3_page_rt<NT, true>(page, P, L, stored, &sp);
            const uint8_t cls = scrub_class(sp, h == stored);
            if (L.g == 0) {
                st_nt(ok + pg, cls);
                st_nt(scrub_types(out) + pg, (uint8_t)sp.type);
            }
        } else {
            const uint64_t h = BODY == 2   ? xxh3_page_any<NT>(page, P, L, stored)
                               : BODY == 1 ? xxh3_page_rt4<NT>(page, P, L, stored)
                                           : xxh3_page_rt<NT>(page, P, L, stored);
            if (L.g == 0) emit(MODE, pg, h, stored, const_cast<uint8_t*>(page), out, ok, first_bad);
        }
    }
}

// Page list: page pg is the absolute address ptrs[pg], all of size P
// (P % 256 == 0, 16-byte aligned; checked by the caller).  Used for pool pages
// in registered host memory, read in place over PCIe (zero-copy): the list
// and the results live in pinned host memory too, so a batch is one launch.
// PF > 0 uses the compile-time page size (a 4 KiB page is then one batch of
// loads: one PCIe round trip instead of one per 1 KiB block).
template <int MODE, int PF, typename PageAt>
__device__ __forceinline__ void xxh3_list_body(PageAt page_at, uint32_t P, uint64_t n, uint64_t* __restrict__ out,
                                               uint8_t* __restrict__ ok) {
    const Xxh3Lane L = make_xxh3_lane(threadIdx.x & 15);
    for (uint64_t t = blockIdx.x; t < (n + 15) / 16; t += gridDim.x) {
        const uint64_t pg = t * 16 + (threadIdx.x >> 4);
        if (pg >= n) continue;
        const uint8_t* page = page_at(pg);
        uint64_t stored = 0;
        uint64_t h;
        if constexpr (PF > 0) {
            u32x4 first;
            h = xxh3_page_fixed<PF, false>(page, L, stored, first);
        } else {
            h = xxh3_page_rt4<false>(page, P, L, stored);
        }
        if (L.g == 0) {
            if (MODE == kStamp && ok) {
                // small stamp batches: a done byte per page that the host
                // polls instead of the completion signal.  The header and
                // the done byte are system-scope stores, the byte released
                // after the header, as the validate service writes them.
                // With the header as a non-temporal store behind a release
                // fence, the host saw the done byte before the header ~1 in
                // 10^5 stamps under eight threads (service_threads_test
                // --soak, profiles/r05/soak_bisect.txt).
                __hip_atomic_store(reinterpret_cast<uint64_t*>(const_cast<uint8_t*>(page)), h, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
                // the digest word an async stamp batch returns: system-scope
                // too, since the host reads it as soon as the done byte lands
                if (out) __hip_atomic_store(out + pg, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(ok + pg, (uint8_t)1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            } else {
                emit(MODE, pg, h, stored, const_cast<uint8_t*>(page), out, ok, nullptr);
            }
        }
    }
}

template <int MODE, int PF>
__global__ __launch_bounds__(256) void k_xxh3_list(const uint64_t* __restrict__ ptrs, uint32_t P, uint64_t n,
                                                  uint64_t* __restrict__ out, uint8_t* __restrict__ ok) {
    xxh3_list_body<MODE, PF>([=](uint64_t pg) { return reinterpret_cast<const uint8_t*>(ptrs[pg]); }, P, n, out, ok);
}

// Small batches (a ReadPages / FlushBatchPages batch is <= 256 pages,
// kv_options.h:18-19, 70) carry the page list in the kernel arguments: the
// waves then go straight to the pages instead of first fetching the list
// from host memory, one PCIe round trip less.
constexpr int kInlinePages = 256;
struct InlineList {
    uint64_t p[kInlinePages];
};

template <int MODE, int PF>
__global__ __launch_bounds__(256) void k_xxh3_list_inl(InlineList list, uint32_t P, uint64_t n,
                                                      uint64_t* __restrict__ out, uint8_t* __restrict__ ok) {
    xxh3_list_body<MODE, PF>([&](uint64_t pg) { return reinterpret_cast<const uint8_t*>(list.p[pg]); }, P, n, out,
                             ok);
}

// ---------------------------------------------------------------------------
// XXH64 page hash, one quad per page (lane a = accumulator a)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t xxh64_init(int a) {
    // XXH64_initAccs with seed 0 (xxhash.h:3521-3528)
    return a == 0 ? kP64_1 + kP64_2 : a == 1 ? kP64_2 : a == 2 ? 0ull : (uint64_t)0 - kP64_1;
}

__device__ __forceinline__ uint64_t ld64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// XXH64_finalize (xxhash.h:3611-3634) over the (len & 31) bytes at tail.
__device__ __forceinline__ uint64_t xxh64_tail(uint64_t h, const uint8_t* tail, uint64_t len) {
    uint32_t rem = (uint32_t)(len & 31);
    for (; rem >= 8; rem -= 8, tail += 8) {
        h ^= xxh64_round(0, ld64(tail));
        h = rotl64(h, 27) * kP64_1 + kP64_4;
    }
    if (rem >= 4) {
        h ^= (uint64_t)ld32(tail) * kP64_1;
        h = rotl64(h, 23) * kP64_2 + kP64_3;
        rem -= 4;
        tail += 4;
    }
    for (; rem > 0; --rem, ++tail) {
        h ^= (uint64_t)(*tail) * kP64_5;
        h = rotl64(h, 11) * kP64_1;
    }
    return xxh64_avalanche(h);
}

// XXH64_mergeAccs (xxhash.h:3573-3593) for a quad whose lane a holds acc a.
__device__ __forceinline__ uint64_t xxh64_quad_merge(uint64_t v) {
    const uint64_t v0 = dpp64<quad_bcast(0)>(v);
    const uint64_t v1 = dpp64<quad_bcast(1)>(v);
    const uint64_t v2 = dpp64<quad_bcast(2)>(v);
    const uint64_t v3 = dpp64<quad_bcast(3)>(v);
    uint64_t h = rotl64(v0, 1) + rotl64(v1, 7) + rotl64(v2, 12) + rotl64(v3, 18);
    h = (h ^ xxh64_round(0, v0)) * kP64_1 + kP64_4;
    h = (h ^ xxh64_round(0, v1)) * kP64_1 + kP64_4;
    h = (h ^ xxh64_round(0, v2)) * kP64_1 + kP64_4;
    h = (h ^ xxh64_round(0, v3)) * kP64_1 + kP64_4;
    return h;
}

// Page convention: XXH64 over [8, P).  Needs 8-byte aligned page, P % 8 == 0,
// P >= 40 (so the hashed length is >= 32 and the 4-accumulator loop runs).
constexpr int kX64Unroll = 16;
// Segments in flight per LDS-kernel step (profiles/r01/x64_depth_lab.txt).  Round 5
// (profiles/r05/x64_depth3_lab_r05z.txt): depth 3 (124 VGPRs, 4 waves per SIMD)
// is -3.2 % on config 3 and +0.9 % on config 2, depth 4 -10.3 % / +0.5 %; 2 stays.
constexpr int kX64LdsDepth = 2;
template <bool NT>
__device__ __forceinline__ uint64_t ld8(const uint64_t* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT>
__device__ __forceinline__ uint64_t xxh64_page(const uint8_t* __restrict__ page, uint32_t P, int a,
                                               uint64_t& stored) {
    const uint64_t len = P - 8;
    const uint32_t ns = (uint32_t)(len / 32);
    const uint64_t* w = reinterpret_cast<const uint64_t*>(page + 8) + a;
    stored = *reinterpret_cast<const uint64_t*>(page);
    uint64_t v = xxh64_init(a);
    uint32_t s = 0;
    for (; s + kX64Unroll <= ns; s += kX64Unroll) {
        uint64_t x[kX64Unroll];
#pragma unroll
        for (int u = 0; u < kX64Unroll; ++u) x[u] = ld8<NT>(w + 4 * (s + u));
#pragma unroll
        for (int u = 0; u < kX64Unroll; ++u) v = xxh64_round(v, x[u]);
    }
    for (; s < ns; ++s) v = xxh64_round(v, ld8<NT>(w + 4 * s));
    const uint64_t h = xxh64_quad_merge(v) + len;
    return xxh64_tail(h, page + 8 + 32 * (uint64_t)ns, len);
}

// XXH64 chunk arithmetic for 64-byte pieces (page_size % 64 == 0, 16-byte
// aligned page), used by k_xxh64_lds below.
//
// Lane q of a quad holds page bytes [64k + 16q, +16) of chunk k — page words
// 8k + 2q (half e0) and 8k + 2q + 1 (e1).  XXH64 stripe s covers page words
// 4s+1 .. 4s+4 and accumulator a consumes page word 4s + a + 1.  Accumulators are placed as
// lane q -> acc {0, 1, 3, 2}[q]; acc 3 runs one stripe behind (stripes 2k-1
// and 2k per chunk).  Then each lane needs its own half of one word and its
// partner's (q ^ 2) other half:
//   lane 0 (acc 0): own e1 (stripe 2k),   partner e1 (2k+1)
//   lane 1 (acc 1): own e0 (2k),          partner e0 (2k+1)
//   lane 2 (acc 3): partner e0 (2k-1),    own e0 (2k)
//   lane 3 (acc 2): partner e1 (2k),      own e1 (2k+1)
// i.e. one DPP quad_perm [2,3,0,1] exchange of a selected half per chunk.
// acc 3 skips stripe -1 (page word 0 is the stored digest); in the last
// chunk accs 0-2 skip stripe 2k+1, which is the 24-byte tail (page words
// P/8-3 .. P/8-1: lane 2 e1, lane 3 e0, lane 3 e1), consumed after the merge
// (xxhash.h:3537-3566, 3611-3634).
constexpr int kQuadSwap = 2 | (3 << 2) | (0 << 4) | (1 << 6);  // quad_perm [2,3,0,1]

template <bool SKIP>
__device__ __forceinline__ void xxh64_chunk(uint64_t& v, u32x4 d, int q, bool skip_first, bool skip_second) {
    const uint64_t e0 = lo64(d), e1 = hi64(d);
    const bool sends_e0 = (q == 0) || (q == 3);
    const uint64_t send = sends_e0 ? e0 : e1;
    const uint64_t keep = sends_e0 ? e1 : e0;
    const uint64_t recv = dpp64<kQuadSwap>(send);
    const uint64_t first = q < 2 ? keep : recv;
    const uint64_t second = q < 2 ? recv : keep;
    if constexpr (SKIP) {
        const uint64_t v1 = xxh64_round(v, first);
        v = skip_first ? v : v1;
        const uint64_t v2 = xxh64_round(v, second);
        v = skip_second ? v : v2;
    } else {
        v = xxh64_round(xxh64_round(v, first), second);
    }
}

__device__ __forceinline__ bool xxh64_lines_ok(uint64_t off, uint32_t P) {
    return (P % 64u) == 0 && P >= 128u && (off % 16u) == 0;
}

// XXH64 with the 16-lane load pattern, words handed to quads through LDS.
//
// A wave owns 16 pages.  Loads use the XXH3 layout: for 256-byte segment c,
// wave-instruction ii has row r (lanes 16r..16r+15) load page 4ii + r, lane t
// of the row taking bytes [256c + 16t, +16): four fully used 256 B pieces per
// instruction (the quad-per-page layout reads 64 B pieces, 2x the L2 requests
// per byte, measured ~10 % slower).  The quad that hashes page 4i + r sits in
// the same row r at position i (lanes 16r + 4i + q), so a page's bytes never
// leave its row.  Through LDS, quad lane q takes 16-byte slot 4k + q of the
// segment for chunk 4c + k; the slot is stored at (slot + 4i) mod 16, which
// puts the 16 lanes of every ds_read_b128 lane group on 16 distinct 16-byte
// bank slots (MI355X_MICROARCH.md §LDS: groups {0-3,12-15,20-27}, ...) and
// keeps each 8-lane ds_write_b128 group contiguous.  The chunk arithmetic is
// xxh64_chunk above (quad DPP exchange), unchanged.
// offshape (descriptor batches): a descriptor off the line shape makes the
// kernel store call_id there, and the generic pass that follows runs only
// when it finds this call's id (config 3 has no such page: the pass used to
// read every descriptor for nothing, 6.3 us per call).
// ADDR selects where page pg lives: kAddrStride base + pg * Pfixed,
// kAddrDesc base + off[pg] (length len[pg]), kAddrList the absolute address
// off[pg] (length Pfixed; registered host pages, zero-copy).
enum Addr : int { kAddrStride = 0, kAddrDesc = 1, kAddrList = 2 };

// DEPTH segments are loaded before the first of them is hashed (DEPTH x 4 KiB
// per wave in flight).
// WPB waves per workgroup (PCS_TUNE_XXH64_WAVES): a workgroup owns 16 * WPB
// consecutive pages.  Sorting a tile's pages by size before handing them to
// the waves measured 4 % slower on config 3 (profiles/r01/x64_sort_lab.txt:
// the block is held until its all-16 KiB wave ends) and was retired in round 2.
template <int MODE, bool NT, int ADDR, int DEPTH, int WPB = 4>
__global__ __launch_bounds__(64 * WPB) void k_xxh64_lds(const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
                                                       const uint32_t* __restrict__ len, uint32_t Pfixed, uint64_t n,
                                                       uint64_t* __restrict__ out, uint8_t* __restrict__ ok,
                                                       unsigned long long* first_bad,
                                                       unsigned long long* offshape, uint64_t call_id) {
    __shared__ __attribute__((aligned(16))) u32x4 lds[WPB][16][16];  // [wave][page slot][16 B slot]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = lane >> 4, t = lane & 15;        // loader role
    const int i = (lane >> 2) & 3, q = lane & 3;   // hasher role: page 4i + r, quad lane q
    const int a = q == 2 ? 3 : q == 3 ? 2 : q;
    constexpr uint64_t kTile = 16 * WPB;
    const uint64_t ntiles = (n + kTile - 1) / kTile;
    const bool remap = gridDim.x == ntiles;
    for (uint64_t t0 = blockIdx.x; t0 < ntiles; t0 += gridDim.x) {
        const uint64_t T = (remap ? xcd_tile_eighths(t0, ntiles) : t0) * kTile;
        // page in wave slot j (0..15) of this wave
        auto page_at = [&](int j) -> uint64_t { return T + wv * 16 + j; };
        // loader pages (4ii + r) and hasher page (4i + r)
        const uint8_t* lp[4];
        uint32_t lP[4];
        uint32_t segs = 0;  // segments this wave must walk (max over its pages)
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const uint64_t pg = page_at(4 * ii + r);
            uint32_t P = 0;
            const uint8_t* p = nullptr;
            if (pg < n) {
                if (ADDR == kAddrDesc) {
                    const uint64_t o = off[pg];
                    const uint32_t L = len[pg];
                    if (xxh64_lines_ok(o, L)) { P = L; p = base + o; }
                    else if (offshape) *offshape = call_id;  // left to k_generic_desc: it must run
                } else if (ADDR == kAddrList) {
                    P = Pfixed;
                    p = reinterpret_cast<const uint8_t*>(off[pg]);
                } else {
                    P = Pfixed;
                    p = base + pg * (uint64_t)Pfixed;
                }
            }
            lp[ii] = p;
            lP[ii] = P;
        }
        const uint64_t hp = page_at(4 * i + r);
        uint32_t Ph = 0;
        const uint8_t* hptr = nullptr;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
            if (ii == i) { Ph = lP[ii]; hptr = lp[ii]; }
        {
            uint32_t m = 0;
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) m = max(m, lP[ii]);
            // wave-wide maximum so every lane walks the same segment count
            m = max(m, (uint32_t)__shfl_xor((int)m, 16));
            m = max(m, (uint32_t)__shfl_xor((int)m, 32));
            segs = (m + 255) / 256;
        }
        const int K = (int)(Ph / 64);
        uint64_t v = xxh64_init(a), stored = 0;
        u32x4 last = {0, 0, 0, 0};
        for (uint32_t c0 = 0; c0 < segs; c0 += DEPTH) {
            u32x4 d[DEPTH][4];
#pragma unroll
            for (int j = 0; j < DEPTH; ++j)
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
                    if (256 * (c0 + j) + 16 * t < lP[ii])
                        d[j][ii] = ld16<NT>(reinterpret_cast<const u32x4*>(lp[ii] + 256 * (c0 + j)) + t);
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) {
                const uint32_t c = c0 + j;
                if (c >= segs) break;  // wave-uniform
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
                    if (256 * c + 16 * t < lP[ii]) lds[wv][4 * ii + r][(t + 4 * ii) & 15] = d[j][ii];
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int kk = 4 * (int)c + k;
                    if (kk < K) {
                        const u32x4 e = lds[wv][4 * i + r][(4 * k + q + 4 * i) & 15];
                        if (kk == 0) stored = dpp64<quad_bcast(0)>(lo64(e));
                        if (kk == 0 || kk == K - 1)
                            xxh64_chunk<true>(v, e, q, q == 2 && kk == 0, q != 2 && kk == K - 1);
                        else xxh64_chunk<false>(v, e, q, false, false);
                        if (kk == K - 1) last = e;
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (K > 0) {
            const uint64_t v0 = dpp64<quad_bcast(0)>(v);
            const uint64_t v1 = dpp64<quad_bcast(1)>(v);
            const uint64_t v2 = dpp64<quad_bcast(3)>(v);
            const uint64_t v3 = dpp64<quad_bcast(2)>(v);
            uint64_t h = rotl64(v0, 1) + rotl64(v1, 7) + rotl64(v2, 12) + rotl64(v3, 18);
            h = (h ^ xxh64_round(0, v0)) * kP64_1 + kP64_4;
            h = (h ^ xxh64_round(0, v1)) * kP64_1 + kP64_4;
            h = (h ^ xxh64_round(0, v2)) * kP64_1 + kP64_4;
            h = (h ^ xxh64_round(0, v3)) * kP64_1 + kP64_4;
            h += (uint64_t)(Ph - 8);
            const uint64_t t0w = dpp64<quad_bcast(2)>(hi64(last));
            const uint64_t t1w = dpp64<quad_bcast(3)>(lo64(last));
            const uint64_t t2w = dpp64<quad_bcast(3)>(hi64(last));
            h ^= xxh64_round(0, t0w);
            h = rotl64(h, 27) * kP64_1 + kP64_4;
            h ^= xxh64_round(0, t1w);
            h = rotl64(h, 27) * kP64_1 + kP64_4;
            h ^= xxh64_round(0, t2w);
            h = rotl64(h, 27) * kP64_1 + kP64_4;
            h = xxh64_avalanche(h);
            if (q == 0) emit(MODE, hp, h, stored, const_cast<uint8_t*>(hptr), out, ok, first_bad);
        }
    }
}

// Pages off the 64-byte-piece shape (P % 64 != 0 or 8-byte-aligned only): one
// quad per page, lane a reading accumulator a's words (xxh64_page).  The quad
// layout for line-shaped pages (each quad loading its own 64 B pieces, 80 % of
// spec) was retired in round 2 for k_xxh64_lds.
template <int MODE>
__global__ __launch_bounds__(256) void k_xxh64_stride(const uint8_t* __restrict__ pages, uint32_t P, uint64_t n,
                                                     uint64_t* __restrict__ out, uint8_t* __restrict__ ok,
                                                     unsigned long long* first_bad) {
    const int a = threadIdx.x & 3;
    const uint64_t ntiles = (n + 63) / 64;
    const bool remap = gridDim.x == ntiles;
    for (uint64_t t0 = blockIdx.x; t0 < ntiles; t0 += gridDim.x) {
        const uint64_t pg = (remap ? xcd_tile_eighths(t0, ntiles) : t0) * 64 + (threadIdx.x >> 2);
        if (pg >= n) continue;
        const uint8_t* page = pages + pg * (uint64_t)P;
        uint64_t stored = 0;
        const uint64_t h = xxh64_page<false>(page, P, a, stored);
        if (a == 0) emit(MODE, pg, h, stored, const_cast<uint8_t*>(page), out, ok, first_bad);
    }
}

// long raw-range shape (k_xxh3_long, below); the lane kernel skips these
constexpr int kLongWin = 64;             // blocks per window (64 KiB of input)
constexpr uint32_t kLongMin = 2048;      // shorter ranges stay on the lane kernel
constexpr int kQuadSwap1 = 1 | (0 << 2) | (3 << 4) | (2 << 6);  // quad_perm [1,0,3,2]

__device__ __forceinline__ bool xxh3_long_ok(const uint8_t* p, uint32_t L) {
    return L >= kLongMin && ((uintptr_t)p % 8u) == 0;
}

// ---------------------------------------------------------------------------
// generic single-lane XXH3_64bits / XXH64 over any byte range (any alignment)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t rrmxmx(uint64_t h, uint64_t len) {  // xxhash.h:4595-4603
    h ^= rotl64(h, 49) ^ rotl64(h, 24);
    h *= kMX2;
    h ^= (h >> 35) + len;
    h *= kMX2;
    return h ^ (h >> 28);
}

// XXH3_mix16B, seed 0 (xxhash.h:4740-4763); SOFF is a compile-time secret offset
__device__ __forceinline__ uint64_t mix16(const uint8_t* in, uint64_t k0, uint64_t k1) {
    return mul_fold64(ld64(in) ^ k0, ld64(in + 8) ^ k1);
}

// XXH3_64bits for len <= 240 (the short and mid-size classes)
__device__ __forceinline__ uint64_t xxh3_short(const uint8_t* in, uint64_t len) {
    if (len <= 16) {  // XXH3_len_0to16_64b, :4696-4704
        if (len > 8) {
            const uint64_t lo = ld64(in) ^ (secret64(24) ^ secret64(32));
            const uint64_t hi = ld64(in + len - 8) ^ (secret64(40) ^ secret64(48));
            const uint64_t acc = len + __builtin_bswap64(lo) + hi + mul_fold64(lo, hi);
            return xxh3_avalanche(acc);
        }
        if (len >= 4) {
            const uint64_t in1 = ld32(in), in2 = ld32(in + len - 4);
            const uint64_t keyed = (in2 + (in1 << 32)) ^ (secret64(8) ^ secret64(16));
            return rrmxmx(keyed, len);
        }
        if (len > 0) {
            const uint32_t combined = ((uint32_t)in[0] << 16) | ((uint32_t)in[len >> 1] << 24) |
                                      (uint32_t)in[len - 1] | ((uint32_t)len << 8);
            return xxh64_avalanche((uint64_t)combined ^ (uint64_t)(secret32(0) ^ secret32(4)));
        }
        return xxh64_avalanche(secret64(56) ^ secret64(64));
    }
    if (len <= 128) {  // XXH3_len_17to128_64b, :4766-4799
        uint64_t acc = len * kP64_1;
        const int rounds = (int)((len - 1) / 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i > rounds) break;
            acc += mix16(in + 16 * i, secret64(32 * i), secret64(32 * i + 8));
            acc += mix16(in + len - 16 * (i + 1), secret64(32 * i + 16), secret64(32 * i + 24));
        }
        return xxh3_avalanche(acc);
    }
    {  // XXH3_len_129to240_64b, :4802-4856 (len <= 240 here)
        uint64_t acc = len * kP64_1;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc += mix16(in + 16 * i, secret64(16 * i), secret64(16 * i + 8));
        acc = xxh3_avalanche(acc);
        uint64_t tail = mix16(in + len - 16, secret64(119), secret64(127));
        const int rounds = (int)(len / 16);
#pragma unroll
        for (int i = 8; i < 15; ++i) {
            if (i >= rounds) break;
            tail += mix16(in + 16 * i, secret64(16 * (i - 8) + 3), secret64(16 * (i - 8) + 11));
        }
        return xxh3_avalanche(acc + tail);
    }
}

__device__ uint64_t xxh3_any(const uint8_t* in, uint64_t len) {
    if (len <= 240) return xxh3_short(in, len);
    // long input, scalar (xxhash.h:5988-6081)
    uint64_t acc[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) acc[l] = c_init_acc[l];
    const uint64_t blocks = (len - 1) / 1024;
    auto stripe = [&](const uint8_t* p, int koff, bool last) {
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            const uint64_t v = ld64(p + 8 * l);
            const uint64_t k = v ^ (last ? c_keys.last[l] : c_keys.acc[koff + l]);
            acc[l ^ 1] += v;
            acc[l] += mul32x32(k);
        }
    };
    for (uint64_t b = 0; b < blocks; ++b) {
        for (int s = 0; s < 16; ++s) stripe(in + 1024 * b + 64 * s, s, false);
#pragma unroll
        for (int l = 0; l < 8; ++l) acc[l] = xxh3_scramble(acc[l], c_keys.scr[l]);
    }
    const int ns = (int)(((len - 1) - 1024 * blocks) / 64);
    for (int s = 0; s < ns; ++s) stripe(in + 1024 * blocks + 64 * s, s, false);
    stripe(in + len - 64, 0, true);
    uint64_t r = len * kP64_1;
#pragma unroll
    for (int i = 0; i < 4; ++i) r += mul_fold64(acc[2 * i] ^ c_keys.merge[2 * i], acc[2 * i + 1] ^ c_keys.merge[2 * i + 1]);
    return xxh3_avalanche(r);
}

__device__ uint64_t xxh64_any(const uint8_t* p, uint64_t len, uint64_t seed) {  // xxhash.h:3655-3673
    uint64_t h;
    const uint8_t* q = p;
    if (len >= 32) {
        uint64_t v[4] = {seed + kP64_1 + kP64_2, seed + kP64_2, seed, seed - kP64_1};
        const uint64_t ns = len / 32;
        for (uint64_t s = 0; s < ns; ++s, q += 32)
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = xxh64_round(v[i], ld64(q + 8 * i));
        h = rotl64(v[0], 1) + rotl64(v[1], 7) + rotl64(v[2], 12) + rotl64(v[3], 18);
#pragma unroll
        for (int i = 0; i < 4; ++i) h = (h ^ xxh64_round(0, v[i])) * kP64_1 + kP64_4;
    } else {
        h = seed + kP64_5;
    }
    return xxh64_tail(h + len, q, len);
}

// One lane per range.  SKIP = 8 applies the page convention (hash [8, len),
// stored digest in [0, 8)); SKIP = 0 hashes the raw range.  With FILTER set,
// ranges the fast kernels handle are skipped.
template <int MODE>
__device__ __forceinline__ void generic_one(const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
                                            const uint32_t* __restrict__ len, uint64_t i, int algo, uint64_t seed,
                                            int skip, uint64_t* __restrict__ out, uint8_t* __restrict__ ok,
                                            unsigned long long* first_bad) {
    const uint64_t o = off[i];
    const uint32_t L = len[i];
    const uint8_t* p = base + o;
    if ((uint32_t)skip > L) {  // page shorter than its digest header: never valid
        if (MODE == kValidate) {
            ok[i] = 0;
            if (out) out[i] = 0;
            if (first_bad) note_bad(first_bad, i);
        } else if (MODE == kDigest) {
            out[i] = 0;
        }
        return;
    }
    const uint64_t h = algo == 0 ? xxh3_any(p + skip, L - skip) : xxh64_any(p + skip, L - skip, seed);
    const uint64_t stored = skip ? ld64(p) : 0;
    if (MODE == kStamp) {
        __builtin_memcpy(const_cast<uint8_t*>(p), &h, 8);
        if (out) out[i] = h;
    } else {
        emit(MODE, i, h, stored, nullptr, out, ok, first_bad);
    }
}

// Descriptor batch (mixed sizes), one group per page, every shape: pages on
// the 256-byte chunk grid at 16-byte offsets take the chunked body, other
// long-path pages (P >= 249) the any-size body, shorter ones one lane of the
// group (xxh3_short).  So no generic pass follows.  (In the earlier
// grid-stride form the any-size branch cost 1.2 %, 152 against 136 VGPRs,
// profiles/r02/desc_any_lab.txt; one tile per workgroup compiles all three
// branches in 126.)  Measured alternatives, all
// bit-exact and all slower on config 3: 4 KiB slices dealt
// to the groups in rounds (-8 %), byte-budget slice windows (-12..-30 %),
// per-tile size sort (+-1 %), LPT page pairs (-2 %), a 128-VGPR cap (-0.3 %);
// round 2 (commit 99804f2): pages dealt to a wave's groups as they free up
// (+-1 %), a wave's pages as a stream of adjacent 4 KiB slices (-5..-8 %).
// One workgroup per tile, grid = tiles (no grid-stride loop): 125 VGPRs and
// 4 waves per SIMD, against 136 and 3 for the same body inside a grid-stride
// loop: +1.1 % digest / +0.8 % validate on config 3
// (profiles/r02/desc_tp_lab.txt, list 1 vs 0).  Loading the next tile's
// descriptors ahead with 2 or 4 tiles per workgroup was slower (-0.4..-2.7 %).
template <int MODE, bool NT, bool B4>
__global__ __launch_bounds__(256) void k_xxh3_desc(const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
                                                  const uint32_t* __restrict__ len, uint64_t n,
                                                  uint64_t* __restrict__ out, uint8_t* __restrict__ ok,
                                                  unsigned long long* first_bad) {
    __shared__ uint64_t tile_h[16];
    __shared__ uint8_t tile_st[16];  // 0 bad, 1 good, 2 not this kernel's page
    const Xxh3Lane L = make_xxh3_lane(threadIdx.x & 15);
    const uint64_t ntiles = (n + 15) / 16;
    const uint64_t t = xcd_tile(blockIdx.x, ntiles);  // the launch covers every tile once
    // results staged per tile: one coalesced store per tile instead of 16
    // scattered 8-byte (1-byte) stores inside the read stream, +1.0-1.7 % on
    // config 3 (profiles/r02/desc_staged_lab.txt); stamps write headers
    constexpr bool staged = MODE != kStamp;
    const int grp = threadIdx.x >> 4;
    const uint64_t pg = t * 16 + grp;
    uint8_t st = 2;
    if (pg < n) {
        const uint64_t o = off[pg];
        const uint32_t P = len[pg];
        if (xxh3_fast_ok(o, P)) {
            const uint8_t* page = base + o;
            uint64_t stored = 0;
            const uint64_t h = B4 ? xxh3_page_rt4<NT>(page, P, L, stored) : xxh3_page_rt<NT>(page, P, L, stored);
            if (!staged) {
                if (L.g == 0) emit(MODE, pg, h, stored, const_cast<uint8_t*>(page), out, ok, first_bad);
            } else {
                st = h == stored ? 1 : 0;
                if (L.g == 0) tile_h[grp] = h;
            }
        } else if (xxh3_group_ok(P)) {  // off the chunk grid or unaligned: the any-size body
            const uint8_t* page = base + o;
            uint64_t stored = 0;
            const uint64_t h = xxh3_page_any<NT>(page, P, L, stored);
            if (!staged) {
                if (L.g == 0) emit(MODE, pg, h, stored, const_cast<uint8_t*>(page), out, ok, first_bad);
            } else {
                st = h == stored ? 1 : 0;
                if (L.g == 0) tile_h[grp] = h;
            }
        } else if (L.g == 0) {  // shorter than the long path: one lane, results written directly
            if (P < 8) {  // shorter than its header: never valid (as generic_one)
                if (MODE == kValidate) {
                    ok[pg] = 0;
                    if (out) out[pg] = 0;
                    if (first_bad) note_bad(first_bad, pg);
                } else if (MODE == kDigest) {
                    out[pg] = 0;
                }
            } else {
                const uint8_t* page = base + o;
                const uint64_t h = xxh3_short(page + 8, P - 8);
                if (MODE != kStamp) emit(MODE, pg, h, ld64(page), nullptr, out, ok, first_bad);
            }
        }
    }
    if (staged) {
        if (L.g == 0) tile_st[grp] = st;
        __syncthreads();
        const uint64_t i = t * 16 + threadIdx.x;
        const int s = threadIdx.x < 16 && i < n ? tile_st[threadIdx.x] : 2;
        if (s != 2) {
            if (MODE == kDigest || out) st_nt(out + i, tile_h[threadIdx.x]);
            if (MODE == kValidate) st_nt(ok + i, (uint8_t)s);
        }
        if (MODE == kValidate && first_bad && threadIdx.x == 0) {
            for (int k = 0; k < 16 && t * 16 + k < n; ++k)
                if (tile_st[k] == 0) {
                    note_bad(first_bad, t * 16 + k);
                    break;
                }
        }
    }
}

// One lane per range.  SKIP = 8 applies the page convention (hash [8, len),
// stored digest in [0, 8)); SKIP = 0 hashes the raw range.  FILTER 1: XXH64
// pages k_xxh64_lds took are skipped, and with `gate` the whole pass exits
// unless k_xxh64_lds stored this call's id there (it found an off-shape
// page); FILTER 2: raw XXH3 ranges k_xxh3_long took are skipped.  (XXH3 descriptor pages never come here: k_xxh3_desc
// takes every shape.)
template <int MODE>
__global__ __launch_bounds__(256) void k_generic_desc(const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
                                                     const uint32_t* __restrict__ len, uint64_t n, int algo,
                                                     uint64_t seed, int skip, int filter, uint64_t* __restrict__ out,
                                                     uint8_t* __restrict__ ok, unsigned long long* first_bad,
                                                     const unsigned long long* gate, uint64_t call_id) {
    if (gate && *gate != call_id) return;  // the fast kernel left no page to this pass
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (filter == 1 && algo == 1 && xxh64_lines_ok(off[i], len[i])) continue;
        if (filter == 2 && xxh3_long_ok(base + off[i], len[i])) continue;
        generic_one<MODE>(base, off, len, i, algo, seed, skip, out, ok, first_bad);
    }
}

// ---------------------------------------------------------------------------
// XXH3 over long raw ranges: one workgroup per range
// ---------------------------------------------------------------------------
// For a single long input (a manifest chunk of up to 1 MiB,
// root_meta.cpp:150-174; a whole object) the page kernels' one-group-per-input
// mapping leaves the GPU idle.  XXH3's long loop (xxhash.h:5988-6017) is a
// chain acc <- scramble(acc + S_b) over 1 KiB blocks whose block sums S_b are
// independent, so the 16 groups of a workgroup compute S_b for a window of
// 64 blocks in parallel into LDS and 8 lanes then run the short serial
// scramble chain over the window.
//
// Lane g of a group loads words g + 16j (j < 8) of a block: 128 contiguous
// bytes per group-instruction.  Word w = g + 16j has stripe s = g/8 + 2j and
// accumulator lane l = g & 7, so a lane's multiply terms all go to acc[l] and
// its raw words to acc[l ^ 1]: one quad_perm swap and one row_ror:8 fold give
// each lane l < 8 the block sum of acc[l].

// block sum for the lane's accumulator l = g & 7 (valid in lanes 0..7)
__device__ __forceinline__ uint64_t xxh3_long_block(const uint64_t* __restrict__ blk, int g, int nstripes) {
    const int l = g & 7;
    uint64_t w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = (g / 8 + 2 * j < nstripes) ? blk[g + 16 * j] : 0;
    uint64_t M = 0, R = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int s = g / 8 + 2 * j;
        if (s < nstripes) {
            M += mul32x32(w[j] ^ c_keys.acc[s + l]);
            R += w[j];
        }
    }
    uint64_t T = M + dpp64<kQuadSwap1>(R);
    T += dpp64<kRowRor8>(T);
    return T;
}

// One long range (xxh3_long_ok) by the whole 256-thread workgroup: *out =
// XXH3_64bits(in8, L).  S is the workgroup's window of block sums.
__device__ __forceinline__ void xxh3_long_range(uint64_t (*S)[8], const uint8_t* __restrict__ in8, uint32_t L,
                                                uint64_t* __restrict__ out) {
    const int tid = threadIdx.x, g = tid & 15, grp = tid >> 4;
    const uint64_t* in = reinterpret_cast<const uint64_t*>(in8);
    const uint32_t nb = (L - 1) / 1024;
    uint64_t acc = tid < 8 ? c_init_acc[tid] : 0;  // threads 0..7 own acc[tid]
    for (uint32_t w0 = 0; w0 < nb; w0 += kLongWin) {
        const int nw = (int)min((uint32_t)kLongWin, nb - w0);
#pragma unroll
        for (int i = 0; i < kLongWin / 16; ++i) {
            const int b = grp + 16 * i;
            if (b < nw) {
                const uint64_t T = xxh3_long_block(in + (size_t)(w0 + b) * 128, g, 16);
                if (g < 8) S[b][g] = T;
            }
        }
        __syncthreads();
        if (tid < 8)
            for (int b = 0; b < nw; ++b) acc = xxh3_scramble(acc + S[b][tid], c_keys.scr[tid]);
        __syncthreads();
    }
    if (grp == 0) {
        const int nst = (int)(((L - 1) - 1024 * nb) / 64);
        uint64_t T = xxh3_long_block(in + (size_t)nb * 128, g, nst);
        // last stripe at input + L - 64, keyed with secret + 121 (xxhash.h:6013-6015)
        uint64_t M = 0, R = 0;
        if (g < 8) {
            const uint64_t v = ld64(in8 + L - 64 + 8 * g);
            M = mul32x32(v ^ c_keys.last[g]);
            R = v;
        }
        T += M + dpp64<kQuadSwap1>(R);
        acc += T;
        // mergeAccs (xxhash.h:6029-6052): even lanes fold pairs (l, l + 1)
        const uint64_t nxt = dpp64<kRowRor15>(acc);
        uint64_t m = (g < 8 && (g & 1) == 0) ? mul_fold64(acc ^ c_keys.merge[g], nxt ^ c_keys.merge[g + 1]) : 0;
        m += dpp64<kRowRor2>(m);
        m += dpp64<kRowRor4>(m);  // lane 0..7: m0+m2+m4+m6 (lanes 0,2,4,6 of 0..7)
        if (g == 6) *out = xxh3_avalanche((uint64_t)L * kP64_1 + m);
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_xxh3_long(const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
                                                  const uint32_t* __restrict__ len, uint64_t n,
                                                  uint64_t* __restrict__ out) {
    __shared__ uint64_t S[kLongWin][8];
    for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const uint8_t* in8 = base + off[r];
        const uint32_t L = len[r];
        if (!xxh3_long_ok(in8, L)) continue;  // uniform over the workgroup
        xxh3_long_range(S, in8, L, out + r);
    }
}

// Manifest record aggregate (ManifestBuilder::CalcChecksum, root_meta.cpp:150-174):
// chunk digests folded serially, agg = rotl(agg, 1) ^ h; agg *= 0x9e3779b97f4a7c15.
// ---------------------------------------------------------------------------
// Manifest checksum, wide form: few long chunks (ManifestBuilder::CalcChecksum,
// root_meta.cpp:150-174, 1 MiB per chunk)
// ---------------------------------------------------------------------------
// One workgroup per chunk (k_xxh3_long) leaves a small manifest on a handful
// of CUs: a 1 MiB record took 121 us.  Here the block sums of all chunks are
// computed by 16-block windows spread over the whole GPU (k_manifest_sums),
// then one workgroup per chunk loads its sums into LDS and runs the serial
// scramble chain and the tail (k_manifest_chain).  The chain itself
// (P/1024 - 1 dependent 64x32-bit scrambles) is the floor: ~20-30 us per
// 1 MiB chunk.
constexpr uint32_t kManifestChunk = 1u << 20;  // kCheckSumBatchSize, root_meta.cpp:157
constexpr int kChunkBlocks = kManifestChunk / 1024;
// With 16-byte block-sum loads (k_manifest_sums16), chains staged in LDS
// halves and the scalar fold, the wide form wins at every size, 1 GiB
// included (283 vs 305 us; it lost above 256 chunks before, 380 vs 332 us;
// profiles/r01/manifest_lab.txt).

__device__ __forceinline__ uint32_t manifest_chunk_len(uint64_t total, uint64_t c) {
    return (uint32_t)min((uint64_t)kManifestChunk, total - c * kManifestChunk);
}

__global__ __launch_bounds__(256) void k_manifest_sums(const uint8_t* __restrict__ content, uint64_t total,
                                                      uint64_t* __restrict__ S) {
    const uint64_t c = blockIdx.y;
    const uint32_t L = manifest_chunk_len(total, c);
    if (L < kLongMin) return;  // a short last chunk is hashed whole by the chain kernel
    const int g = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const uint32_t nb = (L - 1) / 1024;
    const uint32_t b = blockIdx.x * 16 + grp;
    if (b >= nb) return;
    const uint64_t* in = reinterpret_cast<const uint64_t*>(content + c * kManifestChunk);
    const uint64_t T = xxh3_long_block(in + (size_t)b * 128, g, 16);
    if (g < 8) S[(c * kChunkBlocks + b) * 8 + g] = T;
}

// The same block sums with 16-byte loads (content 16-byte aligned).  Lane g
// of a 16-lane group holds words 2g and 2g + 1 of each 256-byte chunk cc of a
// 1 KiB block: stripe 4cc + g/4, accumulator lanes 2(g & 3) and 2(g & 3) + 1
// (the page kernels' layout without their one-word page offset).  Word 2g
// adds its multiply term to the even accumulator of pair g & 3 and its raw
// value to the odd one; word 2g + 1 the other way round (xxhash.h:5778-5817).
// Two row rotations (4, 8) finish the block sum of each pair.  A group
// folds four consecutive blocks (16 loads in flight per lane).
constexpr int kSums16Blocks = 4;  // 1 KiB blocks per group
__global__ __launch_bounds__(256) void k_manifest_sums16(const uint8_t* __restrict__ content, uint64_t total,
                                                        uint64_t* __restrict__ S) {
    // workgroups in the page kernels' tile order over (chunk, 64 KiB window):
    // 1 GiB 292.6 -> 284.0 us against dispatch order (profiles/r03/manifest_order_ab.txt)
    const uint64_t lin = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const uint64_t t = xcd_tile(lin, (uint64_t)gridDim.x * gridDim.y);
    const uint64_t c = t / gridDim.x;
    const uint32_t bx = (uint32_t)(t % gridDim.x);
    const uint32_t L = manifest_chunk_len(total, c);
    if (L < kLongMin) return;  // a short last chunk is hashed whole by the chain kernel
    const int g = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const uint32_t nb = (L - 1) / 1024;
    const uint32_t b0 = (bx * 16 + grp) * kSums16Blocks;
    if (b0 >= nb) return;
    uint64_t key[4][2];
#pragma unroll
    for (int cc = 0; cc < 4; ++cc)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int jb = 32 * cc + 2 * g + e;  // word of the block: stripe jb / 8, lane jb % 8
            key[cc][e] = c_keys.acc[(jb >> 3) + (jb & 7)];
        }
    const u32x4* in = reinterpret_cast<const u32x4*>(content + c * kManifestChunk + (size_t)b0 * 1024) + g;
    u32x4 d[kSums16Blocks][4];
#pragma unroll
    for (int i = 0; i < kSums16Blocks; ++i)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
            if (b0 + i < nb) d[i][cc] = ld16<true>(in + i * 64 + cc * 16);
#pragma unroll
    for (int i = 0; i < kSums16Blocks; ++i) {
        if (b0 + i >= nb) break;
        uint64_t E = 0, O = 0;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const uint64_t w0 = lo64(d[i][cc]), w1 = hi64(d[i][cc]);
            E += mul32x32(w0 ^ key[cc][0]) + w1;
            O += mul32x32(w1 ^ key[cc][1]) + w0;
        }
        E += dpp64<kRowRor4>(E);
        E += dpp64<kRowRor8>(E);
        O += dpp64<kRowRor4>(O);
        O += dpp64<kRowRor8>(O);
        if (g < 4) {
            uint64_t* r = S + (c * kChunkBlocks + b0 + i) * 8 + 2 * g;
            r[0] = E;  // plain stores: the chain kernel reads them back from cache
            r[1] = O;  // (nt: sums 182 -> 186 us, chains 55 -> 74 us at 1 GiB)
        }
    }
}

__global__ __launch_bounds__(256) void k_manifest_chain(const uint8_t* __restrict__ content, uint64_t total,
                                                       const uint64_t* __restrict__ S, uint64_t* __restrict__ h) {
    // The chunk's block sums pass through LDS in halves of 512 blocks (32 KiB),
    // so five workgroups fit a CU and 1,024 chains run in one round (a whole
    // 64 KiB chunk of sums allowed two per CU).
    constexpr uint32_t kHalf = kChunkBlocks / 2;
    __shared__ uint64_t sums[kHalf][8];
    const uint64_t c = blockIdx.x;
    const uint32_t L = manifest_chunk_len(total, c);
    const uint8_t* in8 = content + c * kManifestChunk;
    const int tid = threadIdx.x, g = tid & 15;
    if (L < kLongMin) {
        if (tid == 0) h[c] = xxh3_any(in8, L);
        return;
    }
    const uint32_t nb = (L - 1) / 1024;
    uint64_t acc = tid < 8 ? c_init_acc[tid] : 0;
    for (uint32_t h0 = 0; h0 < nb; h0 += kHalf) {  // trip count uniform across the workgroup
        const uint32_t hn = min(kHalf, nb - h0);
        const u32x4* src = reinterpret_cast<const u32x4*>(S + (c * kChunkBlocks + h0) * 8);
        u32x4* dst = reinterpret_cast<u32x4*>(&sums[0][0]);
        for (uint32_t i = tid; i < hn * 4; i += blockDim.x) dst[i] = src[i];  // hn blocks x 64 B
        __syncthreads();
        if (tid < 8) {
            const uint64_t key = c_keys.scr[tid];
            uint32_t b = 0;
            for (; b + 8 <= hn; b += 8) {  // sums do not depend on acc: read 8 ahead
                uint64_t v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = sums[b + k][tid];
#pragma unroll
                for (int k = 0; k < 8; ++k) acc = xxh3_scramble(acc + v[k], key);
            }
            for (; b < hn; ++b) acc = xxh3_scramble(acc + sums[b][tid], key);
        }
        __syncthreads();  // sums is refilled by the next half
    }
    if (tid >= 64) return;
    if (tid < 16) {  // tail block, last stripe and merge, as in k_xxh3_long
        const uint64_t* in = reinterpret_cast<const uint64_t*>(in8);
        const int nst = (int)(((L - 1) - 1024 * nb) / 64);
        uint64_t T = xxh3_long_block(in + (size_t)nb * 128, g, nst);
        uint64_t M = 0, R = 0;
        if (g < 8) {
            const uint64_t v = ld64(in8 + L - 64 + 8 * g);
            M = mul32x32(v ^ c_keys.last[g]);
            R = v;
        }
        T += M + dpp64<kQuadSwap1>(R);
        acc += T;
        const uint64_t nxt = dpp64<kRowRor15>(acc);
        uint64_t m = (g < 8 && (g & 1) == 0) ? mul_fold64(acc ^ c_keys.merge[g], nxt ^ c_keys.merge[g + 1]) : 0;
        m += dpp64<kRowRor2>(m);
        m += dpp64<kRowRor4>(m);
        if (g == 6) h[c] = xxh3_avalanche((uint64_t)L * kP64_1 + m);
    }
}

// The fold is a serial chain over the chunk digests.  One wave loads 64
// digests at a time (the next batch in flight while this one is folded) and
// walks them with readlane, so the chain waits on multiplies, not on a global
// load per chunk (1,024 chunks: 64-75 us -> see profiles/r01/manifest_lab.txt).
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}
__global__ __launch_bounds__(64) void k_manifest_fold(const uint64_t* __restrict__ chunk_h, uint64_t nchunks,
                                                     uint64_t* __restrict__ out) {
    const int lane = threadIdx.x;
    uint64_t agg = 0;
    uint64_t cur = (uint64_t)lane < nchunks ? chunk_h[lane] : 0;
    for (uint64_t b = 0; b < nchunks; b += 64) {
        const uint64_t nb = b + 64 + (uint64_t)lane;
        const uint64_t nxt = nb < nchunks ? chunk_h[nb] : 0;
        const int m = (int)min<uint64_t>(64, nchunks - b);
        // rotl by shifts, not rotl64: the rotate would be a VALU v_alignbit and a
        // round trip out of the scalar unit on every step of the chain
        if (m == 64) {
#pragma unroll 16
            for (int k = 0; k < 64; ++k) agg = (((agg << 1) | (agg >> 63)) ^ readlane64(cur, k)) * 0x9e3779b97f4a7c15ull;
        } else {
            for (int k = 0; k < m; ++k) agg = (((agg << 1) | (agg >> 63)) ^ readlane64(cur, k)) * 0x9e3779b97f4a7c15ull;
        }
        cur = nxt;
    }
    if (lane == 0) *out = agg;
}

__global__ void k_make_chunks(uint64_t total, uint64_t chunk, uint64_t n, uint64_t* __restrict__ off,
                              uint32_t* __restrict__ len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        off[i] = i * chunk;
        len[i] = (uint32_t)min(chunk, total - i * chunk);
    }
}

// ---------------------------------------------------------------------------
// workload generation / corruption / read-ceiling (benchmark + test tooling)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix_word(uint64_t seed, uint64_t page, uint64_t w) {
    uint64_t z = (seed ^ page) + (w + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void k_gen_pages(uint64_t* __restrict__ pages, uint64_t words_per_page, uint64_t n,
                                                  uint64_t seed, uint64_t first_page) {
    for (uint64_t p = blockIdx.x; p < n; p += gridDim.x) {
        uint64_t* dst = pages + p * words_per_page;
        for (uint64_t w = threadIdx.x; w < words_per_page; w += blockDim.x)
            dst[w] = splitmix_word(seed, first_page + p, w);
    }
}

__global__ __launch_bounds__(256) void k_gen_desc(uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
                                                 const uint32_t* __restrict__ len, uint64_t n, uint64_t seed,
                                                 uint64_t first_page) {
    for (uint64_t p = blockIdx.x; p < n; p += gridDim.x) {
        uint8_t* dst = base + off[p];
        const uint32_t L = len[p];
        for (uint32_t w = threadIdx.x; w * 8u < L; w += blockDim.x) {
            const uint64_t v = splitmix_word(seed, first_page + p, w);
            const uint32_t nb = (L - w * 8u) < 8u ? (L - w * 8u) : 8u;
            if (nb == 8 && ((off[p] & 7) == 0)) *reinterpret_cast<uint64_t*>(dst + 8u * w) = v;
            else
                for (uint32_t b = 0; b < nb; ++b) dst[8u * w + b] = (uint8_t)(v >> (8 * b));
        }
    }
}

__global__ void k_flip_byte(uint8_t* pages, uint64_t P, uint64_t n, uint64_t every, uint64_t byte_off) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t p = k * every;
    if (p < n) pages[p * P + byte_off] ^= 0xFF;
}

// Second pass of a two-pass stamp: page i bytes [0, 8) = digest[i], one
// non-temporal store per page.  A plain store makes this kernel faster (33 vs
// 55 us for 1 M headers) but leaves the lines dirty in cache, and their
// write-back then lands inside the next launch: back-to-back stamps took 711
// us each with plain stores against 644 us with nt.  Whole 64-byte header
// lines from a compact copy (pass 1 keeping the page's first line) cost more
// in pass 1 than they save here (725-745 us per stamp;
// tools/lab/stamp_line_lab.hip, profiles/r01/stamp_line_lab.txt).
__global__ __launch_bounds__(256) void k_scatter_stamp(uint8_t* __restrict__ pages, uint64_t P, uint64_t n,
                                                      const uint64_t* __restrict__ dig) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t* p = pages + i * P;
    if (((uintptr_t)p & 7) == 0) st_nt(reinterpret_cast<uint64_t*>(p), dig[i]);
    else __builtin_memcpy(p, &dig[i], 8);  // odd page sizes / unaligned batches
}

// descriptor form of the header pass: page i at base + off[i], len[i] bytes
// (pages shorter than the 8-byte header are left alone, as the digest pass
// leaves them)
__global__ __launch_bounds__(256) void k_scatter_stamp_desc(uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
                                                           const uint32_t* __restrict__ len, uint64_t n,
                                                           const uint64_t* __restrict__ dig) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && len[i] >= 8) {
        uint8_t* p = base + off[i];
        if (((uintptr_t)p & 7) == 0) st_nt(reinterpret_cast<uint64_t*>(p), dig[i]);
        else __builtin_memcpy(p, &dig[i], 8);
    }
}

// ---------------------------------------------------------------------------
// Scrub reduction (pcs_pages_scrub_dev): summary and the capped, ascending
// list of corrupt pages from the class and type bytes the scrub pass wrote.
// Pages are not read again.  Three launches, all ordered by construction (no
// atomic append):
//   k_scrub_count  one block per kScrubSpan pages: its counts and its first
//                  corrupt page into a record;
//   k_scrub_scan   one block: exclusive scan of the records' corrupt counts
//                  (each block's rank in the list), the totals, the summary;
//   k_scrub_list   one block per span again: the blocks whose rank is below
//                  the cap scan their 16-page lane counts and write their
//                  corrupt page indices at rank + position.
// ---------------------------------------------------------------------------
constexpr uint64_t kScrubSpan = 4096;  // pages per block: 256 lanes x 16 class bytes
constexpr int kScrubRec = 10;          // u32 per record: corrupt, blank, ok_by_type[6], first corrupt, pad
constexpr int kSummaryWords = 12;      // pcs_scrub_summary

// 16 bytes at p, any alignment; bytes at cnt and beyond read as `fill`
__device__ __forceinline__ void ld_bytes16(const uint8_t* p, uint64_t cnt, uint8_t fill, uint64_t& lo, uint64_t& hi) {
    if (cnt >= 16) {
        lo = ld64u(p);
        hi = ld64u(p + 8);
        return;
    }
    lo = hi = 0x0101010101010101ull * fill;
    for (uint64_t k = 0; k < cnt; ++k) {
        uint64_t& w = k < 8 ? lo : hi;
        const int sh = 8 * (int)(k & 7);
        w = (w & ~(0xFFull << sh)) | ((uint64_t)p[k] << sh);
    }
}
__device__ __forceinline__ uint32_t byte_of(uint64_t lo, uint64_t hi, int k) {
    return (uint32_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xFF);
}

// Exclusive scan of v over a 256-thread block (w4: four words of LDS, free
// for reuse after the caller's next barrier); total receives the block sum.
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t* w4, uint64_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)incl, d, 64);
        if (lane >= d) incl += t;
    }
    if (lane == 63) w4[wave] = incl;
    __syncthreads();
    uint64_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint64_t x = w4[w];
        if (w < wave) before += x;
        total += x;
    }
    return before + incl - v;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor((unsigned long long)v, d, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_scrub_count(const uint8_t* __restrict__ cls, const uint8_t* __restrict__ type,
                                                    uint64_t n, uint32_t* __restrict__ rec) {
    __shared__ uint32_t cnt[kScrubRec];
    if (threadIdx.x < kScrubRec) cnt[threadIdx.x] = threadIdx.x == 8 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    const uint64_t p0 = (uint64_t)blockIdx.x * kScrubSpan + threadIdx.x * 16u;
    // eight 8-bit counters (at most 16 each): corrupt, blank, ok by type bucket 0..5
    uint64_t pack = 0;
    uint32_t first = 0xFFFFFFFFu;
    if (p0 < n) {
        uint64_t cl, ch, tl, th;
        ld_bytes16(cls + p0, n - p0, 0xFF, cl, ch);
        ld_bytes16(type + p0, n - p0, 0, tl, th);
#pragma unroll
        for (int k = 15; k >= 0; --k) {
            const uint32_t c = byte_of(cl, ch, k), t = byte_of(tl, th, k);
            const int bucket = t < 4 ? (int)t : t == 255 ? 4 : 5;
            const int field = c == kClassCorrupt ? 0 : c == kClassBlank ? 1 : 2 + bucket;
            pack += (c <= kClassBlank) ? 1ull << (8 * field) : 0;
            if (c == kClassCorrupt) first = threadIdx.x * 16u + k;
        }
    }
    // widen to 16-bit counters (a span holds 4096 pages) and add up per wave
    auto widen = [](uint32_t v) {
        return (uint64_t)(v & 0xFF) | (uint64_t)((v >> 8) & 0xFF) << 16 | (uint64_t)((v >> 16) & 0xFF) << 32 |
               (uint64_t)(v >> 24) << 48;
    };
    const uint64_t a = wave_sum(widen((uint32_t)pack)), b = wave_sum(widen((uint32_t)(pack >> 32)));
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            if (const uint32_t x = (uint32_t)(a >> (16 * f)) & 0xFFFF) atomicAdd(&cnt[f], x);
            if (const uint32_t x = (uint32_t)(b >> (16 * f)) & 0xFFFF) atomicAdd(&cnt[4 + f], x);
        }
    }
    if (first != 0xFFFFFFFFu) atomicMin(&cnt[8], first);
    __syncthreads();
    if (threadIdx.x < kScrubRec) rec[(uint64_t)blockIdx.x * kScrubRec + threadIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_scrub_scan(const uint32_t* __restrict__ rec, uint64_t nblocks, uint64_t n,
                                                   uint64_t cap, uint64_t* __restrict__ rank,
                                                   uint64_t* __restrict__ summary) {
    __shared__ uint64_t w4[4];
    __shared__ unsigned long long tot[kSummaryWords];
    if (threadIdx.x < kSummaryWords) tot[threadIdx.x] = threadIdx.x == 10 ? ~0ull : 0ull;
    __syncthreads();
    uint64_t corrupt = 0;   // corrupt pages in the spans before this round (uniform)
    uint64_t acc[7] = {};   // blank, ok by type: this thread's spans
    uint64_t first = ~0ull;
    for (uint64_t base = 0; base < nblocks; base += 256) {
        const uint64_t b = base + threadIdx.x;
        uint64_t c = 0;
        if (b < nblocks) {
            const uint32_t* r = rec + b * kScrubRec;
            c = r[0];
#pragma unroll
            for (int k = 0; k < 7; ++k) acc[k] += r[1 + k];
            if (r[8] != 0xFFFFFFFFu && first == ~0ull) first = b * kScrubSpan + r[8];
        }
        uint64_t total;
        const uint64_t before = block_excl_scan(c, w4, total);
        if (b < nblocks) rank[b] = corrupt + before;
        corrupt += total;
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const uint64_t v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&tot[3 + k], (unsigned long long)v);  // 3 blank, 4..9 ok by type
    }
    if (first != ~0ull) atomicMin(&tot[10], (unsigned long long)first);
    __syncthreads();
    if (threadIdx.x < kSummaryWords) {
        const int i = threadIdx.x;
        uint64_t v = tot[i];
        if (i == 0) v = n;
        if (i == 1) v = tot[4] + tot[5] + tot[6] + tot[7] + tot[8] + tot[9];
        if (i == 2) v = corrupt;
        if (i == 11) v = corrupt < cap ? corrupt : cap;
        summary[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_scrub_list(const uint8_t* __restrict__ cls, uint64_t n,
                                                   const uint32_t* __restrict__ rec,
                                                   const uint64_t* __restrict__ rank, uint64_t cap,
                                                   uint64_t* __restrict__ list) {
    __shared__ uint64_t w4[4];
    const uint64_t r0 = rank[blockIdx.x];
    if (rec[(uint64_t)blockIdx.x * kScrubRec] == 0 || r0 >= cap) return;  // uniform over the block
    const uint64_t p0 = (uint64_t)blockIdx.x * kScrubSpan + threadIdx.x * 16u;
    uint32_t mask = 0;
    if (p0 < n) {
        uint64_t cl, ch;
        ld_bytes16(cls + p0, n - p0, 0xFF, cl, ch);
#pragma unroll
        for (int k = 0; k < 16; ++k) mask |= (byte_of(cl, ch, k) == kClassCorrupt ? 1u : 0u) << k;
    }
    uint64_t total;
    uint64_t pos = r0 + block_excl_scan(__builtin_popcount(mask), w4, total);
    while (mask && pos < cap) {
        const int k = __builtin_ctz(mask);
        mask &= mask - 1;
        list[pos++] = p0 + k;
    }
}

// ---------------------------------------------------------------------------
// Scrub extents (pcs_scrub_extents_dev): the maximal runs of equal class byte
// as (first page, pages, class), ascending and capped, and the summary of the
// written extent, the blank tail and the holes, from class bytes alone (any
// sub-range of a scrub's, at any byte alignment).  The scrub reduction's
// shape again, three launches ordered by construction:
//   k_extent_count  one block per kScrubSpan pages: a page starts a run when
//                   its byte differs from the byte before it (read from
//                   memory, also across lanes and spans; page 0 always); the
//                   span's run starts, blank-run starts, blank pages, first
//                   run start, first blank-run start and last non-blank page
//                   into a record;
//   k_extent_scan   one block: exclusive scan of the records' run starts
//                   (each span's rank in the list), an exclusive suffix
//                   minimum of the spans' first run starts (where the run
//                   that is open at a span's end stops), the summary;
//   k_extent_emit   one block per span again: the spans whose rank is below
//                   the cap write their runs at rank + position; a run's
//                   length is the distance to the next start in the lane, in
//                   the span's later lanes or in a later span, so a listed
//                   run is whole whatever the cap.
// ---------------------------------------------------------------------------
constexpr int kExtentRec = 6;           // u32 per record: starts, blank starts, blank pages, first start, first blank start, last non-blank + 1
constexpr int kExtentWords = 12;        // pcs_extent_summary
constexpr int kExtentRunWords = 3;      // pcs_extent: first_page, n_pages, cls | reserved << 32
constexpr uint32_t kExtentNone = 0xFFFFFFFFu;

// Exclusive suffix minimum of v over a 256-thread block (the minimum over the
// threads after this one, ~0 for the last; w4 as for block_excl_scan); all
// receives the block minimum.
__device__ __forceinline__ uint64_t block_excl_suffix_min(uint64_t v, uint64_t* w4, uint64_t& all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_down((unsigned long long)incl, d, 64);
        if (lane + d < 64 && t < incl) incl = t;
    }
    const uint64_t next = __shfl_down((unsigned long long)incl, 1, 64);
    if (lane == 0) w4[wave] = incl;
    __syncthreads();
    uint64_t after = lane < 63 ? next : ~0ull;
    all = ~0ull;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint64_t x = w4[w];
        if (w > wave && x < after) after = x;
        if (x < all) all = x;
    }
    return after;
}

// This lane's 16 class bytes at page p0 < n: bit k of `starts` when page
// p0 + k starts a run, bit k of `blank` when it is blank, `valid` = the bits
// of the pages below n.
__device__ __forceinline__ void extent_masks(const uint8_t* __restrict__ cls, uint64_t n, uint64_t p0, uint32_t& starts,
                                             uint32_t& blank, uint32_t& valid) {
    const uint64_t cnt = n - p0;
    uint64_t cl, ch;
    ld_bytes16(cls + p0, cnt, 0xFF, cl, ch);
    valid = cnt >= 16 ? 0xFFFFu : (1u << cnt) - 1u;
    uint32_t prev = p0 ? cls[p0 - 1] : 0x100u;  // no byte equals 0x100: page 0 always starts a run
    starts = blank = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t c = byte_of(cl, ch, k);
        starts |= (c != prev ? 1u : 0u) << k;
        blank |= (c == kClassBlank ? 1u : 0u) << k;
        prev = c;
    }
    starts &= valid;
    blank &= valid;
}

__global__ __launch_bounds__(256) void k_extent_count(const uint8_t* __restrict__ cls, uint64_t n,
                                                     uint32_t* __restrict__ rec) {
    __shared__ uint32_t cnt[kExtentRec];
    if (threadIdx.x < kExtentRec) cnt[threadIdx.x] = (threadIdx.x == 3 || threadIdx.x == 4) ? kExtentNone : 0u;
    __syncthreads();
    const uint64_t p0 = (uint64_t)blockIdx.x * kScrubSpan + threadIdx.x * 16u;
    uint64_t pack = 0;  // three 16-bit counters (a wave adds up to 1024 each): starts, blank starts, blank pages
    uint32_t first = kExtentNone, first_blank = kExtentNone, last_written = 0;
    if (p0 < n) {
        uint32_t starts, blank, valid;
        extent_masks(cls, n, p0, starts, blank, valid);
        pack = (uint64_t)__builtin_popcount(starts) | (uint64_t)__builtin_popcount(starts & blank) << 16 |
               (uint64_t)__builtin_popcount(blank) << 32;
        if (starts) first = threadIdx.x * 16u + __builtin_ctz(starts);
        if (starts & blank) first_blank = threadIdx.x * 16u + __builtin_ctz(starts & blank);
        if (const uint32_t w = valid & ~blank) last_written = threadIdx.x * 16u + (32 - __builtin_clz(w));
    }
    const uint64_t sum = wave_sum(pack);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int f = 0; f < 3; ++f)
            if (const uint32_t x = (uint32_t)(sum >> (16 * f)) & 0xFFFF) atomicAdd(&cnt[f], x);
    }
    if (first != kExtentNone) atomicMin(&cnt[3], first);
    if (first_blank != kExtentNone) atomicMin(&cnt[4], first_blank);
    if (last_written) atomicMax(&cnt[5], last_written);
    __syncthreads();
    if (threadIdx.x < kExtentRec) rec[(uint64_t)blockIdx.x * kExtentRec + threadIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_extent_scan(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ rec,
                                                    uint64_t nblocks, uint64_t n, uint64_t cap,
                                                    uint64_t* __restrict__ rank, uint64_t* __restrict__ next,
                                                    uint64_t* __restrict__ summary) {
    __shared__ uint64_t w4[4];
    __shared__ unsigned long long tot[4];  // blank runs, blank pages, first blank, written pages
    if (threadIdx.x < 4) tot[threadIdx.x] = threadIdx.x == 2 ? ~0ull : 0ull;
    __syncthreads();
    uint64_t runs = 0;  // run starts in the spans before this round (uniform)
    uint64_t blank_runs = 0, blank_pages = 0, first_blank = ~0ull, written = 0;  // this thread's spans
    for (uint64_t base = 0; base < nblocks; base += 256) {
        const uint64_t b = base + threadIdx.x;
        uint64_t c = 0;
        if (b < nblocks) {
            const uint32_t* r = rec + b * kExtentRec;
            c = r[0];
            blank_runs += r[1];
            blank_pages += r[2];
            if (r[4] != kExtentNone && first_blank == ~0ull) first_blank = b * kScrubSpan + r[4];
            if (r[5]) written = b * kScrubSpan + r[5];
        }
        uint64_t total;
        const uint64_t before = block_excl_scan(c, w4, total);
        if (b < nblocks) rank[b] = runs + before;
        runs += total;
        __syncthreads();
    }
    // next[b] = the first run start in the spans after b, n when there is none
    uint64_t carry = n;
    for (uint64_t base = (nblocks + 255) / 256 * 256; base != 0;) {
        base -= 256;
        const uint64_t b = base + threadIdx.x;
        uint64_t v = ~0ull;
        if (b < nblocks) {
            const uint32_t f = rec[b * kExtentRec + 3];
            if (f != kExtentNone) v = b * kScrubSpan + f;
        }
        uint64_t all;
        const uint64_t after = block_excl_suffix_min(v, w4, all);
        if (b < nblocks) next[b] = after < carry ? after : carry;
        if (all < carry) carry = all;
        __syncthreads();
    }
    const uint64_t a = wave_sum(blank_runs), p = wave_sum(blank_pages);
    if ((threadIdx.x & 63) == 0) {
        if (a) atomicAdd(&tot[0], (unsigned long long)a);
        if (p) atomicAdd(&tot[1], (unsigned long long)p);
    }
    if (first_blank != ~0ull) atomicMin(&tot[2], (unsigned long long)first_blank);
    if (written) atomicMax(&tot[3], (unsigned long long)written);
    __syncthreads();
    if (threadIdx.x < kExtentWords) {
        const uint64_t n_blank_runs = tot[0], n_blank = tot[1], first = tot[2], w = tot[3];
        const uint64_t last = n ? cls[n - 1] : ~0ull;
        // every blank run but the tail (the one that starts at w) lies below w
        const uint64_t holes = n_blank_runs - (last == kClassBlank ? 1 : 0);
        uint64_t v = 0;
        switch (threadIdx.x) {
            case 0: v = n; break;
            case 1: v = runs; break;
            case 2: v = runs < cap ? runs : cap; break;
            case 3: v = w; break;
            case 4: v = n_blank; break;
            case 5: v = n_blank_runs; break;
            case 6: v = first; break;
            case 7: v = holes; break;
            case 8: v = n_blank - (n - w); break;
            case 9: v = holes ? first : ~0ull; break;
            case 10: v = n ? cls[0] : ~0ull; break;
            default: v = last; break;
        }
        summary[threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(256) void k_extent_emit(const uint8_t* __restrict__ cls, uint64_t n,
                                                    const uint32_t* __restrict__ rec,
                                                    const uint64_t* __restrict__ rank,
                                                    const uint64_t* __restrict__ next, uint64_t cap,
                                                    uint64_t* __restrict__ runs) {
    __shared__ uint64_t w4[4];
    const uint64_t r0 = rank[blockIdx.x];
    if (rec[(uint64_t)blockIdx.x * kExtentRec] == 0 || r0 >= cap) return;  // uniform over the block
    const uint64_t p0 = (uint64_t)blockIdx.x * kScrubSpan + threadIdx.x * 16u;
    uint32_t starts = 0, blank, valid;
    uint64_t cl = 0, ch = 0;
    if (p0 < n) {
        extent_masks(cls, n, p0, starts, blank, valid);
        ld_bytes16(cls + p0, n - p0, 0xFF, cl, ch);
    }
    uint64_t total, all;
    uint64_t pos = r0 + block_excl_scan(__builtin_popcount(starts), w4, total);
    __syncthreads();
    // where the last run that starts in this lane ends: the next start in the span's later lanes, or after the span
    uint64_t end = block_excl_suffix_min(starts ? p0 + __builtin_ctz(starts) : ~0ull, w4, all);
    const uint64_t after = next[blockIdx.x];
    if (after < end) end = after;
    while (starts && pos < cap) {
        const int k = __builtin_ctz(starts);
        starts &= starts - 1;
        const uint64_t stop = starts ? p0 + __builtin_ctz(starts) : end;
        uint64_t* r = runs + pos++ * kExtentRunWords;
        r[0] = p0 + k;
        r[1] = stop - (p0 + k);
        r[2] = byte_of(cl, ch, k);
    }
}

// Streaming-read ceiling, built on k_xxh3_fixed<4096>'s exact
// structure (round 5's 64 KiB-window reader ran ~4 % below
// the hash kernel it was meant to bound): 256-thread blocks of 16 four-KiB
// "pages", a 16-lane group each, loading xxh3_page_fixed<4096>'s chunks in its
// order (chunk 0, then the other 15 dwordx4 non-temporal loads, all issued
// before any is used), xcd_tile order over a grid that covers every tile
// once, and the tile's 16 results staged in LDS and written as one 128-byte
// non-temporal store.  Only the hash is gone: each lane folds its 16 pieces
// with xor/add and the group xor-reduces them into the page's word.
// Occupancy: with 72 VGPRs this body would run 7 waves per SIMD and read
// 3-4 % slower than the hash kernel (4 waves, 120 VGPRs); over 1-7 waves per
// SIMD a plain read of 4 KiB pages is fastest at 2 (7.40 TB/s on 4 GiB, 7.42
// on 32 GiB: tools/lab/occupancy_lab.hip, profiles/r06/occupancy_lab_r06e.txt),
// so run_stream_read caps it there with dynamic LDS (kStreamLdsPad bytes per
// workgroup: two workgroups per CU).  The ceiling is the best plain read of
// these bytes found, not the reader at one arbitrary occupancy.
constexpr uint64_t kStreamPage = 4096;
constexpr size_t kStreamLdsPad = 163840 / 2 - 2048;
__global__ __launch_bounds__(256) void k_stream_read(const uint8_t* __restrict__ buf, uint64_t bytes,
                                                    uint64_t* __restrict__ out) {
    extern __shared__ uint64_t occupancy_pad[];  // allocated for the cap, never used
    __shared__ uint64_t tile_h[16];
    const int g = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const uint64_t npages = (bytes + kStreamPage - 1) / kStreamPage;
    const uint64_t ntiles = (npages + 15) / 16;
    const uint64_t t = xcd_tile(blockIdx.x, ntiles);
    const uint64_t pg = t * 16 + grp;
    if (pg < npages) {
        const u32x4* base = reinterpret_cast<const u32x4*>(buf + pg * kStreamPage) + g;
        const uint64_t lim = bytes - pg * kStreamPage;  // bytes of this page (whole pages: >= 4096)
        u32x4 d[16];
        if (lim >= kStreamPage) {
#pragma unroll
            for (int c = 0; c < 16; ++c) d[c] = ld16<true>(base + c * 16);
        } else {
#pragma unroll
            for (int c = 0; c < 16; ++c)
                d[c] = 256u * c + 16u * g + 16 <= lim ? ld16<true>(base + c * 16) : u32x4{0, 0, 0, 0};
        }
        uint32_t x = 0, y = 0, z = 0, v = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            x ^= d[c].x;
            y += d[c].y;
            z ^= d[c].z;
            v += d[c].w;
        }
        uint64_t r = ((uint64_t)(x ^ z) << 32) | (y + v);
        r ^= dpp64<kRowRor1>(r);
        r ^= dpp64<kRowRor2>(r);
        r ^= dpp64<kRowRor4>(r);
        r ^= dpp64<kRowRor8>(r);
        if (g == 0) tile_h[grp] = r;
    }
    __syncthreads();
    const uint64_t i = t * 16 + threadIdx.x;
    if (threadIdx.x < 16 && i < npages) st_nt(out + i, tile_h[threadIdx.x]);
    if (bytes == 0) occupancy_pad[threadIdx.x] = 0;  // never taken (bytes >= 16): keeps the array
}

// ---------------------------------------------------------------------------
// launch plumbing
// ---------------------------------------------------------------------------
namespace {

int g_cu_count[64];
std::once_flag g_cu_once[64];

int cu_count() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    std::call_once(g_cu_once[dev], [dev] {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        g_cu_count[dev] = cus;
    });
    return g_cu_count[dev];
}

// Grid for a grid-stride kernel: enough 256-thread blocks to cover the work,
// capped at blocks_per_cu resident blocks per CU.
unsigned grid_for(uint64_t units, unsigned units_per_block, unsigned blocks_per_cu) {
    const uint64_t need = (units + units_per_block - 1) / units_per_block;
    const uint64_t cap = (uint64_t)cu_count() * blocks_per_cu;
    return (unsigned)(need < cap ? (need ? need : 1) : cap);
}

constexpr unsigned kBlock = 256;
constexpr unsigned kBlocksPerCu = 8;  // grid-stride cap for the auxiliary kernels

// Device scratch for multi-kernel operations (two-pass stamp, manifest
// chunk tables), fenced by events instead of the stream-ordered allocator.
// hipMallocAsync / hipFreeAsync scratch was measured to lose writes: a stamp
// enqueued while the GPU was still busy left 7 % of the page headers zero
// (tools/lab/read_lab.hip "stamp", profiles/r01/stamp_lab.txt).  A buffer
// here is handed out only when the event recorded after its last use has
// completed, so concurrent streams and host threads never share one in
// flight.  Buffers are kept for reuse (bounded by the number of operations
// in flight at once).
class ScratchPool {
public:
    hipError_t acquire(size_t bytes, void** out, int* id) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        // Oversized idle buffers given back here are freed after the mutex is
        // released: hipFree synchronises the device, and other threads'
        // acquire/release calls must not wait behind it.
        std::vector<void*> to_free;
        e = acquire_locked(dev, bytes, out, id, to_free);
        for (void* p : to_free) (void)hipFree(p);
        return e;
    }
    // The buffer becomes reusable once the work queued on s so far completes.
    hipError_t release(int id, hipStream_t s) {
        std::lock_guard<std::mutex> lk(mu_);
        Buf& b = bufs_[(size_t)id];
        const hipError_t e = hipEventRecord(b.done, s);
        b.busy = false;
        return e;
    }

private:
    hipError_t acquire_locked(int dev, size_t bytes, void** out, int* id, std::vector<void*>& to_free) {
        hipError_t e = hipSuccess;
        std::lock_guard<std::mutex> lk(mu_);
        int empty = -1;
        for (size_t i = 0; i < bufs_.size(); ++i) {
            Buf& b = bufs_[i];
            if (b.dev != dev || b.busy) continue;
            if (!b.p) {
                empty = (int)i;
                continue;
            }
            const hipError_t q = hipEventQuery(b.done);
            if (q == hipErrorNotReady) continue;
            if (q != hipSuccess) {
                // The query itself failed, so the buffer cannot be shown idle:
                // leave it to a later call and take another.  Seen as
                // hipErrorCapturedEvent with no capture anywhere in the process,
                // for an event last recorded on a stream that no longer exists;
                // the scratch of a caller whose stream is gone must not fail the
                // next caller.  The error is cleared so that the launches that
                // follow do not report it as theirs; a real device error comes
                // back from them or from hipMalloc below.
                (void)hipGetLastError();
                continue;
            }
            // An idle buffer above kKeepBytes serves only a request of at least
            // half its size; any other request gives it back, so one large
            // manifest or stamp does not pin its scratch for the process life.
            const bool fits = b.bytes >= bytes && (b.bytes <= kKeepBytes || 2 * bytes >= b.bytes);
            if (!fits) {
                if (b.bytes > kKeepBytes) {
                    to_free.push_back(b.p);
                    b.p = nullptr;
                    b.bytes = 0;
                    if (empty < 0) empty = (int)i;
                }
                continue;
            }
            b.busy = true;
            *out = b.p;
            *id = (int)i;
            return hipSuccess;
        }
        Buf b;
        b.dev = dev;
        b.bytes = std::max<size_t>(bytes, 1u << 20);
        if ((e = hipMalloc(&b.p, b.bytes)) != hipSuccess) return e;
        b.busy = true;
        if (empty >= 0) {
            b.done = bufs_[(size_t)empty].done;
            bufs_[(size_t)empty] = b;
            *id = empty;
        } else {
            if ((e = hipEventCreateWithFlags(&b.done, hipEventDisableTiming)) != hipSuccess) {
                (void)hipFree(b.p);
                return e;
            }
            bufs_.push_back(b);
            *id = (int)bufs_.size() - 1;
        }
        *out = b.p;
        return hipSuccess;
    }

    static constexpr size_t kKeepBytes = 256u << 20;  // larger idle buffers are freed, not kept
    struct Buf {
        void* p = nullptr;
        size_t bytes = 0;
        hipEvent_t done = nullptr;
        int dev = 0;
        bool busy = false;
    };
    std::mutex mu_;
    std::vector<Buf> bufs_;
};
ScratchPool g_scratch;

// RAII lease of a scratch buffer for the work enqueued on one stream.
struct ScratchLease {
    void* p = nullptr;
    int id = -1;
    hipStream_t s;
    explicit ScratchLease(hipStream_t st) : s(st) {}
    hipError_t get(size_t bytes) { return g_scratch.acquire(bytes, &p, &id); }
    ~ScratchLease() {
        if (id >= 0) (void)g_scratch.release(id, s);
    }
};

bool is_pow2_page(uint64_t P) { return P >= 256 && P <= 65536 && (P & (P - 1)) == 0; }

// Process-unique launch ids for the off-shape flag word (k_xxh64_lds ->
// k_generic_desc): a random start, so a scratch word's stale contents (an
// older id, or whatever a fresh allocation holds) never match a new one.
uint64_t next_call_id() {
    static std::atomic<uint64_t> next{[] {
        uint64_t x = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count() ^ 0x9E3779B97F4A7C15ull;
        x ^= x >> 33;
        x *= 0xFF51AFD7ED558CCDull;
        return x ^ (x >> 33);
    }()};
    return next.fetch_add(1, std::memory_order_relaxed);
}

}  // namespace

// ---------------------------------------------------------------------------
// tuning knobs (pcs_set_tuning): read at every launch
// ---------------------------------------------------------------------------
namespace {
constexpr int kTuneKeys = 40;
// Keys retired in round 2 with the variants they selected (measured slower,
// DESIGN.md §4): 4 XXH64 nt loads, 5 in-place stamp width, 10 descriptor tile
// sort, 12 descriptor slices, 14 XXH64 descriptor sort; round-2 experiments
// (commit 99804f2): 16 pages dealt to a wave's groups as they free up (+-1 %,
// profiles/r02/desc_wave_lab.txt), 17 pipelined split tiles (-2..-22 %,
// split_pipe_lab.txt), 18 plain result stores (+-0.2 %, result_store_lab.txt),
// 19 descriptor pages as a slice stream (-5..-8 %, desc_slices_lab.txt),
// 20 4 KiB-aligned descriptor steps (+-0.2 %, aligned_steps_lab.txt), 21 the
// descriptor body at 4 waves per SIMD (-0.6..-2.3 %, desc_lean_lab.txt);
// round 3: 22 the XXH64 direct-to-LDS segment ring (config 3 -0.8..-34 %,
// profiles/r03/x64_glds_ab_*.txt), 25 XXH64 tile-order chunks (no gain, a lab
// knob in commit 01e849b); round 5: 32 service polls kept in flight (+0.7 to
// +2.8 us per request, profiles/r05/service_poll_lab_r05k.txt).  Setting one
// fails.
constexpr bool kRetired[kTuneKeys] = {false, false, false, false, true, true, false, false, false, false, true,  false,
                                      true,  false, true,  false, true,  true,  true,  true,  true,  true,  true,  false,
                                      false, true,  false, false, false, true,  false, false, true,  false,
                                      false, false, false, /*37: never assigned*/ true, false, false};
std::atomic<int64_t> g_tune[kTuneKeys] = {0, /*xxh3 blocks/CU*/ 0, /*xxh64 blocks/CU*/ 0, /*xxh3 nt*/ 1,
                                          /*retired*/ 0, /*retired*/ 0, /*xxh64 LDS depth (2/3/4/5 -> 1/2/4/3)*/ 0,
                                          /*zero copy*/ 1, /*xxh3 run-time size: 4-block batches*/ 1,
                                          /*xxh3 split pages from this size (0 = never)*/ 8192,
                                          /*retired*/ 0,
                                          /*zero-copy page list in kernel arguments*/ 1,
                                          /*retired*/ 0,
                                          /*manifest: wide block sums + chain kernel*/ 1,
                                          /*retired*/ 0,
                                          /*xxh64 LDS kernel: waves per workgroup (1, 2; else 4)*/ 4,
                                          /*retired*/ 0, /*retired*/ 0, /*retired*/ 0, /*retired*/ 0,
                                          /*retired*/ 0,
                                          /*retired*/ 0,
                                          /*retired (round 3: XXH64 direct-to-LDS ring)*/ 0,
                                          /*zero-copy validate: completion from the verdicts themselves*/ 1,
                                          /*validate service stream: 1 highest priority, 0 plain*/ 1,
                                          /*retired (round 3 lab: XXH64 tile-order chunks)*/ 0,
                                          /*test only: validate service torn-line drill, microseconds*/ 0,
                                          /*test only: host-batch calls left to fail*/ 0,
                                          /*validate service contention gate: callers (0 = off)*/ 2,
                                          /*retired (round 4 lab: XXH64 equal-byte runs)*/ 0,
                                          /*test only: service requests left to post as a stale partial answer*/ 0,
                                          /*zero-copy XXH3 stamps: done-byte completion up to this many pages*/ 256,
                                          /*retired (round 5 lab: service polls in flight)*/ 0,
                                          /*test only: service kernels serve nothing and leave this many us late*/ 0,
                                          /*zero-copy batches completing from their verdicts: event behind the kernel*/ 0,
                                          /*sync host calls: microseconds of spinning before sleeping between checks (0 = spin)*/ 0,
                                          /*validate service: polls read the kernel's departure words*/ 1,
                                          /*never assigned*/ 0,
                                          /*manifest scan: slots per LDS tile of the walk (power of two, 64..4096)*/ 2048,
                                          /*manifest replay: bytes of a mapping section per decode work item (power of two, 64..4096)*/ 4096};
}
int set_tuning(int key, int64_t value) {
    if (key <= 0 || key >= kTuneKeys || kRetired[key] || value < 0) return -1;
    // the replay's tile is also the unit its scratch is sized by: only a power of two in [64, 4096]
    if (key == 39 && (value < 64 || value > 4096 || (value & (value - 1)) != 0)) return -1;
    g_tune[key].store(value, std::memory_order_relaxed);
    return 0;
}
bool take_tuning(int key) {
    if (key <= 0 || key >= kTuneKeys || kRetired[key]) return false;
    int64_t v = g_tune[key].load(std::memory_order_relaxed);
    while (v > 0)
        if (g_tune[key].compare_exchange_weak(v, v - 1, std::memory_order_relaxed)) return true;
    return false;
}
int64_t get_tuning(int key) {
    return (key <= 0 || key >= kTuneKeys || kRetired[key]) ? -1 : g_tune[key].load(std::memory_order_relaxed);
}

namespace {
// Page kernels: the knob caps the grid at that many 256-thread blocks per CU
// (grid-stride loop beyond); 0 = auto.  Auto launches one block per 16 (XXH3)
// / 64 (XXH64) pages for pages up to 16 KiB and caps at 8 blocks per CU for
// larger pages (measured, profiles/r01_kernel_lab.txt).
unsigned page_grid(uint64_t n, unsigned pages_per_block, int key, uint64_t page_size = 0) {
    int64_t bpc = g_tune[key].load(std::memory_order_relaxed);
    if (bpc == 0) bpc = page_size > 16384 ? 8 : (int64_t)1 << 30;
    const uint64_t need = (n + pages_per_block - 1) / pages_per_block;
    const uint64_t cap = std::min<uint64_t>((uint64_t)cu_count() * (uint64_t)bpc, 0x7FFFFFFFull);
    return (unsigned)(need < cap ? (need ? need : 1) : cap);
}
bool use_nt() { return g_tune[3].load(std::memory_order_relaxed) != 0; }
// Fixed-size XXH3 pages hashed by k_xxh3_split (PCS_TUNE_XXH3_SPLIT_PAGES).
bool split_pages(uint64_t P) {
    const int64_t split = g_tune[9].load(std::memory_order_relaxed);
    return split > 0 && P >= (uint64_t)split && P >= 8192 && P <= 65536 && (P & (P - 1)) == 0;
}
bool rt_batch4() { return g_tune[8].load(std::memory_order_relaxed) != 0; }

// XXH64 LDS kernel launch with the segment depth from PCS_TUNE_XXH64_LAYOUT
// (0 or 1 = default depth, 2/3/4/5 = depth 1/2/4/3) and the waves per workgroup
// from PCS_TUNE_XXH64_WAVES.
template <int MODE, bool NT, int ADDR>
void launch_xxh64_lds(unsigned grid, hipStream_t s, const uint8_t* base, const uint64_t* off, const uint32_t* len,
                      uint32_t P, uint64_t n, uint64_t* out, uint8_t* ok, unsigned long long* fb,
                      unsigned long long* offshape = nullptr, uint64_t call_id = 0) {
    const int64_t lay = g_tune[6].load(std::memory_order_relaxed);
    const int depth = lay == 2 ? 1 : lay == 3 ? 2 : lay == 4 ? 4 : lay == 5 ? 3 : kX64LdsDepth;
    const int64_t wpb = g_tune[15].load(std::memory_order_relaxed);
    if (wpb == 1 || wpb == 2) {
        // one workgroup per 16 * wpb pages, every tile covered once
        const unsigned g = (unsigned)std::min<uint64_t>((n + 16 * wpb - 1) / (16 * wpb), 0x7FFFFFFFull);
#define LW(D, W) hipLaunchKernelGGL((k_xxh64_lds<MODE, NT, ADDR, D, W>), dim3(g), dim3(64 * W), 0, s, base, off, len, P, n, out, ok, fb, offshape, call_id)
        if (wpb == 1) {
            if (depth == 1) LW(1, 1);
            else if (depth == 2) LW(2, 1);
            else if (depth == 3) LW(3, 1);
            else LW(4, 1);
        } else {
            if (depth == 1) LW(1, 2);
            else if (depth == 2) LW(2, 2);
            else if (depth == 3) LW(3, 2);
            else LW(4, 2);
        }
#undef LW
        return;
    }
#define L(D) hipLaunchKernelGGL((k_xxh64_lds<MODE, NT, ADDR, D>), dim3(grid), dim3(kBlock), 0, s, base, off, len, P, n, out, ok, fb, offshape, call_id)
    if (depth == 1) L(1);
    else if (depth == 2) L(2);
    else if (depth == 3) L(3);
    else L(4);
#undef L
}

template <int MODE, bool NT>
hipError_t launch_xxh3_pages(uint64_t P, const uint8_t* pages, uint64_t n, uint64_t* out, uint8_t* ok,
                             unsigned long long* fb, hipStream_t s) {
    const unsigned grid = page_grid(n, kBlock / 16, 1, P);  // kBlock/16 = one 16-page tile per block
    if (P % 256 != 0) {  // off the chunk grid: the any-size body
        hipLaunchKernelGGL((k_xxh3_stride<MODE, NT, 2>), dim3(grid), dim3(kBlock), 0, s, pages, (uint32_t)P, n, out, ok,
                           fb);
        return hipGetLastError();
    }
    if ((uintptr_t)pages % 16 != 0) {
        // on the grid but not 16-byte aligned: the chunked run-time-size body
        // reads unaligned 16-byte pieces at ~6 TB/s (4 KiB pages at base + 8),
        // the any-size body's 8-byte final-block loads at ~4.5
        hipLaunchKernelGGL((k_xxh3_stride<MODE, NT, 1>), dim3(grid), dim3(kBlock), 0, s, pages, (uint32_t)P, n, out, ok,
                           fb);
        return hipGetLastError();
    }
    if (split_pages(P)) {
        const uint64_t ppb = 16 / (P / 4096);
        const uint64_t need = (n + ppb - 1) / ppb;
        const unsigned g = (unsigned)std::min<uint64_t>(need, 0x7FFFFFFFull);
        switch (P) {
#define CASE(SZ) \
    case SZ: hipLaunchKernelGGL((k_xxh3_split<SZ, MODE, NT>), dim3(g), dim3(kBlock), 0, s, pages, n, out, ok, fb); break;
            CASE(8192) CASE(16384) CASE(32768) CASE(65536)
#undef CASE
        }
        return hipGetLastError();
    }
    switch (P) {
#define CASE(SZ)                                                                                             \
    case SZ:                                                                                                 \
        hipLaunchKernelGGL((k_xxh3_fixed<SZ, MODE, NT>), dim3(grid), dim3(kBlock), 0, s, pages, n, out, ok, fb);     \
        break;
        CASE(256) CASE(512) CASE(1024) CASE(2048) CASE(4096) CASE(8192) CASE(16384) CASE(32768) CASE(65536)
#undef CASE
        default:
            if (rt_batch4())
                hipLaunchKernelGGL((k_xxh3_stride<MODE, NT, 1>), dim3(grid), dim3(kBlock), 0, s, pages, (uint32_t)P,
                                   n, out, ok, fb);
            else
                hipLaunchKernelGGL((k_xxh3_stride<MODE, NT, 0>), dim3(grid), dim3(kBlock), 0, s, pages, (uint32_t)P,
                                   n, out, ok, fb);
    }
    return hipGetLastError();
}

}  // namespace

// Fixed-stride pages.  Shape checks are done by the caller (capi).
template <int MODE>
static hipError_t pages_impl(int algo, const uint8_t* pages, uint64_t P, uint64_t n, uint64_t* out, uint8_t* ok,
                             unsigned long long* fb, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const bool aligned16 = ((uintptr_t)pages % 16) == 0;
    const bool aligned8 = ((uintptr_t)pages % 8) == 0;
    // XXH3: the chunked kernels on the 256-byte grid at 16-byte alignment, the
    // any-size body (k_xxh3_stride<..., 2>) for every other long-path size
    if (algo == 0 && P >= 249 && P <= 0xFFFFFFFFull) {
        if constexpr (MODE == kStamp) {
            // two-pass stamp: digests into a compact array (the fast digest
            // kernel), then one scattered 8-byte write per page
            uint64_t* dig = out;
            hipError_t e = hipSuccess;
            ScratchLease scratch(s);
            if (!dig) {
                e = scratch.get(n * 8);
                dig = static_cast<uint64_t*>(scratch.p);
            }
            if (e == hipSuccess)
                e = use_nt() ? launch_xxh3_pages<kDigest, true>(P, pages, n, dig, nullptr, nullptr, s)
                             : launch_xxh3_pages<kDigest, false>(P, pages, n, dig, nullptr, nullptr, s);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_scatter_stamp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                                   const_cast<uint8_t*>(pages), P, n, dig);
                e = hipGetLastError();
            }
            return e;
        } else {
            return use_nt() ? launch_xxh3_pages<MODE, true>(P, pages, n, out, ok, fb, s)
                            : launch_xxh3_pages<MODE, false>(P, pages, n, out, ok, fb, s);
        }
    }
    if (algo == 1 && aligned8 && P % 8 == 0 && P >= 40 && P <= 0xFFFFFFFFull) {
        const bool lines = aligned16 && P % 64 == 0 && P >= 128;
        if (lines) {
            // one workgroup per 64 pages at every page size: the large-page
            // cap of page_grid (8 per CU) cost the LDS kernel 7-8 % on 64 KiB
            // pages (profiles/r01/x64_depth_lab.txt, x64_waves_lab.txt)
            const unsigned lgrid = page_grid(n, kBlock / 4, 2);
            if (use_nt()) launch_xxh64_lds<MODE, true, kAddrStride>(lgrid, s, pages, nullptr, nullptr, (uint32_t)P, n, out, ok, fb);
            else launch_xxh64_lds<MODE, false, kAddrStride>(lgrid, s, pages, nullptr, nullptr, (uint32_t)P, n, out, ok, fb);
            return hipGetLastError();
        }
        const unsigned grid = page_grid(n, kBlock / 4, 2, P);
        hipLaunchKernelGGL((k_xxh64_stride<MODE>), dim3(grid), dim3(kBlock), 0, s, pages, (uint32_t)P, n, out, ok, fb);
        return hipGetLastError();
    }
    return hipErrorNotSupported;  // caller falls back to the descriptor path
}

__global__ void k_uniform_desc(uint64_t P, uint64_t n, uint64_t* __restrict__ off, uint32_t* __restrict__ len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        off[i] = i * P;
        len[i] = (uint32_t)P;
    }
}

hipError_t run_pages(int mode, int algo, const uint8_t* pages, uint64_t P, uint64_t n, uint64_t* out, uint8_t* ok,
                     unsigned long long* fb, hipStream_t s) {
    hipError_t e;
    switch (mode) {
        case kDigest: e = pages_impl<kDigest>(algo, pages, P, n, out, ok, fb, s); break;
        case kValidate: e = pages_impl<kValidate>(algo, pages, P, n, out, ok, fb, s); break;
        default: e = pages_impl<kStamp>(algo, pages, P, n, out, ok, fb, s); break;
    }
    if (e != hipErrorNotSupported) return e;
    // Odd shape (unaligned base, page size off the fast kernels): the same
    // pages as a descriptor batch (off = i * P, len = P) built on the device.
    ScratchLease scratch(s);
    if ((e = scratch.get(n * 12)) != hipSuccess) return e;
    uint64_t* off = static_cast<uint64_t*>(scratch.p);
    uint32_t* len = reinterpret_cast<uint32_t*>(off + n);
    hipLaunchKernelGGL(k_uniform_desc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, n, off, len);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return run_desc(mode, algo, pages, off, len, n, 8, 0, out, ok, fb, s);
}

// Scrub: the XXH3 page kernels in kScrub mode (one read of the pages; class
// and type bytes out), then the ordered reduction over those bytes.  Nothing
// here waits for the stream; n == 0 still writes the whole summary.
hipError_t run_scrub(const uint8_t* pages, uint64_t P, uint64_t n, uint8_t* cls, uint8_t* type, uint64_t* summary,
                     uint64_t* list, uint64_t cap, hipStream_t s) {
    const uint64_t nblocks = (n + kScrubSpan - 1) / kScrubSpan;
    if (nblocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    ScratchLease scratch(s);  // ranks, records and (when the caller wants no type bytes) the types
    uint64_t* rank = nullptr;
    uint32_t* rec = nullptr;
    if (n) {
        const size_t rec_bytes = (nblocks * kScrubRec * 4 + 7) & ~size_t(7);
        hipError_t e = scratch.get(nblocks * 8 + rec_bytes + (type ? 0 : n));
        if (e != hipSuccess) return e;
        rank = static_cast<uint64_t*>(scratch.p);
        rec = reinterpret_cast<uint32_t*>(rank + nblocks);
        if (!type) type = reinterpret_cast<uint8_t*>(rec) + rec_bytes;
        uint64_t* types_slot = reinterpret_cast<uint64_t*>(type);  // the digest slot carries the type array (scrub_types)
        e = use_nt() ? launch_xxh3_pages<kScrub, true>(P, pages, n, types_slot, cls, nullptr, s)
                     : launch_xxh3_pages<kScrub, false>(P, pages, n, types_slot, cls, nullptr, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_scrub_count, dim3((unsigned)nblocks), dim3(256), 0, s, cls, type, n, rec);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_scrub_scan, dim3(1), dim3(256), 0, s, rec, nblocks, n, cap, rank, summary);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && n && cap) {
        hipLaunchKernelGGL(k_scrub_list, dim3((unsigned)nblocks), dim3(256), 0, s, cls, n, rec, rank, cap, list);
        e = hipGetLastError();
    }
    return e;
}

// Extents of n class bytes: summary and the first min(runs, cap) runs.  Reads
// cls only; nothing here waits for the stream; n == 0 still writes the whole
// summary.
hipError_t run_extents(const uint8_t* cls, uint64_t n, uint64_t* summary, uint64_t* runs, uint64_t cap,
                       hipStream_t s) {
    const uint64_t nblocks = (n + kScrubSpan - 1) / kScrubSpan;
    if (nblocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    ScratchLease scratch(s);  // ranks, next starts and records
    uint64_t *rank = nullptr, *next = nullptr;
    uint32_t* rec = nullptr;
    if (n) {
        hipError_t e = scratch.get(nblocks * (16 + kExtentRec * 4));
        if (e != hipSuccess) return e;
        rank = static_cast<uint64_t*>(scratch.p);
        next = rank + nblocks;
        rec = reinterpret_cast<uint32_t*>(next + nblocks);
        hipLaunchKernelGGL(k_extent_count, dim3((unsigned)nblocks), dim3(256), 0, s, cls, n, rec);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_extent_scan, dim3(1), dim3(256), 0, s, cls, rec, nblocks, n, cap, rank, next, summary);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && n && cap) {
        hipLaunchKernelGGL(k_extent_emit, dim3((unsigned)nblocks), dim3(256), 0, s, cls, n, rec, rank, next, cap, runs);
        e = hipGetLastError();
    }
    return e;
}

// ---------------------------------------------------------------------------
// Scrub files (pcs_scrub_files_dev): one report per data file of a batch from
// the class and type bytes a scrub wrote.  File f is pages [first[f],
// first[f + 1]); the boundaries live on the device, so nothing here may trust
// them.  A segmented form of the two reductions above, four launches ordered
// by construction (no atomic on global memory):
//   k_files_plan     one block, rounds of 256 x kFilesPerThread files, each
//                    thread taking consecutive files so that a round's loads
//                    are in flight together: checks every boundary pair (first[f] <=
//                    first[f + 1] <= n) and scans the files' work items, an
//                    item being a span of at most kScrubSpan pages that never
//                    crosses a file boundary: items_before[f] = sum of
//                    ceil(len / kScrubSpan) over the files before f.  The
//                    first invalid file and the item total go into two status
//                    words; every later kernel leaves at once when the status
//                    names an invalid file, so no page index is ever formed
//                    from an unchecked boundary;
//   k_files_count    one block per item (the host sizes the grid by the bound
//                    n / kScrubSpan + n_files; blocks past the total leave):
//                    finds its file by a block-uniform binary search over
//                    items_before, reads its span's class and type bytes,
//                    clipped to the file, and writes a record: the eight
//                    scrub counters, the first corrupt page, the blank-run
//                    starts, the first of them and the last non-blank page.
//                    The byte before a lane's pages is read only inside the
//                    file: a file's first page has no predecessor;
//   k_files_reduce   a wave per file over the file's contiguous records: the
//                    16-word report (hole fields derived as k_extent_scan
//                    derives them) and a flag byte (corrupt, hole, unwritten);
//   k_files_summary  one block, the same rounds: totals, an exclusive scan of
//                    the bad flags and the capped ascending list of bad files.
// ---------------------------------------------------------------------------
constexpr int kFileRec = 12;  // u32 per record: corrupt, blank, ok_by_type[6], first corrupt, blank-run starts, first blank-run start, last non-blank + 1
constexpr int kFileReportWords = 16;    // pcs_file_report
constexpr int kFilesSummaryWords = 12;  // pcs_files_summary
constexpr uint32_t kFileCorrupt = 1, kFileHole = 2, kFileUnwritten = 4;  // flag byte of a file
constexpr int kFilesPerThread = 8;  // consecutive files per thread and round of the two one-block kernels

__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t t = __shfl_xor((unsigned long long)v, d, 64);
        if (t < v) v = t;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t t = __shfl_xor((unsigned long long)v, d, 64);
        if (t > v) v = t;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_files_plan(const uint64_t* __restrict__ first, uint64_t n_files, uint64_t n,
                                                   uint64_t* __restrict__ items_before,
                                                   uint64_t* __restrict__ status) {
    __shared__ uint64_t w4[4];
    __shared__ unsigned long long bad;
    if (threadIdx.x == 0) bad = ~0ull;
    __syncthreads();
    uint64_t items = 0;        // items of the files before this round (uniform)
    uint64_t invalid = ~0ull;  // this thread's first invalid file
    for (uint64_t base = 0; base < n_files; base += 256 * kFilesPerThread) {
        const uint64_t f0 = base + (uint64_t)threadIdx.x * kFilesPerThread;  // this thread's consecutive files
        uint64_t c[kFilesPerThread], sum = 0;
        uint64_t a = f0 < n_files ? first[f0] : 0;
#pragma unroll
        for (int k = 0; k < kFilesPerThread; ++k) {
            c[k] = 0;
            if (f0 + k < n_files) {
                const uint64_t b = first[f0 + k + 1];
                if (a > b || b > n) {
                    if (invalid == ~0ull) invalid = f0 + k;
                } else {
                    c[k] = (b - a + kScrubSpan - 1) / kScrubSpan;
                }
                a = b;
            }
            sum += c[k];
        }
        uint64_t total;
        uint64_t run = items + block_excl_scan(sum, w4, total);
#pragma unroll
        for (int k = 0; k < kFilesPerThread; ++k) {
            if (f0 + k < n_files) items_before[f0 + k] = run;
            run += c[k];
        }
        items += total;
        __syncthreads();
    }
    if (invalid != ~0ull) atomicMin(&bad, (unsigned long long)invalid);
    __syncthreads();
    if (threadIdx.x == 0) {
        items_before[n_files] = items;
        status[0] = bad;
        status[1] = items;
    }
}

__global__ __launch_bounds__(256) void k_files_count(const uint8_t* __restrict__ cls, const uint8_t* __restrict__ type,
                                                    const uint64_t* __restrict__ first, uint64_t n_files,
                                                    const uint64_t* __restrict__ items_before,
                                                    const uint64_t* __restrict__ status, uint32_t* __restrict__ rec) {
    const uint64_t item = blockIdx.x;
    if (status[0] != ~0ull || item >= status[1]) return;  // uniform over the block
    // the file that holds the item: items_before[lo] <= item < items_before[hi] (empty files share their
    // successor's count, so the search ends on the file that has items)
    uint64_t lo = 0, hi = n_files;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (items_before[mid] <= item) lo = mid;
        else hi = mid;
    }
    const uint64_t begin = first[lo], end = first[lo + 1];
    const uint64_t s0 = begin + (item - items_before[lo]) * kScrubSpan;
    const uint64_t s1 = end - s0 < kScrubSpan ? end : s0 + kScrubSpan;
    __shared__ uint32_t cnt[kFileRec];
    if (threadIdx.x < kFileRec) cnt[threadIdx.x] = (threadIdx.x == 8 || threadIdx.x == 10) ? kExtentNone : 0u;
    __syncthreads();
    const uint64_t p0 = s0 + threadIdx.x * 16u;
    uint64_t pack = 0;  // eight 8-bit counters (at most 16 each): corrupt, blank, ok by type bucket 0..5
    uint32_t first_corrupt = kExtentNone, first_blank = kExtentNone, last_written = 0, nstarts = 0;
    if (p0 < s1) {
        const uint64_t left = s1 - p0;
        uint64_t cl, ch, tl, th;
        ld_bytes16(cls + p0, left, 0xFF, cl, ch);
        ld_bytes16(type + p0, left, 0, tl, th);
        const uint32_t valid = left >= 16 ? 0xFFFFu : (1u << left) - 1u;
        uint32_t blank = 0;
#pragma unroll
        for (int k = 15; k >= 0; --k) {
            const uint32_t c = byte_of(cl, ch, k), t = byte_of(tl, th, k);
            const int bucket = t < 4 ? (int)t : t == 255 ? 4 : 5;
            const int field = c == kClassCorrupt ? 0 : c == kClassBlank ? 1 : 2 + bucket;
            pack += (c <= kClassBlank) ? 1ull << (8 * field) : 0;
            if (c == kClassCorrupt) first_corrupt = threadIdx.x * 16u + k;
            blank |= (c == kClassBlank ? 1u : 0u) << k;
        }
        blank &= valid;
        // a blank page starts a blank run unless the page before it, in the same file, is blank
        const uint32_t prev_blank = (p0 > begin && cls[p0 - 1] == kClassBlank) ? 1u : 0u;
        const uint32_t starts = blank & ~((blank << 1) | prev_blank);
        nstarts = __builtin_popcount(starts);
        if (starts) first_blank = threadIdx.x * 16u + __builtin_ctz(starts);
        if (const uint32_t w = valid & ~blank) last_written = threadIdx.x * 16u + (32 - __builtin_clz(w));
    }
    auto widen = [](uint32_t v) {
        return (uint64_t)(v & 0xFF) | (uint64_t)((v >> 8) & 0xFF) << 16 | (uint64_t)((v >> 16) & 0xFF) << 32 |
               (uint64_t)(v >> 24) << 48;
    };
    const uint64_t a = wave_sum(widen((uint32_t)pack)), b = wave_sum(widen((uint32_t)(pack >> 32)));
    const uint64_t st = wave_sum(nstarts);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            if (const uint32_t x = (uint32_t)(a >> (16 * f)) & 0xFFFF) atomicAdd(&cnt[f], x);
            if (const uint32_t x = (uint32_t)(b >> (16 * f)) & 0xFFFF) atomicAdd(&cnt[4 + f], x);
        }
        if (st) atomicAdd(&cnt[9], (uint32_t)st);
    }
    if (first_corrupt != kExtentNone) atomicMin(&cnt[8], first_corrupt);
    if (first_blank != kExtentNone) atomicMin(&cnt[10], first_blank);
    if (last_written) atomicMax(&cnt[11], last_written);
    __syncthreads();
    if (threadIdx.x < kFileRec) rec[item * kFileRec + threadIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_files_reduce(const uint64_t* __restrict__ first, uint64_t n_files,
                                                     const uint64_t* __restrict__ items_before,
                                                     const uint64_t* __restrict__ status,
                                                     const uint32_t* __restrict__ rec, uint64_t* __restrict__ reports,
                                                     uint8_t* __restrict__ flags) {
    if (status[0] != ~0ull) return;
    const int lane = threadIdx.x & 63;
    const uint64_t f = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= n_files) return;  // uniform over the wave
    const uint64_t begin = first[f], len = first[f + 1] - begin;
    const uint64_t r0 = items_before[f], r1 = items_before[f + 1];
    uint64_t acc[9] = {};  // corrupt, blank, ok by type, blank-run starts
    uint64_t first_corrupt = ~0ull, first_blank = ~0ull, written = 0;
    for (uint64_t r = r0 + lane; r < r1; r += 64) {  // a lane's records ascend
        const uint32_t* q = rec + r * kFileRec;
        const uint64_t off = (r - r0) * kScrubSpan;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += q[k];
        acc[8] += q[9];
        if (q[8] != kExtentNone && first_corrupt == ~0ull) first_corrupt = off + q[8];
        if (q[10] != kExtentNone && first_blank == ~0ull) first_blank = off + q[10];
        if (q[11]) written = off + q[11];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = wave_sum(acc[k]);
    first_corrupt = wave_min(first_corrupt);
    first_blank = wave_min(first_blank);
    written = wave_max(written);
    // every blank run but the tail (the one that starts at `written`) lies below `written`
    const uint64_t holes = acc[8] - (written < len ? 1 : 0);
    if (lane < kFileReportWords) {
        uint64_t v;
        switch (lane) {
            case 0: v = begin; break;
            case 1: v = len; break;
            case 2: v = acc[2] + acc[3] + acc[4] + acc[5] + acc[6] + acc[7]; break;
            case 3: v = acc[0]; break;
            case 4: v = acc[1]; break;
            case 11: v = first_corrupt; break;
            case 12: v = written; break;
            case 13: v = holes; break;
            case 14: v = acc[1] - (len - written); break;
            case 15: v = holes ? first_blank : ~0ull; break;
            default: v = acc[lane - 3]; break;  // 5..10: ok by type
        }
        reports[f * kFileReportWords + lane] = v;
    }
    if (lane == 0)
        flags[f] = (uint8_t)((acc[0] ? kFileCorrupt : 0u) | (holes ? kFileHole : 0u) | (written ? 0u : kFileUnwritten));
}

__global__ __launch_bounds__(256) void k_files_summary(uint64_t n_files, const uint64_t* __restrict__ status,
                                                      const uint64_t* __restrict__ reports,
                                                      const uint8_t* __restrict__ flags, uint64_t cap,
                                                      uint64_t* __restrict__ list, uint64_t* __restrict__ summary) {
    __shared__ uint64_t w4[4];
    __shared__ unsigned long long tot[8];  // pages, ok, corrupt, blank, corrupt files, hole files, unwritten files, first bad file
    const uint64_t invalid = status[0];
    if (invalid != ~0ull) {  // uniform: only n_files and the invalid file are reported
        if (threadIdx.x < kFilesSummaryWords) summary[threadIdx.x] = threadIdx.x == 0 ? n_files : threadIdx.x == 11 ? invalid : 0;
        return;
    }
    if (threadIdx.x < 8) tot[threadIdx.x] = threadIdx.x == 7 ? ~0ull : 0ull;
    __syncthreads();
    uint64_t n_bad = 0;    // bad files before this round (uniform)
    uint64_t acc[7] = {};  // this thread's files
    uint64_t first_bad = ~0ull;
    for (uint64_t base = 0; base < n_files; base += 256 * kFilesPerThread) {
        const uint64_t f0 = base + (uint64_t)threadIdx.x * kFilesPerThread;  // this thread's consecutive files
        uint32_t bad = 0;  // bit k: file f0 + k is bad
#pragma unroll
        for (int k = 0; k < kFilesPerThread; ++k) {
            const uint64_t f = f0 + k;
            if (f < n_files) {
                const uint64_t* q = reports + f * kFileReportWords;
                const uint32_t fl = flags[f];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += q[1 + j];  // n_pages, n_ok, n_corrupt, n_blank
                acc[4] += fl & kFileCorrupt ? 1 : 0;
                acc[5] += fl & kFileHole ? 1 : 0;
                acc[6] += fl & kFileUnwritten ? 1 : 0;
                if (fl & (kFileCorrupt | kFileHole)) {
                    bad |= 1u << k;
                    if (first_bad == ~0ull) first_bad = f;
                }
            }
        }
        uint64_t total;
        uint64_t pos = n_bad + block_excl_scan(__builtin_popcount(bad), w4, total);
        while (bad && pos < cap) {
            list[pos++] = f0 + __builtin_ctz(bad);
            bad &= bad - 1;
        }
        n_bad += total;
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const uint64_t v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&tot[k], (unsigned long long)v);
    }
    if (first_bad != ~0ull) atomicMin(&tot[7], (unsigned long long)first_bad);
    __syncthreads();
    if (threadIdx.x < kFilesSummaryWords) {
        uint64_t v;
        switch (threadIdx.x) {
            case 0: v = n_files; break;
            case 7: v = n_bad; break;
            case 8: v = tot[6]; break;
            case 9: v = tot[7]; break;
            case 10: v = n_bad < cap ? n_bad : cap; break;
            case 11: v = ~0ull; break;
            default: v = tot[threadIdx.x - 1]; break;  // 1..6: pages, ok, corrupt, blank, corrupt files, hole files
        }
        summary[threadIdx.x] = v;
    }
}

// Per-file reports of the class and type bytes cls / type[0 .. n) cut at the
// device-resident boundaries first[0 .. n_files].  Nothing here waits for the
// stream; the whole summary is written whatever n and n_files are.
hipError_t run_files(const uint8_t* cls, const uint8_t* type, uint64_t n, const uint64_t* first, uint64_t n_files,
                     uint64_t* reports, uint64_t* summary, uint64_t* list, uint64_t cap, hipStream_t s) {
    // the most items valid boundaries can give: sum of ceil(len / span) <= sum of len / span + n_files
    const uint64_t max_items = n / kScrubSpan + n_files;
    if (n_files > 0x7FFFFFFFull || max_items > 0x7FFFFFFFull) return hipErrorInvalidValue;
    ScratchLease scratch(s);  // status, items before each file, records, flags
    const size_t before_bytes = ((n_files + 1) * 8 + 15) & ~size_t(15);
    const size_t rec_bytes = (max_items * kFileRec * 4 + 15) & ~size_t(15);
    hipError_t e = scratch.get(16 + before_bytes + rec_bytes + n_files);
    if (e != hipSuccess) return e;
    uint64_t* status = static_cast<uint64_t*>(scratch.p);
    uint64_t* items_before = status + 2;
    uint32_t* rec = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(items_before) + before_bytes);
    uint8_t* flags = reinterpret_cast<uint8_t*>(rec) + rec_bytes;
    hipLaunchKernelGGL(k_files_plan, dim3(1), dim3(256), 0, s, first, n_files, n, items_before, status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (max_items) {
        hipLaunchKernelGGL(k_files_count, dim3((unsigned)max_items), dim3(256), 0, s, cls, type, first, n_files,
                           items_before, status, rec);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (n_files) {
        hipLaunchKernelGGL(k_files_reduce, dim3((unsigned)((n_files + 3) / 4)), dim3(256), 0, s, first, n_files,
                           items_before, status, rec, reports, flags);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_files_summary, dim3(1), dim3(256), 0, s, n_files, status, reports, flags, cap, list, summary);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Manifest scan (pcs_manifest_scan_dev): walk and verify every record of many
// manifest images (Replayer::ParseNextRecord, src/replayer.cpp:74-140).  Image
// i is [base + off[i], + size[i]); a record is checksum(8) | root(4) |
// ttl_root(4) | payload_len(4) | payload, padded to `align`.  Offsets and sizes
// are a device array, so nothing here may trust them.  Nine launches ordered by
// construction (the one atomic on global memory adds up a count, so the output
// is the same on every call):
//   k_mscan_layout  one block: checks every image against the layout rules and
//                   scans the images' slot counts ceil(size / align) into
//                   slot_base.  The first invalid image goes into ctl[0];
//                   every later kernel leaves at once when it is set, so no
//                   address is ever formed from an unchecked offset;
//   k_mscan_slots   one lane per align-slot of every image, each a candidate
//                   record start: the header bounds test and one aligned 4-byte
//                   load of payload_len, the only image bytes the walk needs,
//                   all independent.  Writes the slot's word (the next slot, or
//                   an end code) and its payload_len;
//   k_mscan_walk    one wave per image: tiles of the slot words and lengths
//                   pass through LDS and the chain is followed there, never
//                   through the image, 64 slots at a time: runs of one-slot
//                   records in one scalar step, any other record by a
//                   readlane; a record whose next slot lies tiles ahead moves
//                   the tile window straight to it.  The records met in a tile
//                   are noted in LDS in walk order; the wave then takes their
//                   chunk counts ceil((12 + len) / 1 MiB) and scans them, so
//                   every record gets its ordinal and its image-local first
//                   chunk;
//   k_mscan_plan    one block: exclusive sums of the images' record and chunk
//                   counts (first_record, first_chunk);
//   k_mscan_emit    one lane per record: (offset, length) of each of its chunks,
//                   offsets in the page convention (content 8 bytes on), and
//                   the number of chunks of kLongMin bytes and more;
//   k_mscan_hash    one 16-lane group per chunk shorter than kLongMin: the
//                   any-size group body from 241 content bytes up, xxh3_short
//                   on the group's first lane below;
//   k_mscan_long    a workgroup per chunk of kLongMin bytes and more, the 1 MiB
//                   chunks of snapshots (k_xxh3_long's body); leaves at once
//                   when the batch has none;
//   k_mscan_report  one block per image, a lane per record: folds the chunk
//                   digests, compares, writes the record entry below the cap
//                   and reduces the image's report;
//   k_mscan_summary one block: totals, verdict census, first bad image.
// ---------------------------------------------------------------------------
constexpr int kMscanReportWords = 12;   // pcs_manifest_report
constexpr int kMscanSummaryWords = 12;  // pcs_manifest_summary
constexpr int kMscanRecordWords = 5;    // pcs_manifest_record: offset, stored, computed, len | root, ttl_root | ok
constexpr uint64_t kMscanHeader = 20;   // checksum(8) root(4) ttl_root(4) payload_len(4)
// slot words above every slot index: why the chain ends at this slot
constexpr uint32_t kSlotShortHeader = 0xFFFFFFF1u;   // fewer than 20 bytes left: no record
constexpr uint32_t kSlotShortPayload = 0xFFFFFFF2u;  // the payload runs past the image: no record
constexpr uint32_t kSlotLastPadding = 0xFFFFFFF3u;   // a record, its padding cut by the end of the image
constexpr uint32_t kSlotLastClean = 0xFFFFFFF0u;     // a record that ends the image exactly
constexpr int kMscanCtlWords = 8;  // ctl: invalid image, slots, records, chunks, long chunks
constexpr int kMscanMaxTile = 4096;

// the image that holds global slot (or record position) j: the last i with slot_base[i] <= j
__device__ __forceinline__ uint64_t mscan_image_of(const uint64_t* __restrict__ slot_base, uint64_t n_images, uint64_t j) {
    uint64_t lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (slot_base[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_mscan_layout(const uint64_t* __restrict__ off, const uint64_t* __restrict__ size,
                                                     uint64_t n_images, uint64_t total, uint32_t shift,
                                                     uint64_t* __restrict__ slot_base, uint64_t* __restrict__ ctl) {
    __shared__ uint64_t w4[4];
    __shared__ unsigned long long bad;
    if (threadIdx.x == 0) bad = ~0ull;
    __syncthreads();
    const uint64_t mask = (1ull << shift) - 1;
    uint64_t slots = 0;  // slots of the images before this round (uniform)
    for (uint64_t base = 0; base < n_images; base += 256) {
        const uint64_t i = base + threadIdx.x;
        uint64_t c = 0;
        if (i < n_images) {
            const uint64_t o = off[i], sz = size[i];
            bool ok = (o & mask) == 0 && o <= total && sz <= total - o;
            if (ok && i > 0) {
                const uint64_t po = off[i - 1], ps = size[i - 1];
                // the predecessor's own check makes po + ps <= total when it is valid; when it
                // is not, the whole layout is invalid whatever this comparison gives
                ok = po <= total && ps <= total - po && o >= ((po + ps + mask) & ~mask);
            }
            if (!ok) atomicMin(&bad, (unsigned long long)i);
            else c = (sz + mask) >> shift;
        }
        uint64_t t;
        const uint64_t before = slots + block_excl_scan(c, w4, t);
        if (i < n_images) slot_base[i] = before;
        slots += t;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        slot_base[n_images] = slots;
        ctl[0] = bad;
        ctl[1] = bad == ~0ull ? slots : 0;
        ctl[2] = 0;
        ctl[3] = 0;
        ctl[4] = 0;  // k_mscan_emit counts the long chunks here
    }
}

__global__ __launch_bounds__(256) void k_mscan_slots(const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
                                                    const uint64_t* __restrict__ size, uint64_t n_images,
                                                    uint32_t shift, const uint64_t* __restrict__ slot_base,
                                                    const uint64_t* __restrict__ ctl, uint32_t* __restrict__ slot_next,
                                                    uint32_t* __restrict__ slot_len) {
    if (ctl[0] != ~0ull) return;
    const uint64_t n_slots = ctl[1];
    const uint64_t mask = (1ull << shift) - 1;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_slots; j += stride) {
        const uint64_t i = mscan_image_of(slot_base, n_images, j);
        const uint64_t o = (j - slot_base[i]) << shift, sz = size[i];
        const uint64_t left = sz - o;  // >= 1: slot s exists only for s * align < size
        uint32_t next = kSlotShortHeader, len = 0;
        if (left >= kMscanHeader) {
            // base is 8-byte aligned, off[i] and o multiples of align >= 64: an aligned word
            len = *reinterpret_cast<const uint32_t*>(base + off[i] + o + 16);
            const uint64_t need = kMscanHeader + (uint64_t)len;
            if (need > left) {
                next = kSlotShortPayload;
            } else {
                const uint64_t o2 = (o + need + mask) & ~mask;
                next = o2 > sz ? kSlotLastPadding : o2 == sz ? kSlotLastClean : (uint32_t)(o2 >> shift);
            }
        }
        slot_next[j] = next;
        slot_len[j] = len;
    }
}

__device__ __forceinline__ uint64_t wave_excl_scan(uint64_t v, uint64_t& total) {
    const int lane = threadIdx.x & 63;
    uint64_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)incl, d, 64);
        if (lane >= d) incl += t;
    }
    total = __shfl((unsigned long long)incl, 63, 64);
    return incl - v;
}

// img: 4 words per image: records, chunks, end offset, end reason
__global__ __launch_bounds__(64) void k_mscan_walk(const uint64_t* __restrict__ size, uint64_t n_images, uint32_t shift,
                                                  uint32_t tile, const uint64_t* __restrict__ slot_base,
                                                  const uint64_t* __restrict__ ctl,
                                                  const uint32_t* __restrict__ slot_next,
                                                  const uint32_t* __restrict__ slot_len, uint32_t* __restrict__ rec_slot,
                                                  uint32_t* __restrict__ rec_chunk, uint64_t* __restrict__ img) {
    extern __shared__ uint32_t mscan_lds[];  // the tile's slot words and lengths, then its records' slots in walk order
    if (ctl[0] != ~0ull) return;
    uint32_t* t_next = mscan_lds;
    uint32_t* t_len = mscan_lds + tile;
    uint32_t* t_rec = mscan_lds + 2 * tile;
    const uint64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    const uint64_t sb = slot_base[i];
    const uint32_t ns = (uint32_t)(slot_base[i + 1] - sb);
    const uint64_t sz = size[i];
    uint32_t cur = 0;  // the slot the chain stands on (uniform)
    uint64_t n_rec = 0, n_chunks = 0, end_off = 0, reason = 0;  // size 0: END_CLEAN at 0
    bool done = ns == 0;
    while (!done) {
        const uint32_t t0 = cur & ~(tile - 1);  // the tile that holds cur, however far the last record reached
        const uint32_t cnt = min(tile, ns - t0);
        for (uint32_t k0 = 0; k0 < cnt; k0 += 64 * 8) {  // eight loads of each array in flight per lane
            uint32_t a[8], b[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t k = k0 + 64 * j + lane;
                a[j] = k < cnt ? slot_next[sb + t0 + k] : 0;
                b[j] = k < cnt ? slot_len[sb + t0 + k] : 0;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t k = k0 + 64 * j + lane;
                if (k < cnt) {
                    t_next[k] = a[j];
                    t_len[k] = b[j];
                }
            }
        }
        __syncthreads();
        // The chain is followed 64 slots at a time: each lane takes one slot word of
        // the window from LDS and the walk inside the window is scalar.  `seq` marks
        // the lanes whose record ends inside its own slot (next == slot + 1): a run
        // of them is taken in one step, any other record with one readlane.  (A walk
        // that read LDS once per record took 130 ns a step, 270 of the 332 us of an
        // 8 MiB image of one-slot records)  A slot word is an
        // end code, all of which lie above every slot index, or a slot index above
        // cur and below ns.  The window's records are the set bits of `hit`,
        // ascending as the chain is.
        uint32_t m = 0;
        while (!done && cur < t0 + cnt) {
            const uint32_t w0 = cur & ~63u;  // tiles are multiples of 64 slots
            const uint32_t k = w0 - t0 + lane;
            const uint32_t mine = k < cnt ? t_next[k] : kSlotShortHeader;
            const uint64_t seq = __ballot(mine == w0 + lane + 1);
            const uint32_t wend = min(w0 + 64, t0 + cnt);
            uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur);
            uint64_t hit = 0;
            while (c < wend) {
                const uint32_t p = c - w0;
                const uint64_t stop = ~(seq >> p);  // the shift leaves zeros above bit 63 - p: they stop a run
                const uint32_t run = stop ? (uint32_t)__builtin_ctzll(stop) : 64u;
                if (run) {
                    hit |= (run == 64 ? ~0ull : (1ull << run) - 1) << p;
                    c += run;
                    continue;
                }
                const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)p);
                if (w == kSlotShortHeader || w == kSlotShortPayload) {
                    done = true;
                    end_off = (uint64_t)c << shift;
                    reason = w == kSlotShortHeader ? 1 : 2;
                    break;
                }
                hit |= 1ull << p;
                if (w == kSlotLastClean || w == kSlotLastPadding) {
                    done = true;
                    end_off = sz;
                    reason = w == kSlotLastClean ? 0 : 3;
                    break;
                }
                c = w;
            }
            cur = c;
            if ((hit >> lane) & 1) t_rec[m + __builtin_popcountll(hit & ((1ull << lane) - 1))] = w0 + lane;
            m += (uint32_t)__builtin_popcountll(hit);
        }
        __syncthreads();
        for (uint32_t q0 = 0; q0 < m; q0 += 64) {  // the tile's records, 64 at a time in walk order
            const uint32_t q = q0 + lane;
            uint32_t slot = 0;
            uint64_t nc = 0;
            if (q < m) {
                slot = t_rec[q];
                nc = (12ull + t_len[slot - t0] + (kManifestChunk - 1)) >> 20;
            }
            uint64_t t;
            const uint64_t before = wave_excl_scan(nc, t);
            if (q < m) {
                rec_slot[sb + n_rec + q] = slot;
                rec_chunk[sb + n_rec + q] = (uint32_t)(n_chunks + before);
            }
            n_chunks += t;
        }
        n_rec += m;
        __syncthreads();  // the tile arrays are refilled by the next tile
    }
    if (lane == 0) {
        img[4 * i + 0] = n_rec;
        img[4 * i + 1] = n_chunks;
        img[4 * i + 2] = end_off;
        img[4 * i + 3] = reason;
    }
}

__global__ __launch_bounds__(256) void k_mscan_plan(uint64_t n_images, const uint64_t* __restrict__ img,
                                                   uint64_t* __restrict__ first_rec, uint64_t* __restrict__ first_chunk,
                                                   uint64_t* __restrict__ ctl) {
    __shared__ uint64_t w4[4];
    if (ctl[0] != ~0ull) return;
    uint64_t recs = 0, chunks = 0;  // of the images before this round (uniform)
    for (uint64_t base = 0; base < n_images; base += 256) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t r = i < n_images ? img[4 * i] : 0, c = i < n_images ? img[4 * i + 1] : 0;
        uint64_t tr, tc;
        const uint64_t br = recs + block_excl_scan(r, w4, tr);
        __syncthreads();
        const uint64_t bc = chunks + block_excl_scan(c, w4, tc);
        if (i < n_images) {
            first_rec[i] = br;
            first_chunk[i] = bc;
        }
        recs += tr;
        chunks += tc;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ctl[2] = recs;
        ctl[3] = chunks;
    }
}

__global__ __launch_bounds__(256) void k_mscan_emit(const uint64_t* __restrict__ off, uint64_t n_images, uint32_t shift,
                                                   const uint64_t* __restrict__ slot_base,
                                                   const uint64_t* __restrict__ ctl, const uint64_t* __restrict__ img,
                                                   const uint64_t* __restrict__ first_chunk,
                                                   const uint32_t* __restrict__ slot_len,
                                                   const uint32_t* __restrict__ rec_slot,
                                                   const uint32_t* __restrict__ rec_chunk,
                                                   uint64_t* __restrict__ chunk_off, uint32_t* __restrict__ chunk_len,
                                                   unsigned long long* __restrict__ n_long) {
    if (ctl[0] != ~0ull) return;
    const uint64_t n_slots = ctl[1];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t longs = 0;  // this lane's chunks of kLongMin bytes and more
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_slots; j += stride) {
        const uint64_t i = mscan_image_of(slot_base, n_images, j);
        const uint64_t sb = slot_base[i];
        if (j - sb >= img[4 * i]) continue;  // positions past the image's records
        const uint32_t slot = rec_slot[j];
        const uint64_t content = 12ull + slot_len[sb + slot];
        const uint64_t rec = off[i] + ((uint64_t)slot << shift);
        uint64_t c = first_chunk[i] + rec_chunk[j];
        for (uint64_t done = 0; done < content; done += kManifestChunk, ++c) {
            const uint32_t len = (uint32_t)min((uint64_t)kManifestChunk, content - done);
            chunk_off[c] = rec + done;  // page convention: the chunk's content starts 8 bytes on
            chunk_len[c] = len;
            longs += len >= kLongMin ? 1 : 0;
        }
    }
    // a count, the same whatever the order of the additions: k_mscan_long leaves at once when it is 0
    longs = wave_sum(longs);
    if ((threadIdx.x & 63) == 0 && longs) atomicAdd(n_long, (unsigned long long)longs);
}

__global__ __launch_bounds__(256) void k_mscan_hash(const uint8_t* __restrict__ base, const uint64_t* __restrict__ ctl,
                                                   const uint64_t* __restrict__ chunk_off,
                                                   const uint32_t* __restrict__ chunk_len,
                                                   uint64_t* __restrict__ chunk_h) {
    if (ctl[0] != ~0ull) return;
    const uint64_t n_chunks = ctl[3];
    const Xxh3Lane L = make_xxh3_lane(threadIdx.x & 15);
    const uint64_t ntiles = (n_chunks + 15) / 16;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t c = t * 16 + (threadIdx.x >> 4);
        if (c >= n_chunks) continue;
        const uint64_t o = chunk_off[c];
        const uint32_t len = chunk_len[c];
        if (len >= kLongMin) continue;  // k_mscan_long's
        const uint8_t* page = base + o;
        if (xxh3_group_ok(len + 8)) {
            uint64_t stored;
            const uint64_t h = xxh3_page_any<false>(page, len + 8, L, stored);
            if (L.g == 0) chunk_h[c] = h;
        } else if (L.g == 0) {
            chunk_h[c] = xxh3_short(page + 8, len);
        }
    }
}

// The chunks of kLongMin bytes and more, a workgroup each (k_xxh3_long's body):
// the 1 MiB chunks of snapshots and their long tails.  The content starts at
// 8 mod 16, so the range is 8-byte aligned as that body needs.
__global__ __launch_bounds__(256) void k_mscan_long(const uint8_t* __restrict__ base, const uint64_t* __restrict__ ctl,
                                                   const uint64_t* __restrict__ chunk_off,
                                                   const uint32_t* __restrict__ chunk_len,
                                                   uint64_t* __restrict__ chunk_h) {
    __shared__ uint64_t S[kLongWin][8];
    if (ctl[0] != ~0ull || ctl[4] == 0) return;
    const uint64_t n_chunks = ctl[3];
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t len = chunk_len[c];
        if (len < kLongMin) continue;  // uniform over the workgroup
        xxh3_long_range(S, base + chunk_off[c] + 8, len, chunk_h + c);
    }
}

__global__ __launch_bounds__(256) void k_mscan_report(const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
                                                     const uint64_t* __restrict__ size, uint32_t shift,
                                                     const uint64_t* __restrict__ slot_base,
                                                     const uint64_t* __restrict__ ctl, const uint64_t* __restrict__ img,
                                                     const uint64_t* __restrict__ first_rec,
                                                     const uint64_t* __restrict__ first_chunk,
                                                     const uint32_t* __restrict__ slot_len,
                                                     const uint32_t* __restrict__ rec_slot,
                                                     const uint32_t* __restrict__ rec_chunk,
                                                     const uint64_t* __restrict__ chunk_h, uint64_t cap,
                                                     uint64_t* __restrict__ records, uint64_t* __restrict__ reports) {
    __shared__ unsigned long long red[3];  // ok records, first corrupt record, largest record
    if (ctl[0] != ~0ull) return;
    const uint64_t i = blockIdx.x;
    if (threadIdx.x < 3) red[threadIdx.x] = threadIdx.x == 1 ? ~0ull : 0ull;
    __syncthreads();
    const uint64_t sb = slot_base[i], n_rec = img[4 * i], r0 = first_rec[i], c0 = first_chunk[i];
    const uint8_t* image = base + off[i];
    uint64_t n_ok = 0, first_bad = ~0ull, largest = 0;
    for (uint64_t k = threadIdx.x; k < n_rec; k += 256) {
        const uint32_t slot = rec_slot[sb + k];
        const uint32_t len = slot_len[sb + slot];
        const uint64_t o = (uint64_t)slot << shift;
        const uint64_t content = 12ull + len;
        const uint64_t* h = chunk_h + c0 + rec_chunk[sb + k];
        uint64_t agg = 0;
        for (uint64_t done = 0; done < content; done += kManifestChunk, ++h)
            agg = (((agg << 1) | (agg >> 63)) ^ *h) * 0x9e3779b97f4a7c15ull;
        const uint64_t* head = reinterpret_cast<const uint64_t*>(image + o);  // 8-byte aligned
        const uint64_t stored = head[0], roots = head[1];
        const bool ok = stored == agg;
        if (ok) ++n_ok;
        else if (first_bad == ~0ull) first_bad = k;  // a lane's records ascend
        largest = max(largest, kMscanHeader + len);
        if (r0 + k < cap) {
            uint64_t* e = records + (r0 + k) * kMscanRecordWords;
            e[0] = o;
            e[1] = stored;
            e[2] = agg;
            e[3] = (uint64_t)len | (roots << 32);
            e[4] = (roots >> 32) | ((uint64_t)(ok ? 1 : 0) << 32);
        }
    }
    n_ok = wave_sum(n_ok);
    first_bad = wave_min(first_bad);
    largest = wave_max(largest);
    if ((threadIdx.x & 63) == 0) {
        if (n_ok) atomicAdd(&red[0], (unsigned long long)n_ok);
        atomicMin(&red[1], (unsigned long long)first_bad);
        atomicMax(&red[2], (unsigned long long)largest);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t ok = red[0], fc = red[1];
        const uint64_t after = fc == ~0ull ? 0 : ok - fc;  // every record before the first corrupt one is ok
        const uint64_t end_off = img[4 * i + 2];
        uint64_t* r = reports + i * kMscanReportWords;
        r[0] = size[i];
        r[1] = n_rec;
        r[2] = ok;
        r[3] = n_rec - ok;
        r[4] = fc;
        r[5] = after;
        r[6] = fc == ~0ull ? end_off : (uint64_t)rec_slot[sb + fc] << shift;
        r[7] = end_off;
        r[8] = img[4 * i + 3];
        r[9] = n_rec == 0 ? 4 : fc == 0 ? 3 : fc == ~0ull ? 0 : after ? 2 : 1;
        r[10] = r0;
        r[11] = red[2];
    }
}

__global__ __launch_bounds__(256) void k_mscan_summary(uint64_t n_images, const uint64_t* __restrict__ ctl,
                                                      const uint64_t* __restrict__ reports, uint64_t cap,
                                                      uint64_t* __restrict__ summary) {
    __shared__ unsigned long long tot[9];  // records, ok, corrupt, images by verdict 0..4, first bad image
    const uint64_t invalid = ctl[0];
    if (invalid != ~0ull) {  // uniform: only n_images and the invalid image are reported
        if (threadIdx.x < kMscanSummaryWords) summary[threadIdx.x] = threadIdx.x == 0 ? n_images : threadIdx.x == 11 ? invalid : 0;
        return;
    }
    if (threadIdx.x < 9) tot[threadIdx.x] = threadIdx.x == 8 ? ~0ull : 0ull;
    __syncthreads();
    uint64_t acc[8] = {};
    uint64_t first_bad = ~0ull;
    for (uint64_t i = threadIdx.x; i < n_images; i += 256) {
        const uint64_t* r = reports + i * kMscanReportWords;
        acc[0] += r[1];
        acc[1] += r[2];
        acc[2] += r[3];
        const uint64_t v = r[9];
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[3 + k] += v == (uint64_t)k ? 1 : 0;
        if (v != 0 && first_bad == ~0ull) first_bad = i;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint64_t v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&tot[k], (unsigned long long)v);
    }
    if (first_bad != ~0ull) atomicMin(&tot[8], (unsigned long long)first_bad);
    __syncthreads();
    if (threadIdx.x < kMscanSummaryWords) {
        uint64_t v;
        switch (threadIdx.x) {
            case 0: v = n_images; break;
            case 10: v = tot[0] < cap ? tot[0] : cap; break;
            case 11: v = ~0ull; break;
            default: v = tot[threadIdx.x - 1]; break;  // 1..9: records, ok, corrupt, verdicts, first bad image
        }
        summary[threadIdx.x] = v;
    }
}

// Slots per LDS tile of k_mscan_walk (PCS_TUNE_MANIFEST_WALK_TILE): a power of
// two in [64, kMscanMaxTile]; anything else runs at the default.
constexpr uint32_t kMscanDefaultTile = 2048;
uint32_t mscan_tile() {
    const int64_t t = g_tune[38].load(std::memory_order_relaxed);
    if (t < 64 || t > kMscanMaxTile || (t & (t - 1)) != 0) return kMscanDefaultTile;
    return (uint32_t)t;
}

hipError_t run_manifest_scan(const uint8_t* base, uint64_t total, const uint64_t* off, const uint64_t* size,
                             uint64_t n_images, uint32_t align, uint64_t* reports, uint64_t* summary,
                             uint64_t* records, uint64_t cap, hipStream_t s) {
    uint32_t shift = 0;
    while ((1u << shift) < align) ++shift;
    // the most slots and chunks a valid layout can give
    const uint64_t max_slots = (total >> shift) + n_images;
    const uint64_t max_chunks = max_slots + (total >> 20);
    if (n_images > 0x7FFFFFFFull || max_chunks > 0x7FFFFFF0ull) return hipErrorInvalidValue;
    ScratchLease scratch(s);
    // u64: ctl, slot_base[n + 1], img[4 n], first_rec[n], first_chunk[n], chunk_off, chunk_h[max_chunks];
    // u32: slot_next, slot_len, rec_slot, rec_chunk[max_slots], chunk_len[max_chunks]
    const size_t words = kMscanCtlWords + (n_images + 1) + 6 * n_images + 2 * max_chunks;
    hipError_t e = scratch.get(words * 8 + (4 * max_slots + max_chunks) * 4);
    if (e != hipSuccess) return e;
    uint64_t* ctl = static_cast<uint64_t*>(scratch.p);
    uint64_t* slot_base = ctl + kMscanCtlWords;
    uint64_t* img = slot_base + n_images + 1;
    uint64_t* first_rec = img + 4 * n_images;
    uint64_t* first_chunk = first_rec + n_images;
    uint64_t* chunk_off = first_chunk + n_images;
    uint64_t* chunk_h = chunk_off + max_chunks;
    uint32_t* slot_next = reinterpret_cast<uint32_t*>(chunk_h + max_chunks);
    uint32_t* slot_len = slot_next + max_slots;
    uint32_t* rec_slot = slot_len + max_slots;
    uint32_t* rec_chunk = rec_slot + max_slots;
    uint32_t* chunk_len = rec_chunk + max_slots;
    hipLaunchKernelGGL(k_mscan_layout, dim3(1), dim3(256), 0, s, off, size, n_images, total, shift, slot_base, ctl);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (n_images) {
        const uint32_t tile = mscan_tile();
        hipLaunchKernelGGL(k_mscan_slots, dim3(grid_for(max_slots, kBlock, kBlocksPerCu)), dim3(kBlock), 0, s, base, off,
                           size, n_images, shift, slot_base, ctl, slot_next, slot_len);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_mscan_walk, dim3((unsigned)n_images), dim3(64), 3 * tile * sizeof(uint32_t), s, size,
                           n_images, shift, tile, slot_base, ctl, slot_next, slot_len, rec_slot, rec_chunk, img);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_mscan_plan, dim3(1), dim3(256), 0, s, n_images, img, first_rec, first_chunk, ctl);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_mscan_emit, dim3(grid_for(max_chunks, kBlock, kBlocksPerCu)), dim3(kBlock), 0, s, off,
                           n_images, shift, slot_base, ctl, img, first_chunk, slot_len, rec_slot, rec_chunk, chunk_off,
                           chunk_len, reinterpret_cast<unsigned long long*>(ctl + 4));
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_mscan_hash, dim3(grid_for(max_chunks, 16, 32)), dim3(kBlock), 0, s, base, ctl, chunk_off,
                           chunk_len, chunk_h);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_mscan_long, dim3(grid_for(max_chunks, 1, 8)), dim3(kBlock), 0, s, base, ctl, chunk_off,
                           chunk_len, chunk_h);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_mscan_report, dim3((unsigned)n_images), dim3(256), 0, s, base, off, size, shift, slot_base,
                           ctl, img, first_rec, first_chunk, slot_len, rec_slot, rec_chunk, chunk_h, cap, records,
                           reports);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_mscan_summary, dim3(1), dim3(256), 0, s, n_images, ctl, reports, cap, summary);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Manifest replay (pcs_manifest_replay_dev): what Replayer::Replay computes,
// for every image of a batch.  The scan above runs first with a record array
// in scratch, so every record's offset, length and ok flag are on the device.
// A record's payload is a prelude (snapshot: varint64 max_fp_id, varint32
// dict_len and the dict bytes) followed by LE32 mapping_len, the mapping
// section, LE32 term_len and the term section; sections are runs of varints.
// The decode is byte-parallel: a varint ends at every byte below 0x80, so the
// ordinal of a varint in its section is the number of such bytes before it,
// which a count per tile and two exclusive sums give.  Launches, ordered by
// construction; the only atomics on global memory are max, min and integer
// add, so the output is the same on every call:
//   k_replay_sections  one block per image, a lane per replayed record: the
//                      prelude with a bounds test before every read, up to two
//                      sections (byte offset, length) per record;
//   k_replay_plan      one block: exclusive sum of the sections' tile counts;
//   k_replay_count     one wave per tile: 16 bytes per lane, terminators by
//                      mask and popcount, one count per tile;
//   k_replay_scan      one block: exclusive sum of the tile counts, so every
//                      tile knows the ordinal of its first varint and every
//                      section its varint count;
//   k_replay_decode<1> one wave per tile: each terminator lane looks back at
//                      most 10 bytes, never before its section's start, flags
//                      over-long runs, folds 1 + the largest logged page id
//                      and max_fp_id; the first tile of a section checks its
//                      last byte and the parity of its count;
//   k_replay_images    one block: status, table_size and its exclusive sum;
//   k_replay_fill      rows to be written become 7, their sequence words 0;
//   k_replay_decode<2> snapshot values go to their rows; a log entry does
//                      atomicMax(seq[row], s), s = the global ordinal of its
//                      value varint, which ascends in record, then byte order;
//   k_replay_decode<3> the log entry whose s won stores its value;
//   k_replay_stats     one lane per written row: mapped rows, smallest and
//                      largest file page, file pages at or above max_fp_id;
//   k_replay_report    one block: the reports and the summary.
// ---------------------------------------------------------------------------
constexpr int kReplayReportWords = 16;   // pcs_replay_report
constexpr int kReplaySummaryWords = 12;  // pcs_replay_summary
constexpr int kReplayCtlWords = 8;       // ctl: invalid image, records, tiles, rows, rows written
constexpr uint64_t kReplayInvalidValue = 7;  // MappingSnapshot::InvalidValue
constexpr uint32_t kReplayDefaultTile = 4096;  // profiles/replay/replay_rate.txt
constexpr uint64_t kReplayOk = 0, kReplayNotReplayable = 1, kReplayMalformed = 2, kReplayTableCap = 3;

// per-image words (u64), kReplayImgWords each
constexpr int kRiBad = 0;     // lowest record with a violation, ~0 when none (atomicMin)
constexpr int kRiMaxPid = 1;  // 1 + largest page id of a replayed log entry (atomicMax)
constexpr int kRiMaxFp = 2;   // max_fp_id (the snapshot's, then atomicMax)
constexpr int kRiDict = 3;    // dict_len
constexpr int kRiSnap = 4;    // varints in the snapshot's mapping section
constexpr int kRiLog = 5;     // log entries (atomicAdd)
constexpr int kRiTerm = 6;    // term pairs (atomicAdd)
constexpr int kRiNrep = 7;    // records replayed
constexpr int kRiStatus = 8;
constexpr int kRiSize = 9;    // table_size
constexpr int kRiFirst = 10;  // table_first
constexpr int kRiMapped = 11, kRiMinFp = 12, kRiMaxMapped = 13, kRiBeyond = 14;  // k_replay_stats
constexpr int kReplayImgWords = 16;

uint32_t replay_tile() {
    const int64_t t = g_tune[39].load(std::memory_order_relaxed);
    if (t < 64 || t > 4096 || (t & (t - 1)) != 0) return kReplayDefaultTile;
    return (uint32_t)t;
}

// A varint of at most `limit` bytes at p[pos ..), inside [0, L): false when it
// does not end within its limit or within L.
__device__ __forceinline__ bool replay_varint(const uint8_t* p, uint64_t L, uint64_t& pos, int limit, uint64_t& v) {
    v = 0;
    for (int n = 0;; ++n) {
        if (pos >= L || n == limit) return false;
        const uint8_t b = p[pos++];
        v |= (uint64_t)(b & 0x7F) << (7 * n);  // n = 9: only bit 0 stays, the rest wraps away
        if (b < 0x80) return true;
    }
}
__device__ __forceinline__ uint32_t replay_le32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// sec_off / sec_len: two sections per record g (2g mapping, 2g + 1 term)
__global__ __launch_bounds__(256) void k_replay_sections(const uint8_t* __restrict__ base, const uint64_t* __restrict__ off,
                                                        uint64_t n_images, const uint64_t* __restrict__ scan_sum,
                                                        const uint64_t* __restrict__ scan_rep,
                                                        const uint64_t* __restrict__ recs, uint64_t* __restrict__ ctl,
                                                        uint64_t* __restrict__ img, uint32_t* __restrict__ rec_img,
                                                        uint32_t* __restrict__ rec_k, uint32_t* __restrict__ sec_off,
                                                        uint32_t* __restrict__ sec_len) {
    const uint64_t invalid = scan_sum[11];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl[0] = invalid;
        ctl[1] = invalid == ~0ull ? scan_sum[1] : 0;
        ctl[2] = ctl[3] = ctl[4] = 0;
    }
    if (invalid != ~0ull || blockIdx.x >= n_images) return;  // uniform over the block
    const uint64_t i = blockIdx.x;
    const uint64_t* rep = scan_rep + i * kMscanReportWords;
    const uint64_t n_rec = rep[1], fc = rep[4], verdict = rep[9], r0 = rep[10];
    const uint64_t n_rep = verdict <= 1 ? (fc == ~0ull ? n_rec : fc) : 0;  // CLEAN or TORN_TAIL
    uint64_t* im = img + i * kReplayImgWords;
    if (threadIdx.x < kReplayImgWords)
        im[threadIdx.x] = threadIdx.x == kRiBad ? ~0ull : threadIdx.x == kRiNrep ? n_rep : threadIdx.x == kRiMinFp ? ~0ull : 0;
    __syncthreads();
    for (uint64_t k = threadIdx.x; k < n_rec; k += 256) {
        const uint64_t g = r0 + k;
        uint32_t mo = 0, ml = 0, to = 0, tl = 0;
        if (k < n_rep) {
            const uint64_t* e = recs + g * kMscanRecordWords;
            const uint64_t pay = off[i] + e[0] + kMscanHeader;  // the scan found the record inside its image
            const uint64_t L = e[3] & 0xFFFFFFFFull;
            const uint8_t* p = base + pay;
            uint64_t pos = 0, maxfp = 0, dict = 0;
            bool ok = true;
            if (k == 0) {
                ok = replay_varint(p, L, pos, 10, maxfp);
                ok = ok && replay_varint(p, L, pos, 5, dict);
                dict &= 0xFFFFFFFFull;
                ok = ok && dict <= L - pos;
                if (ok) pos += dict;
            }
            const uint64_t rem = ok ? L - pos : 0;
            ok = ok && rem >= 8;
            if (ok) {
                const uint64_t mlen = replay_le32(p + pos);
                if (mlen + 8 > rem) {
                    ok = false;
                } else {
                    const uint64_t tlen = replay_le32(p + pos + 4 + mlen);
                    if (tlen > rem - mlen - 8) {
                        ok = false;
                    } else {
                        mo = (uint32_t)(pay + pos + 4);  // total_bytes < 2^32
                        ml = (uint32_t)mlen;
                        to = (uint32_t)(pay + pos + 8 + mlen);
                        tl = (uint32_t)tlen;
                    }
                }
            }
            if (!ok) atomicMin(reinterpret_cast<unsigned long long*>(im + kRiBad), (unsigned long long)k);
            if (k == 0 && ok) {
                im[kRiMaxFp] = maxfp;
                im[kRiDict] = dict;
            }
        }
        rec_img[g] = (uint32_t)i;
        rec_k[g] = (uint32_t)k;
        sec_off[2 * g] = mo;
        sec_len[2 * g] = ml;
        sec_off[2 * g + 1] = to;
        sec_len[2 * g + 1] = tl;
    }
}

// out[j] = exclusive sum over j < n of f(j); out[n] = the total, also into *total_out
template <typename F>
__device__ __forceinline__ void replay_block_scan(uint64_t n, F f, uint32_t* __restrict__ out, uint64_t* total_out) {
    __shared__ uint64_t w4[4];
    uint64_t run = 0;  // the sum of the rounds before this one (uniform)
    for (uint64_t b0 = 0; b0 < n; b0 += 256 * 4) {
        const uint64_t j0 = b0 + threadIdx.x * 4u;  // four consecutive items per thread
        uint64_t c[4], mine = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            c[x] = j0 + x < n ? f(j0 + x) : 0;
            mine += c[x];
        }
        uint64_t t;
        uint64_t before = run + block_excl_scan(mine, w4, t);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            if (j0 + x < n) out[j0 + x] = (uint32_t)before;
            before += c[x];
        }
        run += t;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[n] = (uint32_t)run;
        if (total_out) *total_out = run;
    }
}

__global__ __launch_bounds__(256) void k_replay_plan(uint64_t* __restrict__ ctl, uint32_t tile_shift,
                                                    const uint32_t* __restrict__ sec_len,
                                                    uint32_t* __restrict__ sec_tile) {
    if (ctl[0] != ~0ull) return;
    const uint64_t mask = (1ull << tile_shift) - 1;
    replay_block_scan(2 * ctl[1], [&](uint64_t q) { return ((uint64_t)sec_len[q] + mask) >> tile_shift; }, sec_tile,
                      ctl + 2);
}

__global__ __launch_bounds__(256) void k_replay_scan(const uint64_t* __restrict__ ctl, const uint32_t* __restrict__ tile_cnt,
                                                    uint32_t* __restrict__ tile_pre) {
    if (ctl[0] != ~0ull) return;
    replay_block_scan(ctl[2], [&](uint64_t t) { return (uint64_t)tile_cnt[t]; }, tile_pre, nullptr);
}

// the section that holds tile t: the last q below n_sec with sec_tile[q] <= t
__device__ __forceinline__ uint64_t replay_section_of(const uint32_t* __restrict__ sec_tile, uint64_t n_sec, uint64_t t) {
    uint64_t lo = 0, hi = n_sec;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (sec_tile[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// bit k set: byte k of the 16 is below 0x80 (a varint ends there)
__device__ __forceinline__ uint32_t replay_term_mask(uint64_t lo, uint64_t hi) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) m |= (byte_of(lo, hi, k) < 0x80 ? 1u : 0u) << k;
    return m;
}

__global__ __launch_bounds__(256) void k_replay_count(const uint8_t* __restrict__ base, const uint64_t* __restrict__ ctl,
                                                     uint32_t tile_shift, const uint32_t* __restrict__ sec_off,
                                                     const uint32_t* __restrict__ sec_len,
                                                     const uint32_t* __restrict__ sec_tile,
                                                     uint32_t* __restrict__ tile_cnt) {
    if (ctl[0] != ~0ull) return;
    const uint64_t n_tiles = ctl[2], n_sec = 2 * ctl[1];
    const uint64_t tile = 1ull << tile_shift;
    const int lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 4;
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += stride) {
        const uint64_t q = replay_section_of(sec_tile, n_sec, t);
        const uint8_t* sec = base + sec_off[q];
        const uint64_t len = sec_len[q];
        const uint64_t start = (t - sec_tile[q]) << tile_shift, end = min(start + tile, len);
        uint64_t c = 0;
        for (uint64_t P = start + lane * 16u; P < end; P += 1024) {
            uint64_t lo, hi;
            ld_bytes16(sec + P, end - P, 0x80, lo, hi);
            c += __builtin_popcount(replay_term_mask(lo, hi));
        }
        c = wave_sum(c);
        if (lane == 0) tile_cnt[t] = (uint32_t)c;
    }
}

// The varint that ends at sec[pos]: its length, limit + 1 when the run of
// continuation bytes before it is longer than the limit allows; never reads
// before sec[0].
__device__ __forceinline__ int replay_run(const uint8_t* sec, uint64_t pos, int limit) {
    int len = 1;
    while (len <= limit && pos >= (uint64_t)len && sec[pos - len] >= 0x80) ++len;
    return len;
}
__device__ __forceinline__ uint64_t replay_value(const uint8_t* sec, uint64_t pos, int len) {
    uint64_t v = 0;
    for (int x = 0; x < len; ++x) v |= (uint64_t)(sec[pos - len + 1 + x] & 0x7F) << (7 * x);
    return v;
}

// MODE 1 checks and folds, MODE 2 stores snapshot values and bids for log
// rows, MODE 3 stores the winning log entries.
template <int MODE>
__global__ __launch_bounds__(256) void k_replay_decode(const uint8_t* __restrict__ base, const uint64_t* __restrict__ ctl,
                                                      uint32_t tile_shift, const uint32_t* __restrict__ sec_off,
                                                      const uint32_t* __restrict__ sec_len,
                                                      const uint32_t* __restrict__ sec_tile,
                                                      const uint32_t* __restrict__ rec_img,
                                                      const uint32_t* __restrict__ rec_k,
                                                      const uint32_t* __restrict__ tile_pre, uint64_t* __restrict__ img,
                                                      uint64_t* __restrict__ table, uint32_t* __restrict__ seq) {
    if (ctl[0] != ~0ull) return;
    const uint64_t n_tiles = ctl[2], n_sec = 2 * ctl[1];
    const uint64_t tile = 1ull << tile_shift;
    const int lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * 4;
    for (uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += stride) {
        // everything up to the byte loop is uniform over the wave
        const uint64_t q = replay_section_of(sec_tile, n_sec, t);
        const uint64_t g = q >> 1, k = rec_k[g];
        const int kind = (q & 1) ? 2 : k == 0 ? 0 : 1;  // snapshot mapping, log mapping, term
        uint64_t* im = img + (uint64_t)rec_img[g] * kReplayImgWords;
        if (MODE >= 2 && (kind == 2 || im[kRiStatus] != kReplayOk)) continue;
        if (MODE == 3 && kind == 0) continue;
        const uint8_t* sec = base + sec_off[q];
        const uint64_t len = sec_len[q];
        const uint64_t t0 = sec_tile[q];
        const uint64_t start = (t - t0) << tile_shift, end = min(start + tile, len);
        const uint64_t sec_ord = tile_pre[t0];  // global ordinal of the section's first varint
        const uint64_t tf = MODE >= 2 ? im[kRiFirst] : 0;
        bool bad = false;
        uint64_t max_pid = 0, max_fp = 0;
        if (MODE == 1 && t == t0 && lane == 0) {
            const uint64_t cnt = tile_pre[sec_tile[q + 1]] - sec_ord;
            bad = sec[len - 1] >= 0x80 || (kind != 0 && (cnt & 1));  // a tile exists, so len >= 1
            if (kind == 0) im[kRiSnap] = cnt;
            else if (cnt >= 2)
                atomicAdd(reinterpret_cast<unsigned long long*>(im + (kind == 1 ? kRiLog : kRiTerm)),
                          (unsigned long long)(cnt / 2));
        }
        uint64_t ord = tile_pre[t] - sec_ord;  // ordinal in the section of the tile's first varint
        for (uint64_t p0 = start; p0 < end; p0 += 1024) {
            const uint64_t P = p0 + lane * 16u;
            uint64_t lo, hi;
            ld_bytes16(sec + P, P < end ? end - P : 0, 0x80, lo, hi);
            uint32_t mask = replay_term_mask(lo, hi);
            uint64_t tot;
            uint64_t o = ord + wave_excl_scan((uint64_t)__builtin_popcount(mask), tot);
            ord += tot;
            for (; mask; mask &= mask - 1, ++o) {
                const uint64_t pos = P + __builtin_ctz(mask);
                const bool is_pid = kind == 1 && (o & 1) == 0;
                const int limit = is_pid ? 5 : 10;
                const int n = replay_run(sec, pos, limit);
                if (n > limit) {
                    bad = true;
                    continue;
                }
                if (kind == 2 || is_pid) continue;  // a page id is read with its value
                if (kind == 0) {
                    if (MODE == 2) table[tf + o] = replay_value(sec, pos, n);
                    continue;
                }
                const uint64_t v = replay_value(sec, pos, n);
                if (pos < (uint64_t)n) continue;  // no page id before the value: an over-long run was flagged
                const uint64_t ppos = pos - n;
                const int pn = replay_run(sec, ppos, 5);
                if (pn > 5) continue;  // flagged at the page id
                const uint64_t pid = replay_value(sec, ppos, pn) & 0xFFFFFFFFull;
                if (MODE == 1) {
                    max_pid = max(max_pid, pid + 1);
                    if ((v & 7) == 1) max_fp = max(max_fp, (v >> 3) + 1);
                } else {
                    const uint32_t s = (uint32_t)(sec_ord + o);  // odd ordinal in the section: never 0
                    if (MODE == 2) atomicMax(seq + tf + pid, s);
                    else if (seq[tf + pid] == s) table[tf + pid] = v;
                }
            }
        }
        if (MODE == 1) {
            const bool any_bad = __any(bad);
            max_pid = wave_max(max_pid);
            max_fp = wave_max(max_fp);
            if (lane == 0) {
                if (any_bad) atomicMin(reinterpret_cast<unsigned long long*>(im + kRiBad), (unsigned long long)k);
                if (max_pid) atomicMax(reinterpret_cast<unsigned long long*>(im + kRiMaxPid), (unsigned long long)max_pid);
                if (max_fp) atomicMax(reinterpret_cast<unsigned long long*>(im + kRiMaxFp), (unsigned long long)max_fp);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_replay_images(uint64_t n_images, const uint64_t* __restrict__ scan_rep,
                                                      uint64_t* __restrict__ ctl, uint64_t* __restrict__ img,
                                                      uint64_t table_base, uint64_t table_cap) {
    __shared__ uint64_t w4[4];
    if (ctl[0] != ~0ull) return;
    uint64_t rows = 0, written = 0;  // of the images before this round (uniform)
    for (uint64_t b0 = 0; b0 < n_images; b0 += 256) {
        const uint64_t i = b0 + threadIdx.x;
        uint64_t size = 0, status = kReplayNotReplayable;
        uint64_t* im = img + i * kReplayImgWords;
        if (i < n_images) {
            const uint64_t verdict = scan_rep[i * kMscanReportWords + 9];
            if (verdict <= 1) {
                status = im[kRiBad] != ~0ull ? kReplayMalformed : kReplayOk;
                if (status == kReplayOk) size = max(im[kRiSnap], im[kRiMaxPid]);
            }
        }
        uint64_t t;
        const uint64_t first = table_base + rows + block_excl_scan(size, w4, t);
        rows += t;
        __syncthreads();
        if (i < n_images && status == kReplayOk && first + size > table_cap) status = kReplayTableCap;
        const uint64_t w = status == kReplayOk ? size : 0;
        uint64_t tw;
        (void)block_excl_scan(w, w4, tw);
        written += tw;
        if (i < n_images) {
            im[kRiStatus] = status;
            im[kRiSize] = size;
            im[kRiFirst] = first;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ctl[3] = rows;
        ctl[4] = written;
    }
}

__global__ __launch_bounds__(256) void k_replay_fill(const uint64_t* __restrict__ ctl, uint64_t table_base,
                                                    uint64_t* __restrict__ table, uint32_t* __restrict__ seq) {
    if (ctl[0] != ~0ull) return;
    const uint64_t n = ctl[4];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        table[table_base + r] = kReplayInvalidValue;
        seq[table_base + r] = 0;
    }
}

__global__ __launch_bounds__(256) void k_replay_stats(uint64_t n_images, const uint64_t* __restrict__ ctl,
                                                     uint64_t table_base, const uint64_t* __restrict__ table,
                                                     uint64_t* __restrict__ img) {
    if (ctl[0] != ~0ull) return;
    const uint64_t n = ctl[4];
    const int lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~63ull; r0 < n; r0 += stride) {
        const uint64_t r = r0 + lane;
        const bool valid = r < n;
        uint64_t i = 0, mapped = 0, lo_fp = ~0ull, hi_fp = 0, beyond = 0;
        if (valid) {
            const uint64_t row = table_base + r;
            // the image that holds the row: the last i with table_first <= row (an image after
            // the holder starts at or after the holder's end, whatever its status)
            uint64_t a = 0, b = n_images;
            while (b - a > 1) {
                const uint64_t mid = a + (b - a) / 2;
                if (img[mid * kReplayImgWords + kRiFirst] <= row) a = mid;
                else b = mid;
            }
            i = a;
            const uint64_t v = table[row];
            if ((v & 7) == 1) {
                const uint64_t id = v >> 3;
                mapped = 1;
                lo_fp = hi_fp = id;
                beyond = id >= img[i * kReplayImgWords + kRiMaxFp] ? 1 : 0;
            }
        }
        const uint64_t i0 = __shfl((unsigned long long)i, 0, 64);  // lane 0 of a live wave is valid
        unsigned long long* im = reinterpret_cast<unsigned long long*>(img + i * kReplayImgWords);
        if (__all(!valid || i == i0)) {  // one image over the wave: one set of atomics
            mapped = wave_sum(mapped);
            beyond = wave_sum(beyond);
            lo_fp = wave_min(lo_fp);
            hi_fp = wave_max(hi_fp);
            if (lane == 0 && mapped) {
                atomicAdd(im + kRiMapped, (unsigned long long)mapped);
                atomicMin(im + kRiMinFp, (unsigned long long)lo_fp);
                atomicMax(im + kRiMaxMapped, (unsigned long long)hi_fp);
                if (beyond) atomicAdd(im + kRiBeyond, (unsigned long long)beyond);
            }
        } else if (mapped) {
            atomicAdd(im + kRiMapped, 1ull);
            atomicMin(im + kRiMinFp, (unsigned long long)lo_fp);
            atomicMax(im + kRiMaxMapped, (unsigned long long)hi_fp);
            if (beyond) atomicAdd(im + kRiBeyond, 1ull);
        }
    }
}

__global__ __launch_bounds__(256) void k_replay_report(uint64_t n_images, const uint64_t* __restrict__ ctl,
                                                      const uint64_t* __restrict__ scan_rep,
                                                      const uint64_t* __restrict__ recs, const uint64_t* __restrict__ img,
                                                      uint64_t* __restrict__ reports, uint64_t* __restrict__ summary) {
    __shared__ unsigned long long tot[7];  // images by status 0..3, mapped, log entries, first bad image
    const uint64_t invalid = ctl[0];
    if (invalid != ~0ull) {  // uniform: only n_images and the invalid image are reported
        if (threadIdx.x < kReplaySummaryWords)
            summary[threadIdx.x] = threadIdx.x == 0 ? n_images : threadIdx.x == 10 ? invalid : 0;
        return;
    }
    if (threadIdx.x < 7) tot[threadIdx.x] = threadIdx.x == 6 ? ~0ull : 0ull;
    __syncthreads();
    uint64_t acc[6] = {};
    uint64_t first_bad = ~0ull;
    for (uint64_t i = threadIdx.x; i < n_images; i += 256) {
        const uint64_t* im = img + i * kReplayImgWords;
        const uint64_t status = im[kRiStatus];
        const bool counted = status == kReplayOk || status == kReplayTableCap;
        const bool ok = status == kReplayOk;
        uint64_t root = 0, ttl = 0;
        if (counted) {
            const uint64_t* e = recs + (scan_rep[i * kMscanReportWords + 10] + im[kRiNrep] - 1) * kMscanRecordWords;
            root = e[3] >> 32;
            ttl = e[4] & 0xFFFFFFFFull;
        }
        uint64_t* r = reports + i * kReplayReportWords;
        r[0] = status;
        r[1] = im[kRiNrep];
        r[2] = status == kReplayMalformed ? im[kRiBad] : ~0ull;
        r[3] = root;
        r[4] = ttl;
        r[5] = counted ? im[kRiMaxFp] : 0;
        r[6] = counted ? im[kRiDict] : 0;
        r[7] = counted ? im[kRiSnap] : 0;
        r[8] = counted ? im[kRiLog] : 0;
        r[9] = im[kRiSize];
        r[10] = im[kRiFirst];
        r[11] = ok ? im[kRiMapped] : 0;
        r[12] = ok && im[kRiMapped] ? im[kRiMinFp] : ~0ull;
        r[13] = ok && im[kRiMapped] ? im[kRiMaxMapped] : ~0ull;
        r[14] = ok ? im[kRiBeyond] : 0;
        r[15] = counted ? im[kRiTerm] : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += status == (uint64_t)k ? 1 : 0;
        acc[4] += r[11];
        acc[5] += r[8];
        if (!ok && first_bad == ~0ull) first_bad = i;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint64_t v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&tot[k], (unsigned long long)v);
    }
    if (first_bad != ~0ull) atomicMin(&tot[6], (unsigned long long)first_bad);
    __syncthreads();
    if (threadIdx.x < kReplaySummaryWords) {
        uint64_t v = 0;
        switch (threadIdx.x) {
            case 0: v = n_images; break;
            case 1: case 2: case 3: case 4: v = tot[threadIdx.x - 1]; break;
            case 5: v = ctl[3]; break;
            case 6: v = ctl[4]; break;
            case 7: v = tot[4]; break;
            case 8: v = tot[5]; break;
            case 9: v = tot[6]; break;
            case 10: v = ~0ull; break;
            default: v = 0; break;
        }
        summary[threadIdx.x] = v;
    }
}

hipError_t run_manifest_replay(const uint8_t* base, uint64_t total, const uint64_t* off, const uint64_t* size,
                               uint64_t n_images, uint32_t align, uint64_t* scan_reports, uint64_t* reports,
                               uint64_t* summary, uint64_t* table, uint64_t table_base, uint64_t table_cap,
                               hipStream_t s) {
    uint32_t shift = 0;
    while ((1u << shift) < align) ++shift;
    const uint32_t tile = replay_tile();
    uint32_t tile_shift = 0;
    while ((1u << tile_shift) < tile) ++tile_shift;
    if (total >= (1ull << 32) || n_images > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint64_t max_recs = (total >> shift) + n_images;             // the scan's own bound
    const uint64_t max_tiles = (total >> tile_shift) + 2 * max_recs;  // sections are disjoint byte ranges
    ScratchLease scratch(s);
    // u64: ctl, scan summary, scan reports (when the caller wants none), records, image words;
    // u32: rec_img, rec_k [max_recs], sec_off, sec_len [2 max_recs], sec_tile [2 max_recs + 1],
    //      tile_cnt [max_tiles], tile_pre [max_tiles + 1], seq [table_cap]
    const size_t words = kReplayCtlWords + kMscanSummaryWords + (scan_reports ? 0 : kMscanReportWords * n_images) +
                         kMscanRecordWords * max_recs + kReplayImgWords * n_images;
    const size_t u32s = 8 * max_recs + 2 * max_tiles + 4 + (table_cap > table_base ? table_cap : 0);
    hipError_t e = scratch.get(words * 8 + u32s * 4);
    if (e != hipSuccess) return e;
    uint64_t* ctl = static_cast<uint64_t*>(scratch.p);
    uint64_t* scan_sum = ctl + kReplayCtlWords;
    uint64_t* scan_rep = scan_sum + kMscanSummaryWords;
    uint64_t* recs = scan_rep + (scan_reports ? 0 : kMscanReportWords * n_images);
    if (scan_reports) scan_rep = scan_reports;
    uint64_t* img = recs + kMscanRecordWords * max_recs;
    uint32_t* rec_img = reinterpret_cast<uint32_t*>(img + kReplayImgWords * n_images);
    uint32_t* rec_k = rec_img + max_recs;
    uint32_t* sec_off = rec_k + max_recs;
    uint32_t* sec_len = sec_off + 2 * max_recs;
    uint32_t* sec_tile = sec_len + 2 * max_recs;
    uint32_t* tile_cnt = sec_tile + 2 * max_recs + 1;
    uint32_t* tile_pre = tile_cnt + max_tiles;
    uint32_t* seq = tile_pre + max_tiles + 1;
    e = run_manifest_scan(base, total, off, size, n_images, align, scan_rep, scan_sum, recs, max_recs, s);
    if (e != hipSuccess) return e;
    if (n_images) {
        const unsigned tgrid = grid_for(max_tiles, 4, kBlocksPerCu);
        hipLaunchKernelGGL(k_replay_sections, dim3((unsigned)n_images), dim3(256), 0, s, base, off, n_images, scan_sum,
                           scan_rep, recs, ctl, img, rec_img, rec_k, sec_off, sec_len);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_replay_plan, dim3(1), dim3(256), 0, s, ctl, tile_shift, sec_len, sec_tile);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_replay_count, dim3(tgrid), dim3(256), 0, s, base, ctl, tile_shift, sec_off, sec_len,
                           sec_tile, tile_cnt);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_replay_scan, dim3(1), dim3(256), 0, s, ctl, tile_cnt, tile_pre);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_replay_decode<1>, dim3(tgrid), dim3(256), 0, s, base, ctl, tile_shift, sec_off, sec_len,
                           sec_tile, rec_img, rec_k, tile_pre, img, table, seq);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_replay_images, dim3(1), dim3(256), 0, s, n_images, scan_rep, ctl, img, table_base,
                           table_cap);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (table_cap > table_base) {  // otherwise no image can be OK with rows to write
            const unsigned rgrid = grid_for(table_cap - table_base, kBlock, kBlocksPerCu);
            hipLaunchKernelGGL(k_replay_fill, dim3(rgrid), dim3(256), 0, s, ctl, table_base, table, seq);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            hipLaunchKernelGGL(k_replay_decode<2>, dim3(tgrid), dim3(256), 0, s, base, ctl, tile_shift, sec_off, sec_len,
                               sec_tile, rec_img, rec_k, tile_pre, img, table, seq);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            hipLaunchKernelGGL(k_replay_decode<3>, dim3(tgrid), dim3(256), 0, s, base, ctl, tile_shift, sec_off, sec_len,
                               sec_tile, rec_img, rec_k, tile_pre, img, table, seq);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            hipLaunchKernelGGL(k_replay_stats, dim3(rgrid), dim3(256), 0, s, n_images, ctl, table_base, table, img);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_replay_report, dim3(1), dim3(256), 0, s, n_images, ctl, scan_rep, recs, img, reports,
                           summary);
        return hipGetLastError();
    }
    // no image: the scan's summary says so; the replay's own is all zero but for "none"
    hipLaunchKernelGGL(k_replay_sections, dim3(1), dim3(256), 0, s, base, off, n_images, scan_sum, scan_rep, recs,
                       ctl, img, rec_img, rec_k, sec_off, sec_len);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_replay_report, dim3(1), dim3(256), 0, s, n_images, ctl, scan_rep, recs, img, reports, summary);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Scrub live (pcs_scrub_live_dev): which file pages of a window a replayed
// mapping table still points to, who owns each, and the class census of the
// live and the dead set.  A row v maps file page v >> 3 iff (v & 7) == 1.
//   k_live_fill   owner[i] = UINT32_MAX, the three counters 0;
//   k_live_owner  one lane per table row: atomicMin(owner[page], row) for rows
//                 that point into the window, counts of mapped rows;
//   k_live_count  one block per kScrubSpan pages: the six live/dead x class
//                 cells, damaged live pages, first damaged, last live;
//   k_live_scan   one block: each span's rank in the damaged list, summary;
//   k_live_list   the spans whose rank is below the cap write their damaged
//                 pages at rank + position (the scrub list's pattern: ascending
//                 and the same on every call).
// ---------------------------------------------------------------------------
constexpr int kLiveRec = 10;           // u32 per span: damaged, live ok/blank/corrupt, dead ok/blank/corrupt, first damaged, last live + 1, live
constexpr int kLiveSummaryWords = 16;  // pcs_live_summary

__global__ __launch_bounds__(256) void k_live_fill(uint64_t n, uint32_t* __restrict__ owner, uint64_t* __restrict__ ctl) {
    if (blockIdx.x == 0 && threadIdx.x < 4) ctl[threadIdx.x] = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) owner[i] = 0xFFFFFFFFu;
}

__global__ __launch_bounds__(256) void k_live_owner(const uint64_t* __restrict__ table, uint64_t rows, uint64_t fp_first,
                                                   uint64_t n, uint32_t* __restrict__ owner, uint64_t* __restrict__ ctl) {
    uint64_t mapped = 0, inside = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < rows; p += stride) {
        const uint64_t v = table[p];
        if ((v & 7) != 1) continue;
        ++mapped;
        const uint64_t id = v >> 3;
        if (id >= fp_first && id - fp_first < n) {
            ++inside;
            atomicMin(owner + (id - fp_first), (uint32_t)p);
        }
    }
    mapped = wave_sum(mapped);
    inside = wave_sum(inside);
    if ((threadIdx.x & 63) == 0) {
        if (mapped) atomicAdd(reinterpret_cast<unsigned long long*>(ctl), (unsigned long long)mapped);
        if (inside) atomicAdd(reinterpret_cast<unsigned long long*>(ctl + 1), (unsigned long long)inside);
    }
}

__global__ __launch_bounds__(256) void k_live_count(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ owner,
                                                   uint64_t n, uint32_t* __restrict__ rec) {
    __shared__ uint32_t cnt[kLiveRec];
    if (threadIdx.x < kLiveRec) cnt[threadIdx.x] = threadIdx.x == 7 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    const uint64_t p0 = (uint64_t)blockIdx.x * kScrubSpan + threadIdx.x * 16u;
    uint32_t c7[7] = {};
    uint32_t first = 0xFFFFFFFFu, last = 0, n_live = 0;
    if (p0 < n) {
        uint64_t cl, ch;
        ld_bytes16(cls + p0, n - p0, 0xFF, cl, ch);
        const int m = (int)min((uint64_t)16, n - p0);
        for (int k = 0; k < m; ++k) {
            const uint32_t c = byte_of(cl, ch, k);
            const bool live = owner[p0 + k] != 0xFFFFFFFFu;
            if (c <= kClassBlank) ++c7[(live ? 1 : 4) + (c == kClassOk ? 0 : c == kClassBlank ? 1 : 2)];
            if (live) {
                ++n_live;
                last = threadIdx.x * 16u + k + 1;
                if (c != kClassOk) {
                    ++c7[0];
                    if (first == 0xFFFFFFFFu) first = threadIdx.x * 16u + k;
                }
            }
        }
    }
#pragma unroll
    for (int f = 0; f < 7; ++f) {
        const uint32_t v = (uint32_t)wave_sum(c7[f]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&cnt[f], v);
    }
    n_live = (uint32_t)wave_sum(n_live);
    if ((threadIdx.x & 63) == 0 && n_live) atomicAdd(&cnt[9], n_live);
    if (first != 0xFFFFFFFFu) atomicMin(&cnt[7], first);
    if (last) atomicMax(&cnt[8], last);
    __syncthreads();
    if (threadIdx.x < kLiveRec) rec[(uint64_t)blockIdx.x * kLiveRec + threadIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_live_scan(const uint32_t* __restrict__ rec, uint64_t nblocks, uint64_t n,
                                                  uint64_t rows, uint64_t cap, const uint64_t* __restrict__ ctl,
                                                  uint64_t* __restrict__ rank, uint64_t* __restrict__ summary) {
    __shared__ uint64_t w4[4];
    __shared__ unsigned long long tot[9];  // six cells, first damaged, last live + 1, live pages
    if (threadIdx.x < 9) tot[threadIdx.x] = threadIdx.x == 6 ? ~0ull : 0ull;
    __syncthreads();
    uint64_t damaged = 0;  // in the spans before this round (uniform)
    uint64_t acc[6] = {}, live = 0;
    uint64_t first = ~0ull, last = 0;
    for (uint64_t base = 0; base < nblocks; base += 256) {
        const uint64_t b = base + threadIdx.x;
        uint64_t c = 0;
        if (b < nblocks) {
            const uint32_t* r = rec + b * kLiveRec;
            c = r[0];
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[k] += r[1 + k];
            live += r[9];
            if (r[7] != 0xFFFFFFFFu && first == ~0ull) first = b * kScrubSpan + r[7];
            if (r[8]) last = b * kScrubSpan + r[8];  // a thread's spans ascend
        }
        uint64_t total;
        const uint64_t before = block_excl_scan(c, w4, total);
        if (b < nblocks) rank[b] = damaged + before;
        damaged += total;
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint64_t v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&tot[k], (unsigned long long)v);
    }
    live = wave_sum(live);
    if ((threadIdx.x & 63) == 0 && live) atomicAdd(&tot[8], (unsigned long long)live);
    if (first != ~0ull) atomicMin(&tot[6], (unsigned long long)first);
    if (last) atomicMax(&tot[7], (unsigned long long)last);
    __syncthreads();
    if (threadIdx.x < kLiveSummaryWords) {
        const int i = threadIdx.x;
        const uint64_t n_live = tot[8];  // every owned page, whatever its class byte
        uint64_t v = 0;
        switch (i) {
            case 0: v = n; break;
            case 1: v = rows; break;
            case 2: v = ctl[0]; break;
            case 3: v = ctl[1]; break;
            case 4: v = ctl[1] - n_live; break;  // rows that point into the window but own nothing
            case 5: case 6: case 7: case 8: case 9: case 10: v = tot[i - 5]; break;
            case 11: v = damaged; break;
            case 12: v = tot[6]; break;
            case 13: v = tot[7] ? tot[7] - 1 : ~0ull; break;
            case 14: v = damaged < cap ? damaged : cap; break;
            default: v = 0; break;
        }
        summary[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_live_list(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ owner,
                                                  uint64_t n, const uint32_t* __restrict__ rec,
                                                  const uint64_t* __restrict__ rank, uint64_t cap,
                                                  uint64_t* __restrict__ list) {
    __shared__ uint64_t w4[4];
    const uint64_t r0 = rank[blockIdx.x];
    if (rec[(uint64_t)blockIdx.x * kLiveRec] == 0 || r0 >= cap) return;  // uniform over the block
    const uint64_t p0 = (uint64_t)blockIdx.x * kScrubSpan + threadIdx.x * 16u;
    uint32_t mask = 0;
    uint64_t cl = 0, ch = 0;
    if (p0 < n) {
        ld_bytes16(cls + p0, n - p0, 0xFF, cl, ch);
        const int m = (int)min((uint64_t)16, n - p0);
        for (int k = 0; k < m; ++k)
            mask |= (owner[p0 + k] != 0xFFFFFFFFu && byte_of(cl, ch, k) != kClassOk ? 1u : 0u) << k;
    }
    uint64_t total;
    uint64_t pos = r0 + block_excl_scan(__builtin_popcount(mask), w4, total);
    while (mask && pos < cap) {
        const int k = __builtin_ctz(mask);
        mask &= mask - 1;
        list[2 * pos] = p0 + k;  // pcs_live_page: index, then page_id | cls << 32
        list[2 * pos + 1] = (uint64_t)owner[p0 + k] | (uint64_t)byte_of(cl, ch, k) << 32;
        ++pos;
    }
}

hipError_t run_scrub_live(const uint8_t* cls, uint64_t n, uint64_t fp_first, const uint64_t* table, uint64_t rows,
                          uint32_t* owner, uint64_t* summary, uint64_t* list, uint64_t cap, hipStream_t s) {
    const uint64_t nblocks = (n + kScrubSpan - 1) / kScrubSpan;
    if (nblocks > 0x7FFFFFFFull || rows > 0xFFFFFFFFull) return hipErrorInvalidValue;
    ScratchLease scratch(s);  // counters, ranks, span records and (when the caller wants none) the owners
    hipError_t e = scratch.get(4 * 8 + nblocks * 8 + nblocks * kLiveRec * 4 + (owner ? 0 : n * 4));
    if (e != hipSuccess) return e;
    uint64_t* ctl = static_cast<uint64_t*>(scratch.p);
    uint64_t* rank = ctl + 4;
    uint32_t* rec = reinterpret_cast<uint32_t*>(rank + nblocks);
    if (!owner) owner = rec + nblocks * kLiveRec;
    hipLaunchKernelGGL(k_live_fill, dim3(grid_for(n, kBlock, kBlocksPerCu)), dim3(kBlock), 0, s, n, owner, ctl);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (rows) {
        hipLaunchKernelGGL(k_live_owner, dim3(grid_for(rows, kBlock, kBlocksPerCu)), dim3(kBlock), 0, s, table, rows,
                           fp_first, n, owner, ctl);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (nblocks) {
        hipLaunchKernelGGL(k_live_count, dim3((unsigned)nblocks), dim3(256), 0, s, cls, owner, n, rec);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_live_scan, dim3(1), dim3(256), 0, s, rec, nblocks, n, rows, cap, ctl, rank, summary);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (nblocks && cap) {
        hipLaunchKernelGGL(k_live_list, dim3((unsigned)nblocks), dim3(256), 0, s, cls, owner, n, rec, rank, cap, list);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t scratch_acquire(size_t bytes, void** out, int* id) { return g_scratch.acquire(bytes, out, id); }
hipError_t scratch_release(int id, hipStream_t s) { return g_scratch.release(id, s); }

template <int MODE>
static hipError_t desc_impl(int algo, const uint8_t* base, const uint64_t* off, const uint32_t* len, uint64_t n,
                            int skip, uint64_t seed, uint64_t* out, uint8_t* ok, unsigned long long* fb,
                            hipStream_t s) {
    if (n == 0) return hipSuccess;
    if constexpr (MODE == kStamp) {
        if (skip == 8 && seed == 0) {
            // two-pass stamp, as for fixed-size pages: digests of every page
            // into a compact array (the descriptor digest kernels), then one
            // 8-byte header write per page.  Against headers written by the
            // digest kernel inside its read stream: +2.5 % (XXH3) and +7.1 %
            // (XXH64) on config 3 (profiles/r02/desc_stamp_lab.txt).
            uint64_t* dig = out;
            ScratchLease scratch(s);
            hipError_t e = hipSuccess;
            if (!dig) {
                e = scratch.get(n * 8);
                dig = static_cast<uint64_t*>(scratch.p);
            }
            if (e == hipSuccess) e = desc_impl<kDigest>(algo, base, off, len, n, skip, seed, dig, nullptr, nullptr, s);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_scatter_stamp_desc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                                   const_cast<uint8_t*>(base), off, len, n, dig);
                e = hipGetLastError();
            }
            return e;
        }
    }
    if (skip == 8 && seed == 0) {
        // fast kernels for conforming pages, generic lanes for the rest
        if (algo == 0) {
            // one workgroup per 16-page tile, every tile covered once
            const uint64_t ntiles = (n + 15) / 16;
            if (ntiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
            const unsigned grid = (unsigned)ntiles;
#define L(NT_, B4_) \
    hipLaunchKernelGGL((k_xxh3_desc<MODE, NT_, B4_>), dim3(grid), dim3(kBlock), 0, s, base, off, len, n, out, ok, fb)
            if (use_nt()) {
                if (rt_batch4()) L(true, true);
                else L(true, false);
            } else {
                if (rt_batch4()) L(false, true);
                else L(false, false);
            }
#undef L
            // every page is the descriptor kernel's (fast body, any-size body,
            // short pages on one lane): no generic pass, which cost 4.7-5.2 us
            // per call on config 3 (profiles/r02d_sweep.json, r02e_sweep.json)
            return hipGetLastError();
        } else {
            // Pages off the line shape (usually none) are left to the generic
            // lanes below.  A separate quad-per-page pass over the
            // descriptors for them cost 9.7 us per call on config 3 even when
            // it found nothing to do (profiles/r02a_sweep.json); the generic
            // pass itself, reading every descriptor, 6.3 us
            // (profiles/r03/r03k_kernel_stats.csv).  Now the LDS kernel
            // stores this call's id in a scratch word when it leaves a page
            // behind, and the generic pass exits at once unless it finds it.
            ScratchLease flag(s);
            hipError_t e = flag.get(sizeof(unsigned long long));
            if (e != hipSuccess) return e;
            auto* word = static_cast<unsigned long long*>(flag.p);
            const uint64_t id = next_call_id();
            const unsigned grid = page_grid(n, kBlock / 4, 2);
            if (use_nt()) launch_xxh64_lds<MODE, true, kAddrDesc>(grid, s, base, off, len, 0u, n, out, ok, fb, word, id);
            else launch_xxh64_lds<MODE, false, kAddrDesc>(grid, s, base, off, len, 0u, n, out, ok, fb, word, id);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
            // one block per CU: when every page conforms (the usual case)
            // each block only reads the flag and leaves (a full-size grid
            // took 4.3 us to do that, profiles/r04b_sweep.json); rare
            // off-shape pages take the grid-stride loop
            const unsigned ggrid = std::min(grid_for(n, kBlock, kBlocksPerCu), (unsigned)cu_count());
            hipLaunchKernelGGL((k_generic_desc<MODE>), dim3(ggrid), dim3(kBlock), 0, s, base, off, len, n, algo, seed,
                               skip, 1, out, ok, fb, word, id);
            return hipGetLastError();
        }
    }
    int filter = 0;
    if (MODE == kDigest && algo == 0 && skip == 0) {
        // raw XXH3 ranges: long ones get a workgroup each
        const unsigned lgrid = grid_for(n, 1, 8);
        hipLaunchKernelGGL(k_xxh3_long, dim3(lgrid), dim3(kBlock), 0, s, base, off, len, n, out);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        filter = 2;
    }
    const unsigned grid = grid_for(n, kBlock, kBlocksPerCu);
    hipLaunchKernelGGL((k_generic_desc<MODE>), dim3(grid), dim3(kBlock), 0, s, base, off, len, n, algo, seed, skip,
                       filter, out, ok, fb, nullptr, 0ull);
    return hipGetLastError();
}

hipError_t run_manifest(const uint8_t* content, uint64_t len, uint64_t* out, hipStream_t s) {
    constexpr uint64_t kChunk = kManifestChunk;
    if (len == 0) return hipMemsetAsync(out, 0, 8, s);
    const uint64_t n = (len + kChunk - 1) / kChunk;
    if (((uintptr_t)content % 8) == 0 && g_tune[13].load(std::memory_order_relaxed) != 0) {
        // wide form: block sums over the whole GPU, then one chain per chunk
        ScratchLease scratch(s);  // block sums (64 KiB per chunk) + chunk digests
        hipError_t e = scratch.get(n * kChunkBlocks * 64 + n * 8);
        if (e != hipSuccess) return e;
        uint64_t* S = static_cast<uint64_t*>(scratch.p);
        uint64_t* h = S + n * kChunkBlocks * 8;
        if ((uintptr_t)content % 16 == 0)
            hipLaunchKernelGGL(k_manifest_sums16, dim3(kChunkBlocks / (16 * kSums16Blocks), (unsigned)n), dim3(256), 0, s,
                               content, len, S);
        else
            hipLaunchKernelGGL(k_manifest_sums, dim3(kChunkBlocks / 16, (unsigned)n), dim3(256), 0, s, content, len, S);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_manifest_chain, dim3((unsigned)n), dim3(256), 0, s, content, len, S, h);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_manifest_fold, dim3(1), dim3(64), 0, s, h, n, out);
        return hipGetLastError();
    }
    ScratchLease scratch(s);  // chunk offsets, lengths and digests
    hipError_t e = scratch.get(n * 20);
    if (e != hipSuccess) return e;
    uint64_t* off = static_cast<uint64_t*>(scratch.p);
    uint64_t* h = off + n;
    uint32_t* ln = reinterpret_cast<uint32_t*>(h + n);
    {
        hipLaunchKernelGGL(k_make_chunks, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, len, kChunk, n, off, ln);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = desc_impl<kDigest>(0, content, off, ln, n, 0, 0, h, nullptr, nullptr, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_manifest_fold, dim3(1), dim3(64), 0, s, h, n, out);
        e = hipGetLastError();
    }
    return e;
}

hipError_t run_desc(int mode, int algo, const uint8_t* base, const uint64_t* off, const uint32_t* len, uint64_t n,
                    int skip, uint64_t seed, uint64_t* out, uint8_t* ok, unsigned long long* fb, hipStream_t s) {
    switch (mode) {
        case kDigest: return desc_impl<kDigest>(algo, base, off, len, n, skip, seed, out, ok, fb, s);
        case kValidate: return desc_impl<kValidate>(algo, base, off, len, n, skip, seed, out, ok, fb, s);
        default: return desc_impl<kStamp>(algo, base, off, len, n, skip, seed, out, ok, fb, s);
    }
}

hipError_t run_list(int mode, int algo, const uint64_t* ptrs, const uint64_t* host_ptrs, uint64_t P, uint64_t n,
                    uint64_t* out, uint8_t* ok, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!list_shape_ok(algo, P)) return hipErrorNotSupported;
    if (algo == 0) {
        const unsigned grid = (unsigned)std::min<uint64_t>((n + 15) / 16, (uint64_t)cu_count() * kBlocksPerCu);
        const bool inl = host_ptrs && n <= (uint64_t)kInlinePages && g_tune[11].load(std::memory_order_relaxed) != 0;
        InlineList list;
        if (inl) std::memcpy(list.p, host_ptrs, n * 8);
#define LAUNCH(M, PF)                                                                                                \
    do {                                                                                                             \
        if (inl)                                                                                                     \
            hipLaunchKernelGGL((k_xxh3_list_inl<M, PF>), dim3(grid), dim3(kBlock), 0, s, list, (uint32_t)P, n, out, ok); \
        else                                                                                                         \
            hipLaunchKernelGGL((k_xxh3_list<M, PF>), dim3(grid), dim3(kBlock), 0, s, ptrs, (uint32_t)P, n, out, ok);  \
    } while (0)
#define BY_SIZE(M)                                    \
    switch (P) {                                      \
        case 4096: LAUNCH(M, 4096); break;            \
        case 8192: LAUNCH(M, 8192); break;            \
        case 16384: LAUNCH(M, 16384); break;          \
        default: LAUNCH(M, 0);                        \
    }
        if (mode == kDigest) BY_SIZE(kDigest)
        else if (mode == kValidate) BY_SIZE(kValidate)
        else BY_SIZE(kStamp)
#undef BY_SIZE
#undef LAUNCH
    } else {
        const unsigned grid = (unsigned)std::min<uint64_t>((n + 63) / 64, (uint64_t)cu_count() * kBlocksPerCu);
        // deepest pipeline: over PCIe every segment is a round trip
#define LAUNCH(M)                                                                                              \
    hipLaunchKernelGGL((k_xxh64_lds<M, false, kAddrList, 4>), dim3(grid), dim3(kBlock), 0, s, nullptr, ptrs, nullptr, \
                       (uint32_t)P, n, out, ok, nullptr, nullptr, 0ull)
        if (mode == kDigest) LAUNCH(kDigest);
        else if (mode == kValidate) LAUNCH(kValidate);
        else LAUNCH(kStamp);
#undef LAUNCH
    }
    return hipGetLastError();
}

hipError_t run_gen_pages(uint8_t* pages, uint64_t P, uint64_t n, uint64_t seed, uint64_t first, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned grid = grid_for(n, 1, 16);
    hipLaunchKernelGGL(k_gen_pages, dim3(grid), dim3(kBlock), 0, s, reinterpret_cast<uint64_t*>(pages), P / 8, n, seed,
                       first);
    return hipGetLastError();
}

hipError_t run_gen_desc(uint8_t* base, const uint64_t* off, const uint32_t* len, uint64_t n, uint64_t seed,
                        uint64_t first, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned grid = grid_for(n, 1, 16);
    hipLaunchKernelGGL(k_gen_desc, dim3(grid), dim3(kBlock), 0, s, base, off, len, n, seed, first);
    return hipGetLastError();
}

hipError_t run_flip(uint8_t* pages, uint64_t P, uint64_t n, uint64_t every, uint64_t byte_off, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t count = (n + every - 1) / every;
    const unsigned grid = (unsigned)((count + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_flip_byte, dim3(grid), dim3(kBlock), 0, s, pages, P, n, every, byte_off);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Pre-armed validate service (pcs_service_*, SURVEY.md §8f-1: small
// ReadPages batches).  A launch per host batch costs ~14 µs before its first
// page is read; here a kernel stays resident between requests, polling the
// request line in pinned host memory, so a request finds it waiting: ~7.5 µs
// for one page (tools/lab/service_lab.hip, profiles/r03/service_lab.txt).
// The kernel leaves after idle_ticks without a request and, between
// requests, once it has lived life_ticks, so a device-synchronising call
// elsewhere in the process waits at most that long (a grid that never leaves
// blocks such calls for as long as requests keep coming); the
// host starts the next generation of it when it can no longer be sure one is
// waiting.  A kernel serves only requests of its own generation (the high 32
// bits of seq), so a late kernel of an earlier generation never serves a
// request twice, and leaves as soon as the box names a newer one, so the next
// kernel (queued behind it on the stream) starts at once.  Workgroup w
// serves request line w / wpl, as the (w % wpl)-th of the line's wpl
// workgroups.  18 of its lanes poll: 16 load the line's request words (seq,
// n, page_size, check, ptrs[0..12), eloqstore_pcs_internal.h) and two the
// box's stop and gen words, one 8-byte load each.  Those loads are separate,
// so a poll can see the new seq beside an older request's words: the
// workgroup serves a request only when the 15 words' mixes add up to the
// check word the host wrote with them, and otherwise reads the line again (a
// torn view of one request is ignored, never served).  A request of another
// generation is not this kernel's (the host re-posts it once its own kernel
// has left).  Then the polling lanes run a system-scope acquire (pages and
// ptrs[12..n) are read fresh from host memory, ordered after the seq that
// announced them), and the workgroup hashes pages j * 16 + group, stride
// wpl * 16 (the run-time-size XXH3 body: registered 16-byte-aligned pages,
// page_size % 256 == 0), storing each verdict word system-scope, which
// reaches host memory without a release fence.  A stamp request (high half
// of the page-size word) stores the digest into the page header instead and
// then a done word, released after it.
// One poll of the line in flight per lane.  Keeping 2 or 4 in flight (each
// lane issuing its next load before examining the previous one) measured
// +0.7 / +2.8 us per request (round 5, profiles/r05/service_poll_lab_r05k.txt):
// the acquire that follows a served poll waits for the newer polls still in
// flight, one more PCIe round trip on every request.
//
// exit_ticks (test only, PCS_TUNE_SERVICE_SLOW_EXIT_TEST): nonzero makes the
// kernel a slow leaver for the non-blocking-poll test: it serves no request
// and, once it has decided to leave, stays that many ticks longer.
__global__ __launch_bounds__(256) void k_service(ServiceBox* box, int wpl, uint64_t gen, uint64_t idle_ticks,
                                                 uint64_t life_ticks, uint64_t exit_ticks) {
    constexpr int W = kServiceLineWords;
    __shared__ uint64_t s_line[W];
    __shared__ int s_go;
    ServiceLine* line = &box->line[blockIdx.x / wpl];
    const int j = blockIdx.x % wpl;
    const Xxh3Lane L = make_xxh3_lane(threadIdx.x & 15);
    const uint64_t born = __builtin_amdgcn_s_memrealtime();
    uint64_t t_last = born;
    uint64_t last = 0;  // the last seq this workgroup served
    uint64_t torn_noted = 0;
    for (;;) {
        if (threadIdx.x < W + 2) {
            const uint64_t* src = threadIdx.x < W ? &line->seq + threadIdx.x : &box->stop + (threadIdx.x - W);
            uint64_t w = 0;
            int go = 0;
            for (;;) {
                w = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                const uint64_t w0 = __shfl(w, 0, 32);
                // stop, or a newer generation queued behind this kernel
                if (__shfl(w, W, 32) != 0 || __shfl(w, W + 1, 32) != gen) break;
                if (w0 != last && (w0 >> 32) == gen && exit_ticks == 0) {
                    uint64_t m = threadIdx.x == kServiceCheckWord || threadIdx.x >= W ? 0 : service_word_mix(w, threadIdx.x);
#pragma unroll
                    for (int d = 1; d < W; d <<= 1) m += __shfl_xor(m, d, W);
                    // lane 0's sum for all 18 lanes, so every decision below is uniform
                    if (__shfl(m, 0, 32) == __shfl(w, kServiceCheckWord, 32)) {
                        go = 1;
                        break;
                    }
                    // torn: seq is new, some word is not yet this request's
                    if (j == 0 && threadIdx.x == 0 && torn_noted != w0) {
                        torn_noted = w0;
                        __hip_atomic_store(&line->torn_seq, w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                }
                const uint64_t now = __builtin_amdgcn_s_memrealtime();
                if (now - t_last > idle_ticks || now - born > life_ticks) break;
            }
            // acquire here, in the lanes whose loads saw the new seq; the
            // barrier then orders every lane's reads after it
            if (go) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            if (threadIdx.x < W) s_line[threadIdx.x] = w;
            if (threadIdx.x == 0) s_go = go;
        }
        __syncthreads();
        if (!s_go) {  // uniform per workgroup: idle, lifetime, stop or a newer generation
            if (exit_ticks) {
                const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
                while (__builtin_amdgcn_s_memrealtime() - t0 < exit_ticks) __builtin_amdgcn_s_sleep(127);
            }
            // Departure: each wave's verdict and header stores complete at
            // system scope, then one word says this workgroup has gone, so a
            // host that sees it may re-arm the line (no store of this
            // generation can land in it any more).
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            __syncthreads();
            if (threadIdx.x == 0)
                __hip_atomic_store(&box->departed[blockIdx.x], (uint32_t)gen, __ATOMIC_RELEASE,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        last = s_line[0];
        const uint64_t n = s_line[1];
        const uint32_t P = (uint32_t)s_line[2];
        const bool stamp = (s_line[2] >> 32) != 0;  // kServiceStamp: write the digest into the header
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        for (uint64_t pg = (uint64_t)j * 16 + (threadIdx.x >> 4); pg < n; pg += (uint64_t)wpl * 16) {
            const uint64_t a = pg < (uint64_t)kServiceLinePtrs
                                   ? s_line[4 + pg]  // came with the checked poll
                                   : __hip_atomic_load(&line->ptrs[pg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            uint64_t stored = 0;
            const uint64_t h = xxh3_page_rt4<false>(reinterpret_cast<const uint8_t*>(a), P, L, stored);
            if (L.g == 0) {
                if (stamp) {
                    // the header, then the done word released after it: the
                    // host sees the word only once the header has landed
                    __hip_atomic_store(reinterpret_cast<uint64_t*>(a), h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(&line->ok[pg], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                } else {
                    __hip_atomic_store(&line->ok[pg], h == stored ? 1u : 0u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
        __syncthreads();  // every lane has read s_line and s_go before the next poll rewrites them
        t_last = __builtin_amdgcn_s_memrealtime();  // the idle clock starts after this workgroup's verdicts
    }
}

hipError_t run_service(ServiceBox* d_box, int lines, int wpl, uint32_t gen, uint64_t idle_ticks, uint64_t life_ticks,
                       uint64_t exit_ticks, hipStream_t s) {
    if (lines < 1 || lines > kServiceMaxLines || wpl < 1 || lines * wpl > kServiceMaxWorkgroups) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_service, dim3((unsigned)(lines * wpl)), dim3(kBlock), 0, s, d_box, wpl, (uint64_t)gen,
                       idle_ticks, life_ticks, exit_ticks);
    return hipGetLastError();
}

hipError_t run_stream_read(const uint8_t* buf, uint64_t bytes, uint64_t* out, hipStream_t s) {
    if (bytes < 16) return hipSuccess;
    const uint64_t ntiles = ((bytes + kStreamPage - 1) / kStreamPage + 15) / 16;
    if (ntiles > 0x7FFFFFFFull) return hipErrorNotSupported;
    static std::once_flag once;
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] {
        attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_stream_read),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)kStreamLdsPad);
    });
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(k_stream_read, dim3((unsigned)ntiles), dim3(kBlock), kStreamLdsPad, s, buf,
                       bytes & ~uint64_t(15), out);
    return hipGetLastError();
}

}  // namespace pcs
