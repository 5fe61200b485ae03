// leaf_check.hip — kernels of the leaf check (pcs_leaf_check_dev): every data
// page the tree check reached in good health is decoded, and the overflow chain
// of every large value is walked.  The page rules are csrc/leaf_check.h,
// compiled here for the device and by tests/cpp/leaf_logic_test.cpp for the CPU.
//
//   k_leaf_init    key[p] = UINT64_MAX, refs[p] = 0, leaf[p] = "nothing", counters 0;
//   k_leaf_walk    one wavefront per table row that the tree reached as a
//                  healthy data page: the page is staged in LDS (as the tree
//                  check stages index pages; larger ones are decoded from global
//                  memory), lane k validates regions k, k + 64, ..., a ballot
//                  says whether every region passed, and only then a second
//                  pass counts entries, values and value bytes.  In that pass
//                  every lane stops at the next overflow entry of its region;
//                  the wave then takes the stopped lanes' entries one by one
//                  and walks each value's chain together: lanes j, j + 64 take
//                  pointer j of the group, bid atomicMin(key[c], entry key),
//                  add one to refs[c] and classify c from the table, the class
//                  bytes and the page alone.  Whether the walk goes on is read
//                  from the group's last page, never from a claim, so key and
//                  refs end as the minimum and the sum over the same set of
//                  bids whatever the schedule;
//   k_leaf_count   one block per kLeafSpan rows: owner, references and SHARED of
//                  the claimed rows, the summary's counters (integer sums) and
//                  the span's number of problems;
//   k_leaf_scan    one block: each span's rank in the problem list, summary;
//   k_leaf_list    the spans whose rank is below the cap write their problems
//                  at rank + position: ascending and the same on every call.
// Every grid and the number of launches follow from the arguments alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eloqstore_pcs_internal.h"
#include "leaf_check.h"
#include "page_stage.h"

namespace pcs {
namespace {

constexpr int kLeafWaves = 4;            // pages in flight per workgroup
constexpr uint32_t kLeafLdsPage = 8192;  // pages up to this size are staged in LDS
constexpr uint32_t kLeafSpan = 1024;     // rows per block of the count and list passes
constexpr int kLeafCtlWords = 32;        // accumulates summary word i
constexpr uint64_t kLeafNothing = 0x00000000FFFFFFFFull;  // owner UINT32_MAX, entry 0, bits 0
enum { S_PAGES, S_ROWS, S_DATA, S_DATA_OK, S_ENTRIES, S_VALUES, S_EXPIRING, S_COMPRESSED, S_INLINE, S_OVBYTES, S_REFS,
       S_OOR, S_EXTRA, S_TOTREE, S_MISPLACED, S_CAPPED, S_MAXGROUPS, S_OVPAGES, S_BIT0, S_PROBLEMS = 27, S_FIRST,
       S_LISTED, S_LEAKED, S_OV_OK };

using ull = unsigned long long;

// the tree check's node word 0: parent | depth << 32 | tree << 40 | type << 48 | bits << 56
__device__ inline bool tree_reached(uint64_t w) { return (uint32_t)w != kTreeNoPage; }
__device__ inline bool tree_good_data(uint64_t w) {
    return tree_reached(w) && ((uint32_t)(w >> 48) & 0xFF) == kTreeData && ((uint32_t)(w >> 56) & kTreeSixBits) == 0;
}
// leaf node word 0: owner | owner_entry << 32 | bits << 48; word 1: a | b << 32
__device__ inline uint64_t leaf_word0(uint32_t owner, uint32_t entry, uint32_t bits) {
    return (uint64_t)owner | (uint64_t)entry << 32 | (uint64_t)bits << 48;
}

__device__ inline uint64_t leaf_wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline uint32_t leaf_wave_or(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}
__device__ inline uint64_t leaf_wave_max(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// exclusive sum of v over the 256 threads of a block, total = the block's sum
__device__ inline uint64_t leaf_block_scan(uint64_t v, uint64_t* w4, uint64_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();  // w4 may still be read from the round before
    if (lane == 63) w4[w] = inc;
    __syncthreads();
    uint64_t before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < w) before += w4[k];
        total += w4[k];
    }
    return before + inc - v;
}

// where row p's page lies in the window; false when the row maps no page of it
__device__ inline bool leaf_in_window(uint64_t v, uint64_t fp_first, uint64_t n_pages, uint64_t& idx) {
    if ((v & 7) != 1) return false;
    const uint64_t fp = v >> 3;
    if (fp < fp_first || fp - fp_first >= n_pages) return false;
    idx = fp - fp_first;
    return true;
}

// Row c as a chain page, from the table, the class bytes and the page alone:
// the first of the six bits that applies, else 0 with V, n and the page.
__device__ inline uint32_t leaf_classify(uint32_t c, const uint8_t* __restrict__ pages, uint32_t P, uint64_t n_pages,
                                         uint64_t fp_first, const uint8_t* __restrict__ cls,
                                         const uint64_t* __restrict__ table, uint32_t& V, uint32_t& n,
                                         const uint8_t*& pg) {
    const uint64_t v = table[c];
    uint64_t idx = 0;
    V = n = 0;
    pg = nullptr;
    if ((v & 7) != 1) return PCS_TREE_UNMAPPED;
    if (!leaf_in_window(v, fp_first, n_pages, idx) || cls[idx] > PCS_PAGE_BLANK) return PCS_TREE_ABSENT;
    if (cls[idx] == PCS_PAGE_BLANK) return PCS_TREE_BLANK;
    if (cls[idx] == PCS_PAGE_CORRUPT) return PCS_TREE_CORRUPT;
    pg = pages + idx * P;
    if (pg[kTreeTypeOffset] != kLeafOverflow) return PCS_TREE_WRONG_TYPE;
    if (!leaf_overflow_page(pg, P, V, n)) {
        V = n = 0;
        return PCS_TREE_MALFORMED;
    }
    return 0;
}

__global__ __launch_bounds__(256) void k_leaf_init(uint64_t rows, ull* __restrict__ key, uint32_t* __restrict__ refs,
                                                  uint64_t* __restrict__ leaves, uint64_t* __restrict__ ctl) {
    if (blockIdx.x == 0 && threadIdx.x < kLeafCtlWords) ctl[threadIdx.x] = threadIdx.x == S_FIRST ? ~0ull : 0ull;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < rows; p += stride) {
        key[p] = ~0ull;
        refs[p] = 0;
        leaves[2 * p] = kLeafNothing;
        leaves[2 * p + 1] = 0;
    }
}

// per-lane counters of the walk, summed over the wave when the kernel ends
struct LeafCounts {
    uint64_t entries = 0, values = 0, expiring = 0, compressed = 0, inline_bytes = 0, refs = 0, oor = 0, to_tree = 0,
             misplaced = 0, capped = 0, max_groups = 0;
};

__global__ __launch_bounds__(256) void k_leaf_walk(const uint8_t* __restrict__ pages, uint32_t P, uint64_t n_pages,
                                                  uint64_t fp_first, const uint8_t* __restrict__ cls,
                                                  const uint64_t* __restrict__ table, uint64_t rows,
                                                  const uint64_t* __restrict__ tree_nodes, ull* __restrict__ key,
                                                  uint32_t* __restrict__ refs, uint64_t* __restrict__ leaves,
                                                  uint64_t* __restrict__ ctl) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLeafWaves][kLeafLdsPage + 16];
    const int w = threadIdx.x >> 6;
    const uint32_t lane = threadIdx.x & 63;
    const bool staged = P <= kLeafLdsPage;
    LeafCounts cnt;
    // the trip count is the same for the four waves of a block, so the barriers below are met by all
    for (uint64_t p0 = (uint64_t)blockIdx.x * kLeafWaves; p0 < rows; p0 += (uint64_t)gridDim.x * kLeafWaves) {
        const uint64_t p = p0 + w;
        // uniform over the wave; a page the tree check read lies in the window with class byte 1, and
        // nodes that say otherwise (not this table's) make no page readable
        uint64_t idx = 0;
        const bool have = p < rows && tree_good_data(tree_nodes[2 * p]) &&
                          leaf_in_window(table[p], fp_first, n_pages, idx) && cls[idx] == PCS_PAGE_OK;
        const uint8_t* src = have ? pages + idx * P : nullptr;
        if (staged) {
            if (have) src = stage_page_lds(src, P, lane, lds[w]);
            __syncthreads();
        }
        if (have) {
            uint32_t R = 0, E = 0, dbits = 0;
            uint64_t page_entries = 0, page_values = 0;
            bool ok = leaf_data_header(src, P, R, E);  // uniform
            if (ok) {
                for (uint32_t k = lane; k < R; k += 64) {
                    uint32_t lo, hi;
                    if (!leaf_region_bounds(src, R, E, k, lo, hi) ||
                        leaf_region_decode(src, lo, hi, [](const LeafEntry&) {}) < 0) {
                        ok = false;
                        break;
                    }
                }
            }
            ok = __ballot(!ok) == 0;
            if (!ok) {
                dbits = PCS_TREE_MALFORMED;
            } else {
                for (uint32_t k0 = 0; k0 < R; k0 += 64) {  // uniform
                    uint32_t pos = 0, hi = 0;
                    if (k0 + lane < R) leaf_region_bounds(src, R, E, k0 + lane, pos, hi);
                    for (;;) {
                        // every lane moves to the next overflow entry of its region
                        LeafEntry e;
                        bool found = false;
                        while (pos < hi && !found) {
                            // validated above, so the previous key's length is not needed
                            if (!leaf_entry_decode(src, pos, hi, ~0ull, e)) {
                                pos = hi;
                                break;
                            }
                            ++page_entries;
                            if (e.flags & kLeafFlagExpire) ++cnt.expiring;
                            if (e.flags & kLeafFlagCompression) ++cnt.compressed;
                            if (e.flags & kLeafFlagOverflow) found = true;
                            else cnt.inline_bytes += e.value_len;
                        }
                        uint64_t todo = __ballot(found);
                        if (!todo) break;
                        if (found) ++page_values;
                        while (todo) {  // one value at a time, the whole wave on its chain
                            const int from = __ffsll((long long)todo) - 1;
                            todo &= todo - 1;
                            const uint32_t e_off = __shfl(found ? e.offset : 0u, from, 64);
                            const uint32_t e_val = __shfl(found ? e.value_offset : 0u, from, 64);
                            uint32_t n = __shfl(found ? e.value_len : 0u, from, 64) / 4;
                            const ull bid_key = (ull)p << 32 | (ull)e_off << 16;
                            const uint8_t* group = src + e_val;  // n LE32 pointers
                            uint64_t groups = 0;
                            for (;;) {
                                if (groups == PCS_LEAF_MAX_GROUPS) {
                                    if (lane == 0) ++cnt.capped;
                                    dbits |= PCS_LEAF_BAD_CHAIN;
                                    break;
                                }
                                ++groups;
                                uint32_t next_n = 0;  // set by the lane that holds the group's last pointer
                                uint64_t next_group = 0;
                                for (uint32_t j = lane; j < n; j += 64) {
                                    const uint32_t c = tree_le32(group + 4 * j);
                                    ++cnt.refs;
                                    if (c >= rows) {
                                        ++cnt.oor;
                                        dbits |= PCS_LEAF_BAD_POINTER;
                                    } else if (tree_reached(tree_nodes[2 * (uint64_t)c])) {
                                        ++cnt.to_tree;
                                        dbits |= PCS_LEAF_BAD_CHAIN;
                                    } else {
                                        atomicMin(key + c, bid_key);
                                        atomicAdd(refs + c, 1u);
                                        uint32_t V, nc;
                                        const uint8_t* pg;
                                        const uint32_t cb = leaf_classify(c, pages, P, n_pages, fp_first, cls, table, V, nc, pg);
                                        // the same words from every bidder: the row's bits and V | n << 16
                                        reinterpret_cast<uint16_t*>(leaves)[8 * (uint64_t)c + 3] = (uint16_t)cb;
                                        reinterpret_cast<uint32_t*>(leaves)[4 * (uint64_t)c + 3] = V | nc << 16;
                                        if (cb) {
                                            dbits |= PCS_LEAF_BAD_CHAIN;
                                        } else if (nc) {
                                            if (j + 1 != n) {
                                                ++cnt.misplaced;
                                                dbits |= PCS_LEAF_BAD_CHAIN;
                                            } else {
                                                next_n = nc;
                                                next_group = reinterpret_cast<uint64_t>(pg + leaf_pointer_offset(P, nc));
                                            }
                                        }
                                    }
                                }
                                const int last = (int)((n - 1) & 63);
                                n = __shfl(next_n, last, 64);
                                if (!n) break;
                                group = reinterpret_cast<const uint8_t*>(__shfl(next_group, last, 64));
                            }
                            if (groups > cnt.max_groups) cnt.max_groups = groups;
                        }
                    }
                }
                page_entries = leaf_wave_sum(page_entries);
                page_values = leaf_wave_sum(page_values);
                if (lane == 0) {
                    cnt.entries += page_entries;
                    cnt.values += page_values;
                }
            }
            dbits = leaf_wave_or(dbits);
            if (lane == 0) {
                leaves[2 * p] = leaf_word0((uint32_t)p, 0, dbits);
                leaves[2 * p + 1] = (uint64_t)(uint32_t)page_entries | page_values << 32;
            }
        }
        if (staged) __syncthreads();  // the next page of this wave overwrites its slot
    }
    const uint64_t sums[10] = {cnt.entries, cnt.values, cnt.expiring, cnt.compressed, cnt.inline_bytes,
                               cnt.refs,    cnt.oor,    cnt.to_tree,  cnt.misplaced,  cnt.capped};
    const int where[10] = {S_ENTRIES, S_VALUES, S_EXPIRING, S_COMPRESSED, S_INLINE, S_REFS, S_OOR, S_TOTREE, S_MISPLACED,
                           S_CAPPED};
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t v = leaf_wave_sum(sums[i]);
        if (lane == 0 && v) atomicAdd(reinterpret_cast<ull*>(ctl + where[i]), (ull)v);
    }
    const uint64_t mg = leaf_wave_max(cnt.max_groups);
    if (lane == 0 && mg) atomicMax(reinterpret_cast<ull*>(ctl + S_MAXGROUPS), (ull)mg);
}

__global__ __launch_bounds__(256) void k_leaf_count(const uint8_t* __restrict__ pages, uint32_t P, uint64_t n_pages,
                                                   uint64_t fp_first, const uint8_t* __restrict__ cls,
                                                   const uint64_t* __restrict__ table, uint64_t rows,
                                                   const uint64_t* __restrict__ tree_nodes,
                                                   const ull* __restrict__ key, const uint32_t* __restrict__ refs,
                                                   uint64_t* __restrict__ leaves, uint64_t* __restrict__ ctl,
                                                   uint32_t* __restrict__ blk) {
    __shared__ ull acc[kLeafCtlWords];
    if (threadIdx.x < kLeafCtlWords) acc[threadIdx.x] = threadIdx.x == S_FIRST ? ~0ull : 0ull;
    __syncthreads();
    const uint64_t p0 = (uint64_t)blockIdx.x * kLeafSpan + threadIdx.x * 4u;
    for (int k = 0; k < 4; ++k) {
        const uint64_t p = p0 + k;
        if (p >= rows) break;
        const uint64_t tw = tree_nodes[2 * p];
        uint32_t bits;
        if (tree_good_data(tw)) {  // written whole by its wave
            bits = (uint32_t)(leaves[2 * p] >> 48);
            atomicAdd(&acc[S_DATA], 1ull);
            if (!bits) atomicAdd(&acc[S_DATA_OK], 1ull);
        } else if (key[p] != ~0ull) {  // claimed: bits and V | n << 16 are in place
            const ull kw = key[p];
            const uint32_t r = refs[p], vn = (uint32_t)(leaves[2 * p + 1] >> 32);
            bits = (uint32_t)(leaves[2 * p] >> 48) | (r > 1 ? PCS_LEAF_SHARED : 0u);
            leaves[2 * p] = leaf_word0((uint32_t)(kw >> 32), (uint32_t)(kw >> 16) & 0xFFFFu, bits);
            leaves[2 * p + 1] = (uint64_t)r | (uint64_t)vn << 32;
            atomicAdd(&acc[S_OVPAGES], 1ull);
            if (!(bits & kTreeSixBits)) atomicAdd(&acc[S_OVBYTES], (ull)(vn & 0xFFFFu));
            if (!bits) atomicAdd(&acc[S_OV_OK], 1ull);
        } else {
            uint64_t idx = 0;
            if (!tree_reached(tw) && leaf_in_window(table[p], fp_first, n_pages, idx) && cls[idx] == PCS_PAGE_OK &&
                pages[idx * P + kTreeTypeOffset] == kLeafOverflow)
                atomicAdd(&acc[S_LEAKED], 1ull);
            continue;
        }
        if (bits) {
            for (int b = 0; b < 9; ++b)
                if (bits >> b & 1) atomicAdd(&acc[S_BIT0 + b], 1ull);
            atomicAdd(&acc[S_PROBLEMS], 1ull);
            atomicMin(&acc[S_FIRST], (ull)p);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = (uint32_t)acc[S_PROBLEMS];
    if (threadIdx.x < kLeafCtlWords) {
        ull* g = reinterpret_cast<ull*>(ctl + threadIdx.x);
        const ull a = acc[threadIdx.x];
        if (threadIdx.x == S_FIRST) {
            if (a != ~0ull) atomicMin(g, a);
        } else if (a) {
            atomicAdd(g, a);
        }
    }
}

__global__ __launch_bounds__(256) void k_leaf_scan(const uint32_t* __restrict__ blk, uint64_t nblocks, uint64_t n_pages,
                                                  uint64_t rows, uint64_t cap, const uint64_t* __restrict__ ctl,
                                                  uint64_t* __restrict__ rank, uint64_t* __restrict__ summary) {
    __shared__ uint64_t w4[4];
    uint64_t problems = 0;  // in the spans before this round (uniform)
    for (uint64_t base = 0; base < nblocks; base += 256) {
        const uint64_t b = base + threadIdx.x;
        uint64_t total;
        const uint64_t before = leaf_block_scan(b < nblocks ? blk[b] : 0, w4, total);
        if (b < nblocks) rank[b] = problems + before;
        problems += total;
    }
    if (threadIdx.x < kLeafCtlWords) {
        const int i = threadIdx.x;
        uint64_t v = ctl[i];
        switch (i) {
            case S_PAGES: v = n_pages; break;
            case S_ROWS: v = rows; break;
            case S_EXTRA: v = ctl[S_REFS] - ctl[S_OOR] - ctl[S_TOTREE] - ctl[S_OVPAGES]; break;
            case S_LISTED: v = problems < cap ? problems : cap; break;
            default: break;
        }
        summary[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_leaf_list(const uint64_t* __restrict__ leaves, uint64_t rows,
                                                  const uint32_t* __restrict__ blk, const uint64_t* __restrict__ rank,
                                                  uint64_t cap, uint64_t* __restrict__ list) {
    __shared__ uint64_t w4[4];
    const uint64_t r0 = rank[blockIdx.x];
    if (blk[blockIdx.x] == 0 || r0 >= cap) return;  // uniform over the block
    const uint64_t p0 = (uint64_t)blockIdx.x * kLeafSpan + threadIdx.x * 4u;
    uint64_t w[4];
    uint32_t mask = 0;
    for (int k = 0; k < 4; ++k) {
        w[k] = p0 + k < rows ? leaves[2 * (p0 + k)] : kLeafNothing;
        if (w[k] >> 48) mask |= 1u << k;  // rows that are neither checked nor claimed have no bits
    }
    uint64_t total;
    uint64_t pos = r0 + leaf_block_scan(__builtin_popcount(mask), w4, total);
    for (int k = 0; k < 4; ++k) {
        if (!(mask >> k & 1) || pos >= cap) continue;
        list[2 * pos] = (p0 + k) | (w[k] & 0xFFFFFFFFull) << 32;               // pcs_leaf_problem: page_id, owner,
        list[2 * pos + 1] = (w[k] >> 48) | ((w[k] >> 32) & 0xFFFFull) << 32;  // bits, owner_entry
        ++pos;
    }
}

}  // namespace

hipError_t run_leaf_check(const uint8_t* pages, uint64_t page_size, uint64_t n_pages, uint64_t fp_first,
                          const uint8_t* cls, const uint64_t* table, uint64_t rows, const uint64_t* tree_nodes,
                          uint64_t* leaves, uint64_t* summary, uint64_t* list, uint64_t cap, hipStream_t s) {
    if (rows > 0xFFFFFFFFull || page_size < 32 || page_size > 65535 || (rows && !tree_nodes)) return hipErrorInvalidValue;
    const uint32_t P = (uint32_t)page_size;
    const uint64_t nblocks = (rows + kLeafSpan - 1) / kLeafSpan;
    // control words, ranks, span counts, keys, reference counts and (when the caller wants none) the leaf nodes
    const uint64_t blk_bytes = (nblocks * 4 + 7) & ~7ull, refs_bytes = (rows * 4 + 7) & ~7ull;
    void* buf = nullptr;
    int id = -1;
    hipError_t e = scratch_acquire(kLeafCtlWords * 8 + nblocks * 8 + blk_bytes + rows * 8 + refs_bytes +
                                       (leaves ? 0 : rows * 16) + 8,
                                   &buf, &id);
    if (e != hipSuccess) return e;
    uint64_t* ctl = static_cast<uint64_t*>(buf);
    uint64_t* rank = ctl + kLeafCtlWords;
    uint32_t* blk = reinterpret_cast<uint32_t*>(rank + nblocks);
    ull* key = reinterpret_cast<ull*>(reinterpret_cast<uint8_t*>(blk) + blk_bytes);
    uint32_t* refs = reinterpret_cast<uint32_t*>(key + rows);
    if (!leaves) leaves = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(refs) + refs_bytes);
    const unsigned row_grid = (unsigned)(rows ? (rows + 255) / 256 < 2048 ? (rows + 255) / 256 : 2048 : 1);
    const unsigned walk_grid = (unsigned)(rows ? (rows + kLeafWaves - 1) / kLeafWaves < 1024 ? (rows + kLeafWaves - 1) / kLeafWaves : 1024 : 1);
    auto launched = [&]() { return (e = hipGetLastError()) == hipSuccess; };
    do {
        hipLaunchKernelGGL(k_leaf_init, dim3(row_grid), dim3(256), 0, s, rows, key, refs, leaves, ctl);
        if (!launched()) break;
        if (rows) {
            hipLaunchKernelGGL(k_leaf_walk, dim3(walk_grid), dim3(256), 0, s, pages, P, n_pages, fp_first, cls, table, rows,
                               tree_nodes, key, refs, leaves, ctl);
            if (!launched()) break;
            hipLaunchKernelGGL(k_leaf_count, dim3((unsigned)nblocks), dim3(256), 0, s, pages, P, n_pages, fp_first, cls,
                               table, rows, tree_nodes, key, refs, leaves, ctl, blk);
            if (!launched()) break;
        }
        hipLaunchKernelGGL(k_leaf_scan, dim3(1), dim3(256), 0, s, blk, nblocks, n_pages, rows, cap, ctl, rank, summary);
        if (!launched()) break;
        if (rows && cap) {
            hipLaunchKernelGGL(k_leaf_list, dim3((unsigned)nblocks), dim3(256), 0, s, leaves, rows, blk, rank, cap, list);
            if (!launched()) break;
        }
    } while (false);
    (void)scratch_release(id, s);
    return e;
}

}  // namespace pcs
