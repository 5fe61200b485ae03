// tree_check.hip — kernels of the tree check (pcs_tree_check_dev): a
// level-synchronous breadth-first walk of the index tree from the replayed
// roots.  The page rules are csrc/tree_check.h, compiled here for the device
// and by tests/cpp/tree_logic_test.cpp for the CPU.
//
//   k_tree_init    key[p] = UINT64_MAX, node[p] = "not reached", counters 0;
//   k_tree_roots   one thread: the roots claim depth 0 in tree order (of equal
//                  roots the lowest tree wins) and form level 0;
//   k_tree_level   x 17, one wavefront per page of the level: the claim's key
//                  gives depth and parent, the table row and the class byte say
//                  whether the page may be read, the type byte whether it fits;
//                  an index page of depth < 16 is staged in LDS (16-byte loads,
//                  pages up to kTreeLdsPage; larger ones are decoded from global
//                  memory), validated with a lane per restart region, and only
//                  when every region passed are its children bid with
//                  atomicMin(key[child], (depth + 1) << 32 | page).  The bidder
//                  that finds the key unclaimed appends the child to the
//                  frontier: once per page, in any order.  Bids of one level all
//                  carry the same depth, so the final key is the lowest parent
//                  of the smallest depth whatever the schedule, and it is final
//                  before the next level reads it;
//   k_tree_mark    one thread between two levels: where the next level ends;
//   k_tree_links   the sibling links of the reached healthy data pages;
//   k_tree_count   one block per kTreeSpan rows: the summary's counters
//                  (integer sums, so any order gives the same words) and the
//                  span's number of problems;
//   k_tree_scan    one block: each span's rank in the problem list, summary;
//   k_tree_list    the spans whose rank is below the cap write their problems
//                  at rank + position: ascending and the same on every call.
// Every grid and the number of launches follow from the arguments alone; a
// level whose frontier is empty returns at once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eloqstore_pcs_internal.h"
#include "page_stage.h"
#include "tree_check.h"

namespace pcs {
namespace {

constexpr int kTreeWaves = 4;               // pages in flight per workgroup
constexpr uint32_t kTreeLdsPage = 8192;     // pages up to this size are staged in LDS
constexpr uint32_t kTreeSpan = 1024;        // rows per block of the count and list passes
constexpr int kTreeLevels = PCS_TREE_MAX_DEPTH + 1;  // depths 0 .. 16 are classified, 0 .. 15 decoded
// control words: [0] frontier length, [1 + d] first frontier entry of level d
// ([1 + d + 1] its end), [kTreeAcc + i] accumulates summary word i
constexpr int kTreeLvl = 1, kTreeAcc = 24, kTreeCtlWords = kTreeAcc + 32;
constexpr uint64_t kTreeUnreached = 0x00FFFFFFFFFFFFFFull;  // parent, depth, tree, type all ones, bits 0
enum { S_PAGES, S_ROWS, S_MAPPED, S_REACHED, S_NONLEAF, S_LEAF, S_DATA, S_REFS, S_EXTRA, S_OOR, S_MAXDEPTH, S_CAPPED,
       S_BIT0, S_PROBLEMS = 20, S_FIRST, S_LISTED, S_UNREACHED, S_UTYPE0, S_UNREAD = 30, S_HEADS = 31 };

using ull = unsigned long long;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ inline uint32_t node_parent(uint64_t w) { return (uint32_t)w; }
__device__ inline uint32_t node_depth(uint64_t w) { return (uint32_t)(w >> 32) & 0xFF; }
__device__ inline uint32_t node_tree(uint64_t w) { return (uint32_t)(w >> 40) & 0xFF; }
__device__ inline uint32_t node_type(uint64_t w) { return (uint32_t)(w >> 48) & 0xFF; }
__device__ inline uint32_t node_bits(uint64_t w) { return (uint32_t)(w >> 56); }
__device__ inline uint64_t node_word(uint32_t parent, uint32_t depth, uint32_t tree, uint32_t type, uint32_t bits) {
    return (uint64_t)parent | (uint64_t)depth << 32 | (uint64_t)tree << 40 | (uint64_t)type << 48 | (uint64_t)bits << 56;
}

__device__ inline uint64_t tree_wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// exclusive sum of v over the 256 threads of a block, total = the block's sum
__device__ inline uint64_t tree_block_scan(uint64_t v, uint64_t* w4, uint64_t& total) {
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
__device__ inline bool tree_in_window(uint64_t v, uint64_t fp_first, uint64_t n_pages, uint64_t& idx) {
    if ((v & 7) != 1) return false;
    const uint64_t fp = v >> 3;
    if (fp < fp_first || fp - fp_first >= n_pages) return false;
    idx = fp - fp_first;
    return true;
}

__global__ __launch_bounds__(256) void k_tree_init(uint64_t rows, ull* __restrict__ key, uint64_t* __restrict__ nodes,
                                                  uint64_t* __restrict__ ctl) {
    if (blockIdx.x == 0 && threadIdx.x < kTreeCtlWords)
        ctl[threadIdx.x] = threadIdx.x == kTreeAcc + S_FIRST ? ~0ull : 0ull;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < rows; p += stride) {
        key[p] = ~0ull;
        nodes[2 * p] = kTreeUnreached;
        nodes[2 * p + 1] = 0;
    }
}

__global__ void k_tree_roots(const uint64_t* __restrict__ roots, uint32_t n_roots, uint64_t rows, ull* __restrict__ key,
                             uint64_t* __restrict__ nodes, uint32_t* __restrict__ frontier, uint64_t* __restrict__ ctl) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t count = 0, refs = 0, oor = 0;
    for (uint32_t t = 0; t < n_roots; ++t) {
        const uint64_t r = roots[t];
        if (r >= kTreeNoPage) continue;  // an empty tree
        ++refs;
        if (r >= rows) {
            ++oor;
            continue;
        }
        if (key[r] != ~0ull) continue;  // an equal root of a lower tree
        key[r] = r;                     // depth 0, its own parent
        nodes[2 * r] = node_word(kTreeNoPage, 0xFF, t, 0xFF, 0);  // the tree, for the level pass
        frontier[count++] = (uint32_t)r;
    }
    ctl[0] = count;
    ctl[kTreeLvl] = 0;
    ctl[kTreeLvl + 1] = count;
    ctl[kTreeAcc + S_REFS] = refs;
    ctl[kTreeAcc + S_OOR] = oor;
}

__global__ void k_tree_mark(uint32_t depth, uint64_t* __restrict__ ctl) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl[kTreeLvl + depth + 2] = ctl[0];
}

__global__ __launch_bounds__(256) void k_tree_level(uint32_t depth, const uint8_t* __restrict__ pages, uint32_t P,
                                                   uint64_t n_pages, uint64_t fp_first,
                                                   const uint8_t* __restrict__ cls, const uint64_t* __restrict__ table,
                                                   uint64_t rows, ull* __restrict__ key, uint64_t* __restrict__ nodes,
                                                   uint32_t* __restrict__ frontier, uint64_t* __restrict__ ctl) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kTreeWaves][kTreeLdsPage + 16];
    const uint64_t begin = ctl[kTreeLvl + depth], end = ctl[kTreeLvl + depth + 1];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool staged = P <= kTreeLdsPage;
    // the trip count is the same for the four waves of a block, so the barriers below are met by all
    for (uint64_t i0 = begin + (uint64_t)blockIdx.x * kTreeWaves; i0 < end; i0 += (uint64_t)gridDim.x * kTreeWaves) {
        const uint64_t i = i0 + w;
        const bool have = i < end;
        bool decode = false;
        const uint8_t* pg = nullptr;
        uint32_t c = 0, parent = 0, tree = 0, type = 0xFF, bits = 0;
        if (have) {  // uniform over the wave
            c = frontier[i];
            parent = (uint32_t)key[c];
            const uint64_t pw = nodes[2 * (uint64_t)(depth ? parent : c)];
            tree = node_tree(pw);
            const uint64_t v = table[c];
            uint64_t idx = 0;
            if ((v & 7) != 1) {
                bits = PCS_TREE_UNMAPPED;
            } else if (!tree_in_window(v, fp_first, n_pages, idx) || cls[idx] > PCS_PAGE_BLANK) {
                bits = PCS_TREE_ABSENT;
            } else if (cls[idx] == PCS_PAGE_BLANK) {
                bits = PCS_TREE_BLANK;
            } else if (cls[idx] == PCS_PAGE_CORRUPT) {
                bits = PCS_TREE_CORRUPT;
            } else {
                pg = pages + idx * P;
                type = pg[kTreeTypeOffset];
                if (!tree_type_fits(depth == 0, (uint8_t)node_type(pw), (uint8_t)type)) bits = PCS_TREE_WRONG_TYPE;
                else decode = type != kTreeData && depth < PCS_TREE_MAX_DEPTH;
            }
        }
        const uint8_t* src = pg;
        if (staged) {
            if (decode) src = stage_page_lds(pg, P, lane, lds[w]);
            __syncthreads();
        }
        uint64_t n_children = 0, n_bad = 0;
        if (decode) {
            uint32_t R = 0, E = 0;
            bool ok = tree_index_header(src, P, R, E);  // uniform
            if (ok) {
                for (uint32_t k = lane; k < R; k += 64) {
                    uint32_t lo, hi;
                    if (!tree_region_bounds(src, R, E, k, lo, hi) ||
                        tree_region_decode(src, lo, hi, [](uint32_t) {}) < 0) {
                        ok = false;
                        break;
                    }
                }
            }
            ok = __ballot(!ok) == 0;
            if (!ok) {
                bits = PCS_TREE_MALFORMED;
            } else {
                const ull bid_key = (ull)(depth + 1) << 32 | c;
                auto bid = [&](uint32_t child) {
                    if (child >= rows) {
                        ++n_bad;
                        return;
                    }
                    if (atomicMin(key + child, bid_key) == ~0ull)
                        frontier[atomicAdd(reinterpret_cast<ull*>(ctl), 1ull)] = child;
                };
                if (lane == 0) {
                    n_children = 1;
                    bid(tree_le32(src + kTreeLeftmostOffset));
                }
                for (uint32_t k = lane; k < R; k += 64) {
                    uint32_t lo, hi;
                    tree_region_bounds(src, R, E, k, lo, hi);
                    n_children += (uint64_t)tree_region_decode(src, lo, hi, bid);
                }
                n_children = tree_wave_sum(n_children);
                n_bad = tree_wave_sum(n_bad);
                if (n_bad) bits |= PCS_TREE_BAD_CHILD;
            }
        }
        if (have && lane == 0) {
            nodes[2 * (uint64_t)c] = node_word(parent, depth, tree, type, bits);
            nodes[2 * (uint64_t)c + 1] = n_children | n_bad << 32;
        }
        if (staged) __syncthreads();  // the next page of this wave overwrites its slot
    }
}

// a reached data page with none of the six bits that stop a walk
__device__ inline bool tree_good_data(uint64_t w) {
    return node_parent(w) != kTreeNoPage && node_type(w) == kTreeData && (node_bits(w) & kTreeSixBits) == 0;
}

__global__ __launch_bounds__(256) void k_tree_links(const uint8_t* __restrict__ pages, uint32_t P, uint64_t n_pages,
                                                   uint64_t fp_first, const uint64_t* __restrict__ table, uint64_t rows,
                                                   uint64_t* nodes, uint64_t* __restrict__ ctl) {
    uint64_t heads = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < rows; p += stride) {
        if (!tree_good_data(nodes[2 * p])) continue;
        uint64_t idx = 0;
        tree_in_window(table[p], fp_first, n_pages, idx);  // a page that was read lies in the window
        const uint8_t* pg = pages + idx * P;
        const uint32_t link[2] = {tree_le32(pg + kTreePrevOffset), tree_le32(pg + kTreeNextOffset)};
        if (link[0] == kTreeNoPage) ++heads;
        bool good = true;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const uint32_t q = link[side];
            if (q == kTreeNoPage) continue;
            bool holds = false;
            if (q < rows && tree_good_data(nodes[2 * (uint64_t)q])) {
                uint64_t qi = 0;
                tree_in_window(table[q], fp_first, n_pages, qi);
                // the neighbour's link back: its next for our prev, its prev for our next
                holds = tree_le32(pages + qi * P + (side == 0 ? kTreeNextOffset : kTreePrevOffset)) == (uint32_t)p;
            }
            good = good && holds;
        }
        // the bits byte alone: neighbours read this node's other bytes meanwhile
        if (!good) reinterpret_cast<uint8_t*>(nodes)[16 * p + 7] |= PCS_TREE_BAD_LINK;
    }
    heads = tree_wave_sum(heads);
    if ((threadIdx.x & 63) == 0 && heads) atomicAdd(reinterpret_cast<ull*>(ctl + kTreeAcc + S_HEADS), (ull)heads);
}

__global__ __launch_bounds__(256) void k_tree_count(const uint8_t* __restrict__ pages, uint32_t P, uint64_t n_pages,
                                                   uint64_t fp_first, const uint8_t* __restrict__ cls,
                                                   const uint64_t* __restrict__ table, uint64_t rows,
                                                   const uint64_t* __restrict__ nodes, uint64_t* __restrict__ ctl,
                                                   uint32_t* __restrict__ blk) {
    __shared__ ull acc[32];
    if (threadIdx.x < 32) acc[threadIdx.x] = threadIdx.x == S_FIRST ? ~0ull : 0ull;
    __syncthreads();
    const uint64_t p0 = (uint64_t)blockIdx.x * kTreeSpan + threadIdx.x * 4u;
    for (int k = 0; k < 4; ++k) {
        const uint64_t p = p0 + k;
        if (p >= rows) break;
        const uint64_t w = nodes[2 * p], w1 = nodes[2 * p + 1], v = table[p];
        const bool mapped = (v & 7) == 1;
        if (mapped) atomicAdd(&acc[S_MAPPED], 1ull);
        if (node_parent(w) == kTreeNoPage) {
            if (!mapped) continue;
            uint64_t idx = 0;
            if (tree_in_window(v, fp_first, n_pages, idx) && cls[idx] == PCS_PAGE_OK)
                atomicAdd(&acc[S_UTYPE0 + tree_type_bucket(pages[idx * P + kTreeTypeOffset])], 1ull);
            else
                atomicAdd(&acc[S_UNREAD], 1ull);
            continue;
        }
        const uint32_t bits = node_bits(w), type = node_type(w), depth = node_depth(w);
        atomicAdd(&acc[S_REACHED], 1ull);
        atomicMax(&acc[S_MAXDEPTH], (ull)depth + 1);
        atomicAdd(&acc[S_REFS], (ull)(uint32_t)w1);
        atomicAdd(&acc[S_OOR], (ull)(w1 >> 32));
        if (bits == 0) {
            if (type <= kTreeData) atomicAdd(&acc[S_NONLEAF + type], 1ull);
            if (type < kTreeData && depth == PCS_TREE_MAX_DEPTH) atomicAdd(&acc[S_CAPPED], 1ull);
        } else {
            for (int b = 0; b < 8; ++b)
                if (bits >> b & 1) atomicAdd(&acc[S_BIT0 + b], 1ull);
            atomicAdd(&acc[S_PROBLEMS], 1ull);
            atomicMin(&acc[S_FIRST], (ull)p);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = (uint32_t)acc[S_PROBLEMS];
    if (threadIdx.x < 32) {
        ull* g = reinterpret_cast<ull*>(ctl + kTreeAcc + threadIdx.x);
        const ull a = acc[threadIdx.x];
        if (threadIdx.x == S_FIRST) {
            if (a != ~0ull) atomicMin(g, a);
        } else if (threadIdx.x == S_MAXDEPTH) {
            if (a) atomicMax(g, a);
        } else if (a) {
            atomicAdd(g, a);
        }
    }
}

__global__ __launch_bounds__(256) void k_tree_scan(const uint32_t* __restrict__ blk, uint64_t nblocks, uint64_t n_pages,
                                                  uint64_t rows, uint64_t cap, const uint64_t* __restrict__ ctl,
                                                  uint64_t* __restrict__ rank, uint64_t* __restrict__ summary) {
    __shared__ uint64_t w4[4];
    uint64_t problems = 0;  // in the spans before this round (uniform)
    for (uint64_t base = 0; base < nblocks; base += 256) {
        const uint64_t b = base + threadIdx.x;
        uint64_t total;
        const uint64_t before = tree_block_scan(b < nblocks ? blk[b] : 0, w4, total);
        if (b < nblocks) rank[b] = problems + before;
        problems += total;
    }
    if (threadIdx.x < 32) {
        const int i = threadIdx.x;
        const uint64_t* a = ctl + kTreeAcc;
        uint64_t v = a[i];
        switch (i) {
            case S_PAGES: v = n_pages; break;
            case S_ROWS: v = rows; break;
            case S_EXTRA: v = a[S_REFS] - a[S_OOR] - a[S_REACHED]; break;
            case S_MAXDEPTH: v = v ? v - 1 : ~0ull; break;
            case S_LISTED: v = problems < cap ? problems : cap; break;
            case S_UNREACHED:
                v = a[S_UNREAD];
                for (int k = 0; k < 6; ++k) v += a[S_UTYPE0 + k];
                break;
            default: break;
        }
        summary[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_tree_list(const uint64_t* __restrict__ nodes, uint64_t rows,
                                                  const uint32_t* __restrict__ blk, const uint64_t* __restrict__ rank,
                                                  uint64_t cap, uint64_t* __restrict__ list) {
    __shared__ uint64_t w4[4];
    const uint64_t r0 = rank[blockIdx.x];
    if (blk[blockIdx.x] == 0 || r0 >= cap) return;  // uniform over the block
    const uint64_t p0 = (uint64_t)blockIdx.x * kTreeSpan + threadIdx.x * 4u;
    uint64_t w[4];
    uint32_t mask = 0;
    for (int k = 0; k < 4; ++k) {
        w[k] = p0 + k < rows ? nodes[2 * (p0 + k)] : kTreeUnreached;
        if (node_parent(w[k]) != kTreeNoPage && node_bits(w[k])) mask |= 1u << k;
    }
    uint64_t total;
    uint64_t pos = r0 + tree_block_scan(__builtin_popcount(mask), w4, total);
    for (int k = 0; k < 4; ++k) {
        if (!(mask >> k & 1) || pos >= cap) continue;
        list[2 * pos] = (p0 + k) | (uint64_t)node_parent(w[k]) << 32;  // pcs_tree_problem: page_id, parent,
        list[2 * pos + 1] = node_bits(w[k]) | (uint64_t)node_depth(w[k]) << 32;  // bits, depth
        ++pos;
    }
}

}  // namespace

hipError_t run_tree_check(const uint8_t* pages, uint64_t page_size, uint64_t n_pages, uint64_t fp_first,
                          const uint8_t* cls, const uint64_t* table, uint64_t rows, const uint64_t* roots,
                          uint32_t n_roots, uint64_t* nodes, uint64_t* summary, uint64_t* list, uint64_t cap,
                          hipStream_t s) {
    if (rows > 0xFFFFFFFFull || page_size < 32 || page_size > 65535 || n_roots < 1 || n_roots > 8)
        return hipErrorInvalidValue;
    const uint32_t P = (uint32_t)page_size;
    const uint64_t nblocks = (rows + kTreeSpan - 1) / kTreeSpan;
    // control words, ranks, span counts, keys, the frontier and (when the caller wants none) the nodes
    const uint64_t blk_bytes = (nblocks * 4 + 7) & ~7ull, frontier_bytes = (rows * 4 + 7) & ~7ull;
    void* buf = nullptr;
    int id = -1;
    hipError_t e = scratch_acquire(kTreeCtlWords * 8 + nblocks * 8 + blk_bytes + rows * 8 + frontier_bytes +
                                       (nodes ? 0 : rows * 16) + 8,
                                   &buf, &id);
    if (e != hipSuccess) return e;
    uint64_t* ctl = static_cast<uint64_t*>(buf);
    uint64_t* rank = ctl + kTreeCtlWords;
    uint32_t* blk = reinterpret_cast<uint32_t*>(rank + nblocks);
    ull* key = reinterpret_cast<ull*>(reinterpret_cast<uint8_t*>(blk) + blk_bytes);
    uint32_t* frontier = reinterpret_cast<uint32_t*>(key + rows);
    if (!nodes) nodes = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(frontier) + frontier_bytes);
    const unsigned row_grid = (unsigned)(rows ? (rows + 255) / 256 < 2048 ? (rows + 255) / 256 : 2048 : 1);
    const unsigned level_grid = (unsigned)(rows ? (rows + kTreeWaves - 1) / kTreeWaves < 1024 ? (rows + kTreeWaves - 1) / kTreeWaves : 1024 : 1);
    auto launched = [&]() { return (e = hipGetLastError()) == hipSuccess; };
    do {
        hipLaunchKernelGGL(k_tree_init, dim3(row_grid), dim3(256), 0, s, rows, key, nodes, ctl);
        if (!launched()) break;
        hipLaunchKernelGGL(k_tree_roots, dim3(1), dim3(64), 0, s, roots, n_roots, rows, key, nodes, frontier, ctl);
        if (!launched()) break;
        for (uint32_t d = 0; rows && d < (uint32_t)kTreeLevels; ++d) {
            hipLaunchKernelGGL(k_tree_level, dim3(level_grid), dim3(256), 0, s, d, pages, P, n_pages, fp_first, cls,
                               table, rows, key, nodes, frontier, ctl);
            if (!launched()) break;
            if (d + 1 < (uint32_t)kTreeLevels) {
                hipLaunchKernelGGL(k_tree_mark, dim3(1), dim3(64), 0, s, d, ctl);
                if (!launched()) break;
            }
        }
        if (e != hipSuccess) break;
        if (rows) {
            hipLaunchKernelGGL(k_tree_links, dim3(row_grid), dim3(256), 0, s, pages, P, n_pages, fp_first, table, rows,
                               nodes, ctl);
            if (!launched()) break;
            hipLaunchKernelGGL(k_tree_count, dim3((unsigned)nblocks), dim3(256), 0, s, pages, P, n_pages, fp_first, cls,
                               table, rows, nodes, ctl, blk);
            if (!launched()) break;
        }
        hipLaunchKernelGGL(k_tree_scan, dim3(1), dim3(256), 0, s, blk, nblocks, n_pages, rows, cap, ctl, rank, summary);
        if (!launched()) break;
        if (rows && cap) {
            hipLaunchKernelGGL(k_tree_list, dim3((unsigned)nblocks), dim3(256), 0, s, nodes, rows, blk, rank, cap, list);
            if (!launched()) break;
        }
    } while (false);
    (void)scratch_release(id, s);
    return e;
}

}  // namespace pcs
