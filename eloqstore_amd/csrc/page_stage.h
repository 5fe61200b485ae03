// page_stage.h — one wavefront copies one page into its LDS slot (device only;
// included by tree_check.hip and leaf_check.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pcs {

// Copies the P bytes at pg into slot (16-byte aligned, >= P + 16 bytes) with
// the 64 lanes of one wavefront and returns where byte 0 landed.  Page byte j
// goes to slot[off + j], off = the page's address mod 16: whole aligned 16-byte
// chunks inside the page move as one load, its head and tail bytewise.  The
// caller puts a barrier between this and the first read.
__device__ inline const uint8_t* stage_page_lds(const uint8_t* pg, uint32_t P, uint32_t lane, uint8_t* slot) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint32_t off = (uint32_t)(reinterpret_cast<uintptr_t>(pg) & 15);
    uint8_t* dst = slot + off;
    const uint32_t head = min(P, (16u - off) & 15u);
    const uint32_t chunks = (P - head) / 16;
    for (uint32_t q = lane; q < chunks; q += 64)
        *reinterpret_cast<u32x4*>(dst + head + 16 * q) = *reinterpret_cast<const u32x4*>(pg + head + 16 * q);
    const uint32_t tail0 = head + 16 * chunks;
    for (uint32_t j = lane; j < head + (P - tail0); j += 64) {
        const uint32_t b = j < head ? j : tail0 + (j - head);
        dst[b] = pg[b];
    }
    return dst;
}

}  // namespace pcs
