// The dropout mask shared by the bf16 kernel (small_ops.hip) and the fp32 kernel (deeplab_bwd_f32.hip): one Philox-4x32-10 call
// per group of 8 channels, one 16-bit lane per channel.  Both kernels take the keep decision from here, so the mask of element
// (pixel, c) under (seed, offset, P, C) does not depend on the storage type.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oess {

// Philox-4x32-10 (Salmon et al. 2011): counter = (element group, call offset), key = seed.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u; k.y += 0xBB67AE85u;
    }
    return c;
}

// the four random words of channel group i = pixel * (C / 8) + c / 8 (pixels in dense B H W order)
__device__ __forceinline__ uint4 dropout_words(int64_t i, unsigned long long seed, unsigned long long offset) {
    return philox4x32_10(make_uint4((uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)),
                         make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}

// keep rule of channel k = c % 8 of the group: its 16-bit lane against thr = (unsigned)(p * 65536 + 0.5)
__device__ __forceinline__ bool dropout_keep(const uint32_t (&w)[4], int k, unsigned thr) {
    return ((w[k >> 1] >> (16 * (k & 1))) & 0xffffu) >= thr;
}

// thr of a drop probability p in [0, 1)
static inline unsigned dropout_threshold(float p) { return (unsigned)(p * 65536.0f + 0.5f); }

}  // namespace oess
