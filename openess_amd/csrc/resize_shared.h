// Pieces of the bilinear resampling kernels that more than one translation unit launches (resize_ops.hip, headpool_f32.hip):
// the 16-byte typed row access, the y pass of the bilinear adjoint, the S x C quotient table of the pooled backward and the
// host-side grid / alignment helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess_common.h"
#include "bilinear_axis.h"

namespace oess {
constexpr int RESIZE_THREADS = 256;

// ---- VEC-wide typed access: bf16 x8 / fp32 x4 as one 16-byte access, or scalars
template <bool BF16, int VEC>
__device__ __forceinline__ void loadv(const void* base, int64_t off, float (&v)[VEC]) {
    if constexpr (BF16 && VEC == 8) {
        union { uint4 q; uint16_t h[8]; } u;
        u.q = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(base) + off);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = bf16_to_f32(u.h[k]);
    } else if constexpr (!BF16 && VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + off);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if constexpr (!BF16 && VEC == 8) {
        const float4 q = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + off);
        const float4 r = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + off + 4);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; v[4] = r.x; v[5] = r.y; v[6] = r.z; v[7] = r.w;
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            v[k] = BF16 ? bf16_to_f32(reinterpret_cast<const uint16_t*>(base)[off + k]) : reinterpret_cast<const float*>(base)[off + k];
    }
}
template <bool BF16, int VEC>
__device__ __forceinline__ void storev(void* base, int64_t off, const float (&v)[VEC]) {
    if constexpr (BF16 && VEC == 8) {
        *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(base) + off) = pack_bf16x8(v);
    } else if constexpr (!BF16 && VEC == 4) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + off) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (!BF16 && VEC == 8) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + off) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + off + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if constexpr (BF16) reinterpret_cast<uint16_t*>(base)[off + k] = f32_to_bf16(v[k]);
            else reinterpret_cast<float*>(base)[off + k] = v[k];
        }
    }
}

// backward pass 2 (y): gin[b, iy, ix, c] = sum_oy w(oy -> iy) * tmp[b, oy, ix, c]
template <bool BF16, int VEC>
static __global__ __launch_bounds__(RESIZE_THREADS) void resize_bwd_y_kernel(const float* __restrict__ tmp, int B, int C, Axis ay, Axis ax,
                                                               void* __restrict__ gin, int64_t gps) {
    const int cv = C / VEC;
    const int iy = blockIdx.x % ay.in;
    const int64_t b = blockIdx.x / ay.in;
    int lo, hi;
    candidates(ay, iy, lo, hi);
    const int n = ax.in * cv;
    for (int j = threadIdx.x; j < n; j += RESIZE_THREADS) {
        const int ix = j / cv, c = (j - ix * cv) * VEC;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        for (int oy = lo; oy <= hi; ++oy) {
            const float w = weight_for(ay, oy, iy);
            if (w != 0.f) {
                float g[VEC];
                loadv<false, (VEC == 8 ? 8 : VEC)>(tmp, ((b * ay.out + oy) * ax.in + ix) * (int64_t)C + c, g);
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[k] += w * g[k];
            }
        }
        storev<BF16, VEC>(gin, ((b * ay.in + iy) * ax.in + ix) * gps + c, acc);
    }
}

static __global__ __launch_bounds__(RESIZE_THREADS) void pool_table_kernel(const float* __restrict__ gk, const float* __restrict__ count, int S, int C,
                                                             float* __restrict__ table) {
    const int64_t n = (int64_t)S * C;
    for (int64_t i = (int64_t)blockIdx.x * RESIZE_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * RESIZE_THREADS)
        table[i] = gk[i] / __fadd_rn(count[i / C], 1e-6f);
}

static inline unsigned grid_for(int64_t work) {
    int64_t g = (work + RESIZE_THREADS - 1) / RESIZE_THREADS;
    if (g < 1) g = 1;
    if (g > 262144) g = 262144;
    return (unsigned)g;
}
// 16-byte vector path only when every access is aligned
static inline bool vec_ok(const void* p, long long ps, int C, int is_bf16) {
    const int v = is_bf16 ? 8 : 4;
    return (C % v) == 0 && (ps % v) == 0 && ((uintptr_t)p & 15) == 0;
}

}  // namespace oess
