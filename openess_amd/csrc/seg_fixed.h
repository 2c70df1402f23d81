// 2^-32 fixed-point partial sums of the superpixel scatter-mean (K7), shared by segmean_fwd_fx_kernel (reduce_ops.hip) and the
// fused fp32 head-pool forward (headpool_f32.hip): the conversion, the 96-bit global accumulator pair and the finalize kernel.
// Workspace layout of both (oess_segment_mean_fwd_workspace_bytes(S, Cf), zeroed by the caller's launch):
//   acc_lo u64[S * Cf] | acc_hi u64[S * Cf] | gcnt int[S] | err int
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oess {

typedef unsigned long long u64_t;
constexpr int SEG_FIN_THREADS = 256;
constexpr uint32_t SEG_RANGE_BITS = 0x47000000u;          // |x| >= 32768, inf or NaN as an fp32 bit pattern without its sign

__device__ __forceinline__ long long seg_to_fixed(float v) { return __float2ll_rn(v * 4294967296.0f); }

__device__ __forceinline__ void seg_global_add(u64_t* __restrict__ acc_lo, u64_t* __restrict__ acc_hi, int64_t idx, long long v) {
    if (v == 0) return;
    atomicAdd(&acc_lo[idx], (u64_t)v & 0xffffffffull);
    const long long hi = v >> 32;                                        // arithmetic shift: v = hi * 2^32 + lo, lo in [0, 2^32)
    if (hi != 0) atomicAdd(&acc_hi[idx], (u64_t)hi);
}

// k = fp32( (hi * 2^32 + lo) * 2^-32 ) / (count + 1e-6)   (pretrain_trainer.py:462); count as the fp32 row sum the reference forms
static __global__ __launch_bounds__(SEG_FIN_THREADS) void segmean_fx_finalize_kernel(const u64_t* __restrict__ acc_lo,
                                                                                    const u64_t* __restrict__ acc_hi,
                                                                                    const int* __restrict__ gcnt, const int* __restrict__ err,
                                                                                    float* __restrict__ k, float* __restrict__ count, int S,
                                                                                    int Cf) {
    const int64_t n = (int64_t)S * Cf;
    const bool bad = *err != 0;
    for (int64_t i = (int64_t)blockIdx.x * SEG_FIN_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SEG_FIN_THREADS) {
        const int64_t s = i / Cf;
        const double tot = (double)(long long)acc_hi[i] * 4294967296.0 + (double)acc_lo[i];
        const float sum = (float)(tot * (1.0 / 4294967296.0));
        const float cn = (float)gcnt[s];
        k[i] = bad ? __uint_as_float(0x7fc00000u) : sum / __fadd_rn(cn, 1e-6f);
        if (i - s * Cf == 0) count[s] = cn;
    }
}

static inline size_t seg_workspace_bytes(int S, int Cf) {
    if (S <= 0 || Cf <= 0) return 0;
    return ((size_t)S * Cf * 16 + (size_t)S * 4 + 4 + 15) / 16 * 16;
}

}  // namespace oess
