// K29 CLIP text tower in fp32: the two kernels of it that are no token kernel of vit_f32.hip / conv_f32.hip (the causal attention
// and the end-of-text LayerNorm are instances there, QuickGELU an epilogue of the token GEMM):
//   * token + position embedding: x[n L + t, :] = table[ids[n, t], :] + pos[t, :], one fp32 add per element (exact), 16-byte
//     accesses when C % 4 == 0 and everything is 16-byte aligned;
//   * prompt ensemble: out[k] = normalize(sum over the prompts n of class k of normalize(e[n])), one wave per class, the prompts
//     of a class added in their order, norms by a true sqrtf and a true division.
// No atomics; results repeat bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"

namespace {
using namespace oess;
constexpr int THREADS = 256;

// one thread per VEC consecutive channels of one output row; an id outside [0, V) (the wrapper refuses them) reads no table row
// and gives a NaN row
template <int VEC>
__global__ __launch_bounds__(THREADS) void embed_kernel(const int64_t* __restrict__ ids, int64_t rows, int L, const float* __restrict__ table,
                                                        int64_t ts, int V, int C, const float* __restrict__ pos, int64_t ps,
                                                        float* __restrict__ out, int64_t os) {
    const int per = C / VEC;
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= rows * per) return;
    const int64_t r = e / per;
    const int c = (int)(e - r * per) * VEC;
    const int t = (int)(r % L);
    const int64_t id = ids[r];
    const bool ok = id >= 0 && id < V;
    const float* tp = table + (ok ? id : 0) * ts + c;
    const float* pp = pos + t * ps + c;
    float* op = out + r * os + c;
    if (VEC == 4) {
        const float4 a = *reinterpret_cast<const float4*>(tp), b = *reinterpret_cast<const float4*>(pp);
        float4 o = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        if (!ok) o = make_float4(NAN, NAN, NAN, NAN);
        *reinterpret_cast<float4*>(op) = o;
    } else {
        *op = ok ? *tp + *pp : NAN;
    }
}

// one wave per class; lane handles channels lane, lane + 64, ...  (D <= 64 * 32)
__global__ __launch_bounds__(THREADS) void prompt_mean_kernel(const float* __restrict__ e, int64_t es, int D, const int64_t* __restrict__ offsets,
                                                              int K, float* __restrict__ out, int64_t os) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int MAXE = 32;
    const int k = blockIdx.x * (THREADS / 64) + wave;
    if (k >= K) return;
    const int64_t n0 = offsets[k], n1 = offsets[k + 1];
    float acc[MAXE];
#pragma unroll
    for (int i = 0; i < MAXE; ++i) acc[i] = 0.f;
    for (int64_t n = n0; n < n1; ++n) {                      // prompt order
        float v[MAXE];
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MAXE; ++i) {
            v[i] = 0.f;
            if (i * 64 < D) { const int c = i * 64 + lane; if (c < D) { v[i] = e[n * es + c]; q += v[i] * v[i]; } }
        }
        const float norm = sqrtf(wave_sum(q));
#pragma unroll
        for (int i = 0; i < MAXE; ++i)
            if (i * 64 < D) acc[i] += v[i] / norm;
    }
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXE; ++i)
        if (i * 64 < D) q += acc[i] * acc[i];                // channels past D hold 0
    const float norm = sqrtf(wave_sum(q));
#pragma unroll
    for (int i = 0; i < MAXE; ++i)
        if (i * 64 < D) { const int c = i * 64 + lane; if (c < D) out[k * os + c] = acc[i] / norm; }
}
}  // namespace

extern "C" {

int oess_clip_text_embed_f32(const int64_t* ids, int N, int L, const float* table, long long table_row_stride, int V, int C,
                             const float* pos, long long pos_row_stride, float* out, long long out_row_stride, oess_stream_t stream) {
    if (!ids || !table || !pos || !out || N <= 0 || L <= 0 || V <= 0 || C <= 0 || C > (1 << 20)) return OESS_EINVAL;
    if (table_row_stride < C || pos_row_stride < C || out_row_stride < C) return OESS_EINVAL;
    if ((((uintptr_t)table | (uintptr_t)pos | (uintptr_t)out) & 3) != 0 || ((uintptr_t)ids & 7) != 0) return OESS_EINVAL;
    if ((long long)N * L >= (1ll << 31) || table_row_stride >= (1ll << 31) || pos_row_stride >= (1ll << 31) ||
        out_row_stride >= (1ll << 31))
        return OESS_EINVAL;
    const int64_t rows = (int64_t)N * L;
    const bool vec = (C & 3) == 0 && ((table_row_stride | pos_row_stride | out_row_stride) & 3) == 0 &&
                     ((((uintptr_t)table | (uintptr_t)pos | (uintptr_t)out)) & 15) == 0;
    const int64_t g = (rows * (vec ? C / 4 : C) + THREADS - 1) / THREADS;
    if (g > 0x7fffffffll) return OESS_EINVAL;
    if (vec)
        hipLaunchKernelGGL(embed_kernel<4>, dim3((unsigned)g), dim3(THREADS), 0, (hipStream_t)stream, ids, rows, L, table,
                           (int64_t)table_row_stride, V, C, pos, (int64_t)pos_row_stride, out, (int64_t)out_row_stride);
    else
        hipLaunchKernelGGL(embed_kernel<1>, dim3((unsigned)g), dim3(THREADS), 0, (hipStream_t)stream, ids, rows, L, table,
                           (int64_t)table_row_stride, V, C, pos, (int64_t)pos_row_stride, out, (int64_t)out_row_stride);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_prompt_mean_normalize_f32(const float* e, long long e_row_stride, int64_t N, int D, const int64_t* host_offsets,
                                   const int64_t* dev_offsets, int K, float* out, long long out_row_stride, oess_stream_t stream) {
    if (!e || !host_offsets || !dev_offsets || !out || N <= 0 || N >= (1ll << 31) || D <= 0 || D > 2048 || K <= 0) return OESS_EINVAL;
    if (e_row_stride < D || out_row_stride < D || e_row_stride >= (1ll << 31) || out_row_stride >= (1ll << 31)) return OESS_EINVAL;
    if ((((uintptr_t)e | (uintptr_t)out) & 3) != 0 || (((uintptr_t)host_offsets | (uintptr_t)dev_offsets) & 7) != 0) return OESS_EINVAL;
    if (host_offsets[0] != 0 || host_offsets[K] != N) return OESS_EINVAL;
    for (int k = 0; k < K; ++k)
        if (host_offsets[k + 1] <= host_offsets[k]) return OESS_EINVAL;      // ascending, no empty class
    hipLaunchKernelGGL(prompt_mean_kernel, dim3((unsigned)((K + 3) / 4)), dim3(THREADS), 0, (hipStream_t)stream, e, (int64_t)e_row_stride,
                       D, dev_offsets, K, out, (int64_t)out_row_stride);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
