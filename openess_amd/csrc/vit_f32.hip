// K25 fp32 MaskCLIP ViT-B/16 inference: the token kernels of vit_ops.hip in the reference's arithmetic (the token GEMMs run on
// conv_f32.hip through oess_linear_tokens_f32):
//   * LayerNorm over the channel axis of an fp32 [rows x C] token matrix, two passes over the row held in registers;
//   * multi-head self attention softmax(Q K^T scale) V for head dimension 64 on the f32-input MFMA (v_mfma_f32_32x32x2_f32).
//
// Attention.  A wave owns 32 queries, a workgroup (4 waves) 128; keys come in tiles of 64 staged through LDS, the next tile's
// rows travelling HBM -> registers under the MFMAs.  Rows of a tile past L are zero-filled on load and their scores set to -inf.
//   S^T = K Q^T per 32-key block: A = K[key = lane & 31][d], B = Q[query = lane & 31][d], 32 MFMAs of k = 2; k-step j pairs
//     d = j (lanes 0 .. 31) with d = 32 + j (lanes 32 .. 63), so a lane's Q fragment is 32 consecutive floats of its row and its
//     K reads are 16-byte LDS reads.  Register e of lane (q, hi) is the score of key 8 (e >> 2) + 4 hi + (e & 3) (the 32 x 32
//     C/D map): a lane holds 2 x 16 scores of ITS query.
//   online softmax in fp32 per tile: m' = max(m, tile max), p = expf((s - m') scale), o and l rescaled by expf((m - m') scale);
//     l is summed from the unrounded p per half-wave and the halves are joined at the end.
//   O^T += V^T P^T per 32-key block: B = P^T needs k = lane >> 5, column = query; register e of lane (q, hi) IS that operand for
//     the k-step whose two keys are 8 (e >> 2) + (e & 3) and that + 4, so P never moves and is never rounded; the A lane
//     (d = lane & 31, hi) reads V[8 (e >> 2) + (e & 3) + 4 hi][d] (and d + 32 for the second accumulator) from the row-major
//     V tile.  16 k-steps x 2 accumulators per block.
//   out = o / l, a true division per element.
// Every product is a k-ordered fmaf chain; no atomics; results repeat bit for bit.
//
// K29 (CLIP's text tower): a causal instance of the attention kernel (oess_attention_d64_causal_f32) and the LayerNorm of the
// end-of-text row of each sequence (oess_clip_text_eot_layernorm_f32), which shares the row bodies of the LayerNorm kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"

namespace {
using namespace oess;
constexpr int THREADS = 256;

// one wave per row; lane handles channels lane, lane + 64, ...  (C <= 64 * 32)
__device__ __forceinline__ void layernorm_row(const float* __restrict__ xr, int C, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, float eps, float* __restrict__ yr, int lane) {
    constexpr int MAXE = 32;
    float v[MAXE];                                           // fully unrolled + uniform guards: stays in registers
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXE; ++i) {
        v[i] = 0.f;
        if (i * 64 < C) { const int c = i * 64 + lane; if (c < C) { v[i] = xr[c]; s += v[i]; } }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXE; ++i)
        if (i * 64 < C) { const int c = i * 64 + lane; if (c < C) { const float d = v[i] - mean; q += d * d; } }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);       // biased variance, like nn.LayerNorm
#pragma unroll
    for (int i = 0; i < MAXE; ++i)
        if (i * 64 < C) {
            const int c = i * 64 + lane;
            if (c < C) yr[c] = (v[i] - mean) * rstd * gamma[c] + beta[c];
        }
}

// Same, 16-byte accesses: lane owns the 4 channels of chunk lane, lane + 64, ...  (C % 4 == 0, 16-byte aligned rows)
__device__ __forceinline__ void layernorm_row_vec(const float* __restrict__ xr, int C, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, float eps, float* __restrict__ yr, int lane) {
    constexpr int MAXC = 8;                                  // chunks of 4 channels per lane: C <= 2048
    const int nchunk = C >> 2;
    float4 v[MAXC];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int ch = i * 64 + lane;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ch < nchunk) {
            v[i] = *reinterpret_cast<const float4*>(xr + ch * 4);
            s += v[i].x; s += v[i].y; s += v[i].z; s += v[i].w;
        }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
        if (i * 64 + lane < nchunk) {
            const float d0 = v[i].x - mean, d1 = v[i].y - mean, d2 = v[i].z - mean, d3 = v[i].w - mean;
            q += d0 * d0; q += d1 * d1; q += d2 * d2; q += d3 * d3;
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);       // biased variance, like nn.LayerNorm
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int ch = i * 64 + lane;
        if (ch < nchunk) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + ch * 4), b = *reinterpret_cast<const float4*>(beta + ch * 4);
            float4 o;
            o.x = (v[i].x - mean) * rstd * g.x + b.x;
            o.y = (v[i].y - mean) * rstd * g.y + b.y;
            o.z = (v[i].z - mean) * rstd * g.z + b.z;
            o.w = (v[i].w - mean) * rstd * g.w + b.w;
            *reinterpret_cast<float4*>(yr + ch * 4) = o;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void layernorm_f32_kernel(const float* __restrict__ x, int64_t xs, int64_t rows, int C,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float eps, float* __restrict__ y, int64_t ys) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * (THREADS / 64) + wave;
    if (r >= rows) return;
    if (VEC) layernorm_row_vec(x + r * xs, C, gamma, beta, eps, y + r * ys, lane);
    else layernorm_row(x + r * xs, C, gamma, beta, eps, y + r * ys, lane);
}

// K29: the text tower's pooling.  One wave per sequence: the row of the FIRST largest id (the end-of-text token has the largest
// id of the vocabulary; torch.argmax's tie rule), then the LayerNorm above on that row alone -> y[n]
template <bool VEC>
__global__ __launch_bounds__(THREADS) void eot_layernorm_f32_kernel(const float* __restrict__ x, int64_t xs, const int64_t* __restrict__ ids,
                                                                    int N, int L, int C, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float eps, float* __restrict__ y,
                                                                    int64_t ys) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * (THREADS / 64) + wave;
    if (n >= N) return;
    const int64_t* row = ids + (int64_t)n * L;
    int64_t best = INT64_MIN;                                // a lane walks t upwards: > keeps its first maximum
    int bt = L;                                              // a lane without a token loses every tie below
    if (lane < L) { best = row[lane]; bt = lane; }
    for (int t = lane + 64; t < L; t += 64) {
        const int64_t v = row[t];
        if (v > best) { best = v; bt = t; }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const int64_t ob = __shfl_xor(best, o, 64);
        const int ot = __shfl_xor(bt, o, 64);
        if (ob > best || (ob == best && ot < bt)) { best = ob; bt = ot; }
    }
    const float* xr = x + ((int64_t)n * L + bt) * xs;       // bt < L: lane 0 always holds t = 0
    if (VEC) layernorm_row_vec(xr, C, gamma, beta, eps, y + n * ys, lane);
    else layernorm_row(xr, C, gamma, beta, eps, y + n * ys, lane);
}

// ---------------------------------------------------------------------------------------------
// attention (see the header of this file)
// ---------------------------------------------------------------------------------------------
typedef float af32x16_t __attribute__((ext_vector_type(16)));
constexpr int AQ = 128;                  // queries per workgroup (4 waves x 32)
constexpr int AK = 64;                   // keys per tile
constexpr int KP = 68;                   // K tile pitch in floats (16-byte rows; 4 banks' shift per key)
constexpr int VP = 72;                   // V tile pitch in floats: rows 4 apart (the two lane halves of a k-step) sit 32 banks apart

// CAUSAL (K29): query i sees keys 0 .. i.  A block stops after the last tile any of its queries sees (the same count for its four
// waves, so all of them reach both barriers of every tile); a wave whose 32 queries all lie before a tile skips that tile's
// arithmetic (every p of it is 0).  Key 0 is visible to every query: the running maximum is finite from the first tile on.
template <bool CAUSAL>
__global__ __launch_bounds__(THREADS) void attention_d64_f32_kernel(const float* __restrict__ qkv, int64_t qs, int B, int L, int heads,
                                                                    float scale, float* __restrict__ out, int64_t os) {
    __shared__ __attribute__((aligned(16))) float Ks[AK * KP];
    __shared__ __attribute__((aligned(16))) float Vs[AK * VP];
    const int C = heads * 64;
    const int qblocks = (L + AQ - 1) / AQ;
    int bid = blockIdx.x;
    const int qb = bid % qblocks; bid /= qblocks;
    const int h = bid % heads;
    const int b = bid / heads;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int qi = qb * AQ + wave * 32 + l31;
    const float* base = qkv + (int64_t)b * L * qs + h * 64;
    // Q fragment (B operand of S^T): Q[q][32 hi + j], j = 0 .. 31; a query past L reads row L - 1 and is not written
    float qf[32];
    {
        const float* qp = base + (int64_t)(qi < L ? qi : L - 1) * qs + 32 * hi;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 t = *reinterpret_cast<const float4*>(qp + 4 * j);
            qf[4 * j] = t.x; qf[4 * j + 1] = t.y; qf[4 * j + 2] = t.z; qf[4 * j + 3] = t.w;
        }
    }
    af32x16_t o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { o0[e] = 0.f; o1[e] = 0.f; }
    float m = -INFINITY, l = 0.f;
    // staging: thread -> row tid >> 2 of the tile, 16-byte chunks (tid & 3) + 4 i of its K and V rows
    const int srow = threadIdx.x >> 2, sch = threadIdx.x & 3;
    float4 kreg[4], vreg[4];
    auto gload = [&](int k0) {
        const int kj = k0 + srow;
        const bool ok = kj < L;                              // rows past L: the next batch's, or nothing readable at all
        const float* rp = base + (int64_t)(ok ? kj : 0) * qs;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            kreg[i] = make_float4(0.f, 0.f, 0.f, 0.f); vreg[i] = kreg[i];
            if (ok) {
                kreg[i] = *reinterpret_cast<const float4*>(rp + C + 4 * (sch + 4 * i));
                vreg[i] = *reinterpret_cast<const float4*>(rp + 2 * C + 4 * (sch + 4 * i));
            }
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<float4*>(Ks + srow * KP + 4 * (sch + 4 * i)) = kreg[i];
            *reinterpret_cast<float4*>(Vs + srow * VP + 4 * (sch + 4 * i)) = vreg[i];
        }
    };
    const int kend = CAUSAL && (qb + 1) * AQ < L ? (qb + 1) * AQ : L;       // keys [0, kend) are all this block reads
    const int ntiles = (kend + AK - 1) / AK;
    gload(0);
    for (int it = 0; it < ntiles; ++it) {
        const int k0 = it * AK;
        park();
        __syncthreads();
        if (it + 1 < ntiles) gload(k0 + AK);                 // flies under this tile's MFMAs
        if (!CAUSAL || k0 <= qb * AQ + wave * 32 + 31) {     // wave-uniform
            // S^T = K Q^T for the two 32-key blocks of the tile
            af32x16_t st[2];
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
                for (int e = 0; e < 16; ++e) st[sb][e] = 0.f;
                const float* kr = Ks + (32 * sb + l31) * KP + 32 * hi;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float4 kf = *reinterpret_cast<const float4*>(kr + 4 * j);
                    st[sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[4 * j], st[sb], 0, 0, 0);
                    st[sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[4 * j + 1], st[sb], 0, 0, 0);
                    st[sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[4 * j + 2], st[sb], 0, 0, 0);
                    st[sb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[4 * j + 3], st[sb], 0, 0, 0);
                }
            }
            float tmax = -INFINITY;
#pragma unroll
            for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = k0 + 32 * sb + 8 * (e >> 2) + 4 * hi + (e & 3);
                    if (key >= L || (CAUSAL && key > qi)) st[sb][e] = -INFINITY;
                    tmax = fmaxf(tmax, st[sb][e]);
                }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float m_new = fmaxf(m, tmax);                  // finite from the first tile on: key k0 of a tile is always < L
            const float resc = expf((m - m_new) * scale);
            float ps = 0.f;
#pragma unroll
            for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                for (int e = 0; e < 16; ++e) { st[sb][e] = expf((st[sb][e] - m_new) * scale); ps += st[sb][e]; }
            l = l * resc + ps;                                   // per-half partial sum; the halves are joined at the end
            m = m_new;
#pragma unroll
            for (int e = 0; e < 16; ++e) { o0[e] *= resc; o1[e] *= resc; }
            // O^T += V^T P^T: register e of block sb is the k-step of keys 8 (e >> 2) + (e & 3) (+ 4 for the upper lane half)
#pragma unroll
            for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float* vr = Vs + (32 * sb + 8 * (e >> 2) + (e & 3) + 4 * hi) * VP + l31;
                    o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[0], st[sb][e], o0, 0, 0, 0);        // d = lane & 31
                    o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32], st[sb][e], o1, 0, 0, 0);       // d = 32 + (lane & 31)
                }
        }
        __syncthreads();                                     // every wave is done with the tile before the next one is parked
    }
    l += __shfl_xor(l, 32, 64);
    if (qi < L) {
        float* op = out + ((int64_t)b * L + qi) * os + h * 64;
#pragma unroll
        for (int g = 0; g < 4; ++g) {                        // register 4 g + i: d = 8 g + 4 hi + i
            *reinterpret_cast<float4*>(op + 8 * g + 4 * hi) =
                make_float4(o0[4 * g] / l, o0[4 * g + 1] / l, o0[4 * g + 2] / l, o0[4 * g + 3] / l);
            *reinterpret_cast<float4*>(op + 32 + 8 * g + 4 * hi) =
                make_float4(o1[4 * g] / l, o1[4 * g + 1] / l, o1[4 * g + 2] / l, o1[4 * g + 3] / l);
        }
    }
}

template <bool CAUSAL>
int attention_entry(const float* qkv, long long qkv_row_stride, int B, int L, int heads, float scale, float* out, long long out_row_stride,
                    hipStream_t stream) {
    if (!qkv || !out || B <= 0 || L <= 0 || heads <= 0 || heads > (1 << 20) || !(scale > 0.f) || !(scale < INFINITY))
        return OESS_EINVAL;
    if (qkv_row_stride < 3ll * heads * 64 || out_row_stride < 64ll * heads || (qkv_row_stride & 3) || (out_row_stride & 3) ||
        ((uintptr_t)qkv & 15) || ((uintptr_t)out & 15))
        return OESS_EINVAL;
    if ((long long)B * L >= (1ll << 31) || qkv_row_stride >= (1ll << 31) || out_row_stride >= (1ll << 31)) return OESS_EINVAL;
    const long long blocks = (long long)B * heads * ((L + AQ - 1) / AQ);
    if (blocks > 0x7fffffffll) return OESS_EINVAL;
    hipLaunchKernelGGL(attention_d64_f32_kernel<CAUSAL>, dim3((unsigned)blocks), dim3(THREADS), 0, stream, qkv, (int64_t)qkv_row_stride,
                       B, L, heads, scale, out, (int64_t)out_row_stride);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}
}  // namespace

extern "C" {

int oess_layernorm_f32(const float* x, long long x_row_stride, int64_t rows, int C, const float* gamma, const float* beta, float eps,
                       float* y, long long y_row_stride, oess_stream_t stream) {
    if (!x || !y || !gamma || !beta || rows <= 0 || C <= 0 || C > 2048 || x_row_stride < C || y_row_stride < C || !(eps > 0.f))
        return OESS_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta) & 3) != 0) return OESS_EINVAL;
    const int64_t g = (rows + 3) / 4;                        // one wave per row, no grid-stride loop
    if (g > 0x7fffffffll || x_row_stride >= (1ll << 31) || y_row_stride >= (1ll << 31)) return OESS_EINVAL;
    const bool vec = (C & 3) == 0 && (x_row_stride & 3) == 0 && (y_row_stride & 3) == 0 &&
                     ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta)) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(layernorm_f32_kernel<true>, dim3((unsigned)g), dim3(THREADS), 0, (hipStream_t)stream, x, (int64_t)x_row_stride,
                           rows, C, gamma, beta, eps, y, (int64_t)y_row_stride);
    else
        hipLaunchKernelGGL(layernorm_f32_kernel<false>, dim3((unsigned)g), dim3(THREADS), 0, (hipStream_t)stream, x, (int64_t)x_row_stride,
                           rows, C, gamma, beta, eps, y, (int64_t)y_row_stride);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_attention_d64_f32(const float* qkv, long long qkv_row_stride, int B, int L, int heads, float scale, float* out,
                           long long out_row_stride, oess_stream_t stream) {
    return attention_entry<false>(qkv, qkv_row_stride, B, L, heads, scale, out, out_row_stride, (hipStream_t)stream);
}

int oess_attention_d64_causal_f32(const float* qkv, long long qkv_row_stride, int B, int L, int heads, float scale, float* out,
                                  long long out_row_stride, oess_stream_t stream) {
    return attention_entry<true>(qkv, qkv_row_stride, B, L, heads, scale, out, out_row_stride, (hipStream_t)stream);
}

int oess_clip_text_eot_layernorm_f32(const float* x, long long x_row_stride, const int64_t* ids, int N, int L, int C, const float* gamma,
                                     const float* beta, float eps, float* y, long long y_row_stride, oess_stream_t stream) {
    if (!x || !ids || !y || !gamma || !beta || N <= 0 || L <= 0 || C <= 0 || C > 2048 || x_row_stride < C || y_row_stride < C ||
        !(eps > 0.f))
        return OESS_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta) & 3) != 0 || ((uintptr_t)ids & 7) != 0) return OESS_EINVAL;
    if ((long long)N * L >= (1ll << 31) || x_row_stride >= (1ll << 31) || y_row_stride >= (1ll << 31)) return OESS_EINVAL;
    const int g = (N + 3) / 4;                               // one wave per sequence
    const bool vec = (C & 3) == 0 && (x_row_stride & 3) == 0 && (y_row_stride & 3) == 0 &&
                     ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta)) & 15) == 0;      // oess_layernorm_f32's rule
    if (vec)
        hipLaunchKernelGGL(eot_layernorm_f32_kernel<true>, dim3((unsigned)g), dim3(THREADS), 0, (hipStream_t)stream, x,
                           (int64_t)x_row_stride, ids, N, L, C, gamma, beta, eps, y, (int64_t)y_row_stride);
    else
        hipLaunchKernelGGL(eot_layernorm_f32_kernel<false>, dim3((unsigned)g), dim3(THREADS), 0, (hipStream_t)stream, x,
                           (int64_t)x_row_stride, ids, N, L, C, gamma, beta, eps, y, (int64_t)y_row_stride);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
