// Open-vocabulary rendering (K36): segmentation maps over K classes whose vocabulary has P >= K NAMES, class k owning the
// contiguous channels class_offsets[k] ... class_offsets[k + 1] - 1.  Two kernels, both ending in render_common.h's class walk
// and byte staging, which they share with segment_render.hip (K35):
//   grouped_render_kernel   from P-channel logits, raw at the input size or blended as K35 blends them;
//   head_render_kernel      from the C <= 64 channel map in front of a linear head [P, C]: the P logits of a pixel are formed in
//                           registers and consumed at once, nothing of size [B, P, H, W] exists.
// Values.  Name value v_p: K35's value (grouped), or the explicit chain fmaf(w[p][C-1], x[C-1], ... fmaf(w[p][0], x[0], bias_p))
// in ascending c (head; bf16 taps widened first).  Class value c_k = torch.amax over the group: the largest member, NaN when a
// member is NaN.  Label = torch.argmax's rule over c; confidence = 1 / sum_k exp(c_k - c_max) over the K CLASS values, one walk
// with the running maximum and sum; threshold and colour as K35.
// One lane owns a pixel; no atomics, no cross-lane arithmetic: two calls give the same bits.
// Work split.  Grouped: one workgroup per output row, the two source rows as fp32 [2][w][P] in LDS when they fit LDS_BUDGET,
// global taps otherwise (K35's split).  Head: a workgroup loads the weights and bias into LDS once (every lane reads the same
// address in the p loop: a broadcast) and walks `rows_per_wg` consecutive rows; a lane holds its pixel's C values in registers.
// The class offsets sit in LDS, clamped to 0 ... P on the way in: no offset list, whatever it holds, makes a lane read outside
// its pixel's P channels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"
#include "bilinear_axis.h"
#include "render_common.h"

namespace {
using namespace oess;
using namespace oess::render;
constexpr size_t LDS_BUDGET = 48 * 1024;     // grouped: two fp32 source rows; head: the weights and the bias
constexpr int MAX_P = 1024;
constexpr int MAX_C = 64;
constexpr int HEAD_WGS = 2048;               // head: workgroups a launch aims at (8 per CU); rows are dealt evenly among them

enum { RAW = 0, TAPS_LDS = 1, TAPS_GLOBAL = 2 };

// offs[0 ... K] from the device list (null: one name per class), clamped to 0 ... P
__device__ __forceinline__ void load_offsets(int* offs, const int32_t* __restrict__ class_offsets, int K, int P) {
    for (int j = threadIdx.x; j <= K; j += THREADS) {
        int o = class_offsets ? class_offsets[j] : j;
        o = o < 0 ? 0 : o;
        offs[j] = o > P ? P : o;
    }
}

template <bool BF16, int MODE>
__global__ __launch_bounds__(THREADS) void grouped_render_kernel(const void* __restrict__ in, int64_t ips, int K, int P,
                                                                 const int32_t* __restrict__ class_offsets, Axis ay, Axis ax, Render r) {
    extern __shared__ __attribute__((aligned(16))) float rows[];            // TAPS_LDS: [2][ax.in][P]
    __shared__ Stage st;
    __shared__ int offs[MAX_K + 1];
    const int oy = blockIdx.x % ay.out;
    const int64_t b = blockIdx.x / ay.out;
    const int64_t opix = (b * ay.out + oy) * (int64_t)ax.out;               // first output pixel of this row
    load_palette(st, r, K);
    load_offsets(offs, class_offsets, K, P);
    int y0 = 0, y1 = 0; float wy = 0.f;
    if constexpr (MODE != RAW) src_index(ay, oy, y0, y1, wy);
    const float hy = 1.f - wy;
    const int64_t row0 = (b * ay.in + y0) * ax.in, row1 = (b * ay.in + y1) * ax.in;
    if constexpr (MODE == TAPS_LDS) {
        const int n = ax.in * P;
        for (int j = threadIdx.x; j < n; j += THREADS) {
            const int x = j / P, p = j - x * P;
            rows[j] = tap<BF16>(in, (row0 + x) * ips + p);
            rows[n + j] = tap<BF16>(in, (row1 + x) * ips + p);
        }
    }
    __syncthreads();                                                        // pal, offs and rows
    const int lphase = r.labels ? (int)((uintptr_t)(r.labels + opix) & 3) : 0;
    const int cphase = r.rgb ? (int)((uintptr_t)(r.rgb + 3 * opix) & 3) : 0;
    for (int base = 0; base < ax.out; base += THREADS) {                    // uniform trip count: barriers inside
        const int ox = base + threadIdx.x;
        if (ox < ax.out) {
            int idx; float sum;
            if constexpr (MODE == RAW) {
                const int64_t q = ((b * ay.in + oy) * ax.in + ox) * ips;
                class_walk(offs, K, P, [&](int p) { return tap<BF16>(in, q + p); }, idx, sum);
            } else {
                int x0, x1; float wx;
                src_index(ax, ox, x0, x1, wx);
                const float hx = 1.f - wx;
                class_walk(offs, K, P, [&](int p) {
                    float p00, p01, p10, p11;
                    if constexpr (MODE == TAPS_LDS) {
                        const float* r1 = rows + ax.in * P;
                        p00 = rows[x0 * P + p]; p01 = rows[x1 * P + p];
                        p10 = r1[x0 * P + p];   p11 = r1[x1 * P + p];
                    } else {
                        p00 = tap<BF16>(in, (row0 + x0) * ips + p); p01 = tap<BF16>(in, (row0 + x1) * ips + p);
                        p10 = tap<BF16>(in, (row1 + x0) * ips + p); p11 = tap<BF16>(in, (row1 + x1) * ips + p);
                    }
                    return hy * (hx * p00 + wx * p01) + wy * (hx * p10 + wx * p11);              // resize_fwd_kernel's association
                }, idx, sum);
            }
            emit(st, r, K, opix + ox, lphase, cphase, idx, sum);
        }
        flush_chunk(st, r, opix + base, lphase, cphase, ax.out - base < THREADS ? ax.out - base : THREADS);
    }
}

// CT: the register tile (C <= CT); FULL: C == CT, the channel loops carry no guard.  VEC: the pixel's C values are read as 16-byte
// words (the entry checks the alignment of the pointer, the stride and C).
template <bool BF16, int CT, bool FULL, bool VEC>
__global__ __launch_bounds__(THREADS) void head_render_kernel(const void* __restrict__ in, int64_t ips, int C, int K, int P,
                                                              const float* __restrict__ weight, const float* __restrict__ bias,
                                                              const int32_t* __restrict__ class_offsets, int rows, int W,
                                                              int rows_per_wg, Render r) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];            // [P][C] weights, then [P] bias
    __shared__ Stage st;
    __shared__ int offs[MAX_K + 1];
    load_palette(st, r, K);
    load_offsets(offs, class_offsets, K, P);
    const int nw = P * C;
    for (int j = threadIdx.x; j < nw; j += THREADS) wlds[j] = weight[j];
    for (int j = threadIdx.x; j < P; j += THREADS) wlds[nw + j] = bias ? bias[j] : 0.f;
    __syncthreads();                                                        // pal, offs, weights and bias
    const float* blds = wlds + nw;
    const int row_end = (int)min((int64_t)rows, ((int64_t)blockIdx.x + 1) * rows_per_wg);
    for (int row = blockIdx.x * rows_per_wg; row < row_end; ++row) {        // uniform: barriers inside
        const int64_t opix = (int64_t)row * W;
        const int lphase = r.labels ? (int)((uintptr_t)(r.labels + opix) & 3) : 0;
        const int cphase = r.rgb ? (int)((uintptr_t)(r.rgb + 3 * opix) & 3) : 0;
        for (int base = 0; base < W; base += THREADS) {
            const int ox = base + threadIdx.x;
            if (ox < W) {
                float x[CT];
                const int64_t q = (opix + ox) * ips;
                if constexpr (VEC) {                                        // FULL as well: C == CT
                    if constexpr (BF16) {
                        const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(in) + q);
#pragma unroll
                        for (int j = 0; j < CT / 8; ++j) {
                            const uint4 u = src[j];
                            const uint32_t wds[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                x[8 * j + 2 * t] = __uint_as_float(wds[t] << 16);
                                x[8 * j + 2 * t + 1] = __uint_as_float(wds[t] & 0xffff0000u);
                            }
                        }
                    } else {
                        const float4* src = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(in) + q);
#pragma unroll
                        for (int j = 0; j < CT / 4; ++j) {
                            const float4 u = src[j];
                            x[4 * j] = u.x; x[4 * j + 1] = u.y; x[4 * j + 2] = u.z; x[4 * j + 3] = u.w;
                        }
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < CT; ++c) x[c] = (FULL || c < C) ? tap<BF16>(in, q + c) : 0.f;
                }
                int idx; float sum;
                class_walk(offs, K, P, [&](int p) {
                    float acc = blds[p];
                    if constexpr (FULL) {
                        const float4* wp = reinterpret_cast<const float4*>(wlds + p * CT);      // CT % 4 == 0: 16-byte aligned rows
#pragma unroll
                        for (int j = 0; j < CT / 4; ++j) {
                            const float4 u = wp[j];
                            acc = __fmaf_rn(u.x, x[4 * j], acc);     acc = __fmaf_rn(u.y, x[4 * j + 1], acc);
                            acc = __fmaf_rn(u.z, x[4 * j + 2], acc); acc = __fmaf_rn(u.w, x[4 * j + 3], acc);
                        }
                    } else {
                        const float* wp = wlds + p * C;
#pragma unroll
                        for (int c = 0; c < CT; ++c) {
                            if (c < C) acc = __fmaf_rn(wp[c], x[c], acc);
                        }
                    }
                    return acc;
                }, idx, sum);
                emit(st, r, K, opix + ox, lphase, cphase, idx, sum);
            }
            flush_chunk(st, r, opix + base, lphase, cphase, W - base < THREADS ? W - base : THREADS);
        }
    }
}

}  // namespace

extern "C" {

int oess_segment_render_grouped(const void* logits, int is_bf16, long long pix_stride, int B, int K, int P, int h, int w, int H, int W,
                                int align_corners, const int32_t* class_offsets, const uint8_t* palette, const uint8_t* grey,
                                int alpha256, float min_conf, int ignore_label, uint8_t* labels, float* conf, uint8_t* rgb,
                                oess_stream_t stream) {
    if (!logits || !class_offsets || bad_render_args(palette, labels, conf, rgb, K, alpha256, min_conf, ignore_label) || P < K ||
        P > MAX_P || B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || pix_stride < P)
        return OESS_EINVAL;
    // extents as oess_segment_render: one workgroup per output row, int64 element offsets
    int64_t in_elems, out_elems;
    if ((int64_t)B * H > INT32_MAX || (int64_t)B * h > INT32_MAX || (int64_t)w * P > INT32_MAX ||
        __builtin_mul_overflow((int64_t)B * h * w, (int64_t)pix_stride, &in_elems) ||
        __builtin_mul_overflow((int64_t)B * H, (int64_t)W, &out_elems) || in_elems > INT64_MAX / 4 || out_elems > INT64_MAX / 4)
        return OESS_EINVAL;
    const Axis ay = make_axis(h, H, align_corners), ax = make_axis(w, W, align_corners);
    Render r;
    r.palette = palette; r.grey = grey; r.labels = labels; r.conf = conf; r.rgb = rgb;
    r.alpha256 = alpha256; r.ignore_label = ignore_label; r.min_conf = min_conf;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((int64_t)B * H)), block(THREADS);
    const size_t lds = (size_t)2 * w * P * sizeof(float);
#define OESS_GR(BF, MODE, SH)                                                                                                    \
    hipLaunchKernelGGL((grouped_render_kernel<BF, MODE>), grid, block, SH, st, logits, (int64_t)pix_stride, K, P, class_offsets, \
                       ay, ax, r)
    if (H == h && W == w) { if (is_bf16) OESS_GR(true, RAW, 0); else OESS_GR(false, RAW, 0); }
    else if (lds <= LDS_BUDGET) { if (is_bf16) OESS_GR(true, TAPS_LDS, lds); else OESS_GR(false, TAPS_LDS, lds); }
    else { if (is_bf16) OESS_GR(true, TAPS_GLOBAL, 0); else OESS_GR(false, TAPS_GLOBAL, 0); }
#undef OESS_GR
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

size_t oess_head_render_max_names(int C) {
    return C >= 1 && C <= MAX_C ? (size_t)(LDS_BUDGET / ((size_t)(C + 1) * sizeof(float))) : 0;
}

int oess_head_render(const void* x, int is_bf16, long long pix_stride, int B, int C, int H, int W, const float* weight,
                     const float* bias, int K, int P, const int32_t* class_offsets, const uint8_t* palette, const uint8_t* grey,
                     int alpha256, float min_conf, int ignore_label, uint8_t* labels, float* conf, uint8_t* rgb,
                     oess_stream_t stream) {
    if (!x || !weight || bad_render_args(palette, labels, conf, rgb, K, alpha256, min_conf, ignore_label) || C < 1 || C > MAX_C ||
        P < K || P > MAX_P || (!class_offsets && P != K) || B <= 0 || H <= 0 || W <= 0 || pix_stride < C)
        return OESS_EINVAL;
    const size_t lds = (size_t)P * (C + 1) * sizeof(float);
    if (lds > LDS_BUDGET) return OESS_EINVAL;                                // the caller composes the head conv with the grouped render
    int64_t in_elems, out_elems;
    if ((int64_t)B * H > INT32_MAX || __builtin_mul_overflow((int64_t)B * H, (int64_t)W, &out_elems) ||
        __builtin_mul_overflow(out_elems, (int64_t)pix_stride, &in_elems) || in_elems > INT64_MAX / 4 || out_elems > INT64_MAX / 4)
        return OESS_EINVAL;
    Render r;
    r.palette = palette; r.grey = grey; r.labels = labels; r.conf = conf; r.rgb = rgb;
    r.alpha256 = alpha256; r.ignore_label = ignore_label; r.min_conf = min_conf;
    hipStream_t st = (hipStream_t)stream;
    const int rows = B * H;
    const int rows_per_wg = (rows + HEAD_WGS - 1) / HEAD_WGS;
    const dim3 grid((unsigned)((rows + rows_per_wg - 1) / rows_per_wg)), block(THREADS);
    const int esz = is_bf16 ? 2 : 4;
    const bool full = C == 32 || C == 64;
    const bool vec = full && (uintptr_t)x % 16 == 0 && ((int64_t)pix_stride * esz) % 16 == 0;
#define OESS_HR(BF, CT, FULL, VEC)                                                                                              \
    hipLaunchKernelGGL((head_render_kernel<BF, CT, FULL, VEC>), grid, block, lds, st, x, (int64_t)pix_stride, C, K, P, weight, \
                       bias, class_offsets, rows, W, rows_per_wg, r)
#define OESS_HR_C(BF)                                                                       \
    do {                                                                                    \
        if (C == 32) { if (vec) OESS_HR(BF, 32, true, true); else OESS_HR(BF, 32, true, false); }   \
        else if (C == 64) { if (vec) OESS_HR(BF, 64, true, true); else OESS_HR(BF, 64, true, false); } \
        else if (C < 32) OESS_HR(BF, 32, false, false);                                     \
        else OESS_HR(BF, 64, false, false);                                                 \
    } while (0)
    if (is_bf16) OESS_HR_C(true); else OESS_HR_C(false);
#undef OESS_HR_C
#undef OESS_HR
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
