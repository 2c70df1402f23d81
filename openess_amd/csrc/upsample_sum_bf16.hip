// K30: skip sum + bilinear x2 (align_corners=False) of the E2VID UpsampleConvLayer on NHWC bf16 activations for gfx950.
//   out[b, oy, ox, c] = bf16_rne( bilinear2x( f32(x) + f32(skip) )[b, oy, ox, c] )
// The sum and the interpolation are fp32 and the store is the ONE rounding to bf16.  A streaming kernel bound by its store:
// the output is four times the size of each input.
//
// With scale 2 the source coordinate of output o is max(0, o / 2 - 0.25), so per axis
//   o = 2 i     : taps i - 1 and i, weights 0.25 / 0.75   (i = 0: lambda = 0, pixel 0 alone)
//   o = 2 i + 1 : taps i and i + 1, weights 0.75 / 0.25   (i = n - 1: both taps are pixel n - 1)
// i.e. input pixel (iy, ix) owns the 2 x 2 output quad (2 iy + {0, 1}, 2 ix + {0, 1}), which reads its 3 x 3 neighbourhood.
// At a border the clamped tap gets weight 0 and the edge pixel weight 1, so the edge value passes through unrounded.
//
// Work split: one lane owns 8 channels of one input COLUMN over a strip of ROWS input rows and walks down it.  The blend is
// separable: a row is summed and blended horizontally ONCE into the quad's two output columns (3 + 3 loads), and a quad is the
// vertical blend of three consecutive such rows, two of which the lane still holds.  Per quad that is 6 * (ROWS + 2) / ROWS = 9
// loads at ROWS = 4 (7.5 where a strip touches the map's edge) for 4 stores, and the conversions, sums and horizontal blends of a
// row are done 1.5 times instead of 3.  The first form of this kernel gave every lane one quad and its whole 3 x 3
// neighbourhood, 18 loads per 4 stores: it was bound by its VALU work (3.9 TB/s at 64 @ 220 x 320; EXPERIMENTS.md), not by the
// store.  A lane per OUTPUT pixel would issue 8 loads per store.  HBM traffic is the same in all three: the neighbours come from L2.
// No atomics, no LDS, plain 16-byte vector loads and stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"

namespace {
using namespace oess;
constexpr int THREADS = 256;
constexpr int ROWS = 4;                 // input rows per lane: 2 halo rows per strip, and H / ROWS strips keep small maps parallel

union Pack8 { uint4 q; uint16_t h[8]; };
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// two floats -> packed bf16x2 (low half = a), round to nearest even: the compiler's own conversion (one instruction on gfx950)
__device__ __forceinline__ uint32_t to_bf16x2(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

__device__ __forceinline__ void store8(uint16_t* __restrict__ p, const float (&v)[8]) {
    *reinterpret_cast<uint4*>(p) = make_uint4(to_bf16x2(v[0], v[1]), to_bf16x2(v[2], v[3]), to_bf16x2(v[4], v[5]), to_bf16x2(v[6], v[7]));
}

// f32(x) + f32(skip) of 8 channels of one pixel
template <bool SKIP>
__device__ __forceinline__ void load_sum(const uint16_t* __restrict__ x, const uint16_t* __restrict__ skip, int64_t xo, int64_t so,
                                         float (&v)[8]) {
    Pack8 a, b;
    a.q = *reinterpret_cast<const uint4*>(x + xo);
    if (SKIP) b.q = *reinterpret_cast<const uint4*>(skip + so);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = SKIP ? bf16_to_f32(a.h[k]) + bf16_to_f32(b.h[k]) : bf16_to_f32(a.h[k]);
}

// w * a + (1 - w) * b, w in {0, 0.25}: (1 - w) is exact, and w = 0 returns b itself
__device__ __forceinline__ float lerp(float w, float a, float b) { return __builtin_fmaf(w, a, (1.f - w) * b); }

// one input row (first pixel `row`) summed and blended into the two output columns of input column ix
template <bool SKIP>
__device__ __forceinline__ void blend_row(const uint16_t* __restrict__ x, int64_t xps, const uint16_t* __restrict__ skip, int64_t sps,
                                          int64_t row, int xl, int ix, int xr, float wl, float wr, int c0, float (&left)[8],
                                          float (&right)[8]) {
    float l[8], m[8], r[8];
    load_sum<SKIP>(x, skip, (row + xl) * xps + c0, (row + xl) * sps + c0, l);
    load_sum<SKIP>(x, skip, (row + ix) * xps + c0, (row + ix) * sps + c0, m);
    load_sum<SKIP>(x, skip, (row + xr) * xps + c0, (row + xr) * sps + c0, r);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        left[k] = lerp(wl, l[k], m[k]);
        right[k] = lerp(wr, r[k], m[k]);
    }
}

template <bool SKIP>
__global__ __launch_bounds__(THREADS) void upsample2x_sum_kernel(const uint16_t* __restrict__ x, int64_t xps,
                                                                 const uint16_t* __restrict__ skip, int64_t sps, int B, int H, int W,
                                                                 int C, uint16_t* __restrict__ out, int64_t ops) {
    const int cl = C >> 3;
    const int strips = (H + ROWS - 1) / ROWS;
    const int64_t total = (int64_t)B * strips * W * cl;
    const int64_t Wo = 2 * (int64_t)W;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * THREADS) {
        const int64_t col = i / cl;
        const int c0 = (int)(i - col * cl) * 8;
        const int ix = (int)(col % W);
        const int64_t t = col / W;
        const int iy0 = (int)(t % strips) * ROWS;
        const int64_t b = t / strips;
        // clamped neighbours and the weight of the outer tap (0 where the clamp folded it onto the centre)
        const int xl = ix > 0 ? ix - 1 : 0, xr = ix < W - 1 ? ix + 1 : ix;
        const float wl = ix > 0 ? 0.25f : 0.f, wr = ix < W - 1 ? 0.25f : 0.f;
        // three consecutive blended rows, [.][0] = left output column, [.][1] = right
        float up[2][8], mid[2][8], down[2][8];
        blend_row<SKIP>(x, xps, skip, sps, (b * H + iy0) * W, xl, ix, xr, wl, wr, c0, mid[0], mid[1]);
        if (iy0 > 0) {
            blend_row<SKIP>(x, xps, skip, sps, (b * H + iy0 - 1) * W, xl, ix, xr, wl, wr, c0, up[0], up[1]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) { up[0][k] = mid[0][k]; up[1][k] = mid[1][k]; }     // weight 0 below
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int iy = iy0 + r;
            if (iy >= H) break;
            if (iy < H - 1) {
                blend_row<SKIP>(x, xps, skip, sps, (b * H + iy + 1) * W, xl, ix, xr, wl, wr, c0, down[0], down[1]);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) { down[0][k] = mid[0][k]; down[1][k] = mid[1][k]; }   // weight 0 below
            }
            const float wu = iy > 0 ? 0.25f : 0.f, wd = iy < H - 1 ? 0.25f : 0.f;
            float o00[8], o01[8], o10[8], o11[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                o00[k] = lerp(wu, up[0][k], mid[0][k]);
                o01[k] = lerp(wu, up[1][k], mid[1][k]);
                o10[k] = lerp(wd, down[0][k], mid[0][k]);
                o11[k] = lerp(wd, down[1][k], mid[1][k]);
            }
            const int64_t o0 = ((b * 2 * H + 2 * iy) * Wo + 2 * ix) * ops + c0;
            store8(out + o0, o00);
            store8(out + o0 + ops, o01);
            store8(out + o0 + Wo * ops, o10);
            store8(out + o0 + (Wo + 1) * ops, o11);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                up[0][k] = mid[0][k], up[1][k] = mid[1][k];
                mid[0][k] = down[0][k], mid[1][k] = down[1][k];
            }
        }
    }
}

// byte ranges [p, p + n) and [q, q + m) overlap
bool overlaps(const void* p, int64_t n, const void* q, int64_t m) {
    const uintptr_t a = (uintptr_t)p, c = (uintptr_t)q;
    return a < c + (uintptr_t)m && c < a + (uintptr_t)n;
}

// bytes from a view's first element to one past its last: P pixels of C channels, `ps` elements apart
int64_t span_bytes(int64_t P, int C, int64_t ps) { return ((P - 1) * ps + C) * 2; }
}  // namespace

int oess_upsample_bilinear2x_sum_nhwc_bf16(const void* x, long long x_pix_stride, const void* skip, long long skip_pix_stride, int B,
                                           int H, int W, int C, void* out, long long out_pix_stride, oess_stream_t stream) {
    if (!x || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7) || x_pix_stride < C || out_pix_stride < C ||
        (skip && skip_pix_stride < C))
        return OESS_EINVAL;
    // 16-byte accesses: pixel strides in whole vectors, as every NHWC bf16 entry of norm_ops.hip asks
    if ((x_pix_stride & 7) || (out_pix_stride & 7) || (skip && (skip_pix_stride & 7)))
        return OESS_EINVAL;
    const int64_t P = (int64_t)B * H * W;
    const int64_t out_bytes = span_bytes(4 * P, C, out_pix_stride);
    // a lane's stores land on pixels other lanes still read: out may share no byte range with an input (interleaved channel
    // slices of one buffer are refused with it: the range test is conservative)
    if (overlaps(out, out_bytes, x, span_bytes(P, C, x_pix_stride)) ||
        (skip && overlaps(out, out_bytes, skip, span_bytes(P, C, skip_pix_stride))))
        return OESS_EINVAL;
    const int64_t lanes = (int64_t)B * ((H + ROWS - 1) / ROWS) * W * (C >> 3);
    int64_t grid = (lanes + THREADS - 1) / THREADS;
    if (grid > 8192) grid = 8192;
    if (skip)
        hipLaunchKernelGGL(upsample2x_sum_kernel<true>, dim3((unsigned)grid), dim3(THREADS), 0, (hipStream_t)stream, (const uint16_t*)x,
                           (int64_t)x_pix_stride, (const uint16_t*)skip, (int64_t)skip_pix_stride, B, H, W, C, (uint16_t*)out,
                           (int64_t)out_pix_stride);
    else
        hipLaunchKernelGGL(upsample2x_sum_kernel<false>, dim3((unsigned)grid), dim3(THREADS), 0, (hipStream_t)stream, (const uint16_t*)x,
                           (int64_t)x_pix_stride, (const uint16_t*)nullptr, (int64_t)0, B, H, W, C, (uint16_t*)out,
                           (int64_t)out_pix_stride);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}
