// Segmentation maps straight from logits (K35): per output pixel the class label (u8), the softmax probability of that class
// (fp32) and a colour (u8 x 3, a palette entry, optionally blended over a grey image), without the full-resolution
// [B, K, H, W] logit tensor.  The inference counterpart of K31's label_ops.hip, whose addressing and work split this file keeps.
// Values.  v_k is K31's value: the raw logit when (H, W) == (h, w), otherwise the fp32 blend of resize_fwd_kernel
// (resize_ops.hip): src_index on both axes, bf16 taps widened first, hy * (hx * p00 + wx * p01) + wy * (hx * p10 + wx * p11)
// in that association; compiled with -ffp-contract=off like every other file, so the labels are those of oess_argmax_labels
// and of the composed path, bit for bit.
// Label = torch.argmax's rule: first index among equal maxima, NaN above everything, first NaN wins.
// Confidence = 1 / sum_k exp(v_k - v_max) in fp32, in ONE walk over K (running maximum and running sum: when class k takes
// the maximum the sum so far is rescaled by exp(old - new)); exp is __expf (v_exp_f32 on the log2(e) product).  The winner's
// own term is exp(0) = 1 exactly, so K equal values give exactly 1 / K.
// One lane owns a pixel from the first tap to its bytes: no atomics, no cross-lane floating-point reduction, two calls give the
// same bits.
// One workgroup per OUTPUT ROW (K31's split): the two source rows as fp32 [2][w][K] in LDS when they fit LDS_BUDGET, global
// taps (L1/L2 hits) otherwise, raw global reads at the input size.  The row is walked in chunks of THREADS pixels.  conf leaves
// as one dword per lane.  The label and colour bytes of a chunk are staged in LDS at the byte phase of their global address
// and leave as aligned dwords (64 + 192 dword stores per full chunk instead of 1 024 byte stores); only the ragged first / last
// dword of a chunk, which it shares with the neighbouring chunk or row, is written as bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"
#include "bilinear_axis.h"
#include "render_common.h"

namespace {
using namespace oess;
using namespace oess::render;              // Render, tap, take, emit, flush_chunk: render_common.h, shared with vocab_render.hip
constexpr size_t LDS_BUDGET = 48 * 1024;     // two fp32 source rows; with the 2 KB of staging below the 64 KB a launch gets

enum { RAW = 0, TAPS_LDS = 1, TAPS_GLOBAL = 2 };

template <bool BF16, int MODE>
__global__ __launch_bounds__(THREADS) void segment_render_kernel(const void* __restrict__ in, int64_t ips, int K, Axis ay, Axis ax,
                                                                 Render r) {
    extern __shared__ __attribute__((aligned(16))) float rows[];            // TAPS_LDS: [2][ax.in][K]
    __shared__ Stage st;
    const int oy = blockIdx.x % ay.out;
    const int64_t b = blockIdx.x / ay.out;
    const int64_t opix = (b * ay.out + oy) * (int64_t)ax.out;               // first output pixel of this row
    load_palette(st, r, K);
    int y0 = 0, y1 = 0; float wy = 0.f;
    if constexpr (MODE != RAW) src_index(ay, oy, y0, y1, wy);
    const float hy = 1.f - wy;
    const int64_t row0 = (b * ay.in + y0) * ax.in, row1 = (b * ay.in + y1) * ax.in;
    if constexpr (MODE == TAPS_LDS) {
        const int n = ax.in * K;
        for (int j = threadIdx.x; j < n; j += THREADS) {
            const int x = j / K, k = j - x * K;
            rows[j] = tap<BF16>(in, (row0 + x) * ips + k);
            rows[n + j] = tap<BF16>(in, (row1 + x) * ips + k);
        }
    }
    __syncthreads();                                                        // pal and rows
    // byte phase of the row's first label / colour byte; THREADS and 3 * THREADS are multiples of 4: one phase for every chunk
    const int lphase = r.labels ? (int)((uintptr_t)(r.labels + opix) & 3) : 0;
    const int cphase = r.rgb ? (int)((uintptr_t)(r.rgb + 3 * opix) & 3) : 0;
    for (int base = 0; base < ax.out; base += THREADS) {                    // uniform trip count: barriers inside
        const int ox = base + threadIdx.x;
        if (ox < ax.out) {
            float best, sum = 1.f;
            int idx = 0;
            if constexpr (MODE == RAW) {
                const int64_t q = ((b * ay.in + oy) * ax.in + ox) * ips;
                best = tap<BF16>(in, q);
                for (int k = 1; k < K; ++k) take(tap<BF16>(in, q + k), k, best, idx, sum);
            } else {
                int x0, x1; float wx;
                src_index(ax, ox, x0, x1, wx);
                const float hx = 1.f - wx;
                best = 0.f;
                for (int k = 0; k < K; ++k) {
                    float p00, p01, p10, p11;
                    if constexpr (MODE == TAPS_LDS) {
                        const float* r1 = rows + ax.in * K;
                        p00 = rows[x0 * K + k]; p01 = rows[x1 * K + k];
                        p10 = r1[x0 * K + k];   p11 = r1[x1 * K + k];
                    } else {
                        p00 = tap<BF16>(in, (row0 + x0) * ips + k); p01 = tap<BF16>(in, (row0 + x1) * ips + k);
                        p10 = tap<BF16>(in, (row1 + x0) * ips + k); p11 = tap<BF16>(in, (row1 + x1) * ips + k);
                    }
                    const float v = hy * (hx * p00 + wx * p01) + wy * (hx * p10 + wx * p11);     // resize_fwd_kernel's association
                    if (k == 0) best = v; else take(v, k, best, idx, sum);
                }
            }
            emit(st, r, K, opix + ox, lphase, cphase, idx, sum);
        }
        flush_chunk(st, r, opix + base, lphase, cphase, ax.out - base < THREADS ? ax.out - base : THREADS);
    }
}

}  // namespace

extern "C" {

int oess_segment_render(const void* logits, int is_bf16, long long pix_stride, int B, int K, int h, int w, int H, int W,
                        int align_corners, const uint8_t* palette, const uint8_t* grey, int alpha256, float min_conf,
                        int ignore_label, uint8_t* labels, float* conf, uint8_t* rgb, oess_stream_t stream) {
    if (!logits || (!labels && !conf && !rgb) || (rgb && !palette) || K < 1 || K > MAX_K || ignore_label < K || ignore_label > 255 ||
        alpha256 < 0 || alpha256 > 256 || !(min_conf >= 0.f) || B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || pix_stride < K)
        return OESS_EINVAL;
    // extents: one workgroup per output row (grid.x <= 2^31 - 1); element offsets of every tensor are int64 (rgb: 3 bytes a pixel,
    // conf: 4)
    int64_t in_elems, out_elems;
    if ((int64_t)B * H > INT32_MAX || (int64_t)B * h > INT32_MAX || (int64_t)w * K > INT32_MAX ||
        __builtin_mul_overflow((int64_t)B * h * w, (int64_t)pix_stride, &in_elems) ||
        __builtin_mul_overflow((int64_t)B * H, (int64_t)W, &out_elems) || in_elems > INT64_MAX / 4 || out_elems > INT64_MAX / 4)
        return OESS_EINVAL;
    const Axis ay = make_axis(h, H, align_corners), ax = make_axis(w, W, align_corners);
    Render r;
    r.palette = palette; r.grey = grey; r.labels = labels; r.conf = conf; r.rgb = rgb;
    r.alpha256 = alpha256; r.ignore_label = ignore_label; r.min_conf = min_conf;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((int64_t)B * H)), block(THREADS);
    const size_t lds = (size_t)2 * w * K * sizeof(float);
#define OESS_SR(BF, MODE, SH) \
    hipLaunchKernelGGL((segment_render_kernel<BF, MODE>), grid, block, SH, st, logits, (int64_t)pix_stride, K, ay, ax, r)
    if (H == h && W == w) { if (is_bf16) OESS_SR(true, RAW, 0); else OESS_SR(false, RAW, 0); }
    else if (lds <= LDS_BUDGET) { if (is_bf16) OESS_SR(true, TAPS_LDS, lds); else OESS_SR(false, TAPS_LDS, lds); }
    else { if (is_bf16) OESS_SR(true, TAPS_GLOBAL, 0); else OESS_SR(false, TAPS_GLOBAL, 0); }
#undef OESS_SR
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
