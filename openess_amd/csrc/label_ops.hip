// Class-label maps straight from low-resolution logits (K31): out[b, y, x] = argmax_k up(logits)[b, k, y, x] as int64, without
// the full-resolution [B, K, H, W] tensor that F.interpolate(...).argmax(1) writes and reads again (99 MB at 8 x 11 x 440 x 640
// for 18 MB of labels).
//   training/pretrain_trainer.py:513-514, :556-557   pl = logits.argmax(dim=1)              (if_switchable_train, epoch >= 5)
//   models/maskclip_model.py:903-908                 resize(logits, size=image).argmax(1)   (the online teacher's pseudo-labels)
// Every class value at an output pixel is the fp32 blend of resize_fwd_kernel (resize_ops.hip): src_index on both axes, bf16
// taps widened first, hy * (hx * p00 + wx * p01) + wy * (hx * p10 + wx * p11) in that association; this file is compiled with
// -ffp-contract=off like every other, so the values -- and with them the labels -- are those of the composed path, bit for bit.
// (H, W) == (h, w) interpolates nothing: the raw values are compared, so +-inf never meets a zero weight.
// Argmax rule = torch.argmax: first index among equal maxima, NaN above everything, first NaN wins.
// One workgroup per OUTPUT ROW.  The two source rows go as fp32 [2][w][K] into LDS when they fit LDS_BUDGET (6 KB at w = 40,
// K = 19), each lane then owns output pixels and walks K with a running maximum; neighbouring lanes of an upsampled row share
// their taps (LDS broadcast).  Rows that do not fit read the four taps from global memory (L1/L2 hits) -- no geometry is refused
// for its size.  Launch- and latency-bound at the sizes above: 3 520 workgroups, 0.4 MB read, 18 MB written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"
#include "bilinear_axis.h"

namespace {
using namespace oess;
constexpr int THREADS = 256;
constexpr size_t LDS_BUDGET = 48 * 1024;     // two fp32 source rows; below the 64 KB a launch gets without an attribute

enum { RAW = 0, TAPS_LDS = 1, TAPS_GLOBAL = 2 };

template <bool BF16>
__device__ __forceinline__ float tap(const void* __restrict__ p, int64_t off) {
    return BF16 ? bf16_to_f32(reinterpret_cast<const uint16_t*>(p)[off]) : reinterpret_cast<const float*>(p)[off];
}

// running maximum under torch.argmax's order: v replaces best when it is larger, or when it is the first NaN
__device__ __forceinline__ void take(float v, int k, float& best, int& idx) {
    if (v > best || (v != v && best == best)) { best = v; idx = k; }
}

template <bool BF16, int MODE>
__global__ __launch_bounds__(THREADS) void argmax_labels_kernel(const void* __restrict__ in, int64_t ips, int K, Axis ay, Axis ax,
                                                                int64_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rows[];            // TAPS_LDS: [2][ax.in][K]
    const int oy = blockIdx.x % ay.out;
    const int64_t b = blockIdx.x / ay.out;
    int64_t* __restrict__ orow = out + (b * ay.out + oy) * (int64_t)ax.out;
    if constexpr (MODE == RAW) {
        const int64_t row = (b * ay.in + oy) * ax.in;
        for (int ox = threadIdx.x; ox < ax.out; ox += THREADS) {
            const int64_t p = (row + ox) * ips;
            float best = tap<BF16>(in, p);
            int idx = 0;
            for (int k = 1; k < K; ++k) take(tap<BF16>(in, p + k), k, best, idx);
            orow[ox] = idx;
        }
        return;
    }
    int y0, y1; float wy;
    src_index(ay, oy, y0, y1, wy);
    const float hy = 1.f - wy;
    const int64_t row0 = (b * ay.in + y0) * ax.in, row1 = (b * ay.in + y1) * ax.in;
    if constexpr (MODE == TAPS_LDS) {
        const int n = ax.in * K;
        for (int j = threadIdx.x; j < n; j += THREADS) {
            const int x = j / K, k = j - x * K;
            rows[j] = tap<BF16>(in, (row0 + x) * ips + k);
            rows[n + j] = tap<BF16>(in, (row1 + x) * ips + k);
        }
        __syncthreads();
    }
    for (int ox = threadIdx.x; ox < ax.out; ox += THREADS) {
        int x0, x1; float wx;
        src_index(ax, ox, x0, x1, wx);
        const float hx = 1.f - wx;
        float best = 0.f;
        int idx = 0;
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
            if (k == 0) best = v; else take(v, k, best, idx);
        }
        orow[ox] = idx;
    }
}

}  // namespace

extern "C" {

int oess_argmax_labels(const void* logits, int is_bf16, long long pix_stride, int B, int K, int h, int w, int H, int W,
                       int align_corners, int64_t* out, oess_stream_t stream) {
    if (!logits || !out || K < 1 || K > 256 || B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || pix_stride < K) return OESS_EINVAL;
    // extents: one workgroup per output row (grid.x <= 2^31 - 1); element offsets of both tensors are int64
    int64_t in_elems, out_elems;
    if ((int64_t)B * H > INT32_MAX || (int64_t)B * h > INT32_MAX || (int64_t)w * K > INT32_MAX ||
        __builtin_mul_overflow((int64_t)B * h * w, (int64_t)pix_stride, &in_elems) ||
        __builtin_mul_overflow((int64_t)B * H, (int64_t)W, &out_elems) || in_elems > INT64_MAX / 4 || out_elems > INT64_MAX / 8)
        return OESS_EINVAL;
    const Axis ay = make_axis(h, H, align_corners), ax = make_axis(w, W, align_corners);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((int64_t)B * H)), block(THREADS);
    const size_t lds = (size_t)2 * w * K * sizeof(float);
#define OESS_AL(BF, MODE, SH) \
    hipLaunchKernelGGL((argmax_labels_kernel<BF, MODE>), grid, block, SH, st, logits, (int64_t)pix_stride, K, ay, ax, out)
    if (H == h && W == w) { if (is_bf16) OESS_AL(true, RAW, 0); else OESS_AL(false, RAW, 0); }
    else if (lds <= LDS_BUDGET) { if (is_bf16) OESS_AL(true, TAPS_LDS, lds); else OESS_AL(false, TAPS_LDS, lds); }
    else { if (is_bf16) OESS_AL(true, TAPS_GLOBAL, 0); else OESS_AL(false, TAPS_GLOBAL, 0); }
#undef OESS_AL
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
