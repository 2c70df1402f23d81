// K22 fp32 DeepLabv3-R50 training: what the ASPP head needs next to the K18 / K21 layer set (conv_wgrad_f32.hip,
// resnet_bwd_f32.hip) and the pooling branch's kernels (small_ops.hip, oess_aspp_pool_bwd_f32o).
//
//   Dropout on oess_f32_view_t views: y = x * (1 / (1 - p)) where the element is kept, 0.0f where it is dropped.  One thread
//   owns 8 channels of one pixel and makes ONE Philox-4x32-10 call (philox.h): the keep decision of element (pixel, c) is, bit for
//   bit, that of the bf16 kernel (small_ops.hip) for the same (seed, offset, P, C), so a model that alternates bf16 and fp32
//   steps walks one mask sequence.  The mask is a function of (seed, offset, element) alone: the backward pass is the same kernel
//   on the gradient.  V = 4: two 16-byte loads and stores (dense 16-byte aligned channels in both views); V = 1: element accesses
//   (NCHW and odd strides).  In place (y == x) is fine: a thread reads its 8 elements before it writes them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "oess.h"
#include "oess_common.h"
#include "philox.h"

namespace {
using namespace oess;

#include "f32_view.h"

constexpr int NT = 256;

struct DropParams {
    View in;
    float* out;
    long long ob, oy, ox, oc;
    int H, W, C;
    long long total;                     // B * H * W * (C / 8)
    unsigned thr;
    float scale;
    unsigned long long seed, offset;
};

template <int V>
__global__ __launch_bounds__(NT) void dropout_f32_kernel(const DropParams P) {
    const int c8 = P.C >> 3;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < P.total; i += (long long)gridDim.x * NT) {
        const long long pix = i / c8;
        const int c0 = (int)(i - pix * c8) * 8;
        long long t = pix;
        const int x = (int)(t % P.W);
        t /= P.W;
        const int y = (int)(t % P.H);
        const long long b = t / P.H;
        const uint4 r = dropout_words(i, P.seed, P.offset);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
        const float* src = P.in.p + b * P.in.sb + y * P.in.sy + x * P.in.sx + c0 * P.in.sc;
        float* dst = P.out + b * P.ob + y * P.oy + x * P.ox + c0 * P.oc;
        float f[8];
#pragma unroll
        for (int k = 0; k < 8; k += V) {
            const Vec<V> v = ldv<V>(src + k * P.in.sc);
#pragma unroll
            for (int j = 0; j < V; ++j) f[k + j] = v.v[j];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = dropout_keep(w, k, P.thr) ? f[k] * P.scale : 0.0f;
#pragma unroll
        for (int k = 0; k < 8; k += V) {
            Vec<V> o;
#pragma unroll
            for (int j = 0; j < V; ++j) o.v[j] = f[k + j];
            stv<V>(dst + k * P.oc, o);
        }
    }
}

}  // namespace

extern "C" {

int oess_dropout_f32(const oess_f32_view_t* x, const oess_f32_view_t* y, int B, int H, int W, int C, float p, unsigned long long seed,
                     unsigned long long offset, oess_stream_t stream) {
    if (!view_ok(x) || !view_ok(y) || !geometry_ok(B, H, W, C) || (C & 7) || !(p >= 0.f && p < 1.f)) return OESS_EINVAL;
    DropParams P{};
    P.in = to_view(x);
    P.out = (float*)y->data;
    P.ob = y->sb; P.oy = y->sy; P.ox = y->sx; P.oc = y->sc;
    P.H = H; P.W = W; P.C = C;
    P.total = (long long)B * H * W * (C >> 3);
    P.thr = dropout_threshold(p);
    P.scale = 1.0f / (1.0f - p);
    P.seed = seed; P.offset = offset;
    long long blocks = (P.total + NT - 1) / NT;
    const long long cap = (long long)num_cus() * 16;
    if (blocks > cap) blocks = cap;
    if (vec_ok(x) && vec_ok(y)) hipLaunchKernelGGL(dropout_f32_kernel<4>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(dropout_f32_kernel<1>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, P);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
