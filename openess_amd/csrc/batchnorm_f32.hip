// K17 fp32 image-teacher inference: nn.BatchNorm2d in TRAIN mode (batch statistics over B x H x W per channel, running
// statistics moved one momentum step) [+ residual] [+ ReLU] on oess_f32_view_t views, three launches:
//     1. partials: a workgroup owns (pixel range of the B H W pixels, channel group).  A thread walks its pixels for V channels
//        (V = 4: one 16-byte load per pixel) and keeps sums of (x - K) and (x - K)^2 shifted by its own first element K, which
//        it turns into (count, mean, M2).  The threads of a workgroup that share channels are merged with Chan's pairwise
//        update in a fixed LDS tree (f32_chan.h); one (mean, M2) per (range, channel) goes to the workspace.
//     2. finalize: one workgroup per channel group merges the ranges' partials (rows in parallel, then the same tree), writes
//        save_mean / save_var, moves the running statistics and leaves (mean, gamma * rstd, beta) per channel in the workspace.
//     3. apply: (x - mean) * (gamma * rstd) + beta [+ residual] [ReLU] for every pixel: one load and one store per element.
//   No E[x^2] - E[x]^2 on raw values, no atomics: results repeat bit for bit.  The input is read twice and written once:
//   12 bytes per element (16 with a residual), which is what bounds it.
#include <hip/hip_runtime.h>

#include "oess.h"
#include "oess_common.h"

namespace {

#include "f32_view.h"

constexpr int NT = 256;

#include "f32_chan.h"

constexpr int MAX_CHUNKS = 1024;         // pixel ranges per channel group: bounds the workspace and the merge loop
constexpr int MIN_CHUNK_PIX = 128;
constexpr int TARGET_BLOCKS = 2048;      // 8 workgroups per CU on 256 CUs when the map is large enough

struct BNParams {
    View in, res;
    float* out;
    long long ob, oy, ox, oc;
    int has_res, relu;
    int flat;                            // every view addresses pixel p = (b H + y) W + x at p * sx: no division per pixel
    int W, HW, C;
    int P;                               // B H W
    int lanes_log2;                      // threads that share a pixel (each V channels)
    int nchunk, chunk_pix;
    float eps, momentum;
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    float* save_mean;
    float* save_var;
    float* part;                         // [nchunk][2][C]: mean, M2
    float* coef;                         // [3][C]: mean, gamma * rstd, beta
};

__device__ __forceinline__ long long pix_off(int p, int flat, int HW, int W, long long sb, long long sy, long long sx) {
    if (flat) return p * sx;
    const int b = p / HW, r = p - b * HW, y = r / W, x = r - y * W;
    return b * sb + y * sy + x * sx;
}

template <int V>
__global__ __launch_bounds__(NT) void bn_partials_f32_kernel(const BNParams P) {
    __shared__ float sm[NT * (2 * V + 1)];
    const int tid = threadIdx.x, lane = tid & ((1 << P.lanes_log2) - 1), row = tid >> P.lanes_log2, rows = NT >> P.lanes_log2;
    const int c = ((blockIdx.y << P.lanes_log2) + lane) * V;
    const bool active = c < P.C;
    const int chunk = blockIdx.x;
    const int p0 = chunk * P.chunk_pix, p1 = min(p0 + P.chunk_pix, P.P);
    const float* base = P.in.p + c * P.in.sc;
    float K[V], s1[V], s2[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { K[i] = 0.f; s1[i] = 0.f; s2[i] = 0.f; }
    int cnt = 0;
    if (active) {
#pragma unroll 4
        for (int p = p0 + row; p < p1; p += rows) {
            const Vec<V> v = ldv<V>(base + pix_off(p, P.flat, P.HW, P.W, P.in.sb, P.in.sy, P.in.sx));
            if (cnt == 0) {
#pragma unroll
                for (int i = 0; i < V; ++i) K[i] = v.v[i];
            }
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float d = v.v[i] - K[i];
                s1[i] += d;
                s2[i] += d * d;
            }
            ++cnt;
        }
    }
    float n = (float)cnt, m[V], q[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const float a = cnt ? s1[i] / n : 0.f;
        const float r = cnt ? s2[i] - s1[i] * a : 0.f;
        m[i] = K[i] + a;
        q[i] = r > 0.f ? r : 0.f;
    }
    merge_rows<V>(n, m, q, tid, P.lanes_log2, sm);
    if (row == 0 && active) {
        float* o = P.part + (long long)chunk * 2 * P.C + c;
        Vec<V> vm, vq;
#pragma unroll
        for (int i = 0; i < V; ++i) { vm.v[i] = m[i]; vq.v[i] = q[i]; }
        stv<V>(o, vm);
        stv<V>(o + P.C, vq);
    }
}

template <int V>
__global__ __launch_bounds__(NT) void bn_finalize_f32_kernel(const BNParams P) {
    __shared__ float sm[NT * (2 * V + 1)];
    const int tid = threadIdx.x, lane = tid & ((1 << P.lanes_log2) - 1), row = tid >> P.lanes_log2, rows = NT >> P.lanes_log2;
    const int c = ((blockIdx.x << P.lanes_log2) + lane) * V;
    const bool active = c < P.C;
    float n = 0.f, m[V], q[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { m[i] = 0.f; q[i] = 0.f; }
    if (active) {
        for (int k = row; k < P.nchunk; k += rows) {
            const float* o = P.part + (long long)k * 2 * P.C + c;
            const Vec<V> vm = ldv<V>(o), vq = ldv<V>(o + P.C);
            const int k0 = k * P.chunk_pix;
            chan<V>(n, m, q, (float)(min(k0 + P.chunk_pix, P.P) - k0), vm.v, vq.v);
        }
    }
    merge_rows<V>(n, m, q, tid, P.lanes_log2, sm);
    if (row != 0 || !active) return;
    const float count = (float)P.P;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int ci = c + i;
        const float var = q[i] / count;
        const float rstd = 1.0f / sqrtf(var + P.eps);
        if (P.save_mean) P.save_mean[ci] = m[i];
        if (P.save_var) P.save_var[ci] = var;
        if (P.running_mean) {
            P.running_mean[ci] = (1.0f - P.momentum) * P.running_mean[ci] + P.momentum * m[i];
            P.running_var[ci] = (1.0f - P.momentum) * P.running_var[ci] + P.momentum * (q[i] / (count - 1.0f));
        }
        P.coef[ci] = m[i];
        P.coef[P.C + ci] = P.gamma ? P.gamma[ci] * rstd : rstd;
        P.coef[2 * P.C + ci] = P.beta ? P.beta[ci] : 0.f;
    }
}

template <int V>
__global__ __launch_bounds__(NT) void bn_apply_f32_kernel(const BNParams P) {
    const int tid = threadIdx.x, lane = tid & ((1 << P.lanes_log2) - 1), row = tid >> P.lanes_log2, rows = NT >> P.lanes_log2;
    const int c = ((blockIdx.y << P.lanes_log2) + lane) * V;
    if (c >= P.C) return;
    const Vec<V> mean = ldv<V>(P.coef + c), scale = ldv<V>(P.coef + P.C + c), shift = ldv<V>(P.coef + 2 * P.C + c);
    const int p0 = blockIdx.x * P.chunk_pix, p1 = min(p0 + P.chunk_pix, P.P);
    const float* ib = P.in.p + c * P.in.sc;
    const float* rb = P.has_res ? P.res.p + c * P.res.sc : nullptr;
    float* ob = P.out + c * P.oc;
#pragma unroll 4
    for (int p = p0 + row; p < p1; p += rows) {
        Vec<V> v = ldv<V>(ib + pix_off(p, P.flat, P.HW, P.W, P.in.sb, P.in.sy, P.in.sx));
#pragma unroll
        for (int i = 0; i < V; ++i) v.v[i] = (v.v[i] - mean.v[i]) * scale.v[i] + shift.v[i];
        if (P.has_res) {
            const Vec<V> r = ldv<V>(rb + pix_off(p, P.flat, P.HW, P.W, P.res.sb, P.res.sy, P.res.sx));
#pragma unroll
            for (int i = 0; i < V; ++i) v.v[i] = v.v[i] + r.v[i];
        }
        if (P.relu) {
#pragma unroll
            for (int i = 0; i < V; ++i) v.v[i] = v.v[i] > 0.f ? v.v[i] : 0.f;
        }
        stv<V>(ob + pix_off(p, P.flat, P.HW, P.W, P.ob, P.oy, P.ox), v);
    }
}

bool flat_view(const oess_f32_view_t* v, int H, int W) { return v->sy == W * v->sx && v->sb == H * v->sy; }

// pixel indices are ints: B H W < 2^30 keeps p0 + chunk_pix and p + rows below 2^31
bool bn_geometry_ok(int B, int H, int W, int C) { return geometry_ok(B, H, W, C) && (long long)B * H * W < (1LL << 30); }

}  // namespace

extern "C" {

size_t oess_batch_norm_train_f32_workspace_bytes(int B, int H, int W, int C) {
    if (!bn_geometry_ok(B, H, W, C)) return 0;
    return (size_t)(2 * MAX_CHUNKS + 3) * C * sizeof(float);
}

int oess_batch_norm_train_fwd_f32(const oess_f32_view_t* in, int B, int H, int W, int C, const float* gamma, const float* beta,
                                  float eps, float momentum, float* running_mean, float* running_var, float* save_mean,
                                  float* save_var, int relu, const oess_f32_view_t* residual, const oess_f32_view_t* out, void* ws,
                                  size_t ws_bytes, oess_stream_t stream) {
    if (!view_ok(in) || !view_ok(out) || (residual && !residual->data) || !ws || ((uintptr_t)ws & 15) != 0) return OESS_EINVAL;
    if (!bn_geometry_ok(B, H, W, C) || !(eps >= 0.f) || !(momentum >= 0.f && momentum <= 1.f) || (relu != 0 && relu != 1)) return OESS_EINVAL;
    if ((running_mean == nullptr) != (running_var == nullptr)) return OESS_EINVAL;
    const long long pixels = (long long)B * H * W;
    if (pixels < 2) return OESS_EINVAL;                     // torch: "Expected more than 1 value per channel when training"
    if (ws_bytes < oess_batch_norm_train_f32_workspace_bytes(B, H, W, C)) return OESS_ENOMEM;
    const bool vec = C % 4 == 0 && vec_ok(in) && vec_ok(out) && (!residual || vec_ok(residual));
    const int V = vec ? 4 : 1, max_lanes = vec ? 16 : 64;
    int lanes_log2 = 0;
    while ((1 << lanes_log2) < max_lanes && (1 << lanes_log2) * V < C) ++lanes_log2;
    const int lanes = 1 << lanes_log2, rows = NT / lanes;
    const int ncg = (C + lanes * V - 1) / (lanes * V);
    if (ncg > 65535) return OESS_EINVAL;
    long long nchunk = (TARGET_BLOCKS + ncg - 1) / ncg;
    const long long by_size = (pixels + MIN_CHUNK_PIX - 1) / MIN_CHUNK_PIX;
    nchunk = nchunk < by_size ? nchunk : by_size;
    nchunk = nchunk < MAX_CHUNKS ? nchunk : MAX_CHUNKS;
    long long chunk_pix = (pixels + nchunk - 1) / nchunk;
    chunk_pix = (chunk_pix + rows - 1) / rows * rows;
    nchunk = (pixels + chunk_pix - 1) / chunk_pix;
    BNParams P{};
    P.in = to_view(in);
    P.has_res = residual != nullptr;
    P.res = residual ? to_view(residual) : View{nullptr, 0, 0, 0, 0};
    P.out = (float*)out->data;
    P.ob = out->sb; P.oy = out->sy; P.ox = out->sx; P.oc = out->sc;
    P.relu = relu;
    P.flat = flat_view(in, H, W) && flat_view(out, H, W) && (!residual || flat_view(residual, H, W));
    P.W = W; P.HW = H * W; P.C = C; P.P = (int)pixels;
    P.lanes_log2 = lanes_log2;
    P.nchunk = (int)nchunk; P.chunk_pix = (int)chunk_pix;
    P.eps = eps; P.momentum = momentum;
    P.gamma = gamma; P.beta = beta;
    P.running_mean = running_mean; P.running_var = running_var;
    P.save_mean = save_mean; P.save_var = save_var;
    P.part = (float*)ws;
    P.coef = P.part + (size_t)2 * MAX_CHUNKS * C;
    const dim3 grid((unsigned)nchunk, (unsigned)ncg);
    if (vec) {
        hipLaunchKernelGGL(bn_partials_f32_kernel<4>, grid, dim3(NT), 0, (hipStream_t)stream, P);
        hipLaunchKernelGGL(bn_finalize_f32_kernel<4>, dim3((unsigned)ncg), dim3(NT), 0, (hipStream_t)stream, P);
        hipLaunchKernelGGL(bn_apply_f32_kernel<4>, grid, dim3(NT), 0, (hipStream_t)stream, P);
    } else {
        hipLaunchKernelGGL(bn_partials_f32_kernel<1>, grid, dim3(NT), 0, (hipStream_t)stream, P);
        hipLaunchKernelGGL(bn_finalize_f32_kernel<1>, dim3((unsigned)ncg), dim3(NT), 0, (hipStream_t)stream, P);
        hipLaunchKernelGGL(bn_apply_f32_kernel<1>, grid, dim3(NT), 0, (hipStream_t)stream, P);
    }
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
