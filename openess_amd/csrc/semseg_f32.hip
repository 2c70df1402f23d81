// K15 fp32 SemSegE2VID inference: what the task decoder needs next to the K14 convolutions (conv_f32.hip).
//
//   InstanceNorm2d(affine=False) forward [+ residual] [+ ReLU] on oess_f32_view_t views, two launches:
//     1. partials: a workgroup owns (pixel range, channel group, sample).  A thread walks its pixels for V channels (V = 4: one
//        16-byte load per pixel) and keeps sums of (x - K) and (x - K)^2 shifted by its own first element K, which it turns
//        into (count, mean, M2).  The threads of a workgroup that share channels are merged with Chan's pairwise update in a
//        fixed LDS tree; one (mean, M2) per (sample, range, channel) goes to the workspace.
//     2. apply: every workgroup merges the ranges' partials of its channels (same update, same fixed order, so all workgroups
//        get the same bits), then writes (x - mean) * rstd [+ residual] [ReLU] for its own pixel range.
//   No E[x^2] - E[x]^2 on raw values, no atomics: results repeat bit for bit.
//
//   cat([nearest2x(x), skip], C): one gather kernel into an NHWC view (the fp32 sibling of oess_upsample_nearest2x_nhwc_bf16).
#include <hip/hip_runtime.h>

#include "oess.h"
#include "oess_common.h"

namespace {

#include "f32_view.h"

constexpr int NT = 256;
constexpr int MAX_CHUNKS = 256;          // pixel ranges per (sample, channel group): bounds the workspace and the merge loop
constexpr int MIN_CHUNK_PIX = 128;
constexpr int TARGET_BLOCKS = 2048;      // 8 workgroups per CU on 256 CUs when the map is large enough

struct NormParams {
    View in, res;
    float* out;
    long long ob, oy, ox, oc;
    int has_res, relu;
    int W, C, HW;
    int lanes_log2;                      // threads that share a pixel (each V channels)
    int nchunk, chunk_pix;
    float eps;
    float* part;                         // [B][nchunk][2][C]: mean, M2
    float* save_mean;                    // [B][C], nullable: the statistics, kept for a backward pass (K18)
    float* save_rstd;
};

#include "f32_chan.h"

template <int V>
__global__ __launch_bounds__(NT) void instnorm_partials_f32_kernel(const NormParams P) {
    __shared__ float sm[NT * (2 * V + 1)];
    const int tid = threadIdx.x, lane = tid & ((1 << P.lanes_log2) - 1), row = tid >> P.lanes_log2, rows = NT >> P.lanes_log2;
    const int c = ((blockIdx.y << P.lanes_log2) + lane) * V;
    const bool active = c < P.C;
    const int b = blockIdx.z, chunk = blockIdx.x;
    const int p0 = chunk * P.chunk_pix, p1 = min(p0 + P.chunk_pix, P.HW);
    const float* base = P.in.p + b * P.in.sb + c * P.in.sc;
    float K[V], s1[V], s2[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { K[i] = 0.f; s1[i] = 0.f; s2[i] = 0.f; }
    int cnt = 0;
    if (active) {
#pragma unroll 4
        for (int p = p0 + row; p < p1; p += rows) {
            const int y = p / P.W, x = p - y * P.W;
            const Vec<V> v = ldv<V>(base + y * P.in.sy + x * P.in.sx);
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
        float* o = P.part + ((long long)(b * P.nchunk + chunk) * 2) * P.C + c;
        Vec<V> vm, vq;
#pragma unroll
        for (int i = 0; i < V; ++i) { vm.v[i] = m[i]; vq.v[i] = q[i]; }
        stv<V>(o, vm);
        stv<V>(o + P.C, vq);
    }
}

template <int V>
__global__ __launch_bounds__(NT) void instnorm_apply_f32_kernel(const NormParams P) {
    __shared__ float sm[NT * (2 * V + 1)];
    __shared__ float stat[2 * 64];             // (mean, rstd) of the <= 64 channels of this workgroup
    const int tid = threadIdx.x, L = 1 << P.lanes_log2, lane = tid & (L - 1), row = tid >> P.lanes_log2, rows = NT >> P.lanes_log2;
    const int c = ((blockIdx.y << P.lanes_log2) + lane) * V;
    const bool active = c < P.C;
    const int b = blockIdx.z, chunk = blockIdx.x;
    // the statistics of this workgroup's channels: merge the ranges' partials, rows in parallel, then the fixed tree
    float n = 0.f, m[V], q[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { m[i] = 0.f; q[i] = 0.f; }
    if (active) {
        for (int k = row; k < P.nchunk; k += rows) {
            const float* o = P.part + ((long long)(b * P.nchunk + k) * 2) * P.C + c;
            const Vec<V> vm = ldv<V>(o), vq = ldv<V>(o + P.C);
            const int k0 = k * P.chunk_pix;
            chan<V>(n, m, q, (float)(min(k0 + P.chunk_pix, P.HW) - k0), vm.v, vq.v);
        }
    }
    merge_rows<V>(n, m, q, tid, P.lanes_log2, sm);
    if (row == 0) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
            stat[(lane * V + i) * 2] = m[i];
            stat[(lane * V + i) * 2 + 1] = active ? 1.0f / sqrtf(q[i] / n + P.eps) : 0.f;
        }
        if (P.save_mean && chunk == 0 && active) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                P.save_mean[(long long)b * P.C + c + i] = stat[(lane * V + i) * 2];
                P.save_rstd[(long long)b * P.C + c + i] = stat[(lane * V + i) * 2 + 1];
            }
        }
    }
    __syncthreads();
    if (!active) return;
    float mean[V], rstd[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { mean[i] = stat[(lane * V + i) * 2]; rstd[i] = stat[(lane * V + i) * 2 + 1]; }
    const int p0 = chunk * P.chunk_pix, p1 = min(p0 + P.chunk_pix, P.HW);
    const float* ib = P.in.p + b * P.in.sb + c * P.in.sc;
    const float* rb = P.has_res ? P.res.p + b * P.res.sb + c * P.res.sc : nullptr;
    float* ob = P.out + b * P.ob + c * P.oc;
#pragma unroll 4
    for (int p = p0 + row; p < p1; p += rows) {
        const int y = p / P.W, x = p - y * P.W;
        Vec<V> v = ldv<V>(ib + y * P.in.sy + x * P.in.sx);
#pragma unroll
        for (int i = 0; i < V; ++i) v.v[i] = (v.v[i] - mean[i]) * rstd[i];
        if (P.has_res) {
            const Vec<V> r = ldv<V>(rb + y * P.res.sy + x * P.res.sx);
#pragma unroll
            for (int i = 0; i < V; ++i) v.v[i] = v.v[i] + r.v[i];
        }
        if (P.relu) {
#pragma unroll
            for (int i = 0; i < V; ++i) v.v[i] = v.v[i] > 0.f ? v.v[i] : 0.f;
        }
        stv<V>(ob + y * P.oy + x * P.ox, v);
    }
}

struct CatParams {
    View in, skip;
    float* out;
    long long ob, oy, ox, oc;
    int Ho, Wo, C1, Ct;
    long long total;                     // B * Ho * Wo * (Ct / V)
};

template <int V>
__global__ __launch_bounds__(NT) void upsample_nearest2x_concat_f32_kernel(const CatParams P) {
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e >= P.total) return;
    const int cq = P.Ct / V;
    const int c = (int)(e % cq) * V;
    long long t = e / cq;
    const int x = (int)(t % P.Wo);
    t /= P.Wo;
    const int y = (int)(t % P.Ho), b = (int)(t / P.Ho);
    const float* src = c < P.C1 ? P.in.p + b * P.in.sb + (y >> 1) * P.in.sy + (x >> 1) * P.in.sx + c * P.in.sc
                                : P.skip.p + b * P.skip.sb + y * P.skip.sy + x * P.skip.sx + (c - P.C1) * P.skip.sc;
    stv<V>(P.out + b * P.ob + y * P.oy + x * P.ox + c * P.oc, ldv<V>(src));
}

int norm_forward(const oess_f32_view_t* in, int B, int H, int W, int C, float eps, int relu, const oess_f32_view_t* residual,
                 const oess_f32_view_t* out, float* save_mean, float* save_rstd, void* ws, size_t ws_bytes, oess_stream_t stream) {
    if (!view_ok(in) || !view_ok(out) || (residual && !residual->data) || !ws || ((uintptr_t)ws & 15) != 0) return OESS_EINVAL;
    if (!geometry_ok(B, H, W, C) || !(eps >= 0.f) || (relu != 0 && relu != 1)) return OESS_EINVAL;
    if (ws_bytes < oess_instance_norm_f32_workspace_bytes(B, H, W, C)) return OESS_ENOMEM;
    const bool vec = C % 4 == 0 && vec_ok(in) && vec_ok(out) && (!residual || vec_ok(residual));
    const int V = vec ? 4 : 1, max_lanes = vec ? 16 : 64;
    int lanes_log2 = 0;
    while ((1 << lanes_log2) < max_lanes && (1 << lanes_log2) * V < C) ++lanes_log2;
    const int lanes = 1 << lanes_log2, rows = NT / lanes;
    const int ncg = (C + lanes * V - 1) / (lanes * V);
    if (ncg > 65535) return OESS_EINVAL;
    const int HW = H * W;
    int nchunk = (TARGET_BLOCKS + B * ncg - 1) / (B * ncg);
    const int by_size = (HW + MIN_CHUNK_PIX - 1) / MIN_CHUNK_PIX;
    nchunk = nchunk < by_size ? nchunk : by_size;
    nchunk = nchunk < MAX_CHUNKS ? nchunk : MAX_CHUNKS;
    int chunk_pix = (HW + nchunk - 1) / nchunk;
    chunk_pix = (chunk_pix + rows - 1) / rows * rows;
    nchunk = (HW + chunk_pix - 1) / chunk_pix;
    NormParams P{};
    P.in = to_view(in);
    P.has_res = residual != nullptr;
    P.res = residual ? to_view(residual) : View{nullptr, 0, 0, 0, 0};
    P.out = (float*)out->data;
    P.ob = out->sb; P.oy = out->sy; P.ox = out->sx; P.oc = out->sc;
    P.relu = relu;
    P.W = W; P.C = C; P.HW = HW;
    P.lanes_log2 = lanes_log2;
    P.nchunk = nchunk; P.chunk_pix = chunk_pix;
    P.eps = eps;
    P.part = (float*)ws;
    P.save_mean = save_mean; P.save_rstd = save_rstd;
    const dim3 grid((unsigned)nchunk, (unsigned)ncg, (unsigned)B);
    if (vec) {
        hipLaunchKernelGGL(instnorm_partials_f32_kernel<4>, grid, dim3(NT), 0, (hipStream_t)stream, P);
        hipLaunchKernelGGL(instnorm_apply_f32_kernel<4>, grid, dim3(NT), 0, (hipStream_t)stream, P);
    } else {
        hipLaunchKernelGGL(instnorm_partials_f32_kernel<1>, grid, dim3(NT), 0, (hipStream_t)stream, P);
        hipLaunchKernelGGL(instnorm_apply_f32_kernel<1>, grid, dim3(NT), 0, (hipStream_t)stream, P);
    }
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // namespace

extern "C" {

size_t oess_instance_norm_f32_workspace_bytes(int B, int H, int W, int C) {
    if (!geometry_ok(B, H, W, C)) return 0;
    return (size_t)B * MAX_CHUNKS * 2 * C * sizeof(float);
}

int oess_instance_norm_fwd_f32(const oess_f32_view_t* in, int B, int H, int W, int C, float eps, int relu,
                               const oess_f32_view_t* residual, const oess_f32_view_t* out, void* ws, size_t ws_bytes,
                               oess_stream_t stream) {
    return norm_forward(in, B, H, W, C, eps, relu, residual, out, nullptr, nullptr, ws, ws_bytes, stream);
}

int oess_instance_norm_train_fwd_f32(const oess_f32_view_t* in, int B, int H, int W, int C, float eps, int relu,
                                     const oess_f32_view_t* residual, const oess_f32_view_t* out, float* save_mean, float* save_rstd,
                                     void* ws, size_t ws_bytes, oess_stream_t stream) {
    if (!save_mean || !save_rstd) return OESS_EINVAL;
    return norm_forward(in, B, H, W, C, eps, relu, residual, out, save_mean, save_rstd, ws, ws_bytes, stream);
}

int oess_upsample_nearest2x_concat_f32(const oess_f32_view_t* in, int B, int H, int W, int C, const oess_f32_view_t* skip,
                                       int C_skip, const oess_f32_view_t* out, oess_stream_t stream) {
    if (!view_ok(in) || !view_ok(out) || (skip && !skip->data)) return OESS_EINVAL;
    if (C_skip < 0 || (skip != nullptr) != (C_skip > 0) || H > (1 << 14) || W > (1 << 14)) return OESS_EINVAL;
    if (!geometry_ok(B, H, W, C) || !geometry_ok(B, 2 * H, 2 * W, C + C_skip)) return OESS_EINVAL;
    const bool vec = C % 4 == 0 && C_skip % 4 == 0 && vec_ok(in) && vec_ok(out) && (!skip || vec_ok(skip));
    const int V = vec ? 4 : 1;
    CatParams P{};
    P.in = to_view(in);
    P.skip = skip ? to_view(skip) : View{nullptr, 0, 0, 0, 0};
    P.out = (float*)out->data;
    P.ob = out->sb; P.oy = out->sy; P.ox = out->sx; P.oc = out->sc;
    P.Ho = 2 * H; P.Wo = 2 * W; P.C1 = C; P.Ct = C + C_skip;
    P.total = (long long)B * P.Ho * P.Wo * (P.Ct / V);
    const long long blocks = (P.total + NT - 1) / NT;
    if (blocks >= (1LL << 31)) return OESS_EINVAL;
    if (vec) hipLaunchKernelGGL(upsample_nearest2x_concat_f32_kernel<4>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(upsample_nearest2x_concat_f32_kernel<1>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, P);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
