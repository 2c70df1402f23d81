// K18 fp32 SemSegE2VID training: the backward of the two layers of semseg_f32.hip.
//
//   InstanceNorm2d(affine=False) [+ ReLU] backward on oess_f32_view_t views, two launches.  With xh = (x - mean) rstd (the
//   forward's own expression on the statistics it saved, so the ReLU mask xh > 0 is the forward's, bit for bit) and
//   g = dY [xh > 0] (ReLU) or dY:   dX = rstd (g - mean_hw(g) - xh mean_hw(g xh)).
//     1. partials: a workgroup owns (pixel range, channel group, sample); a thread keeps its own chains of g and g xh for V
//        channels (V = 4: 16-byte loads); the threads that share channels are added in a fixed LDS tree; one (sum g, sum g xh)
//        per (sample, range, channel) goes to the workspace.
//     2. apply: every workgroup adds the ranges' partials of its channels (rows in parallel, then the same tree: all workgroups
//        get the same bits) and writes dX for its own pixel range.
//   The residual variant needs no kernel: the residual's gradient is dY itself.
//
//   nearest x2 gather backward: dX[b, y, x, c] = ((d[2y][2x] + d[2y][2x+1]) + d[2y+1][2x]) + d[2y+1][2x+1] on the first C channels
//   of the concat gradient, read through a view.
//   No atomics: results repeat bit for bit.
#include <hip/hip_runtime.h>

#include "oess.h"
#include "oess_common.h"

namespace {

#include "f32_view.h"

constexpr int NT = 256;
constexpr int MAX_CHUNKS = 256;          // pixel ranges per (sample, channel group), as in the forward
constexpr int MIN_CHUNK_PIX = 128;
constexpr int TARGET_BLOCKS = 2048;

struct BwdParams {
    View x, dy;
    float* dx;
    long long ob, oy, ox, oc;
    int relu;
    int W, C, HW;
    int lanes_log2;                      // threads that share a pixel (each V channels)
    int nchunk, chunk_pix;
    const float* mean;                   // [B][C]
    const float* rstd;
    float* part;                         // [B][nchunk][2][C]: sum g, sum g xh
};

// add the rows (threads with the same lane) of a workgroup; the result is in row 0.  sm: NT * 2 V floats
template <int V>
__device__ __forceinline__ void sum_rows(float (&a)[V], float (&b)[V], int tid, int lanes_log2, float* sm) {
    constexpr int S = 2 * V;
    const int row = tid >> lanes_log2, rows = NT >> lanes_log2;
    float* me = sm + tid * S;
#pragma unroll
    for (int i = 0; i < V; ++i) { me[i] = a[i]; me[V + i] = b[i]; }
    __syncthreads();
    for (int s = rows >> 1; s >= 1; s >>= 1) {
        if (row < s) {
            const float* o = sm + (tid + (s << lanes_log2)) * S;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                a[i] = a[i] + o[i];
                b[i] = b[i] + o[V + i];
                me[i] = a[i];
                me[V + i] = b[i];
            }
        }
        __syncthreads();
    }
}

template <int V>
__global__ __launch_bounds__(NT) void instnorm_bwd_partials_f32_kernel(const BwdParams P) {
    __shared__ float sm[NT * 2 * V];
    const int tid = threadIdx.x, lane = tid & ((1 << P.lanes_log2) - 1), row = tid >> P.lanes_log2, rows = NT >> P.lanes_log2;
    const int c = ((blockIdx.y << P.lanes_log2) + lane) * V;
    const bool active = c < P.C;
    const int b = blockIdx.z, chunk = blockIdx.x;
    const int p0 = chunk * P.chunk_pix, p1 = min(p0 + P.chunk_pix, P.HW);
    float s1[V], s2[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
    if (active) {
        const float* xb = P.x.p + b * P.x.sb + c * P.x.sc;
        const float* gb = P.dy.p + b * P.dy.sb + c * P.dy.sc;
        const Vec<V> mean = ldv<V>(P.mean + (long long)b * P.C + c), rstd = ldv<V>(P.rstd + (long long)b * P.C + c);
#pragma unroll 4
        for (int p = p0 + row; p < p1; p += rows) {
            const int y = p / P.W, x = p - y * P.W;
            const Vec<V> v = ldv<V>(xb + y * P.x.sy + x * P.x.sx), g = ldv<V>(gb + y * P.dy.sy + x * P.dy.sx);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float xh = (v.v[i] - mean.v[i]) * rstd.v[i];
                const float gi = (P.relu && !(xh > 0.f)) ? 0.f : g.v[i];
                s1[i] = s1[i] + gi;
                s2[i] = s2[i] + gi * xh;
            }
        }
    }
    sum_rows<V>(s1, s2, tid, P.lanes_log2, sm);
    if (row == 0 && active) {
        float* o = P.part + ((long long)(b * P.nchunk + chunk) * 2) * P.C + c;
        Vec<V> v1, v2;
#pragma unroll
        for (int i = 0; i < V; ++i) { v1.v[i] = s1[i]; v2.v[i] = s2[i]; }
        stv<V>(o, v1);
        stv<V>(o + P.C, v2);
    }
}

template <int V>
__global__ __launch_bounds__(NT) void instnorm_bwd_apply_f32_kernel(const BwdParams P) {
    __shared__ float sm[NT * 2 * V];
    __shared__ float stat[2 * 64];             // (mean_hw(g), mean_hw(g xh)) of the <= 64 channels of this workgroup
    const int tid = threadIdx.x, L = 1 << P.lanes_log2, lane = tid & (L - 1), row = tid >> P.lanes_log2, rows = NT >> P.lanes_log2;
    const int c = ((blockIdx.y << P.lanes_log2) + lane) * V;
    const bool active = c < P.C;
    const int b = blockIdx.z, chunk = blockIdx.x;
    float s1[V], s2[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
    if (active) {
        for (int k = row; k < P.nchunk; k += rows) {
            const float* o = P.part + ((long long)(b * P.nchunk + k) * 2) * P.C + c;
            const Vec<V> v1 = ldv<V>(o), v2 = ldv<V>(o + P.C);
#pragma unroll
            for (int i = 0; i < V; ++i) { s1[i] = s1[i] + v1.v[i]; s2[i] = s2[i] + v2.v[i]; }
        }
    }
    sum_rows<V>(s1, s2, tid, P.lanes_log2, sm);
    if (row == 0) {
        const float n = (float)P.HW;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            stat[(lane * V + i) * 2] = s1[i] / n;
            stat[(lane * V + i) * 2 + 1] = s2[i] / n;
        }
    }
    __syncthreads();
    if (!active) return;
    float m1[V], m2[V];
#pragma unroll
    for (int i = 0; i < V; ++i) { m1[i] = stat[(lane * V + i) * 2]; m2[i] = stat[(lane * V + i) * 2 + 1]; }
    const Vec<V> mean = ldv<V>(P.mean + (long long)b * P.C + c), rstd = ldv<V>(P.rstd + (long long)b * P.C + c);
    const int p0 = chunk * P.chunk_pix, p1 = min(p0 + P.chunk_pix, P.HW);
    const float* xb = P.x.p + b * P.x.sb + c * P.x.sc;
    const float* gb = P.dy.p + b * P.dy.sb + c * P.dy.sc;
    float* ob = P.dx + b * P.ob + c * P.oc;
#pragma unroll 4
    for (int p = p0 + row; p < p1; p += rows) {
        const int y = p / P.W, x = p - y * P.W;
        const Vec<V> v = ldv<V>(xb + y * P.x.sy + x * P.x.sx), g = ldv<V>(gb + y * P.dy.sy + x * P.dy.sx);
        Vec<V> d;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float xh = (v.v[i] - mean.v[i]) * rstd.v[i];
            const float gi = (P.relu && !(xh > 0.f)) ? 0.f : g.v[i];
            d.v[i] = rstd.v[i] * ((gi - m1[i]) - xh * m2[i]);
        }
        stv<V>(ob + y * P.oy + x * P.ox, d);
    }
}

struct DownParams {
    View in;
    float* out;
    long long ob, oy, ox, oc;
    int H, W, C;
    long long total;                     // B * H * W * (C / V)
};

template <int V>
__global__ __launch_bounds__(NT) void downsample_sum2x_f32_kernel(const DownParams P) {
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e >= P.total) return;
    const int cq = P.C / V;
    const int c = (int)(e % cq) * V;
    long long t = e / cq;
    const int x = (int)(t % P.W);
    t /= P.W;
    const int y = (int)(t % P.H), b = (int)(t / P.H);
    const float* src = P.in.p + b * P.in.sb + (2 * y) * P.in.sy + (2 * x) * P.in.sx + c * P.in.sc;
    const Vec<V> a = ldv<V>(src), bb = ldv<V>(src + P.in.sx), cc = ldv<V>(src + P.in.sy), d = ldv<V>(src + P.in.sy + P.in.sx);
    Vec<V> r;
#pragma unroll
    for (int i = 0; i < V; ++i) r.v[i] = ((a.v[i] + bb.v[i]) + cc.v[i]) + d.v[i];
    stv<V>(P.out + b * P.ob + y * P.oy + x * P.ox + c * P.oc, r);
}

}  // namespace

extern "C" {

size_t oess_instance_norm_bwd_f32_workspace_bytes(int B, int H, int W, int C) {
    if (!geometry_ok(B, H, W, C)) return 0;
    return (size_t)B * MAX_CHUNKS * 2 * C * sizeof(float);
}

int oess_instance_norm_bwd_f32(const oess_f32_view_t* x, const oess_f32_view_t* dy, const float* mean, const float* rstd, int B, int H,
                               int W, int C, int relu, const oess_f32_view_t* dx, void* ws, size_t ws_bytes, oess_stream_t stream) {
    if (!view_ok(x) || !view_ok(dy) || !view_ok(dx) || !mean || !rstd || !ws || ((uintptr_t)ws & 15) != 0) return OESS_EINVAL;
    if (!geometry_ok(B, H, W, C) || (relu != 0 && relu != 1)) return OESS_EINVAL;
    if (ws_bytes < oess_instance_norm_bwd_f32_workspace_bytes(B, H, W, C)) return OESS_ENOMEM;
    const bool vec = C % 4 == 0 && vec_ok(x) && vec_ok(dy) && vec_ok(dx) && (((uintptr_t)mean | (uintptr_t)rstd) & 15) == 0;
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
    BwdParams P{};
    P.x = to_view(x);
    P.dy = to_view(dy);
    P.dx = (float*)dx->data;
    P.ob = dx->sb; P.oy = dx->sy; P.ox = dx->sx; P.oc = dx->sc;
    P.relu = relu;
    P.W = W; P.C = C; P.HW = HW;
    P.lanes_log2 = lanes_log2;
    P.nchunk = nchunk; P.chunk_pix = chunk_pix;
    P.mean = mean; P.rstd = rstd;
    P.part = (float*)ws;
    const dim3 grid((unsigned)nchunk, (unsigned)ncg, (unsigned)B);
    if (vec) {
        hipLaunchKernelGGL(instnorm_bwd_partials_f32_kernel<4>, grid, dim3(NT), 0, (hipStream_t)stream, P);
        hipLaunchKernelGGL(instnorm_bwd_apply_f32_kernel<4>, grid, dim3(NT), 0, (hipStream_t)stream, P);
    } else {
        hipLaunchKernelGGL(instnorm_bwd_partials_f32_kernel<1>, grid, dim3(NT), 0, (hipStream_t)stream, P);
        hipLaunchKernelGGL(instnorm_bwd_apply_f32_kernel<1>, grid, dim3(NT), 0, (hipStream_t)stream, P);
    }
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_downsample_sum2x_f32(const oess_f32_view_t* dout, int B, int H, int W, int C, const oess_f32_view_t* dx, oess_stream_t stream) {
    if (!view_ok(dout) || !view_ok(dx) || H > (1 << 14) || W > (1 << 14)) return OESS_EINVAL;
    if (!geometry_ok(B, H, W, C) || !geometry_ok(B, 2 * H, 2 * W, C)) return OESS_EINVAL;
    const bool vec = C % 4 == 0 && vec_ok(dout) && vec_ok(dx);
    const int V = vec ? 4 : 1;
    DownParams P{};
    P.in = to_view(dout);
    P.out = (float*)dx->data;
    P.ob = dx->sb; P.oy = dx->sy; P.ox = dx->sx; P.oc = dx->sc;
    P.H = H; P.W = W; P.C = C;
    P.total = (long long)B * H * W * (C / V);
    const long long blocks = (P.total + NT - 1) / NT;
    if (blocks >= (1LL << 31)) return OESS_EINVAL;
    if (vec) hipLaunchKernelGGL(downsample_sum2x_f32_kernel<4>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(downsample_sum2x_f32_kernel<1>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, P);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
