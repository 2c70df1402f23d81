// K16 fp32 DeepLabv3-R50 inference: the two pooling layers the network needs next to the fp32 convolutions (conv_f32.hip).
//
//   MaxPool2d(3, stride 2, padding 1) on oess_f32_view_t views: one thread per output pixel and V channels (V = 4: 16-byte
//   loads and stores); padding never wins (-inf), a NaN in the window wins, as in ATen.
//
//   AdaptiveAvgPool2d(1), two launches:
//     1. partials: a workgroup owns (pixel range, channel group, sample); a thread adds its pixels for V channels one after the
//        other, the threads that share channels are added in a fixed LDS tree; one sum per (sample, range, channel) goes to the
//        workspace.
//     2. finish: one thread per (sample, channel) adds the ranges' sums in index order and divides by H W.
//   Fixed order, no atomics: results repeat bit for bit.  A thread's own serial chain is chunk_pix / rows terms: 18 at the ASPP
//   call (a 28 x 40 map, 2048 channels), but MAX_CHUNKS caps the ranges, so it grows with H W beyond that (about 275 terms on a
//   440 x 640 map of 64 or more channels); the tree and the finish loop add log2(rows) + nchunk terms.
#include <hip/hip_runtime.h>

#include "oess.h"
#include "oess_common.h"

namespace {

#include "f32_view.h"

constexpr int NT = 256;
constexpr int MAX_CHUNKS = 64;           // pixel ranges per (sample, channel group): bounds the workspace and the finish loop
constexpr int MIN_CHUNK_PIX = 64;
constexpr int TARGET_BLOCKS = 1024;

struct PoolParams {
    View in;
    float* out;
    long long ob, oy, ox, oc;
    int H, W, Ho, Wo, C;
    long long total;                     // B * Ho * Wo * (C / V)
};

template <int V>
__global__ __launch_bounds__(NT) void maxpool3x3s2_f32_kernel(const PoolParams P) {
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e >= P.total) return;
    const int cq = P.C / V;
    const int c = (int)(e % cq) * V;
    long long t = e / cq;
    const int ox = (int)(t % P.Wo);
    t /= P.Wo;
    const int oy = (int)(t % P.Ho), b = (int)(t / P.Ho);
    Vec<V> m;
#pragma unroll
    for (int i = 0; i < V; ++i) m.v[i] = -INFINITY;
    const float* base = P.in.p + b * P.in.sb + c * P.in.sc;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int y = 2 * oy - 1 + r;
        if (y < 0 || y >= P.H) continue;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int x = 2 * ox - 1 + s;
            if (x < 0 || x >= P.W) continue;
            const Vec<V> v = ldv<V>(base + y * P.in.sy + x * P.in.sx);
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (v.v[i] > m.v[i] || v.v[i] != v.v[i]) m.v[i] = v.v[i];
        }
    }
    stv<V>(P.out + b * P.ob + oy * P.oy + ox * P.ox + c * P.oc, m);
}

struct AvgParams {
    View in;
    int W, C, HW;
    int lanes_log2;                      // threads that share a pixel (each V channels)
    int nchunk, chunk_pix;
    float* part;                         // [B][nchunk][C]
    float* out;                          // [B][C]
    long long total;                     // B * C
};

template <int V>
__global__ __launch_bounds__(NT) void avgpool_partials_f32_kernel(const AvgParams P) {
    __shared__ float sm[NT * V];
    const int tid = threadIdx.x, lane = tid & ((1 << P.lanes_log2) - 1), row = tid >> P.lanes_log2, rows = NT >> P.lanes_log2;
    const int c = ((blockIdx.y << P.lanes_log2) + lane) * V;
    const bool active = c < P.C;
    const int b = blockIdx.z, chunk = blockIdx.x;
    const int p0 = chunk * P.chunk_pix, p1 = min(p0 + P.chunk_pix, P.HW);
    float s[V];
#pragma unroll
    for (int i = 0; i < V; ++i) s[i] = 0.f;
    if (active) {
        const float* base = P.in.p + b * P.in.sb + c * P.in.sc;
#pragma unroll 4
        for (int p = p0 + row; p < p1; p += rows) {
            const int y = p / P.W, x = p - y * P.W;
            const Vec<V> v = ldv<V>(base + y * P.in.sy + x * P.in.sx);
#pragma unroll
            for (int i = 0; i < V; ++i) s[i] += v.v[i];
        }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) sm[tid * V + i] = s[i];
    __syncthreads();
    for (int h = rows >> 1; h >= 1; h >>= 1) {
        if (row < h) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                s[i] += sm[(tid + (h << P.lanes_log2)) * V + i];
                sm[tid * V + i] = s[i];
            }
        }
        __syncthreads();
    }
    if (row == 0 && active) {
        Vec<V> o;
#pragma unroll
        for (int i = 0; i < V; ++i) o.v[i] = s[i];
        stv<V>(P.part + (long long)(b * P.nchunk + chunk) * P.C + c, o);
    }
}

__global__ __launch_bounds__(NT) void avgpool_finish_f32_kernel(const AvgParams P) {
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e >= P.total) return;
    const int b = (int)(e / P.C), c = (int)(e - (long long)b * P.C);
    float s = 0.f;
    for (int k = 0; k < P.nchunk; ++k) s += P.part[(long long)(b * P.nchunk + k) * P.C + c];
    P.out[e] = s / (float)P.HW;
}


}  // namespace

extern "C" {

int oess_maxpool3x3s2_fwd_f32(const oess_f32_view_t* in, int B, int H, int W, int C, const oess_f32_view_t* out,
                              oess_stream_t stream) {
    if (!view_ok(in) || !view_ok(out) || !geometry_ok(B, H, W, C)) return OESS_EINVAL;
    const bool vec = C % 4 == 0 && vec_ok(in) && vec_ok(out);
    const int V = vec ? 4 : 1;
    PoolParams P{};
    P.in = to_view(in);
    P.out = (float*)out->data;
    P.ob = out->sb; P.oy = out->sy; P.ox = out->sx; P.oc = out->sc;
    P.H = H; P.W = W; P.Ho = (H - 1) / 2 + 1; P.Wo = (W - 1) / 2 + 1; P.C = C;
    P.total = (long long)B * P.Ho * P.Wo * (C / V);
    const long long blocks = (P.total + NT - 1) / NT;
    if (blocks >= (1LL << 31)) return OESS_EINVAL;
    if (vec) hipLaunchKernelGGL(maxpool3x3s2_f32_kernel<4>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(maxpool3x3s2_f32_kernel<1>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, P);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

size_t oess_global_avg_pool_f32_workspace_bytes(int B, int H, int W, int C) {
    if (!geometry_ok(B, H, W, C)) return 0;
    return (size_t)B * MAX_CHUNKS * C * sizeof(float);
}

int oess_global_avg_pool_fwd_f32(const oess_f32_view_t* in, int B, int H, int W, int C, float* out, void* ws, size_t ws_bytes,
                                 oess_stream_t stream) {
    if (!view_ok(in) || !out || ((uintptr_t)out & 3) != 0 || !ws || ((uintptr_t)ws & 15) != 0) return OESS_EINVAL;
    if (!geometry_ok(B, H, W, C)) return OESS_EINVAL;
    if (ws_bytes < oess_global_avg_pool_f32_workspace_bytes(B, H, W, C)) return OESS_ENOMEM;
    const bool vec = C % 4 == 0 && vec_ok(in);
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
    AvgParams P{};
    P.in = to_view(in);
    P.W = W; P.C = C; P.HW = HW;
    P.lanes_log2 = lanes_log2;
    P.nchunk = nchunk; P.chunk_pix = chunk_pix;
    P.part = (float*)ws;
    P.out = out;
    P.total = (long long)B * C;
    const dim3 grid((unsigned)nchunk, (unsigned)ncg, (unsigned)B);
    if (vec) hipLaunchKernelGGL(avgpool_partials_f32_kernel<4>, grid, dim3(NT), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(avgpool_partials_f32_kernel<1>, grid, dim3(NT), 0, (hipStream_t)stream, P);
    hipLaunchKernelGGL(avgpool_finish_f32_kernel, dim3((unsigned)((P.total + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, P);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
