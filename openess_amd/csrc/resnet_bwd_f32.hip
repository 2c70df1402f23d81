// K21 fp32 ResNet-50 training: the backward of the two layers the backbone has next to its convolutions.
//
//   BatchNorm2d (train mode) [+ residual] [+ ReLU] backward on oess_f32_view_t views, two launches with the forward's geometry
//   (batchnorm_f32.hip).  With rstd = 1 / sqrt(var + eps), xh = (x - mean) rstd and g = dY [out > 0] (ReLU; out is the forward's
//   OUTPUT, so the mask is the forward's bit for bit) or dY:
//       dbeta = sum g,  dgamma = sum g xh,  dX = gamma rstd (g - mean_P(g) - xh mean_P(g xh)),  d residual = g.
//     1. partials: a workgroup owns (pixel range, channel group); a thread keeps its own sums of g and g xh for V channels
//        (V = 4: 16-byte loads) in two levels of at most CHAIN terms each, so no fp32 chain grows with the map; the threads that
//        share channels are added in a fixed LDS tree; one (sum g, sum g xh) per (range, channel) goes to the workspace.
//     2. apply: every workgroup adds the ranges' partials of its channels (rows in parallel, each in index order, then the same
//        tree: all workgroups get the same bits), the first range's workgroup writes dgamma / dbeta, and each writes dX and
//        d residual for its own pixel range.
//   The number of ranges is a function of the shapes alone; what is not asked for is neither computed nor stored.
//
//   MaxPool2d(3, stride 2, padding 1) backward in gather form: one thread per INPUT pixel and V channels looks at the up to four
//   windows that contain it, recomputes each window's winner from x with ATen's rule (scan in row-major order, a value wins when
//   it is greater than the running maximum or is a NaN; padding never wins) and adds the dY of the windows it won, rows first.
//   No atomics anywhere: results repeat bit for bit.
#include <hip/hip_runtime.h>

#include "oess.h"
#include "oess_common.h"

namespace {

#include "f32_view.h"

constexpr int NT = 256;
constexpr int CHAIN = 64;                // longest run of one fp32 accumulator
constexpr int MIN_CHUNK_PIX = 128;
constexpr int TARGET_BLOCKS = 512;       // every workgroup of launch 2 re-reads the partials of its channels: keep them few

struct BNBwdParams {
    View x, out, dy;
    float* dx;
    long long xb, xy, xx, xc;            // strides of dx
    float* dres;
    long long rb, ry, rx, rc;
    int relu, need_sums;
    int flat;                            // every view addresses pixel p = (b H + y) W + x at p * sx: no division per pixel
    int W, HW, C;
    int P;                               // B H W
    int lanes_log2;                      // threads that share a pixel (each V channels)
    int nchunk, chunk_pix;
    float eps;
    const float* mean;
    const float* var;
    const float* gamma;
    float* dgamma;
    float* dbeta;
    float* part;                         // [nchunk][2][C]: sum g, sum g xh
};

__device__ __forceinline__ long long pix_off(int p, int flat, int HW, int W, long long sb, long long sy, long long sx) {
    if (flat) return p * sx;
    const int b = p / HW, r = p - b * HW, y = r / W, x = r - y * W;
    return b * sb + y * sy + x * sx;
}

// a pair of sums for V channels whose accumulators never run longer than CHAIN terms: s takes CHAIN terms, then moves into t;
// t takes CHAIN such moves, then moves into u.  (u is the only one that grows with the input, by one term per CHAIN^2.)
template <int V>
struct Sums {
    float s1[V], s2[V], t1[V], t2[V], u1[V], u2[V];
    int n0, n1;
    __device__ __forceinline__ Sums() : n0(0), n1(0) {
#pragma unroll
        for (int i = 0; i < V; ++i) { s1[i] = 0.f; s2[i] = 0.f; t1[i] = 0.f; t2[i] = 0.f; u1[i] = 0.f; u2[i] = 0.f; }
    }
    __device__ __forceinline__ void add(const float (&a)[V], const float (&b)[V]) {
#pragma unroll
        for (int i = 0; i < V; ++i) { s1[i] = s1[i] + a[i]; s2[i] = s2[i] + b[i]; }
        if (++n0 == CHAIN) {
            n0 = 0;
#pragma unroll
            for (int i = 0; i < V; ++i) { t1[i] = t1[i] + s1[i]; t2[i] = t2[i] + s2[i]; s1[i] = 0.f; s2[i] = 0.f; }
            if (++n1 == CHAIN) {
                n1 = 0;
#pragma unroll
                for (int i = 0; i < V; ++i) { u1[i] = u1[i] + t1[i]; u2[i] = u2[i] + t2[i]; t1[i] = 0.f; t2[i] = 0.f; }
            }
        }
    }
    __device__ __forceinline__ void total(float (&a)[V], float (&b)[V]) const {
#pragma unroll
        for (int i = 0; i < V; ++i) { a[i] = (u1[i] + t1[i]) + s1[i]; b[i] = (u2[i] + t2[i]) + s2[i]; }
    }
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
__global__ __launch_bounds__(NT) void bn_bwd_partials_f32_kernel(const BNBwdParams P) {
    __shared__ float sm[NT * 2 * V];
    const int tid = threadIdx.x, lane = tid & ((1 << P.lanes_log2) - 1), row = tid >> P.lanes_log2, rows = NT >> P.lanes_log2;
    const int c = ((blockIdx.y << P.lanes_log2) + lane) * V;
    const bool active = c < P.C;
    const int chunk = blockIdx.x;
    const int p0 = chunk * P.chunk_pix, p1 = min(p0 + P.chunk_pix, P.P);
    Sums<V> acc;
    if (active) {
        const float* xb = P.x.p + c * P.x.sc;
        const float* gb = P.dy.p + c * P.dy.sc;
        const float* ob = P.relu ? P.out.p + c * P.out.sc : nullptr;
        const Vec<V> mean = ldv<V>(P.mean + c), var = ldv<V>(P.var + c);
        float rstd[V];
#pragma unroll
        for (int i = 0; i < V; ++i) rstd[i] = 1.0f / sqrtf(var.v[i] + P.eps);
#pragma unroll 2
        for (int p = p0 + row; p < p1; p += rows) {
            const Vec<V> v = ldv<V>(xb + pix_off(p, P.flat, P.HW, P.W, P.x.sb, P.x.sy, P.x.sx));
            const Vec<V> g = ldv<V>(gb + pix_off(p, P.flat, P.HW, P.W, P.dy.sb, P.dy.sy, P.dy.sx));
            float a[V], b[V];
            if (P.relu) {
                const Vec<V> o = ldv<V>(ob + pix_off(p, P.flat, P.HW, P.W, P.out.sb, P.out.sy, P.out.sx));
#pragma unroll
                for (int i = 0; i < V; ++i) a[i] = o.v[i] > 0.f ? g.v[i] : 0.f;
            } else {
#pragma unroll
                for (int i = 0; i < V; ++i) a[i] = g.v[i];
            }
#pragma unroll
            for (int i = 0; i < V; ++i) b[i] = a[i] * ((v.v[i] - mean.v[i]) * rstd[i]);
            acc.add(a, b);
        }
    }
    float s1[V], s2[V];
    acc.total(s1, s2);
    sum_rows<V>(s1, s2, tid, P.lanes_log2, sm);
    if (row == 0 && active) {
        float* o = P.part + (long long)chunk * 2 * P.C + c;
        Vec<V> v1, v2;
#pragma unroll
        for (int i = 0; i < V; ++i) { v1.v[i] = s1[i]; v2.v[i] = s2[i]; }
        stv<V>(o, v1);
        stv<V>(o + P.C, v2);
    }
}

template <int V>
__global__ __launch_bounds__(NT) void bn_bwd_apply_f32_kernel(const BNBwdParams P) {
    __shared__ float sm[NT * 2 * V];
    __shared__ float stat[2 * 64];             // (mean_P(g), mean_P(g xh)) of the <= 64 channels of this workgroup
    const int tid = threadIdx.x, L = 1 << P.lanes_log2, lane = tid & (L - 1), row = tid >> P.lanes_log2, rows = NT >> P.lanes_log2;
    const int c = ((blockIdx.y << P.lanes_log2) + lane) * V;
    const bool active = c < P.C;
    const int chunk = blockIdx.x;
    if (P.need_sums) {
        Sums<V> acc;
        if (active) {
            for (int k = row; k < P.nchunk; k += rows) {
                const float* o = P.part + (long long)k * 2 * P.C + c;
                const Vec<V> v1 = ldv<V>(o), v2 = ldv<V>(o + P.C);
                acc.add(v1.v, v2.v);
            }
        }
        float s1[V], s2[V];
        acc.total(s1, s2);
        sum_rows<V>(s1, s2, tid, P.lanes_log2, sm);
        if (row == 0) {
            const float n = (float)P.P;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                stat[(lane * V + i) * 2] = s1[i] / n;
                stat[(lane * V + i) * 2 + 1] = s2[i] / n;
            }
            if (chunk == 0 && active) {
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    if (P.dbeta) P.dbeta[c + i] = s1[i];
                    if (P.dgamma) P.dgamma[c + i] = s2[i];
                }
            }
        }
        __syncthreads();
    }
    if (!active || (!P.dx && !P.dres)) return;
    float m1[V], m2[V], rstd[V], scale[V];
    const Vec<V> mean = ldv<V>(P.mean + c), var = ldv<V>(P.var + c);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        m1[i] = P.need_sums ? stat[(lane * V + i) * 2] : 0.f;
        m2[i] = P.need_sums ? stat[(lane * V + i) * 2 + 1] : 0.f;
        rstd[i] = 1.0f / sqrtf(var.v[i] + P.eps);
        scale[i] = P.gamma ? P.gamma[c + i] * rstd[i] : rstd[i];
    }
    const int p0 = chunk * P.chunk_pix, p1 = min(p0 + P.chunk_pix, P.P);
    const float* xb = P.x.p + c * P.x.sc;
    const float* gb = P.dy.p + c * P.dy.sc;
    const float* ob = P.relu ? P.out.p + c * P.out.sc : nullptr;
    float* db = P.dx ? P.dx + c * P.xc : nullptr;
    float* rb = P.dres ? P.dres + c * P.rc : nullptr;
#pragma unroll 2
    for (int p = p0 + row; p < p1; p += rows) {
        Vec<V> g = ldv<V>(gb + pix_off(p, P.flat, P.HW, P.W, P.dy.sb, P.dy.sy, P.dy.sx));
        if (P.relu) {
            const Vec<V> o = ldv<V>(ob + pix_off(p, P.flat, P.HW, P.W, P.out.sb, P.out.sy, P.out.sx));
#pragma unroll
            for (int i = 0; i < V; ++i) g.v[i] = o.v[i] > 0.f ? g.v[i] : 0.f;
        }
        if (rb) stv<V>(rb + pix_off(p, P.flat, P.HW, P.W, P.rb, P.ry, P.rx), g);
        if (db) {
            const Vec<V> v = ldv<V>(xb + pix_off(p, P.flat, P.HW, P.W, P.x.sb, P.x.sy, P.x.sx));
            Vec<V> d;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float xh = (v.v[i] - mean.v[i]) * rstd[i];
                d.v[i] = scale[i] * ((g.v[i] - m1[i]) - xh * m2[i]);
            }
            stv<V>(db + pix_off(p, P.flat, P.HW, P.W, P.xb, P.xy, P.xx), d);
        }
    }
}

struct PoolBwdParams {
    View x, dy;
    float* dx;
    long long ob, oy, ox, oc;
    int H, W, Ho, Wo, C;
    long long total;                     // B * H * W * (C / V)
};

template <int V>
__global__ __launch_bounds__(NT) void maxpool3x3s2_bwd_f32_kernel(const PoolBwdParams P) {
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e >= P.total) return;
    const int cq = P.C / V;
    const int c = (int)(e % cq) * V;
    long long t = e / cq;
    const int x = (int)(t % P.W);
    t /= P.W;
    const int y = (int)(t % P.H), b = (int)(t / P.H);
    const float* xb = P.x.p + b * P.x.sb + c * P.x.sc;
    const float* gb = P.dy.p + b * P.dy.sb + c * P.dy.sc;
    const int me = y * P.W + x;
    Vec<V> d;
#pragma unroll
    for (int i = 0; i < V; ++i) d.v[i] = 0.f;
    // windows oy with 2 oy - 1 <= y <= 2 oy + 1: y / 2 and, for an odd y, (y + 1) / 2
    const int oy1 = min((y + 1) / 2, P.Ho - 1), ox1 = min((x + 1) / 2, P.Wo - 1);
    for (int oy = y / 2; oy <= oy1; ++oy) {
        for (int ox = x / 2; ox <= ox1; ++ox) {
            const int ys = max(2 * oy - 1, 0), ye = min(2 * oy + 2, P.H), xs = max(2 * ox - 1, 0), xe = min(2 * ox + 2, P.W);
            float m[V];
            int idx[V];
#pragma unroll
            for (int i = 0; i < V; ++i) { m[i] = -INFINITY; idx[i] = ys * P.W + xs; }
            for (int yy = ys; yy < ye; ++yy) {
                for (int xx = xs; xx < xe; ++xx) {
                    const Vec<V> v = ldv<V>(xb + yy * P.x.sy + xx * P.x.sx);
#pragma unroll
                    for (int i = 0; i < V; ++i)
                        if (v.v[i] > m[i] || v.v[i] != v.v[i]) { m[i] = v.v[i]; idx[i] = yy * P.W + xx; }
                }
            }
            const Vec<V> g = ldv<V>(gb + oy * P.dy.sy + ox * P.dy.sx);
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (idx[i] == me) d.v[i] = d.v[i] + g.v[i];
        }
    }
    stv<V>(P.dx + b * P.ob + y * P.oy + x * P.ox + c * P.oc, d);
}

bool flat_view(const oess_f32_view_t* v, int H, int W) { return v->sy == W * v->sx && v->sb == H * v->sy; }

// pixel indices are ints: B H W < 2^30 keeps p0 + chunk_pix and p + rows below 2^31
bool bn_geometry_ok(int B, int H, int W, int C) { return geometry_ok(B, H, W, C) && (long long)B * H * W < (1LL << 30); }

// the split of the pixels for V channels per thread: a function of the shapes alone.  A thread sums at most CHAIN^2 pixels.
void bn_plan(long long pixels, int C, int V, int& lanes_log2, int& ncg, long long& nchunk, long long& chunk_pix) {
    const int max_lanes = V == 4 ? 16 : 64;
    lanes_log2 = 0;
    while ((1 << lanes_log2) < max_lanes && (1 << lanes_log2) * V < C) ++lanes_log2;
    const int lanes = 1 << lanes_log2, rows = NT / lanes;
    ncg = (C + lanes * V - 1) / (lanes * V);
    nchunk = (TARGET_BLOCKS + ncg - 1) / ncg;
    const long long by_size = (pixels + MIN_CHUNK_PIX - 1) / MIN_CHUNK_PIX;
    const long long per_chunk = (long long)rows * CHAIN * CHAIN, by_chain = (pixels + per_chunk - 1) / per_chunk;
    nchunk = nchunk < by_size ? nchunk : by_size;
    nchunk = nchunk > by_chain ? nchunk : by_chain;
    chunk_pix = (pixels + nchunk - 1) / nchunk;
    chunk_pix = (chunk_pix + rows - 1) / rows * rows;
    nchunk = (pixels + chunk_pix - 1) / chunk_pix;
}

}  // namespace

extern "C" {

size_t oess_batch_norm_bwd_f32_workspace_bytes(int B, int H, int W, int C) {
    if (!bn_geometry_ok(B, H, W, C)) return 0;
    int ll, ncg;
    long long n4 = 0, n1, cp;
    bn_plan((long long)B * H * W, C, 1, ll, ncg, n1, cp);
    if (C % 4 == 0) bn_plan((long long)B * H * W, C, 4, ll, ncg, n4, cp);    // the vector path's split may be the finer one
    return (size_t)(n1 > n4 ? n1 : n4) * 2 * C * sizeof(float);
}

int oess_batch_norm_bwd_f32(const oess_f32_view_t* x, const oess_f32_view_t* out, const oess_f32_view_t* dy, int B, int H, int W, int C,
                            const float* mean, const float* var, float eps, const float* gamma, int relu, const oess_f32_view_t* dx,
                            float* dgamma, float* dbeta, const oess_f32_view_t* dres, void* ws, size_t ws_bytes, oess_stream_t stream) {
    if (!view_ok(x) || !view_ok(dy) || !mean || !var || !ws || ((uintptr_t)ws & 15) != 0) return OESS_EINVAL;
    if ((relu != 0 && relu != 1) || (relu && !view_ok(out)) || (dx && !dx->data) || (dres && !dres->data)) return OESS_EINVAL;
    if (!bn_geometry_ok(B, H, W, C) || !(eps >= 0.f)) return OESS_EINVAL;
    const long long pixels = (long long)B * H * W;
    if (pixels < 2) return OESS_EINVAL;
    if (ws_bytes < oess_batch_norm_bwd_f32_workspace_bytes(B, H, W, C)) return OESS_ENOMEM;
    if (!relu) dres = nullptr;                              // without a ReLU the residual's gradient is dy itself
    const bool need_sums = dx || dgamma || dbeta;
    if (!need_sums && !dres) return OESS_OK;
    const bool vec = C % 4 == 0 && vec_ok(x) && vec_ok(dy) && (!relu || vec_ok(out)) && (!dx || vec_ok(dx)) && (!dres || vec_ok(dres)) &&
                     (((uintptr_t)mean | (uintptr_t)var | (uintptr_t)gamma) & 15) == 0;
    int lanes_log2, ncg;
    long long nchunk, chunk_pix;
    bn_plan(pixels, C, vec ? 4 : 1, lanes_log2, ncg, nchunk, chunk_pix);
    if (ncg > 65535 || nchunk >= (1LL << 31)) return OESS_EINVAL;
    BNBwdParams P{};
    P.x = to_view(x);
    P.dy = to_view(dy);
    P.out = relu ? to_view(out) : View{nullptr, 0, 0, 0, 0};
    if (dx) { P.dx = (float*)dx->data; P.xb = dx->sb; P.xy = dx->sy; P.xx = dx->sx; P.xc = dx->sc; }
    if (dres) { P.dres = (float*)dres->data; P.rb = dres->sb; P.ry = dres->sy; P.rx = dres->sx; P.rc = dres->sc; }
    P.relu = relu;
    P.need_sums = need_sums;
    P.flat = flat_view(x, H, W) && flat_view(dy, H, W) && (!relu || flat_view(out, H, W)) && (!dx || flat_view(dx, H, W)) &&
             (!dres || flat_view(dres, H, W));
    P.W = W; P.HW = H * W; P.C = C; P.P = (int)pixels;
    P.lanes_log2 = lanes_log2;
    P.nchunk = (int)nchunk; P.chunk_pix = (int)chunk_pix;
    P.eps = eps;
    P.mean = mean; P.var = var; P.gamma = gamma;
    P.dgamma = dgamma; P.dbeta = dbeta;
    P.part = (float*)ws;
    const dim3 grid((unsigned)nchunk, (unsigned)ncg);
    const dim3 grid2(dx || dres ? (unsigned)nchunk : 1u, (unsigned)ncg);      // only dgamma / dbeta: the first range's workgroups
    hipStream_t st = (hipStream_t)stream;
    if (vec) {
        if (need_sums) hipLaunchKernelGGL(bn_bwd_partials_f32_kernel<4>, grid, dim3(NT), 0, st, P);
        hipLaunchKernelGGL(bn_bwd_apply_f32_kernel<4>, grid2, dim3(NT), 0, st, P);
    } else {
        if (need_sums) hipLaunchKernelGGL(bn_bwd_partials_f32_kernel<1>, grid, dim3(NT), 0, st, P);
        hipLaunchKernelGGL(bn_bwd_apply_f32_kernel<1>, grid2, dim3(NT), 0, st, P);
    }
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_maxpool3x3s2_bwd_f32(const oess_f32_view_t* x, const oess_f32_view_t* dy, int B, int H, int W, int C, const oess_f32_view_t* dx,
                              oess_stream_t stream) {
    if (!view_ok(x) || !view_ok(dy) || !view_ok(dx) || !geometry_ok(B, H, W, C)) return OESS_EINVAL;
    const bool vec = C % 4 == 0 && vec_ok(x) && vec_ok(dy) && vec_ok(dx);
    const int V = vec ? 4 : 1;
    PoolBwdParams P{};
    P.x = to_view(x);
    P.dy = to_view(dy);
    P.dx = (float*)dx->data;
    P.ob = dx->sb; P.oy = dx->sy; P.ox = dx->sx; P.oc = dx->sc;
    P.H = H; P.W = W; P.Ho = (H - 1) / 2 + 1; P.Wo = (W - 1) / 2 + 1; P.C = C;
    P.total = (long long)B * H * W * (C / V);
    const long long blocks = (P.total + NT - 1) / NT;
    if (blocks >= (1LL << 31)) return OESS_EINVAL;
    if (vec) hipLaunchKernelGGL(maxpool3x3s2_bwd_f32_kernel<4>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(maxpool3x3s2_bwd_f32_kernel<1>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, P);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
