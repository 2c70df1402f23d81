// K23: the joint stage's L1 feature-consistency loss in fp32 on the two low-resolution maps, as one forward and one backward node:
//   loss = mean |F.interpolate(a, bilinear) - F.interpolate(b, bilinear)| = mean |up(a - b)|      training/openess_trainer.py:497
// a, b are the students' ASPP features (fp32 NHWC, 9.2 MB each at 8 x 28 x 40 x 256); their upsampled difference is 2.3 GB at
// 440 x 640 and is NEVER written: forward and backward recompute the blend of every output element from d = a - b.
//
// Forward (ul1_fwd_kernel): one thread owns one channel of UL1_ROWS output rows of one sample.  Per output row it blends the
// two source rows at the current pair of source columns (rows first, then columns: the association of K20) and walks the output
// columns with the two blended neighbours in registers: 2 w loads of d per Wo outputs, coalesced over the channels of a pixel.
// |u| is summed in fp32 over the run of outputs that share a left source column, runs meet in double, workgroups leave one double
// each in the workspace and one block adds those in a fixed order: the rule of oess_loss_partials_bytes without its cap on the
// number of partials.
//
// Backward (ul1_bwd_kernel): gather form, one thread per (pixel, channel) of d with the clamped 3 x 3 neighbourhood in registers.
// Upsampling (Ho >= h, Wo >= w) keeps the two source rows / columns of every output element that touches the pixel inside that
// neighbourhood, so u is recomputed from registers by the forward's own operations and w_y w_x sign(u) accumulated; each gradient
// element is written once, no atomics: bit-repeatable.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"
#include "bilinear_axis.h"

namespace {
using namespace oess;

constexpr int UL1_THREADS = 256;
constexpr int UL1_ROWS = 4;                       // output rows per forward thread
constexpr int UL1_MAX_C = 1024;

__device__ __forceinline__ float ld_d(const float* __restrict__ a, int64_t aps, const float* __restrict__ b, int64_t bps, int64_t pix,
                                      int c) {
    const float va = a[pix * aps + c];
    return b ? va - b[pix * bps + c] : va;
}

__global__ __launch_bounds__(UL1_THREADS) void ul1_fwd_kernel(const float* __restrict__ a, int64_t aps, const float* __restrict__ b,
                                                              int64_t bps, int C, Axis ay, Axis ax, int nchunk, int64_t total,
                                                              double* __restrict__ partials) {
    __shared__ double red[UL1_THREADS / 64];
    const int64_t t = (int64_t)blockIdx.x * UL1_THREADS + threadIdx.x;
    double acc = 0.0;
    if (t < total) {
        const int c = (int)(t % C);
        const int64_t lin = t / C;
        const int chunk = (int)(lin % nchunk);
        const int64_t bi = lin / nchunk;
        const int oy_beg = chunk * UL1_ROWS, oy_end = min(oy_beg + UL1_ROWS, ay.out);
        for (int oy = oy_beg; oy < oy_end; ++oy) {
            int y0, y1; float wy;
            src_index(ay, oy, y0, y1, wy);
            const float hy = 1.f - wy;
            const int64_t row0 = (bi * ay.in + y0) * ax.in, row1 = (bi * ay.in + y1) * ax.in;
            int cur0 = -1, cur1 = -1;
            float v0 = 0.f, v1 = 0.f, run = 0.f;
            for (int ox = 0; ox < ax.out; ++ox) {
                int x0, x1; float lam;
                src_index(ax, ox, x0, x1, lam);
                if (x0 != cur0) {                             // the left source column is monotonic in ox
                    acc += (double)run;
                    run = 0.f;
                    v0 = (x0 == cur1) ? v1 : hy * ld_d(a, aps, b, bps, row0 + x0, c) + wy * ld_d(a, aps, b, bps, row1 + x0, c);
                    v1 = (x1 == x0) ? v0 : hy * ld_d(a, aps, b, bps, row0 + x1, c) + wy * ld_d(a, aps, b, bps, row1 + x1, c);
                    cur0 = x0; cur1 = x1;
                }
                run += fabsf((1.f - lam) * v0 + lam * v1);
            }
            acc += (double)run;
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < UL1_THREADS / 64; ++w) s += red[w];
        partials[blockIdx.x] = s;
    }
}

// second stage: one block adds the workgroup partials in a fixed order
__global__ __launch_bounds__(UL1_THREADS) void ul1_finish_kernel(const double* __restrict__ partials, int64_t n, double scale,
                                                                 float* __restrict__ loss) {
    __shared__ double red[UL1_THREADS];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += UL1_THREADS) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = UL1_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(scale * red[0]);
}

__global__ __launch_bounds__(UL1_THREADS) void ul1_bwd_kernel(const float* __restrict__ a, int64_t aps, const float* __restrict__ b,
                                                              int64_t bps, int C, Axis ay, Axis ax, int64_t total, double inv_n,
                                                              const float* __restrict__ grad_out, float* __restrict__ ga, int64_t gaps,
                                                              float* __restrict__ gb, int64_t gbps) {
    const int64_t t = (int64_t)blockIdx.x * UL1_THREADS + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % C);
    const int64_t pix = t / C;
    const int ix = (int)(pix % ax.in);
    const int64_t lin = pix / ax.in;
    const int iy = (int)(lin % ay.in);
    const int64_t bi = lin / ay.in;
    // d on the clamped 3 x 3 neighbourhood: n[r][s] = d[iy - 1 + r][ix - 1 + s]
    const int ys[3] = {max(iy - 1, 0), iy, min(iy + 1, ay.in - 1)};
    const int xs[3] = {max(ix - 1, 0), ix, min(ix + 1, ax.in - 1)};
    float n[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) n[r][s] = ld_d(a, aps, b, bps, (bi * ay.in + ys[r]) * ax.in + xs[s], c);
    int ylo, yhi, xlo, xhi;
    candidates(ay, iy, ylo, yhi);
    candidates(ax, ix, xlo, xhi);
    float acc = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
        int y0, y1; float wy;
        src_index(ay, oy, y0, y1, wy);
        const float qy = (y0 == iy ? 1.0f - wy : 0.0f) + (y1 == iy ? wy : 0.0f);      // weight_for(ay, oy, iy) from the same indices
        if (qy == 0.f) continue;
        const float hy = 1.f - wy;
        const bool top = y0 == iy;                            // source rows (iy, iy + 1), otherwise (iy - 1, iy)
        float v[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) v[s] = hy * (top ? n[1][s] : n[0][s]) + wy * (top ? n[2][s] : n[1][s]);
        float racc = 0.f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            int x0, x1; float lam;
            src_index(ax, ox, x0, x1, lam);
            const float qx = (x0 == ix ? 1.0f - lam : 0.0f) + (x1 == ix ? lam : 0.0f);
            if (qx == 0.f) continue;
            const bool left = x0 == ix;
            const float u = (1.f - lam) * (left ? v[1] : v[0]) + lam * (left ? v[2] : v[1]);
            const float sg = (float)((u > 0.f) - (u < 0.f));  // sign(0) = 0, ATen's l1_loss backward
            racc += qx * sg;
        }
        acc += qy * racc;
    }
    const float g = (float)((double)grad_out[0] * inv_n) * acc;
    if (ga) ga[pix * gaps + c] = g;
    if (gb) gb[pix * gbps + c] = -g;
}

bool ul1_geometry_ok(int B, int h, int w, int C, int Ho, int Wo) {
    return B > 0 && h > 0 && w > 0 && C > 0 && C % 4 == 0 && C <= UL1_MAX_C && Ho >= h && Wo >= w;
}
int64_t ul1_fwd_threads(int B, int C, int Ho) { return (int64_t)B * ((Ho + UL1_ROWS - 1) / UL1_ROWS) * C; }
int64_t ul1_blocks(int64_t threads) { return (threads + UL1_THREADS - 1) / UL1_THREADS; }
}  // namespace

extern "C" {

size_t oess_upsampled_l1_workspace_bytes(int B, int h, int w, int C, int Ho, int Wo) {
    if (!ul1_geometry_ok(B, h, w, C, Ho, Wo)) return 0;
    return (size_t)ul1_blocks(ul1_fwd_threads(B, C, Ho)) * sizeof(double);
}

int oess_upsampled_l1_fwd_f32(const float* a, long long a_pix_stride, const float* b, long long b_pix_stride, int B, int h, int w, int C,
                              int Ho, int Wo, int align_corners, void* workspace, size_t workspace_bytes, float* loss,
                              oess_stream_t stream) {
    if (!a || !workspace || !loss || !ul1_geometry_ok(B, h, w, C, Ho, Wo) || a_pix_stride < C || (b && b_pix_stride < C) ||
        ((uintptr_t)workspace & 7))
        return OESS_EINVAL;
    const int64_t threads = ul1_fwd_threads(B, C, Ho), blocks = ul1_blocks(threads);
    if (blocks > 0x7fffffffLL) return OESS_EINVAL;
    if (workspace_bytes < (size_t)blocks * sizeof(double)) return OESS_ENOMEM;
    const Axis ay = make_axis(h, Ho, align_corners), ax = make_axis(w, Wo, align_corners);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ul1_fwd_kernel, dim3((unsigned)blocks), dim3(UL1_THREADS), 0, st, a, (int64_t)a_pix_stride, b, (int64_t)b_pix_stride,
                       C, ay, ax, (Ho + UL1_ROWS - 1) / UL1_ROWS, threads, (double*)workspace);
    const double n = (double)B * C * (double)Ho * (double)Wo;
    hipLaunchKernelGGL(ul1_finish_kernel, dim3(1), dim3(UL1_THREADS), 0, st, (const double*)workspace, blocks, 1.0 / n, loss);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_upsampled_l1_bwd_f32(const float* a, long long a_pix_stride, const float* b, long long b_pix_stride, int B, int h, int w, int C,
                              int Ho, int Wo, int align_corners, const float* grad_out, float* grad_a, long long ga_pix_stride,
                              float* grad_b, long long gb_pix_stride, oess_stream_t stream) {
    if (!a || !grad_out || (!grad_a && !grad_b) || (grad_b && !b) || !ul1_geometry_ok(B, h, w, C, Ho, Wo) || a_pix_stride < C || (b && b_pix_stride < C) ||
        (grad_a && ga_pix_stride < C) || (grad_b && gb_pix_stride < C))
        return OESS_EINVAL;
    const int64_t threads = (int64_t)B * h * w * C, blocks = ul1_blocks(threads);
    if (blocks > 0x7fffffffLL) return OESS_EINVAL;
    const Axis ay = make_axis(h, Ho, align_corners), ax = make_axis(w, Wo, align_corners);
    const double n = (double)B * C * (double)Ho * (double)Wo;
    hipLaunchKernelGGL(ul1_bwd_kernel, dim3((unsigned)blocks), dim3(UL1_THREADS), 0, (hipStream_t)stream, a, (int64_t)a_pix_stride, b,
                       (int64_t)b_pix_stride, C, ay, ax, threads, 1.0 / n, grad_out, grad_a, (int64_t)ga_pix_stride, grad_b,
                       (int64_t)gb_pix_stride);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
