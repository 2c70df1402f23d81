// K24: SLIC superpixels on the GPU (data_preparation/superpixel_segmenter_dsec_slic.py:19-24 of the reference:
//   skimage.segmentation.slic(img, n_segments, compactness=6, sigma=3.0, start_label=0); its connectivity pass is slic_connectivity.hip).
// Three passes, all fp32, all bit-repeatable:
//
// slic_lab_kernel: separable Gaussian blur (radius int(4 sigma + 0.5), border rule `reflect`: d c b a | a b c d) of each colour
//   channel, then sRGB -> CIELAB (D65, 2 degrees) and one multiply by 1 / compactness.  A workgroup owns a LAB_T x LAB_T tile of
//   one sample.  Per channel the tile and its halo are read once into LDS through the frame's strides with the border reflected
//   (and clamped: an edge tile's rows below the image are never stored), blurred down the columns into a second LDS tile as
//   scipy.ndimage does (axis 0 first) and along the rows into registers; the three blurred channels of a pixel never leave
//   them before the colour transform.  Bound by the 2 x 25 LDS reads and multiply-adds per pixel and channel (no FMA: the
//   library is built with -ffp-contract=off), not by its 24 bytes per pixel of traffic.
// slic_assign_kernel: one thread per pixel, a 32 x 8 tile per workgroup.  The sample's K <= 256 centres are filtered against
//   the tile (a centre whose 2 step window misses the tile can win none of its pixels) and kept, in increasing k, in LDS;
//   every pixel walks that list with the eligibility test of its own, strict `<` so that ties go to the lowest k, and a pixel
//   eligible for no centre keeps its previous label.  No neighbour tables: the walk is the centre-wise window order.
// slic_update_kernel + slic_finalize_kernel: the new centres as means.  Everything that meets another partial sum is an
//   integer: counts, y and x sums as such, L, a, b as 2^-32 fixed point in 64-bit integers.  A thread sums a run of SLIC_RUN
//   consecutive pixels in registers, adds it to the workgroup's LDS table when the label changes (64-bit integer LDS
//   atomics), and the table leaves through one 64-bit integer atomic per touched (centre, component).  Integer addition
//   commutes: the sums, and with them the centres, repeat bit for bit.  Headroom: a map value is clamped to |v| <= 64 before
//   the conversion (L / compactness is at most 16.7 for a frame in [0, 1]), so one pixel adds less than 2^38 and a sample of at
//   most 2^24 pixels (the entry point refuses more) stays below 2^62.  A mean is the float64 quotient of the exact sum (a colour
//   sum beyond 2^53 is rounded when it becomes a double) and the count, rounded to fp32; an empty centre keeps its previous value.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"

namespace {
using namespace oess;
#include "f32_view.h"

typedef unsigned long long u64_t;

constexpr int SLIC_MAX_K = 256;
constexpr int SLIC_MAX_RADIUS = 24;               // sigma <= 6.1; the reference's 3.0 gives 12
constexpr int LAB_T = 32, LAB_THREADS = 256;      // output tile, threads: LAB_T * LAB_T / LAB_THREADS = 4 pixels per thread
constexpr int LAB_PPT = LAB_T * LAB_T / LAB_THREADS;
constexpr int ASG_TW = 32, ASG_TH = 8;            // assignment tile = 256 threads
constexpr int UPD_THREADS = 256, SLIC_RUN = 8;    // update: pixels per thread, consecutive in the sample's row-major order
constexpr int UPD_COMP = 6;                       // count, sum y, sum x, sum L, sum a, sum b
constexpr int SLIC_MAX_PIXELS = 1 << 24;
// slic_assign_kernel compacts the centres with one 64-lane wave (`tid < 64`, a 64-bit __ballot mask, 1ull << tid): gfx950 only
#if defined(__HIP_DEVICE_COMPILE__) && defined(__AMDGCN_WAVEFRONT_SIZE) && __AMDGCN_WAVEFRONT_SIZE != 64
#error "slic_assign_kernel's centre compaction needs 64-lane waves"
#endif

struct Taps {
    float w[2 * SLIC_MAX_RADIUS + 1];
};

__device__ __forceinline__ int reflect_clamp(int i, int n) {
    if (i < 0) i = -i - 1;
    else if (i >= n) i = 2 * n - 1 - i;
    return min(max(i, 0), n - 1);
}

__device__ __forceinline__ float srgb_linear(float v) { return v > 0.04045f ? powf((v + 0.055f) / 1.055f, 2.4f) : v / 12.92f; }
__device__ __forceinline__ float lab_f(float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + 16.0f / 116.0f; }

__global__ __launch_bounds__(LAB_THREADS) void slic_lab_kernel(View in, int H, int W, int R, Taps taps, float inv_compactness, int ntx,
                                                               int nty, float* __restrict__ lab) {
    extern __shared__ float lab_smem[];
    const int IW = LAB_T + 2 * R, IH = LAB_T + 2 * R;
    float* tile = lab_smem;                        // [IH][IW] one channel with its halo
    float* col = lab_smem + IH * IW;               // [LAB_T][IW] blurred down the columns
    const int tx = blockIdx.x % ntx, lin = blockIdx.x / ntx;
    const int ty = lin % nty;
    const long long b = lin / nty;
    const int x0 = tx * LAB_T, y0 = ty * LAB_T;
    float acc[3][LAB_PPT];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        __syncthreads();                           // the previous channel's tiles are consumed
        for (int i = threadIdx.x; i < IH * IW; i += LAB_THREADS) {
            const int r = i / IW, q = i - r * IW;
            const int gy = reflect_clamp(y0 - R + r, H), gx = reflect_clamp(x0 - R + q, W);
            tile[i] = in.p[b * in.sb + gy * in.sy + gx * in.sx + c * in.sc];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < LAB_T * IW; i += LAB_THREADS) {
            const int r = i / IW, q = i - r * IW;
            float s = 0.f;
            for (int k = 0; k <= 2 * R; ++k) s += taps.w[k] * tile[(r + k) * IW + q];
            col[i] = s;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < LAB_PPT; ++j) {
            const int p = threadIdx.x + j * LAB_THREADS, r = p / LAB_T, q = p - r * LAB_T;
            float s = 0.f;
            for (int k = 0; k <= 2 * R; ++k) s += taps.w[k] * col[r * IW + q + k];
            acc[c][j] = s;
        }
    }
#pragma unroll
    for (int j = 0; j < LAB_PPT; ++j) {
        const int p = threadIdx.x + j * LAB_THREADS, r = p / LAB_T, q = p - r * LAB_T;
        const int y = y0 + r, x = x0 + q;
        if (y >= H || x >= W) continue;
        const float lr = srgb_linear(acc[0][j]), lg = srgb_linear(acc[1][j]), lb = srgb_linear(acc[2][j]);
        const float X = (0.412453f * lr + 0.357580f * lg + 0.180423f * lb) / 0.95047f;
        const float Y = 0.212671f * lr + 0.715160f * lg + 0.072169f * lb;
        const float Z = (0.019334f * lr + 0.119193f * lg + 0.950227f * lb) / 1.08883f;
        const float fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
        float* o = lab + ((b * H + y) * W + x) * 3;
        o[0] = (116.0f * fy - 16.0f) * inv_compactness;
        o[1] = (500.0f * (fx - fy)) * inv_compactness;
        o[2] = (200.0f * (fy - fz)) * inv_compactness;
    }
}

// centre k = i nx + j starts at its lattice pixel with the map's value there
__global__ void slic_init_centers_kernel(const float* __restrict__ lab, int B, int H, int W, int ny, int nx, float* __restrict__ centers) {
    const int K = ny * nx;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * K) return;
    const int b = t / K, k = t - b * K, i = k / nx, j = k - i * nx;
    const int y = min((int)(((2LL * i + 1) * H) / (2LL * ny)), H - 1), x = min((int)(((2LL * j + 1) * W) / (2LL * nx)), W - 1);
    const float* v = lab + (((long long)b * H + y) * W + x) * 3;
    float* c = centers + (long long)t * 5;
    c[0] = (float)y; c[1] = (float)x; c[2] = v[0]; c[3] = v[1]; c[4] = v[2];
}

__global__ __launch_bounds__(ASG_TW * ASG_TH) void slic_assign_kernel(const float* __restrict__ lab, const float* __restrict__ centers,
                                                                      const int64_t* prev, int H, int W, int K, int step,
                                                                      float inv_step2, int ny, int nx, int ntx, int nty,
                                                                      int64_t* labels) {
    __shared__ float cen[SLIC_MAX_K * 5];
    __shared__ int win[SLIC_MAX_K * 4];
    __shared__ int idx[SLIC_MAX_K];
    __shared__ int count;
    const int tx = blockIdx.x % ntx, lin = blockIdx.x / ntx;
    const int ty = lin % nty;
    const long long b = lin / nty;
    const int tid = threadIdx.x;
    const int tile_x0 = tx * ASG_TW, tile_y0 = ty * ASG_TH;
    const int tile_x1 = min(tile_x0 + ASG_TW, W), tile_y1 = min(tile_y0 + ASG_TH, H);
    if (tid < 64) {                                // one 64-lane wave (see the check above) compacts the centres that can reach the tile, in increasing k
        int n = 0;
        for (int base = 0; base < K; base += 64) {
            const int k = base + tid;
            bool ok = false;
            float c[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            int w[4] = {0, 0, 0, 0};
            if (k < K) {
                const float* s = centers + (b * K + k) * 5;
#pragma unroll
                for (int i = 0; i < 5; ++i) c[i] = s[i];
                const float reach = (float)(2 * step);
                w[0] = (int)fmaxf(c[0] - reach, 0.f);
                w[1] = (int)fminf(c[0] + reach + 1.f, (float)H);
                w[2] = (int)fmaxf(c[1] - reach, 0.f);
                w[3] = (int)fminf(c[1] + reach + 1.f, (float)W);
                ok = w[0] < tile_y1 && w[1] > tile_y0 && w[2] < tile_x1 && w[3] > tile_x0;
            }
            const u64_t m = __ballot(ok);
            if (ok) {
                const int at = n + __popcll(m & ((1ull << tid) - 1ull));     // at < K <= SLIC_MAX_K
#pragma unroll
                for (int i = 0; i < 5; ++i) cen[at * 5 + i] = c[i];
#pragma unroll
                for (int i = 0; i < 4; ++i) win[at * 4 + i] = w[i];
                idx[at] = k;
            }
            n += __popcll(m);
        }
        if (tid == 0) count = n;
    }
    __syncthreads();
    const int x = tile_x0 + tid % ASG_TW, y = tile_y0 + tid / ASG_TW;
    if (x >= W || y >= H) return;
    const long long p = (b * H + y) * W + x;
    const float l0 = lab[p * 3], l1 = lab[p * 3 + 1], l2 = lab[p * 3 + 2];
    int64_t best_k = prev ? prev[p] : (int64_t)((long long)y * ny / H) * nx + (long long)x * nx / W;
    float best = INFINITY;
    const float fy = (float)y, fx = (float)x;
    const int n = count;
    for (int i = 0; i < n; ++i) {
        if (y < win[i * 4] || y >= win[i * 4 + 1] || x < win[i * 4 + 2] || x >= win[i * 4 + 3]) continue;
        const float dy = fy - cen[i * 5], dx = fx - cen[i * 5 + 1];
        const float d0 = l0 - cen[i * 5 + 2], d1 = l1 - cen[i * 5 + 3], d2 = l2 - cen[i * 5 + 4];
        const float d = (dy * dy + dx * dx) * inv_step2 + (d0 * d0 + d1 * d1 + d2 * d2);
        if (d < best) { best = d; best_k = idx[i]; }
    }
    labels[p] = best_k;
}

__device__ __forceinline__ long long slic_to_fixed(float v) { return __float2ll_rn(fminf(fmaxf(v, -64.f), 64.f) * 4294967296.0f); }

// acc: [B][K][UPD_COMP] 64-bit sums, zeroed by the caller's launch
__global__ __launch_bounds__(UPD_THREADS) void slic_update_kernel(const float* __restrict__ lab, const int64_t* __restrict__ labels, int HW,
                                                                  int W, int K, int nchunk, u64_t* __restrict__ acc) {
    __shared__ u64_t tab[SLIC_MAX_K * UPD_COMP];
    const int chunk = blockIdx.x % nchunk;
    const long long b = blockIdx.x / nchunk;
    for (int i = threadIdx.x; i < K * UPD_COMP; i += UPD_THREADS) tab[i] = 0ull;
    __syncthreads();
    const int beg = min((chunk * UPD_THREADS + (int)threadIdx.x) * SLIC_RUN, HW), end = min(beg + SLIC_RUN, HW);
    int64_t cur = -1;
    u64_t run[UPD_COMP] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    auto flush = [&]() {
        if (run[0] == 0ull || cur < 0 || cur >= K) return;          // a label outside [0, K) belongs to no centre
        u64_t* r = tab + (int)cur * UPD_COMP;
#pragma unroll
        for (int i = 0; i < UPD_COMP; ++i) atomicAdd(&r[i], run[i]);
    };
    for (int p = beg; p < end; ++p) {
        const long long g = b * HW + p;
        const int64_t id = labels[g];
        if (id != cur) {
            flush();
            cur = id;
#pragma unroll
            for (int i = 0; i < UPD_COMP; ++i) run[i] = 0ull;
        }
        const int y = p / W, x = p - y * W;
        run[0] += 1ull;
        run[1] += (u64_t)y;
        run[2] += (u64_t)x;
#pragma unroll
        for (int c = 0; c < 3; ++c) run[3 + c] += (u64_t)slic_to_fixed(lab[g * 3 + c]);
    }
    flush();
    __syncthreads();
    for (int i = threadIdx.x; i < K * UPD_COMP; i += UPD_THREADS)
        if (tab[i] != 0ull) atomicAdd(&acc[b * K * UPD_COMP + i], tab[i]);
}

__global__ void slic_finalize_kernel(const u64_t* __restrict__ acc, const float* old, int n, float* centers, int* __restrict__ counts) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const u64_t* a = acc + (long long)t * UPD_COMP;
    const float* o = old + (long long)t * 5;
    float v[5];
    const u64_t cnt = a[0];
    if (cnt == 0ull) {
#pragma unroll
        for (int i = 0; i < 5; ++i) v[i] = o[i];
    } else {
        const double c = (double)cnt;
        v[0] = (float)((double)a[1] / c);
        v[1] = (float)((double)a[2] / c);
#pragma unroll
        for (int i = 0; i < 3; ++i) v[2 + i] = (float)((double)(long long)a[3 + i] * (1.0 / 4294967296.0) / c);
    }
    float* d = centers + (long long)t * 5;
#pragma unroll
    for (int i = 0; i < 5; ++i) d[i] = v[i];
    if (counts) counts[t] = (int)cnt;
}

int slic_radius(float sigma) { return (int)(4.0f * sigma + 0.5f); }

bool slic_geometry_ok(int B, int H, int W) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= SLIC_MAX_PIXELS;
}
}  // namespace

extern "C" {

int oess_slic_lab_f32(const oess_f32_view_t* frames, int B, int H, int W, float sigma, float compactness, float* lab, int ny, int nx,
                      float* centers, oess_stream_t stream) {
    if (!view_ok(frames) || !lab || !slic_geometry_ok(B, H, W) || !(sigma > 0.f) || !(compactness > 0.f)) return OESS_EINVAL;
    if (!(sigma <= 6.0f)) return OESS_EINVAL;
    const int R = slic_radius(sigma);
    if (R > SLIC_MAX_RADIUS || (H < W ? H : W) < R + 1) return OESS_EINVAL;       // one reflection must cover the blur radius
    if (centers && (ny < 1 || nx < 1 || ny > H || nx > W || (long long)ny * nx > SLIC_MAX_K)) return OESS_EINVAL;
    Taps taps;
    double w[2 * SLIC_MAX_RADIUS + 1], sum = 0.0;
    for (int k = -R; k <= R; ++k) sum += (w[k + R] = exp(-0.5 * (double)k * k / ((double)sigma * sigma)));
    for (int k = 0; k <= 2 * SLIC_MAX_RADIUS; ++k) taps.w[k] = k <= 2 * R ? (float)(w[k] / sum) : 0.f;
    const int ntx = (W + LAB_T - 1) / LAB_T, nty = (H + LAB_T - 1) / LAB_T;
    const long long nwg = (long long)B * ntx * nty;
    if (nwg > 0x7fffffffLL) return OESS_EINVAL;
    const int IW = LAB_T + 2 * R;
    const size_t lds = (size_t)(IW * IW + LAB_T * IW) * sizeof(float);       // <= 36 KiB at SLIC_MAX_RADIUS
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(slic_lab_kernel, dim3((unsigned)nwg), dim3(LAB_THREADS), lds, st, to_view(frames), H, W, R, taps, 1.0f / compactness,
                       ntx, nty, lab);
    if (centers) {
        const int n = B * ny * nx;
        hipLaunchKernelGGL(slic_init_centers_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)lab, B, H, W, ny, nx, centers);
    }
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_slic_assign_f32(const float* lab, const float* centers, const int64_t* prev_labels, int B, int H, int W, int K, int step, int ny,
                         int nx, int64_t* labels, oess_stream_t stream) {
    if (!lab || !centers || !labels || !slic_geometry_ok(B, H, W) || K < 1 || K > SLIC_MAX_K || step < 1 || step > (1 << 20))
        return OESS_EINVAL;
    if (!prev_labels && (ny < 1 || nx < 1 || (long long)ny * nx != K)) return OESS_EINVAL;
    const int ntx = (W + ASG_TW - 1) / ASG_TW, nty = (H + ASG_TH - 1) / ASG_TH;
    const long long nwg = (long long)B * ntx * nty;
    if (nwg > 0x7fffffffLL) return OESS_EINVAL;
    hipLaunchKernelGGL(slic_assign_kernel, dim3((unsigned)nwg), dim3(ASG_TW * ASG_TH), 0, (hipStream_t)stream, lab, centers, prev_labels, H,
                       W, K, step, 1.0f / ((float)step * (float)step), ny, nx, ntx, nty, labels);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_slic_update_f32(const float* lab, const int64_t* labels, const float* centers, int B, int H, int W, int K, float* new_centers,
                         int* counts, void* workspace, size_t workspace_bytes, oess_stream_t stream) {
    if (!lab || !labels || !centers || !new_centers || !workspace || !slic_geometry_ok(B, H, W) || K < 1 || K > SLIC_MAX_K ||
        ((uintptr_t)workspace & 7))
        return OESS_EINVAL;
    const size_t need = (size_t)B * K * UPD_COMP * sizeof(u64_t);
    if (workspace_bytes < need) return OESS_ENOMEM;
    const int HW = H * W;
    const int nchunk = (HW + UPD_THREADS * SLIC_RUN - 1) / (UPD_THREADS * SLIC_RUN);
    const long long nwg = (long long)B * nchunk;
    if (nwg > 0x7fffffffLL) return OESS_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    OESS_HIP(hipMemsetAsync(workspace, 0, need, st));
    hipLaunchKernelGGL(slic_update_kernel, dim3((unsigned)nwg), dim3(UPD_THREADS), 0, st, lab, labels, HW, W, K, nchunk, (u64_t*)workspace);
    const int n = B * K;
    hipLaunchKernelGGL(slic_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const u64_t*)workspace, centers, n, new_centers, counts);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
