// E2VID post-processing: the reference's PostProcessor (e2vid/image_reconstructor.py:126-140) on the cropped
// reconstruction, fused into one pass per call:
//   UnsharpMaskFilter (e2vid/utils/inference_utils.py:234-252)  img = (1 + a) * img - a * conv2d(img, gkern(5, sigma), padding=2)
//   IntensityRescaler (:90-129)                                  byte = trunc(clamp(255 * (img - Imin) / (Imax - Imin), 0, 255))
//                                                                float = byte / 255
// with the float32 operation order of the reference's torch ops on the device (built with -ffp-contract=off, IEEE divide):
//   s = a > 0 ? fl(fl(c1 * x) - fl(c0 * blur)) : x          c1 = (float)(1 + a), c0 = (float)a, blur = 25 products, fixed order
//   t = fl(fl(255 * fl(s - (float)Imin)) * inv)            inv = (float)(1.0 / (Imax - Imin)), all in double, then rounded
//   (torch's GPU `div` by a host scalar multiplies by the reciprocal of the scalar, taken in double and rounded to fp32: measured
//   on the device, tests/test_hip_e2vid_postprocess.py; the float output likewise is byte * (float)(1.0 / 255))
// Kernels:
//   postproc_apply_kernel<AUTO>  one 64 x 16 output tile per 256-thread workgroup (input tile + 2-pixel zero halo in LDS):
//                                sharpen + tone map -> uint8 (+ fp32).  Bounds from kernel arguments (fixed) or from the
//                                state buffer that postproc_stats_kernel wrote (auto-HDR).
//   postproc_stats_kernel        auto-HDR only: the whole-tensor min / max of the sharpened image (order-independent integer
//                                max on order-preserving keys, so bit-repeatable), then the last-arriving workgroup (integer
//                                ticket) clips them, pushes them into the window ring and takes the float64 medians
//                                (IntensityRescaler's deque + np.median), all on the device: no host synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"

namespace {

constexpr int TW = 64, TH = 16, HALO = 2, LW = TW + 2 * HALO, LH = TH + 2 * HALO;
constexpr int NT = 256, ROWS_PER_THREAD = TH / (NT / TW);
constexpr int WIN_MAX = OESS_E2VID_POSTPROC_MAX_FILTER + 1;          // ring capacity of the largest median window
static_assert(WIN_MAX <= NT, "one window entry per thread in the median");

struct Geom { const float* img; long long img_stride, row_stride; int N, H, W, tiles_x, tiles_y; };
struct Sharpen { float w[25]; float c1, c0; int on; };

// state buffer (caller-owned, zero-filled = fresh): 48-byte header, then ring_lo[cap], ring_hi[cap] (float64)
struct StateHdr {
    uint32_t min_key_inv;     // ~key of the running minimum (atomic max of ~key: a zero-filled slot is the neutral value)
    uint32_t max_key;         // key of the running maximum
    uint32_t ticket;          // workgroups of this call that have published their min / max
    int32_t count, next;      // entries in the ring, slot of the next entry
    float imin_f, inv_f;      // (float)Imin and (float)(1.0 / (Imax - Imin)) for the apply pass
    uint32_t pad;
    double imin, imax;        // the current medians (PostProcessor.current_bounds)
};
static_assert(sizeof(StateHdr) == 48, "state header layout");

// order-preserving float -> uint32 key (larger float <-> larger key; NaN sorts above +inf, -NaN below -inf)
__device__ __forceinline__ uint32_t fkey(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// stage the tile's input (+ zero halo at the edge of the VIEW) in LDS
__device__ __forceinline__ void load_tile(const Geom& g, int n, int y0, int x0, float (*lds)[LW]) {
    const float* src = g.img + (long long)n * g.img_stride;
    for (int i = threadIdx.x; i < LH * LW; i += NT) {
        const int r = i / LW, c = i - r * LW;
        const int y = y0 - HALO + r, x = x0 - HALO + c;
        lds[r][c] = (y >= 0 && y < g.H && x >= 0 && x < g.W) ? src[(long long)y * g.row_stride + x] : 0.0f;
    }
}

// sharpened value at tile-local output (r, c); the 25 products are summed row by row, left to right
__device__ __forceinline__ float sharpen_at(const Sharpen& s, const float (*lds)[LW], int r, int c) {
    const float x = lds[r + HALO][c + HALO];
    if (!s.on) return x;
    float b = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) b += s.w[dy * 5 + dx] * lds[r + dy][c + dx];
    return s.c1 * x - s.c0 * b;
}

__device__ __forceinline__ void tile_of(const Geom& g, int t, int& n, int& y0, int& x0) {
    const int per = g.tiles_x * g.tiles_y;
    n = t / per;
    const int rem = t - n * per;
    y0 = (rem / g.tiles_x) * TH;
    x0 = (rem - (rem / g.tiles_x) * g.tiles_x) * TW;
}

template <bool AUTO>
__global__ __launch_bounds__(NT) void postproc_apply_kernel(Geom g, Sharpen s, float imin_f, float inv_f, const StateHdr* __restrict__ st,
                                                            uint8_t* __restrict__ out_u8, float* __restrict__ out_f32) {
    __shared__ float lds[LH][LW];
    int n, y0, x0;
    tile_of(g, blockIdx.x, n, y0, x0);
    load_tile(g, n, y0, x0, lds);
    if (AUTO) { imin_f = st->imin_f; inv_f = st->inv_f; }     // written by postproc_stats_kernel, the previous launch
    __syncthreads();
    const int c = threadIdx.x % TW, r0 = threadIdx.x / TW, x = x0 + c;
    if (x >= g.W) return;
#pragma unroll
    for (int k = 0; k < ROWS_PER_THREAD; ++k) {
        const int r = r0 + k * (NT / TW), y = y0 + r;
        if (y >= g.H) break;
        const float v = sharpen_at(s, lds, r, c);
        float t = 255.0f * (v - imin_f);
        t = t * inv_f;
        t = fminf(fmaxf(t, 0.0f), 255.0f);                     // clamp_(0, 255) (NaN -> 0), then .byte() truncates
        const uint8_t b = (uint8_t)(uint32_t)t;
        const long long o = ((long long)n * g.H + y) * g.W + x;
        out_u8[o] = b;
        if (out_f32) out_f32[o] = (float)b * (float)(1.0 / 255.0);
    }
}

__global__ __launch_bounds__(NT) void postproc_stats_kernel(Geom g, Sharpen s, int ntiles, int cap, StateHdr* __restrict__ st) {
    __shared__ float lds[LH][LW];
    __shared__ uint32_t red[2][NT / 64];
    __shared__ double wlo[WIN_MAX], whi[WIN_MAX], slo[WIN_MAX], shi[WIN_MAX];
    __shared__ int s_last, s_count, s_slot;
    __shared__ double s_new[2];
    uint32_t kmin_inv = 0, kmax = 0;                           // ~key / key: 0 is neutral for both (max)
    const int c = threadIdx.x % TW, r0 = threadIdx.x / TW;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int n, y0, x0;
        tile_of(g, t, n, y0, x0);
        __syncthreads();                                       // previous tile's reads of lds are done
        load_tile(g, n, y0, x0, lds);
        __syncthreads();
        if (x0 + c < g.W) {
#pragma unroll
            for (int k = 0; k < ROWS_PER_THREAD; ++k) {
                const int r = r0 + k * (NT / TW);
                if (y0 + r >= g.H) break;
                const uint32_t key = fkey(sharpen_at(s, lds, r, c));
                kmin_inv = max(kmin_inv, ~key);
                kmax = max(kmax, key);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kmin_inv = max(kmin_inv, (uint32_t)__shfl_xor((int)kmin_inv, o, 64));
        kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = kmin_inv; red[1][wave] = kmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; ++w) { kmin_inv = max(kmin_inv, red[0][w]); kmax = max(kmax, red[1][w]); }
        __hip_atomic_fetch_max(&st->min_key_inv, kmin_inv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&st->max_key, kmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t arrived = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = arrived == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    // ---- last-arriving workgroup: every other workgroup's maxima are in; read them and reset the slots for the next call
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const uint32_t kmi = ~__hip_atomic_exchange(&st->min_key_inv, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t kma = __hip_atomic_exchange(&st->max_key, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // vector store, for the next call
        // np.clip(Imin, 0.0, 0.45), np.clip(Imax, 0.55, 1.0) in float64 (a NaN passes through, as in np.clip)
        double lo = (double)fkey_inv(kmi), hi = (double)fkey_inv(kma);
        lo = lo < 0.0 ? 0.0 : (lo > 0.45 ? 0.45 : lo);
        hi = hi < 0.55 ? 0.55 : (hi > 1.0 ? 1.0 : hi);
        // deque: pop the oldest only when it holds more than `filter_size` entries, then append -> at most cap = size + 1
        const int cnt = st->count, slot = st->next;
        s_count = cnt < cap ? cnt + 1 : cap;
        s_slot = slot;
        s_new[0] = lo; s_new[1] = hi;
        double* ring = reinterpret_cast<double*>(st + 1);
        ring[slot] = lo;
        ring[cap + slot] = hi;
        st->count = s_count;
        st->next = slot + 1 == cap ? 0 : slot + 1;
    }
    __syncthreads();
    const int i = threadIdx.x, cnt = s_count;
    const double* ring = reinterpret_cast<const double*>(st + 1);
    if (i < cnt) {
        wlo[i] = i == s_slot ? s_new[0] : ring[i];
        whi[i] = i == s_slot ? s_new[1] : ring[cap + i];
    }
    __syncthreads();
    // np.median: rank every entry (ties broken by position), place it, average the two middle ones for an even count
    if (i < cnt) {
        const double vl = wlo[i], vh = whi[i];
        int rl = 0, rh = 0;
        for (int j = 0; j < cnt; ++j) {
            rl += (wlo[j] < vl) || (wlo[j] == vl && j < i);
            rh += (whi[j] < vh) || (whi[j] == vh && j < i);
        }
        slo[rl < cnt ? rl : cnt - 1] = vl;
        shi[rh < cnt ? rh : cnt - 1] = vh;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int m = cnt / 2;
        const double imin = (cnt & 1) ? slo[m] : (slo[m - 1] + slo[m]) / 2.0;
        const double imax = (cnt & 1) ? shi[m] : (shi[m - 1] + shi[m]) / 2.0;
        st->imin = imin;
        st->imax = imax;
        st->imin_f = (float)imin;
        st->inv_f = (float)(1.0 / (imax - imin));
    }
}

int check_common(const float* img, long long img_stride, long long row_stride, int N, int H, int W, const float* weights_host,
                 double amount, const uint8_t* out_u8) {
    if (!img || !out_u8 || (amount > 0.0 && !weights_host)) return OESS_EINVAL;
    if (N <= 0 || H <= 0 || W <= 0 || row_stride < W) return OESS_EINVAL;
    if (N > 1 && img_stride < (long long)(H - 1) * row_stride + W) return OESS_EINVAL;
    const long long tiles = (long long)N * ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
    if (tiles > 0x7fffffffLL) return OESS_EINVAL;
    return OESS_OK;
}

Geom make_geom(const float* img, long long img_stride, long long row_stride, int N, int H, int W) {
    return Geom{img, img_stride, row_stride, N, H, W, (W + TW - 1) / TW, (H + TH - 1) / TH};
}

Sharpen make_sharpen(const float* weights_host, double amount) {
    Sharpen s{};
    s.on = amount > 0.0;                                       // UnsharpMaskFilter: skipped entirely when amount <= 0
    if (s.on) {
        for (int k = 0; k < 25; ++k) s.w[k] = weights_host[k];
        s.c1 = (float)(1.0 + amount);
        s.c0 = (float)amount;
    }
    return s;
}

}  // namespace

extern "C" {

size_t oess_e2vid_postproc_state_bytes(int filter_size) {
    if (filter_size < 0 || filter_size > OESS_E2VID_POSTPROC_MAX_FILTER) return 0;
    return sizeof(StateHdr) + 2 * sizeof(double) * (size_t)(filter_size + 1);
}

int oess_e2vid_postprocess_f32(const float* img, long long img_stride, long long row_stride, int N, int H, int W,
                               const float* weights_host, double amount, double imin, double imax, uint8_t* out_u8, float* out_f32,
                               oess_stream_t stream) {
    const int e = check_common(img, img_stride, row_stride, N, H, W, weights_host, amount, out_u8);
    if (e) return e;
    if (!(imax > imin)) return OESS_EINVAL;                    // the reference divides by zero there
    const Geom g = make_geom(img, img_stride, row_stride, N, H, W);
    const float imin_f = (float)imin, inv_f = (float)(1.0 / (imax - imin));
    const int tiles = N * g.tiles_x * g.tiles_y;
    hipLaunchKernelGGL(postproc_apply_kernel<false>, dim3(tiles), dim3(NT), 0, (hipStream_t)stream, g, make_sharpen(weights_host, amount),
                       imin_f, inv_f, (const StateHdr*)nullptr, out_u8, out_f32);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_e2vid_postprocess_auto_hdr_f32(const float* img, long long img_stride, long long row_stride, int N, int H, int W,
                                        const float* weights_host, double amount, int filter_size, void* state, size_t state_bytes,
                                        uint8_t* out_u8, float* out_f32, oess_stream_t stream) {
    const int e = check_common(img, img_stride, row_stride, N, H, W, weights_host, amount, out_u8);
    if (e) return e;
    if (!state || filter_size < 0 || filter_size > OESS_E2VID_POSTPROC_MAX_FILTER) return OESS_EINVAL;
    if (state_bytes < oess_e2vid_postproc_state_bytes(filter_size)) return OESS_ENOMEM;
    if (((uintptr_t)state & 7) != 0) return OESS_EINVAL;
    const Geom g = make_geom(img, img_stride, row_stride, N, H, W);
    const Sharpen s = make_sharpen(weights_host, amount);
    const int tiles = N * g.tiles_x * g.tiles_y;
    const int grid = tiles < 2 * oess::num_cus() ? tiles : 2 * oess::num_cus();
    StateHdr* st = (StateHdr*)state;
    hipLaunchKernelGGL(postproc_stats_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, g, s, tiles, filter_size + 1, st);
    OESS_HIP(hipGetLastError());
    hipLaunchKernelGGL(postproc_apply_kernel<true>, dim3(tiles), dim3(NT), 0, (hipStream_t)stream, g, s, 0.0f, 0.0f,
                       (const StateHdr*)st, out_u8, out_f32);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
