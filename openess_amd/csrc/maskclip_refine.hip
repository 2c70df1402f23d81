// K26: MaskCLIP's test-time refinement of the class logits (MaskClipHead.refine_output, models/maskclip_model.py:224-250 of the
// reference): prompt denoising and key smoothing, fp32 throughout, no floating-point atomics, fixed summation order.
//
//   conf[n, c] = max_l softmax_c(100 x)[n, c, l];   a class with conf < pd_thresh gets the logit -100 on every pixel
//   P = softmax_c(100 x) of the denoised logits;    k^ = k / max(||k[:, c]||_2 over the L tokens, 1e-12)   (F.normalize's dim 1)
//   a pixel with max_c P < ks_thresh takes its row of (k^ k^T) P, every other pixel keeps P
//
// (k^ k^T) P is evaluated as k (k^T P / n^2): the L x L matrix never exists.  Five launches per call:
//
//   refine_conf_kernel   one thread per pixel: softmax of 100 x (maximum subtracted first), per-class maximum of the block's 256
//                        pixels (wave butterfly, then the four waves in order; a maximum has no rounding)    -> cmax [B, nblk, KP]
//   refine_prob_kernel   one thread per pixel: conf from cmax, mask, then either the masked logits (smoothing off: untouched
//                        values are copied, never recomputed) or P [B, L, KP] (zero past K) and pmax [B, L]
//   refine_gram_kernel   block = 64 channels (one per lane) x a chunk of 128 tokens; P's chunk in LDS, read as broadcasts; a wave
//                        takes every fourth token in ascending order (fmaf chains), the four waves are summed in order
//                                                                                     -> Gp [B, chunks, C, KP], ssp [B, chunks, C]
//   refine_hm_kernel     chunks summed in ascending order; Hm[c, :] = G[c, :] / max(sqrt(ss[c]), 1e-12)^2        -> Hm [B, C, KP]
//   refine_apply_kernel  block = 4 waves x R tokens (R KP = 64 accumulators per lane), lane = channel; Hm staged through LDS 256
//                        channels at a time (rows padded by 4 floats: conflict-free ds_read_b128); the 64 lane partials of the
//                        64 (token, class) results are joined by a reduce-scatter butterfly (63 shuffles), after which lane e
//                        holds result e and selects smoothed / P by pmax < ks_thresh and stores it
//
// KP is K rounded up to 8, 16 or 32 (the register arrays).  k is fp32 or bf16, dense channels, with a row and an image stride,
// read one element per lane (no vector alignment asked of the tower's token matrix).  Every kernel guards l < L; C % 64 == 0.
#include <math.h>

#include "oess.h"
#include "oess_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int PIX = 256;       // pixels per block of the per-pixel kernels
constexpr int CH = 64;         // channels per block of the gram pass
constexpr int ROWS = 128;      // tokens per chunk of the gram pass
constexpr int CT = 256;        // channels of Hm in LDS per round of the apply pass
constexpr int MAX_K = 32, MAX_L = 4096, MAX_C = 1024, MAX_B = 65535;

struct View {                  // an fp32 [B, K, H, W] tensor by element strides
    float* p;
    long long sb, sc, sy, sx;
};

__device__ __forceinline__ float ld_k(const float* p) { return *p; }
__device__ __forceinline__ float ld_k(const uint16_t* p) { return oess::bf16_to_f32(*p); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// t[0 .. K) logits -> softmax(100 t), zeros past K; returns the largest probability
template <int KP>
__device__ __forceinline__ float softmax100(float (&t)[KP], int K) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < KP; ++j)
        if (j < K) {
            t[j] = t[j] * 100.f;
            m = fmaxf(m, t[j]);
        }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < KP; ++j)
        if (j < K) {
            t[j] = expf(t[j] - m);
            s += t[j];
        }
    float pm = 0.f;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        t[j] = j < K ? t[j] / s : 0.f;
        pm = fmaxf(pm, t[j]);
    }
    return pm;
}

template <int KP>
__device__ __forceinline__ void load_pixel(float (&t)[KP], const View& x, int b, int l, int W, int K) {
    const int y = l / W, xx = l - y * W;
    const float* p = x.p + (long long)b * x.sb + (long long)y * x.sy + (long long)xx * x.sx;
#pragma unroll
    for (int j = 0; j < KP; ++j) t[j] = j < K ? p[(long long)j * x.sc] : 0.f;
}

template <int KP>
__global__ __launch_bounds__(THREADS) void refine_conf_kernel(View x, int K, int L, int W, float* __restrict__ cmax) {
    __shared__ float red[THREADS / 64][KP];
    const int b = blockIdx.y, l = blockIdx.x * PIX + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float t[KP];
    if (l < L) {
        load_pixel<KP>(t, x, b, l, W, K);
        softmax100<KP>(t, K);
    } else {
#pragma unroll
        for (int j = 0; j < KP; ++j) t[j] = 0.f;             // a probability is never below 0
    }
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const float v = wave_max(t[j]);
        if (lane == 0) red[wave][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < KP) {
        const int j = threadIdx.x;
        cmax[((size_t)b * gridDim.x + blockIdx.x) * KP + j] = fmaxf(fmaxf(red[0][j], red[1][j]), fmaxf(red[2][j], red[3][j]));
    }
}

template <int KP>
__global__ __launch_bounds__(THREADS) void refine_prob_kernel(View x, int K, int L, int W, const float* __restrict__ cmax, float pd,
                                                              int smooth, View out, float* __restrict__ P, float* __restrict__ pmax) {
    __shared__ int masked[KP];
    const int b = blockIdx.y, l = blockIdx.x * PIX + threadIdx.x, nblk = gridDim.x;
    if (threadIdx.x < KP) {
        int m = 0;
        if (pd > 0.f && (int)threadIdx.x < K) {
            float c = 0.f;
            for (int i = 0; i < nblk; ++i) c = fmaxf(c, cmax[((size_t)b * nblk + i) * KP + threadIdx.x]);
            m = c < pd;
        }
        masked[threadIdx.x] = m;
    }
    __syncthreads();
    if (l >= L) return;
    float t[KP];
    load_pixel<KP>(t, x, b, l, W, K);
#pragma unroll
    for (int j = 0; j < KP; ++j)
        if (masked[j]) t[j] = -100.f;
    if (!smooth) {
        const int y = l / W, xx = l - y * W;
        float* o = out.p + (long long)b * out.sb + (long long)y * out.sy + (long long)xx * out.sx;
#pragma unroll
        for (int j = 0; j < KP; ++j)
            if (j < K) o[(long long)j * out.sc] = t[j];
        return;
    }
    const float pm = softmax100<KP>(t, K);
    float4* dst = reinterpret_cast<float4*>(P + ((size_t)b * L + l) * KP);
#pragma unroll
    for (int q = 0; q < KP / 4; ++q) dst[q] = make_float4(t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]);
    pmax[(size_t)b * L + l] = pm;
}

template <int KP, typename KT>
__global__ __launch_bounds__(THREADS) void refine_gram_kernel(const KT* __restrict__ k, long long krs, long long kis, int L, int C,
                                                              const float* __restrict__ P, float* __restrict__ Gp,
                                                              float* __restrict__ ssp) {
    __shared__ __attribute__((aligned(16))) float ps[ROWS * KP];
    __shared__ float red[THREADS / 64][KP + 1][CH];
    const int b = blockIdx.z, chunk = blockIdx.y, nch = gridDim.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l0 = chunk * ROWS, n = min(ROWS, L - l0);
    const float* src = P + ((size_t)b * L + l0) * KP;
    for (int i = threadIdx.x; i < ROWS * KP; i += THREADS) ps[i] = i < n * KP ? src[i] : 0.f;   // rows past L: zeros, never NaN
    __syncthreads();
    float acc[KP], ss = 0.f;
#pragma unroll
    for (int j = 0; j < KP; ++j) acc[j] = 0.f;
    const KT* kp = k + (long long)b * kis + (long long)l0 * krs + blockIdx.x * CH + lane;
    for (int r0 = wave; r0 < n; r0 += 16) {
        float kv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + 4 * u;
            kv[u] = r < n ? ld_k(kp + (long long)r * krs) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = min(r0 + 4 * u, ROWS - 1);
            ss = fmaf(kv[u], kv[u], ss);
#pragma unroll
            for (int q = 0; q < KP / 4; ++q) {
                const float4 p4 = *reinterpret_cast<const float4*>(&ps[r * KP + 4 * q]);
                acc[4 * q] = fmaf(kv[u], p4.x, acc[4 * q]);
                acc[4 * q + 1] = fmaf(kv[u], p4.y, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(kv[u], p4.z, acc[4 * q + 2]);
                acc[4 * q + 3] = fmaf(kv[u], p4.w, acc[4 * q + 3]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < KP; ++j) red[wave][j][lane] = acc[j];
    red[wave][KP][lane] = ss;
    __syncthreads();
    for (int i = threadIdx.x; i < (KP + 1) * CH; i += THREADS) {
        const int j = i / CH, ln = i - j * CH, c = blockIdx.x * CH + ln;
        const float v = ((red[0][j][ln] + red[1][j][ln]) + red[2][j][ln]) + red[3][j][ln];
        const size_t row = ((size_t)b * nch + chunk) * C + c;
        if (j < KP) Gp[row * KP + j] = v;
        else ssp[row] = v;
    }
}

__global__ __launch_bounds__(THREADS) void refine_hm_kernel(const float* __restrict__ Gp, const float* __restrict__ ssp, int nch, int C,
                                                            int KP, size_t total, float* __restrict__ Hm) {
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i % KP);
    const size_t bc = i / KP;
    const int c = (int)(bc % C);
    const size_t b = bc / C;
    float s = 0.f, g = 0.f;
    for (int ch = 0; ch < nch; ++ch) {
        const size_t row = (b * nch + ch) * C + c;
        s += ssp[row];
        g += Gp[row * KP + j];
    }
    const float nrm = fmaxf(sqrtf(s), 1e-12f);
    Hm[i] = g / (nrm * nrm);
}

template <int KP, typename KT>
__global__ __launch_bounds__(THREADS) void refine_apply_kernel(const KT* __restrict__ k, long long krs, long long kis, int L, int C, int W,
                                                               int K, const float* __restrict__ Hm, const float* __restrict__ P,
                                                               const float* __restrict__ pmax, float ks, View out) {
    constexpr int R = 64 / KP, LS = KP + 4;
    __shared__ __attribute__((aligned(16))) float hs[CT * LS];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l0 = blockIdx.x * (4 * R) + wave * R;
    float v[64];                                              // v[r KP + j]: this lane's channels' share of token l0 + r, class j
#pragma unroll
    for (int e = 0; e < 64; ++e) v[e] = 0.f;
    const float* hm = Hm + (size_t)b * C * KP;
    const KT* kb = k + (long long)b * kis + lane;
    for (int c0 = 0; c0 < C; c0 += CT) {
        const int nc = min(CT, C - c0);                      // a multiple of 64
        if (c0) __syncthreads();
        for (int i = threadIdx.x; i < nc * (KP / 4); i += THREADS) {
            const int c = i / (KP / 4), q = i - c * (KP / 4);
            *reinterpret_cast<float4*>(&hs[c * LS + 4 * q]) = reinterpret_cast<const float4*>(hm + (size_t)c0 * KP)[i];
        }
        __syncthreads();
        if (l0 < L) {
            for (int cs = 0; cs < nc; cs += 64) {
                float kv[R];
#pragma unroll
                for (int r = 0; r < R; ++r) kv[r] = l0 + r < L ? ld_k(kb + (long long)(l0 + r) * krs + c0 + cs) : 0.f;
#pragma unroll
                for (int q = 0; q < KP / 4; ++q) {
                    const float4 h = *reinterpret_cast<const float4*>(&hs[(cs + lane) * LS + 4 * q]);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        v[r * KP + 4 * q] = fmaf(kv[r], h.x, v[r * KP + 4 * q]);
                        v[r * KP + 4 * q + 1] = fmaf(kv[r], h.y, v[r * KP + 4 * q + 1]);
                        v[r * KP + 4 * q + 2] = fmaf(kv[r], h.z, v[r * KP + 4 * q + 2]);
                        v[r * KP + 4 * q + 3] = fmaf(kv[r], h.w, v[r * KP + 4 * q + 3]);
                    }
                }
            }
        }
    }
    if (l0 >= L) return;
    // reduce-scatter over the 64 lanes: after the step with mask m a lane keeps the half of its values whose index has bit m
    // equal to its own lane bit, summed with its partner's; in the end v[0] of lane e is the whole sum of result e
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const bool up = (lane & m) != 0;
#pragma unroll
        for (int i = 0; i < m; ++i) {
            const float keep = up ? v[i + m] : v[i];
            const float send = up ? v[i] : v[i + m];
            v[i] = keep + __shfl_xor(send, m, 64);
        }
    }
    const int r = lane / KP, j = lane - r * KP, l = l0 + r;
    if (l < L && j < K) {
        const float p = P[((size_t)b * L + l) * KP + j];
        const float res = pmax[(size_t)b * L + l] < ks ? v[0] : p;
        const int y = l / W, xx = l - y * W;
        out.p[(long long)b * out.sb + (long long)j * out.sc + (long long)y * out.sy + (long long)xx * out.sx] = res;
    }
}

int pick_kp(int K) { return K <= 8 ? 8 : K <= 16 ? 16 : 32; }

struct Layout {
    size_t cmax, P, pmax, Gp, ssp, Hm, total;
    int nblk, nch, KP;
};

// offsets in floats; every array starts on 256 bytes
bool make_layout(int B, int K, int H, int W, int C, Layout& lay) {
    if (B < 1 || B > MAX_B || K < 1 || K > MAX_K || H < 1 || W < 1 || (long long)H * W > MAX_L) return false;
    if (C != 0 && (C < 64 || C > MAX_C || C % 64 != 0)) return false;
    const size_t L = (size_t)H * W;
    lay.KP = pick_kp(K);
    lay.nblk = (int)((L + PIX - 1) / PIX);
    lay.nch = (int)((L + ROWS - 1) / ROWS);
    size_t off = 0;
    auto take = [&](size_t floats) {
        const size_t at = off;
        off += oess::align_up(floats, 64);
        return at;
    };
    lay.cmax = take((size_t)B * lay.nblk * lay.KP);
    lay.P = take(C ? (size_t)B * L * lay.KP : 0);
    lay.pmax = take(C ? (size_t)B * L : 0);
    lay.Gp = take((size_t)B * lay.nch * C * lay.KP);
    lay.ssp = take((size_t)B * lay.nch * C);
    lay.Hm = take((size_t)B * C * lay.KP);
    lay.total = off * sizeof(float);
    return true;
}

// the elements of a [n0, n1, n2, n3] view are distinct: sorted by stride, each stride clears the span of the smaller ones
bool distinct(const long long (&size)[4], const long long (&stride)[4]) {
    int order[4] = {0, 1, 2, 3};
    for (int a = 0; a < 4; ++a)
        for (int c = a + 1; c < 4; ++c)
            if (stride[order[c]] < stride[order[a]]) {
                const int t = order[a];
                order[a] = order[c];
                order[c] = t;
            }
    long long span = 0;
    for (int a = 0; a < 4; ++a) {
        const int d = order[a];
        if (size[d] == 1) continue;
        if (stride[d] <= span) return false;
        span += (size[d] - 1) * stride[d];
    }
    return true;
}

template <int KP, typename KT>
void launch_smooth(const KT* k, long long krs, long long kis, int B, int K, int L, int W, int C, const Layout& lay, float* ws, float ks,
                   const View& out, hipStream_t st, hipEvent_t* ev) {
    hipLaunchKernelGGL((refine_gram_kernel<KP, KT>), dim3(C / CH, lay.nch, B), dim3(THREADS), 0, st, k, krs, kis, L, C, ws + lay.P,
                       ws + lay.Gp, ws + lay.ssp);
    if (ev) (void)hipEventRecord(ev[3], st);
    const size_t total = (size_t)B * C * KP;
    hipLaunchKernelGGL(refine_hm_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, ws + lay.Gp,
                       ws + lay.ssp, lay.nch, C, KP, total, ws + lay.Hm);
    if (ev) (void)hipEventRecord(ev[4], st);
    constexpr int RB = 4 * (64 / KP);
    hipLaunchKernelGGL((refine_apply_kernel<KP, KT>), dim3((L + RB - 1) / RB, B), dim3(THREADS), 0, st, k, krs, kis, L, C, W, K,
                       ws + lay.Hm, ws + lay.P, ws + lay.pmax, ks, out);
    if (ev) (void)hipEventRecord(ev[5], st);
}

template <int KP>
void launch_all(const View& x, int B, int K, int H, int W, const void* k, int k_dtype, long long krs, long long kis, int C, float pd,
                float ks, const View& out, const Layout& lay, float* ws, hipStream_t st, hipEvent_t* ev) {
    const int L = H * W;
    const bool smooth = k != nullptr && ks > 0.f;
    if (ev) (void)hipEventRecord(ev[0], st);
    if (pd > 0.f)
        hipLaunchKernelGGL(refine_conf_kernel<KP>, dim3(lay.nblk, B), dim3(THREADS), 0, st, x, K, L, W, ws + lay.cmax);
    if (ev) (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(refine_prob_kernel<KP>, dim3(lay.nblk, B), dim3(THREADS), 0, st, x, K, L, W, ws + lay.cmax, pd, smooth ? 1 : 0, out,
                       ws + lay.P, ws + lay.pmax);
    if (ev) (void)hipEventRecord(ev[2], st);
    if (smooth) {
        if (k_dtype == OESS_MASKCLIP_K_F32)
            launch_smooth<KP, float>(static_cast<const float*>(k), krs, kis, B, K, L, W, C, lay, ws, ks, out, st, ev);
        else
            launch_smooth<KP, uint16_t>(static_cast<const uint16_t*>(k), krs, kis, B, K, L, W, C, lay, ws, ks, out, st, ev);
    } else if (ev) {
        for (int i = 3; i < 6; ++i) (void)hipEventRecord(ev[i], st);
    }
}

int refine(const float* logits, long long sb, long long sc, long long sy, long long sx, int B, int K, int H, int W, const void* k,
           int k_dtype, long long k_row_stride, long long k_img_stride, int C, float pd_thresh, float ks_thresh, float* out,
           long long ob, long long oc, long long oy, long long ox, void* workspace, size_t workspace_bytes, hipStream_t st,
           float* phase_ms) {
    if (!logits || !out || !workspace || !(pd_thresh >= 0.f) || !(ks_thresh >= 0.f) || !(pd_thresh < INFINITY) || !(ks_thresh < INFINITY))
        return OESS_EINVAL;
    Layout lay;
    if (!make_layout(B, K, H, W, k ? C : 0, lay) || (k && C == 0)) return OESS_EINVAL;
    const long long lim = 1ll << 40;
    if (sb < 0 || sc < 0 || sy < 0 || sx < 0 || sb >= lim || sc >= lim || sy >= lim || sx >= lim) return OESS_EINVAL;
    if (ob >= lim || oc >= lim || oy >= lim || ox >= lim) return OESS_EINVAL;
    const long long size[4] = {B, K, H, W}, ostride[4] = {ob, oc, oy, ox};
    if (ob < 0 || oc < 0 || oy < 0 || ox < 0 || !distinct(size, ostride)) return OESS_EINVAL;
    if (((uintptr_t)logits & 3) || ((uintptr_t)out & 3) || ((uintptr_t)workspace & 15)) return OESS_EINVAL;
    if (k) {
        const long long L = (long long)H * W;
        if (k_dtype != OESS_MASKCLIP_K_F32 && k_dtype != OESS_MASKCLIP_K_BF16) return OESS_EINVAL;
        if ((uintptr_t)k & (k_dtype == OESS_MASKCLIP_K_F32 ? 3 : 1)) return OESS_EINVAL;
        if (k_row_stride < C || k_row_stride >= lim || k_img_stride < 0 || k_img_stride >= lim) return OESS_EINVAL;
        if (B > 1 && k_img_stride < (L - 1) * k_row_stride + C) return OESS_EINVAL;
    }
    if (workspace_bytes < lay.total) return OESS_ENOMEM;
    const View x{const_cast<float*>(logits), sb, sc, sy, sx}, o{out, ob, oc, oy, ox};
    float* ws = static_cast<float*>(workspace);
    hipEvent_t evs[6];
    hipEvent_t* ev = nullptr;
    if (phase_ms) {
        for (int i = 0; i < 6; ++i) OESS_HIP(hipEventCreate(&evs[i]));
        ev = evs;
    }
    if (lay.KP == 8) launch_all<8>(x, B, K, H, W, k, k_dtype, k_row_stride, k_img_stride, C, pd_thresh, ks_thresh, o, lay, ws, st, ev);
    else if (lay.KP == 16) launch_all<16>(x, B, K, H, W, k, k_dtype, k_row_stride, k_img_stride, C, pd_thresh, ks_thresh, o, lay, ws, st, ev);
    else launch_all<32>(x, B, K, H, W, k, k_dtype, k_row_stride, k_img_stride, C, pd_thresh, ks_thresh, o, lay, ws, st, ev);
    int rc = hipGetLastError() == hipSuccess ? OESS_OK : OESS_ELAUNCH;
    if (ev) {
        if (rc == OESS_OK && hipEventSynchronize(evs[5]) != hipSuccess) rc = OESS_ELAUNCH;
        for (int i = 0; i < 5 && rc == OESS_OK; ++i)
            if (hipEventElapsedTime(&phase_ms[i], evs[i], evs[i + 1]) != hipSuccess) rc = OESS_ELAUNCH;
        for (int i = 0; i < 6; ++i) (void)hipEventDestroy(evs[i]);
    }
    return rc;
}

}  // namespace

extern "C" {

size_t oess_maskclip_refine_workspace_bytes(int B, int K, int H, int W, int C) {
    Layout lay;
    return make_layout(B, K, H, W, C, lay) ? lay.total : 0;
}

int oess_maskclip_refine_f32(const float* logits, long long sb, long long sc, long long sy, long long sx, int B, int K, int H, int W,
                             const void* k, int k_dtype, long long k_row_stride, long long k_img_stride, int C, float pd_thresh,
                             float ks_thresh, float* out, long long ob, long long oc, long long oy, long long ox, void* workspace,
                             size_t workspace_bytes, oess_stream_t stream) {
    return refine(logits, sb, sc, sy, sx, B, K, H, W, k, k_dtype, k_row_stride, k_img_stride, C, pd_thresh, ks_thresh, out, ob, oc, oy,
                  ox, workspace, workspace_bytes, (hipStream_t)stream, nullptr);
}

int oess_maskclip_refine_phase_ms(const float* logits, long long sb, long long sc, long long sy, long long sx, int B, int K, int H, int W,
                                  const void* k, int k_dtype, long long k_row_stride, long long k_img_stride, int C, float pd_thresh,
                                  float ks_thresh, float* out, long long ob, long long oc, long long oy, long long ox, void* workspace,
                                  size_t workspace_bytes, float* phase_ms, oess_stream_t stream) {
    if (!phase_ms) return OESS_EINVAL;
    return refine(logits, sb, sc, sy, sx, B, K, H, W, k, k_dtype, k_row_stride, k_img_stride, C, pd_thresh, ks_thresh, out, ob, oc, oy,
                  ox, workspace, workspace_bytes, (hipStream_t)stream, phase_ms);
}
}
