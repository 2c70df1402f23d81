// K34: the SAM distillation loss of the frame2recon pre-training step on the two SMALL maps, as one forward and one backward node:
//   sam_up = F.interpolate(feat_sam, size=(M, M), bilinear, align_corners=False)[:, :, :H, :]      training/pretrain_trainer.py:519-529
//   loss   = mean(1 - F.cosine_similarity(sam_up, feat_recon, dim=1))
// feat_recon is DeepLabv3's upsampled feature (1.15 GB in bf16 at 8 x 256 x 440 x 640) and sam_up 2.3 GB in fp32; neither is written.
// a: student map [B, h, w, C] NHWC fp32 / bf16, upsampled to Ho x Wo (the index rule and blend of oess_resize_bilinear_nhwc_fwd).
// t: teacher map [B, ht, wt, C] NHWC fp32, resized to a VIRTUAL Mh x Mw grid (align_corners = False, two taps, no antialiasing: up or
//    down) of which only the top-left Ho x Wo is read.
//
// Forward (uc_fwd_kernel): one wave64 per output pixel, a lane owns four channels of every 256 (16-byte loads of the four corners of
// both maps, all L2 hits: the maps are a few MB), the three sums a.t, a.a, t.t meet by wave_sum.  cos follows oess_cosine_mean_fwd
// (norms clamped at eps).  A wave walks UC_PIX consecutive pixels and adds their cos in double; workgroups leave one double each
// and one block adds those in a fixed order (the rule of K23).  Per pixel the two scalars the backward needs are left in `planes`:
//   planes[2 p] = 1 / (max(|a|, eps) max(|t|, eps)),  planes[2 p + 1] = |a| > eps ? cos / (max(|a|, eps) |a|) : 0.
//
// Backward (uc_bwd_kernel): gather form, one wave per pixel of `a` with its clamped 3 x 3 neighbourhood in registers (four channels
// per lane).  Every output pixel whose footprint touches the pixel is visited once: a_p is recomputed from the registers by the
// forward's own operations, t_p from four loads of the teacher, and w_y w_x (t_p k0 - k1 a_p) accumulated: the gradient rule of
// oess_cosine_mean_bwd under the adjoint of the resize.  Each gradient element is written once, no atomics: bit-repeatable.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"
#include "bilinear_axis.h"

namespace {
using namespace oess;

constexpr int UC_THREADS = 256;
constexpr int UC_WAVES = UC_THREADS / 64;
constexpr int UC_PIX = 8;                         // consecutive output pixels per forward wave
constexpr int UC_MAX_C = 1024;

// four channels at element offset `idx`; vec: the address is aligned for one 16-byte (fp32) / 8-byte (bf16) access
template <bool BF16>
__device__ __forceinline__ float4 ld4(const void* __restrict__ p, int64_t idx, bool vec) {
    if constexpr (BF16) {
        const uint16_t* q = (const uint16_t*)p + idx;
        if (vec) {
            const uint2 r = *reinterpret_cast<const uint2*>(q);
            return make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                               __uint_as_float(r.y & 0xffff0000u));
        }
        return make_float4(bf16_to_f32(q[0]), bf16_to_f32(q[1]), bf16_to_f32(q[2]), bf16_to_f32(q[3]));
    }
    const float* q = (const float*)p + idx;
    if (vec) return *reinterpret_cast<const float4*>(q);
    return make_float4(q[0], q[1], q[2], q[3]);
}
template <bool BF16>
__device__ __forceinline__ void st4(void* __restrict__ p, int64_t idx, bool vec, float4 v) {
    if constexpr (BF16) {
        uint16_t* q = (uint16_t*)p + idx;
        if (vec) *reinterpret_cast<uint2*>(q) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
        else { q[0] = f32_to_bf16(v.x); q[1] = f32_to_bf16(v.y); q[2] = f32_to_bf16(v.z); q[3] = f32_to_bf16(v.w); }
        return;
    }
    float* q = (float*)p + idx;
    if (vec) *reinterpret_cast<float4*>(q) = v;
    else { q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w; }
}

// the blend of resize_fwd_kernel (ATen's association: columns inside each row, then the two rows)
__device__ __forceinline__ float blend1(float p00, float p01, float p10, float p11, float hy, float wy, float hx, float wx) {
    return hy * (hx * p00 + wx * p01) + wy * (hx * p10 + wx * p11);
}
__device__ __forceinline__ float4 blend4(float4 p00, float4 p01, float4 p10, float4 p11, float hy, float wy, float hx, float wx) {
    return make_float4(blend1(p00.x, p01.x, p10.x, p11.x, hy, wy, hx, wx), blend1(p00.y, p01.y, p10.y, p11.y, hy, wy, hx, wx),
                       blend1(p00.z, p01.z, p10.z, p11.z, hy, wy, hx, wx), blend1(p00.w, p01.w, p10.w, p11.w, hy, wy, hx, wx));
}

// teacher vector of output pixel (oy, ox) of sample b, channels c .. c + 3
__device__ __forceinline__ float4 teacher4(const float* __restrict__ t, int64_t tps, bool tvec, const Axis& ty, const Axis& tx, int64_t b,
                                           int oy, int ox, int c) {
    int y0, y1, x0, x1; float wy, wx;
    src_index(ty, oy, y0, y1, wy);
    src_index(tx, ox, x0, x1, wx);
    const int64_t r0 = (b * ty.in + y0) * tx.in, r1 = (b * ty.in + y1) * tx.in;
    return blend4(ld4<false>(t, (r0 + x0) * tps + c, tvec), ld4<false>(t, (r0 + x1) * tps + c, tvec), ld4<false>(t, (r1 + x0) * tps + c, tvec),
                  ld4<false>(t, (r1 + x1) * tps + c, tvec), 1.f - wy, wy, 1.f - wx, wx);
}

template <bool BF16>
__global__ __launch_bounds__(UC_THREADS) void uc_fwd_kernel(const void* __restrict__ a, int64_t aps, bool avec, const float* __restrict__ t,
                                                            int64_t tps, bool tvec, int C, Axis ay, Axis ax, Axis ty, Axis tx, int64_t P,
                                                            float eps, float* __restrict__ planes, double* __restrict__ partials) {
    __shared__ double red[UC_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p0 = ((int64_t)blockIdx.x * UC_WAVES + wave) * UC_PIX;
    double acc = 0.0;
    for (int i = 0; i < UC_PIX; ++i) {
        const int64_t p = p0 + i;
        if (p >= P) break;                                    // uniform over the wave
        const int ox = (int)(p % ax.out);
        const int64_t lin = p / ax.out;
        const int oy = (int)(lin % ay.out);
        const int64_t b = lin / ay.out;
        int y0, y1, x0, x1; float wy, wx;
        src_index(ay, oy, y0, y1, wy);
        src_index(ax, ox, x0, x1, wx);
        const float hy = 1.f - wy, hx = 1.f - wx;
        const int64_t r0 = (b * ay.in + y0) * ax.in, r1 = (b * ay.in + y1) * ax.in;
        float dot = 0.f, aa = 0.f, tt = 0.f;
        for (int c = lane * 4; c < C; c += 256) {
            const float4 u = blend4(ld4<BF16>(a, (r0 + x0) * aps + c, avec), ld4<BF16>(a, (r0 + x1) * aps + c, avec),
                                    ld4<BF16>(a, (r1 + x0) * aps + c, avec), ld4<BF16>(a, (r1 + x1) * aps + c, avec), hy, wy, hx, wx);
            const float4 v = teacher4(t, tps, tvec, ty, tx, b, oy, ox, c);
            dot += u.x * v.x; dot += u.y * v.y; dot += u.z * v.z; dot += u.w * v.w;
            aa += u.x * u.x; aa += u.y * u.y; aa += u.z * u.z; aa += u.w * u.w;
            tt += v.x * v.x; tt += v.y * v.y; tt += v.z * v.z; tt += v.w * v.w;
        }
        dot = wave_sum(dot); aa = wave_sum(aa); tt = wave_sum(tt);
        if (lane == 0) {
            const float na = sqrtf(aa), nt = sqrtf(tt);
            const float ca = fmaxf(na, eps), cb = fmaxf(nt, eps);
            acc += (double)(dot / (ca * cb));
            if (planes) {
                const float inv = 1.0f / (ca * cb);
                planes[2 * p] = inv;
                planes[2 * p + 1] = na > eps ? (dot * inv) / (ca * na) : 0.f;      // the clamp has zero gradient below eps
            }
        }
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < UC_WAVES; ++w) s += red[w];
        partials[blockIdx.x] = s;
    }
}

// second stage: one block adds the workgroup partials in a fixed order; loss = 1 - sum(cos) / P
__global__ __launch_bounds__(UC_THREADS) void uc_finish_kernel(const double* __restrict__ partials, int64_t n, double inv_p,
                                                               float* __restrict__ loss) {
    __shared__ double red[UC_THREADS];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += UC_THREADS) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = UC_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(1.0 - inv_p * red[0]);
}

template <bool BF16>
__global__ __launch_bounds__(UC_THREADS) void uc_bwd_kernel(const void* __restrict__ a, int64_t aps, bool avec, const float* __restrict__ t,
                                                            int64_t tps, bool tvec, int C, Axis ay, Axis ax, Axis ty, Axis tx, int64_t NP,
                                                            const float* __restrict__ planes, const float* __restrict__ grad_out,
                                                            double inv_p, void* __restrict__ ga, int64_t gaps, bool gvec) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t pix = (int64_t)blockIdx.x * UC_WAVES + wave;
    if (pix >= NP) return;
    const int ix = (int)(pix % ax.in);
    const int64_t lin = pix / ax.in;
    const int iy = (int)(lin % ay.in);
    const int64_t b = lin / ay.in;
    const int ys[3] = {max(iy - 1, 0), iy, min(iy + 1, ay.in - 1)};
    const int xs[3] = {max(ix - 1, 0), ix, min(ix + 1, ax.in - 1)};
    int ylo, yhi, xlo, xhi;
    candidates(ay, iy, ylo, yhi);
    candidates(ax, ix, xlo, xhi);
    const float g = (float)(-(double)grad_out[0] * inv_p);    // d loss / d cos_p
    for (int c = lane * 4; c < C; c += 256) {
        // a on the clamped 3 x 3 neighbourhood: n[r][s] = a[iy - 1 + r][ix - 1 + s]
        float4 n[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) n[r][s] = ld4<BF16>(a, ((b * ay.in + ys[r]) * ax.in + xs[s]) * aps + c, avec);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int oy = ylo; oy <= yhi; ++oy) {
            int y0, y1; float wy;
            src_index(ay, oy, y0, y1, wy);
            const float qy = (y0 == iy ? 1.0f - wy : 0.0f) + (y1 == iy ? wy : 0.0f);
            if (qy == 0.f) continue;
            const float hy = 1.f - wy;
            const bool top = y0 == iy;                        // source rows (iy, iy + 1), otherwise (iy - 1, iy)
            float4 v0[3], v1[3];                              // the two source rows of this output row
#pragma unroll
            for (int s = 0; s < 3; ++s) { v0[s] = top ? n[1][s] : n[0][s]; v1[s] = top ? n[2][s] : n[1][s]; }
            float4 racc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int ox = xlo; ox <= xhi; ++ox) {
                int x0, x1; float wx;
                src_index(ax, ox, x0, x1, wx);
                const float qx = (x0 == ix ? 1.0f - wx : 0.0f) + (x1 == ix ? wx : 0.0f);
                if (qx == 0.f) continue;
                const bool left = x0 == ix;
                const float4 u = blend4(left ? v0[1] : v0[0], left ? v0[2] : v0[1], left ? v1[1] : v1[0], left ? v1[2] : v1[1], hy, wy,
                                        1.f - wx, wx);
                const float4 v = teacher4(t, tps, tvec, ty, tx, b, oy, ox, c);
                const int64_t p = (b * ay.out + oy) * (int64_t)ax.out + ox;
                const float k0 = planes[2 * p], k1 = planes[2 * p + 1];
                racc.x += qx * (v.x * k0 - k1 * u.x); racc.y += qx * (v.y * k0 - k1 * u.y);
                racc.z += qx * (v.z * k0 - k1 * u.z); racc.w += qx * (v.w * k0 - k1 * u.w);
            }
            acc.x += qy * racc.x; acc.y += qy * racc.y; acc.z += qy * racc.z; acc.w += qy * racc.w;
        }
        st4<BF16>(ga, pix * gaps + c, gvec, make_float4(g * acc.x, g * acc.y, g * acc.z, g * acc.w));
    }
}

bool uc_geometry_ok(int B, int h, int w, int C, int Ho, int Wo) {
    return B > 0 && h > 0 && w > 0 && C > 0 && C % 4 == 0 && C <= UC_MAX_C && Ho >= h && Wo >= w;
}
bool uc_teacher_ok(int ht, int wt, int Mh, int Mw, int Ho, int Wo) { return ht > 0 && wt > 0 && Mh >= Ho && Mw >= Wo; }
int64_t uc_pixels(int B, int Ho, int Wo) { return (int64_t)B * Ho * Wo; }
int64_t uc_fwd_blocks(int64_t P) { return (P + UC_WAVES * UC_PIX - 1) / (UC_WAVES * UC_PIX); }
// every four-channel access of a map is aligned to `bytes` when its base and its pixel stride are (C % 4 == 0 does the rest)
bool uc_vec(const void* p, long long pix_stride, int elt, int bytes) {
    return ((uintptr_t)p % bytes) == 0 && ((size_t)pix_stride * elt) % bytes == 0;
}
}  // namespace

extern "C" {

size_t oess_upsampled_cosine_workspace_bytes(int B, int h, int w, int C, int Ho, int Wo) {
    if (!uc_geometry_ok(B, h, w, C, Ho, Wo)) return 0;
    return (size_t)uc_fwd_blocks(uc_pixels(B, Ho, Wo)) * sizeof(double);
}

size_t oess_upsampled_cosine_planes_floats(int B, int Ho, int Wo) {
    if (B <= 0 || Ho <= 0 || Wo <= 0) return 0;
    return (size_t)2 * (size_t)uc_pixels(B, Ho, Wo);
}

int oess_upsampled_cosine_fwd(const void* a, int a_is_bf16, long long a_pix_stride, const float* t, long long t_pix_stride, int B, int h,
                              int w, int C, int Ho, int Wo, int align_corners, int ht, int wt, int Mh, int Mw, float eps, void* workspace,
                              size_t workspace_bytes, float* planes, float* loss, oess_stream_t stream) {
    if (!a || !t || !workspace || !loss || !uc_geometry_ok(B, h, w, C, Ho, Wo) || !uc_teacher_ok(ht, wt, Mh, Mw, Ho, Wo) ||
        a_pix_stride < C || t_pix_stride < C || ((uintptr_t)workspace & 7))
        return OESS_EINVAL;
    const int64_t P = uc_pixels(B, Ho, Wo), blocks = uc_fwd_blocks(P);
    if (blocks > 0x7fffffffLL || workspace_bytes < (size_t)blocks * sizeof(double)) return OESS_EINVAL;
    const Axis ay = make_axis(h, Ho, align_corners), ax = make_axis(w, Wo, align_corners);
    const Axis ty = make_axis(ht, Mh, 0), tx = make_axis(wt, Mw, 0);
    const bool avec = a_is_bf16 ? uc_vec(a, a_pix_stride, 2, 8) : uc_vec(a, a_pix_stride, 4, 16), tvec = uc_vec(t, t_pix_stride, 4, 16);
    hipStream_t st = (hipStream_t)stream;
    if (a_is_bf16)
        hipLaunchKernelGGL(uc_fwd_kernel<true>, dim3((unsigned)blocks), dim3(UC_THREADS), 0, st, a, (int64_t)a_pix_stride, avec, t,
                           (int64_t)t_pix_stride, tvec, C, ay, ax, ty, tx, P, eps, planes, (double*)workspace);
    else
        hipLaunchKernelGGL(uc_fwd_kernel<false>, dim3((unsigned)blocks), dim3(UC_THREADS), 0, st, a, (int64_t)a_pix_stride, avec, t,
                           (int64_t)t_pix_stride, tvec, C, ay, ax, ty, tx, P, eps, planes, (double*)workspace);
    hipLaunchKernelGGL(uc_finish_kernel, dim3(1), dim3(UC_THREADS), 0, st, (const double*)workspace, blocks, 1.0 / (double)P, loss);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_upsampled_cosine_bwd(const void* a, int a_is_bf16, long long a_pix_stride, const float* t, long long t_pix_stride, int B, int h,
                              int w, int C, int Ho, int Wo, int align_corners, int ht, int wt, int Mh, int Mw, const float* planes,
                              const float* grad_out, void* grad_a, long long ga_pix_stride, oess_stream_t stream) {
    if (!a || !t || !planes || !grad_out || !grad_a || !uc_geometry_ok(B, h, w, C, Ho, Wo) || !uc_teacher_ok(ht, wt, Mh, Mw, Ho, Wo) ||
        a_pix_stride < C || t_pix_stride < C || ga_pix_stride < C)
        return OESS_EINVAL;
    const int64_t NP = (int64_t)B * h * w, blocks = (NP + UC_WAVES - 1) / UC_WAVES;
    if (blocks > 0x7fffffffLL) return OESS_EINVAL;
    const Axis ay = make_axis(h, Ho, align_corners), ax = make_axis(w, Wo, align_corners);
    const Axis ty = make_axis(ht, Mh, 0), tx = make_axis(wt, Mw, 0);
    const int elt = a_is_bf16 ? 2 : 4, bytes = a_is_bf16 ? 8 : 16;
    const bool avec = uc_vec(a, a_pix_stride, elt, bytes), tvec = uc_vec(t, t_pix_stride, 4, 16), gvec = uc_vec(grad_a, ga_pix_stride, elt, bytes);
    const double inv_p = 1.0 / (double)uc_pixels(B, Ho, Wo);
    hipStream_t st = (hipStream_t)stream;
    if (a_is_bf16)
        hipLaunchKernelGGL(uc_bwd_kernel<true>, dim3((unsigned)blocks), dim3(UC_THREADS), 0, st, a, (int64_t)a_pix_stride, avec, t,
                           (int64_t)t_pix_stride, tvec, C, ay, ax, ty, tx, NP, planes, grad_out, inv_p, grad_a, (int64_t)ga_pix_stride, gvec);
    else
        hipLaunchKernelGGL(uc_bwd_kernel<false>, dim3((unsigned)blocks), dim3(UC_THREADS), 0, st, a, (int64_t)a_pix_stride, avec, t,
                           (int64_t)t_pix_stride, tvec, C, ay, ax, ty, tx, NP, planes, grad_out, inv_p, grad_a, (int64_t)ga_pix_stride, gvec);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
