// K27  Reconstructed grey levels -> the augmented three-channel fp32 image the frame2recon student reads: what
// DSEC/dataset/sequence_ov.py:204-221 builds on the host from the reconstruction PNG (image_to_chw_float, torch.flip,
// _io.adjust_brightness, _io.adjust_contrast, + 0.05 randn), from PostProcessor.process_u8's bytes, per sample b of uint8 [B, H, W]:
//   v  = (float)byte / 255.0f                       IEEE division (built with -fhip-fp32-correctly-rounded-divide-sqrt): the bits of
//                                                   np.float32(byte / 255.0), what the PNG path reads; replicated to three channels
//   flip[b]: out(y, x) reads byte(y, W - 1 - x)
//   v  = clamp(fl(bri[b] * v), 0, 1)                adjust_brightness: blend with black (ratio * a + (1 - ratio) * 0)
//   m  = mean over the H W pixels of  g = fl(fl(fl(0.2989f * v) + fl(0.587f * v)) + fl(0.114f * v))      (built with -ffp-contract=off)
//   v  = clamp(fl(fl(con[b] * v) + fl(fl(1 - con[b]) * m)), 0, 1)      adjust_contrast; skipped for con[b] == 1 (same bits, no mean)
//   seed[b] != 0: v = fl(v + fl(0.05f * n))         n ~ N(0, 1) per channel and pixel, no clamp afterwards (as the reference)
// Mean: two levels in a fixed order, no atomics.  Level 1 (gray_partials_kernel): one 256-thread workgroup per PART = 4096
//   consecutive pixels of a sample; thread t adds pixels t, t + 256, ... of its part in ascending order (fp32), the 64 lanes of a
//   wave join by the xor butterfly 32, 16, .., 1, thread 0 adds the four waves in order -> one fp32 partial.  Level 2 (in every
//   workgroup of the apply kernel, wave 0): lane l adds partials l, l + 64, ... in ascending order in float64, same butterfly;
//   m = (float)(sum / (H W)).  Both depend on the sample's own bytes and factor only: not on B, not on its place in the batch.
// Noise: Philox-4x32-10 (philox.h), key = (seed low word, seed high word), counter = (g low, g high, 0, 0) with g the index of
//   the group of four consecutive elements e = 4 g .. 4 g + 3 of the sample's flat [3, H, W] block.  Words (x, y) and (z, w)
//   each give two normals by Box-Muller:  u = ((word >> 8) + 1) * 2^-24  (24 bits, in (0, 1], exact in fp32: the logarithm never
//   sees 0);  r = sqrtf(-2 logf(u_a)), th = 6.2831855f * u_b;  element 4 g + 0: r cosf(th), + 1: r sinf(th) from (x, y), + 2 and
//   + 3 likewise from (z, w).  tests/recon_augment_reference.py restates all of it in float64.
// Launch: the per-sample host arrays travel as kernel arguments, CHUNK = 32 samples per launch (no device copy, no host
//   synchronisation).  Apply: one thread per element group, grid (groups / 256, samples); a 16-byte store per thread when
//   H W % 4 == 0 and out is 16-byte aligned (then a group never straddles a channel plane), four 4-byte stores otherwise.
// Bytes at 8 x 440 x 640: 2.25 MB read (three times, from cache after the first) + 27.0 MB written: bound by the fp32 store.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"
#include "philox.h"

namespace {

constexpr int NT = 256, PART = 4096, CHUNK = 32;

struct Samples {                 // per-sample host arrays of one launch, by value
    unsigned long long seed[CHUNK];
    float bri[CHUNK], con[CHUNK];
    unsigned char flip[CHUNK];
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float level(uint8_t b) { return (float)b / 255.0f; }
__device__ __forceinline__ float unit24(uint32_t w) { return (float)((w >> 8) + 1u) * 0x1p-24f; }

// level 1: partial[blockIdx.y][blockIdx.x] = sum of the brightness-adjusted grey values of pixels [x PART, (x + 1) PART)
__global__ __launch_bounds__(NT) void gray_partials_kernel(const uint8_t* __restrict__ u8, long long P, int nparts, Samples s,
                                                           float* __restrict__ partials) {
    __shared__ float red[NT / 64];
    const int b = blockIdx.y;
    if (s.con[b] == 1.0f) return;                           // no blend for this sample: nothing reads its partials
    const uint8_t* src = u8 + (long long)b * P;
    const float bri = s.bri[b];
    const long long p0 = (long long)blockIdx.x * PART;
    float acc = 0.0f;
    for (int i = 0; i < PART / NT; ++i) {
        const long long p = p0 + threadIdx.x + i * NT;
        if (p < P) {
            const float v = clamp01(bri * level(src[p]));
            acc += 0.2989f * v + 0.587f * v + 0.114f * v;
        }
    }
    acc = oess::wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[(long long)b * nparts + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

template <bool VEC>
__global__ __launch_bounds__(NT) void gray_augment_kernel(const uint8_t* __restrict__ u8, int H, int W, long long P, int nparts,
                                                          Samples s, const float* __restrict__ partials, float* __restrict__ out) {
    __shared__ float s_mean;
    const int b = blockIdx.y;
    const float con = s.con[b], bri = s.bri[b];
    const bool blend = con != 1.0f;
    if (blend) {                                            // level 2, uniform over the workgroup
        if (threadIdx.x < 64) {
            double acc = 0.0;
            for (int i = threadIdx.x; i < nparts; i += 64) acc += (double)partials[(long long)b * nparts + i];
            acc = oess::wave_sum(acc);
            if (threadIdx.x == 0) s_mean = (float)(acc / (double)P);
        }
        __syncthreads();
    }
    const long long E = 3 * P;
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    const long long e0 = 4 * g;
    if (e0 >= E) return;
    const float rest = blend ? (1.0f - con) * s_mean : 0.0f;
    const bool flip = s.flip[b] != 0;
    const unsigned long long seed = s.seed[b];
    const uint8_t* src = u8 + (long long)b * P;
    float v[4];
    int n = E - e0 < 4 ? (int)(E - e0) : 4;
    long long p = e0 % P;                                   // pixel of the first element; its channel does not matter
    int y = (int)(p / W), x = (int)(p - (long long)y * W);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < n) {
            v[k] = level(src[(long long)y * W + (flip ? W - 1 - x : x)]);
            if (++x == W) { x = 0; if (++y == H) y = 0; }   // next row, or the first pixel of the next channel plane
        } else {
            v[k] = 0.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = clamp01(bri * v[k]);
        if (blend) v[k] = clamp01(con * v[k] + rest);
    }
    if (seed != 0) {
        const uint4 w = oess::philox4x32_10(make_uint4((uint32_t)g, (uint32_t)((uint64_t)g >> 32), 0u, 0u),
                                            make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
        const float r0 = sqrtf(-2.0f * logf(unit24(w.x))), t0 = 6.2831855f * unit24(w.y);
        const float r1 = sqrtf(-2.0f * logf(unit24(w.z))), t1 = 6.2831855f * unit24(w.w);
        v[0] = v[0] + 0.05f * (r0 * cosf(t0));
        v[1] = v[1] + 0.05f * (r0 * sinf(t0));
        v[2] = v[2] + 0.05f * (r1 * cosf(t1));
        v[3] = v[3] + 0.05f * (r1 * sinf(t1));
    }
    float* dst = out + (long long)b * E + e0;
    if (VEC) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);      // E % 4 == 0: n == 4 always
    } else {
        for (int k = 0; k < n; ++k) dst[k] = v[k];
    }
}

inline long long parts_of(long long P) { return (P + PART - 1) / PART; }

}  // namespace

extern "C" {

size_t oess_gray_augment_scratch_bytes(int64_t B, int64_t H, int64_t W) {
    if (B < 1 || H < 1 || W < 1 || H > 0x7fffffffLL / W || B > 0x7fffffffLL) return 0;
    return (size_t)B * (size_t)parts_of(H * W) * sizeof(float);
}

int oess_gray_augment_rgb_f32(const uint8_t* u8, int B, int H, int W, const int32_t* flip_host, const float* brightness_host,
                              const float* contrast_host, const uint64_t* noise_seed_host, float* out, void* scratch,
                              size_t scratch_bytes, oess_stream_t stream) {
    if (!u8 || !out || !flip_host || !brightness_host || !contrast_host || !noise_seed_host) return OESS_EINVAL;
    if (B < 1 || H < 1 || W < 1) return OESS_EINVAL;
    const long long P = (long long)H * W;
    if (3 * P > 0x7fffffffLL) return OESS_EINVAL;           // element indices of one sample stay below 2^31
    if (((uintptr_t)out & 3) != 0) return OESS_EINVAL;
    bool any_blend = false;
    for (int b = 0; b < B; ++b) {
        if (flip_host[b] != 0 && flip_host[b] != 1) return OESS_EINVAL;
        if (!(brightness_host[b] >= 0.0f && brightness_host[b] <= 3.4e38f)) return OESS_EINVAL;      // finite, not NaN
        if (!(contrast_host[b] >= 0.0f && contrast_host[b] <= 3.4e38f)) return OESS_EINVAL;
        any_blend = any_blend || contrast_host[b] != 1.0f;
    }
    const int nparts = (int)parts_of(P);
    if (any_blend) {
        if (!scratch || ((uintptr_t)scratch & 3) != 0) return OESS_EINVAL;
        if (scratch_bytes < oess_gray_augment_scratch_bytes(B, H, W)) return OESS_ENOMEM;
    }
    const bool vec = (P % 4 == 0) && (((uintptr_t)out & 15) == 0);
    const long long groups = (3 * P + 3) / 4;
    const unsigned gx = (unsigned)((groups + NT - 1) / NT);
    for (int b0 = 0; b0 < B; b0 += CHUNK) {
        const int nb = B - b0 < CHUNK ? B - b0 : CHUNK;
        Samples s{};
        bool blend = false;
        for (int i = 0; i < nb; ++i) {
            s.seed[i] = noise_seed_host[b0 + i];
            s.bri[i] = brightness_host[b0 + i];
            s.con[i] = contrast_host[b0 + i];
            s.flip[i] = (unsigned char)flip_host[b0 + i];
            blend = blend || s.con[i] != 1.0f;
        }
        const uint8_t* src = u8 + (long long)b0 * P;
        float* part = any_blend ? (float*)scratch + (long long)b0 * nparts : nullptr;
        float* dst = out + (long long)b0 * 3 * P;
        if (blend) {
            hipLaunchKernelGGL(gray_partials_kernel, dim3((unsigned)nparts, (unsigned)nb), dim3(NT), 0, (hipStream_t)stream, src, P,
                               nparts, s, part);
            OESS_HIP(hipGetLastError());
        }
        if (vec)
            hipLaunchKernelGGL(gray_augment_kernel<true>, dim3(gx, (unsigned)nb), dim3(NT), 0, (hipStream_t)stream, src, H, W, P,
                               nparts, s, (const float*)part, dst);
        else
            hipLaunchKernelGGL(gray_augment_kernel<false>, dim3(gx, (unsigned)nb), dim3(NT), 0, (hipStream_t)stream, src, H, W, P,
                               nparts, s, (const float*)part, dst);
        OESS_HIP(hipGetLastError());
    }
    return OESS_OK;
}

}  // extern "C"
