// What the render kernels share (segment_render.hip K35, vocab_render.hip K36): the output bundle, the tap, the running
// (maximum, index, sum) step of the online softmax, the class walk over contiguous groups of names, a pixel's bytes into the
// staging rows and the staging rows to global memory as aligned dwords.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess_common.h"

namespace oess {
namespace render {

constexpr int THREADS = 256;
constexpr int MAX_K = 255;

struct Render {
    const uint8_t* palette;       // [K][3] or null (then rgb is null)
    const uint8_t* grey;          // [B][H][W] or null
    uint8_t* labels;              // [B][H][W] or null
    float* conf;                  // [B][H][W] or null
    uint8_t* rgb;                 // [B][H][W][3] or null
    int alpha256, ignore_label;
    float min_conf;
};

template <bool BF16>
__device__ __forceinline__ float tap(const void* __restrict__ p, int64_t off) {
    return BF16 ? bf16_to_f32(reinterpret_cast<const uint16_t*>(p)[off]) : reinterpret_cast<const float*>(p)[off];
}

// One class value into the running (maximum, index, sum of exp(v - maximum)).  The maximum moves under torch.argmax's order
// (label_ops.hip take()): v replaces best when it is larger, or when it is the first NaN.
__device__ __forceinline__ void take(float v, int k, float& best, int& idx, float& sum) {
    if (v > best || (v != v && best == best)) {
        sum = sum * __expf(best - v) + 1.f;
        best = v; idx = k;
    } else {
        sum = sum + __expf(v - best);
    }
}

// One member value into its class value under torch.amax's rule: the larger one, and a NaN member makes (and keeps) it NaN.
__device__ __forceinline__ void amax_step(float v, float& m) {
    if (v > m || v != v) m = v;
}

// The walk over K classes whose names are the channels offs[k] ... offs[k + 1] - 1 (offs: K + 1 ascending ints in LDS);
// value(p) is the fp32 value of channel p.  Leaves torch.argmax's index over the class values and the sum of
// exp(c_k - c_max); every channel is evaluated once, in ascending p.  Offsets that are no such list (each within 0 ... P, the
// caller's part) give meaningless classes but no channel outside 0 ... P - 1: a class's first member is clamped.
template <typename F>
__device__ __forceinline__ void class_walk(const int* offs, int K, int P, F value, int& idx, float& sum) {
    float best = 0.f;
    idx = 0; sum = 1.f;
    int p = offs[0];
    for (int k = 0; k < K; ++k) {
        const int end = offs[k + 1];
        float m = value(p < P ? p : P - 1);
        for (++p; p < end; ++p) amax_step(value(p), m);
        if (k == 0) best = m; else take(m, k, best, idx, sum);
    }
}

// The staging rows of one chunk of THREADS pixels and the palette: one set per workgroup.
struct Stage {
    __attribute__((aligned(4))) uint8_t lab[THREADS + 4];
    __attribute__((aligned(4))) uint8_t rgb[3 * THREADS + 4];
    uint8_t pal[3 * MAX_K + 3];                                  // the palette, then (0, 0, 0) for ignore_label
};

__device__ __forceinline__ void load_palette(Stage& s, const Render& r, int K) {
    if (r.rgb) {
        for (int j = threadIdx.x; j < 3 * K + 3; j += THREADS) s.pal[j] = j < 3 * K ? r.palette[j] : (uint8_t)0;
    }
}

// A pixel's outputs from its (index, confidence): conf as one dword, the label and colour bytes into the staging rows at the byte
// phase of the row's global address.  pix: the pixel's index in [B][H][W].
__device__ __forceinline__ void emit_conf(Stage& s, const Render& r, int K, int64_t pix, int lphase, int cphase, int idx, float conf) {
    int label = idx;
    if (conf < r.min_conf) label = r.ignore_label;                  // false for a NaN confidence: the label stays
    if (r.conf) r.conf[pix] = conf;
    if (r.labels) s.lab[lphase + threadIdx.x] = (uint8_t)label;
    if (r.rgb) {
        const uint8_t* c = s.pal + 3 * (label == r.ignore_label ? K : label);
        int c0 = c[0], c1 = c[1], c2 = c[2];
        if (r.grey) {
            const int g = (256 - r.alpha256) * (int)r.grey[pix] + 128;
            c0 = (r.alpha256 * c0 + g) >> 8; c1 = (r.alpha256 * c1 + g) >> 8; c2 = (r.alpha256 * c2 + g) >> 8;
        }
        uint8_t* d = s.rgb + cphase + 3 * threadIdx.x;
        d[0] = (uint8_t)c0; d[1] = (uint8_t)c1; d[2] = (uint8_t)c2;
    }
}

// The same from a pixel's (index, sum of exp(v - maximum)): the confidence is 1 / sum.
__device__ __forceinline__ void emit(Stage& s, const Render& r, int K, int64_t pix, int lphase, int cphase, int idx, float sum) {
    emit_conf(s, r, K, pix, lphase, cphase, idx, 1.f / sum);
}

// n staged bytes, stage[phase ... phase + n), to g (phase = g & 3): every dword that lies inside the range is one aligned
// store; the at most two ragged dwords at the ends are written byte by byte (their other bytes belong to someone else).
__device__ __forceinline__ void flush_bytes(const uint8_t* stage, uint8_t* g, int phase, int n) {
    uint8_t* g0 = g - phase;                                               // 4-byte aligned
    const int end = phase + n;
    for (int lo = threadIdx.x * 4; lo < end; lo += THREADS * 4) {
        if (lo >= phase && lo + 4 <= end) {
            *reinterpret_cast<uint32_t*>(g0 + lo) = *reinterpret_cast<const uint32_t*>(stage + lo);
        } else {
            const int a = lo < phase ? phase : lo, b = lo + 4 < end ? lo + 4 : end;
            for (int j = a; j < b; ++j) g0[j] = stage[j];
        }
    }
}

// The chunk's staged bytes to global memory, between two barriers (the next chunk overwrites the staging).  Every lane of the
// workgroup calls it; n: the chunk's pixel count, pix0: its first pixel.
__device__ __forceinline__ void flush_chunk(const Stage& s, const Render& r, int64_t pix0, int lphase, int cphase, int n) {
    __syncthreads();
    if (r.labels) flush_bytes(s.lab, r.labels + pix0, lphase, n);
    if (r.rgb) flush_bytes(s.rgb, r.rgb + 3 * pix0, cphase, 3 * n);
    __syncthreads();
}

// The refusals every render entry shares (oess.h, oess_segment_render).
static inline bool bad_render_args(const uint8_t* palette, const uint8_t* labels, const float* conf, const uint8_t* rgb, int K,
                                   int alpha256, float min_conf, int ignore_label) {
    return (!labels && !conf && !rgb) || (rgb && !palette) || K < 1 || K > MAX_K || ignore_label < K || ignore_label > 255 ||
           alpha256 < 0 || alpha256 > 256 || !(min_conf >= 0.f);
}

}  // namespace render
}  // namespace oess
