// Segmentation maps from the MEAN class probability of V logit maps (K39, flip and multi-scale inference): per output pixel the
// label (u8), the mean probability of that class (fp32) and a colour (u8 x 3), without any full-resolution [B, K, H, W] tensor.
// The ensemble counterpart of segment_render.hip (K35), whose values, addressing, work split and staged byte stores this file keeps.
// Views.  View v is NHWC logits [B x h_v x w_v x K] with its own pixel stride and a horizontal flip flag.  Its class values at
// output pixel (oy, ox) are K35's values at (oy, ox'), ox' = flip_v ? W - 1 - ox : ox: the raw logit when (h_v, w_v) == (H, W),
// otherwise resize_fwd_kernel's blend in its association (src_index on both axes, bf16 taps widened first, no FMA contraction).
// A flipped view is the view rendered as given and then mirrored: resize(model(x.flip(-1))).flip(-1).
// Probabilities.  q_vk = exp(v_vk - m_v) * (1 / S_v), m_v = max_k v_vk, S_v = sum_k exp(v_vk - m_v) (take()'s running walk), fp32,
// exp = __expf.  A view whose maximum is not finite (a NaN, a +inf, only -inf) has 1 / S_v = NaN: every q_vk is NaN there, as
// torch.softmax makes them.
// Mean.  p_k = (sum_v q_vk) * (1.0f / V), ascending v.  Label = torch.argmax's rule over p_k, confidence = p_label.
// Two walks over K per view instead of K accumulators per lane: walk A leaves (m_v, 1 / S_v) of every view in registers, walk B
// forms the values again class by class, sums q_vk over the views and keeps a running first-argmax.  Nothing per class is stored,
// so K up to 255 costs no registers.  The per-view state lives in registers: every loop over the views is fully unrolled over
// MAX_VIEWS with a uniform `v < V` guard, no array is indexed at run time.
// One lane owns a pixel from the first tap to its bytes: no atomics, no cross-lane floating-point reduction, two calls give the
// same bits.  One workgroup per OUTPUT ROW; the two source rows of every resized view as fp32 [2][w_v][K] in LDS when ALL of them
// fit LDS_BUDGET together, global taps otherwise; raw views are always read from global memory.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "oess.h"
#include "oess_common.h"
#include "bilinear_axis.h"
#include "render_common.h"

namespace {
using namespace oess;
using namespace oess::render;
constexpr size_t LDS_BUDGET = 48 * 1024;     // the source rows of all resized views; with the 2 KB of staging below 64 KB
constexpr int MAX_VIEWS = OESS_RENDER_MAX_VIEWS;

struct View {
    const void* p;
    int64_t ips;                  // pixel stride in elements
    Axis ay, ax;
    int flip, raw;                // raw: (h, w) == (H, W), no blend
    int lds_off, pad;             // first float of this view's [2][w][K] rows in LDS
};
struct Views {
    View v[MAX_VIEWS];
    int V;
    float inv_v;                  // 1.0f / V
};

// what a lane keeps of a view along its pixel: the taps' columns and weights (raw: x0 is the column itself)
struct Cols { int x0, x1; float hx, wx; };
// what a workgroup keeps of a view along its row (uniform)
struct Rows { int64_t row0, row1; float hy, wy; };

template <bool BF16, bool LDS>
__device__ __forceinline__ float view_value(const View& vw, const float* rows, int K, const Rows& rw, const Cols& c, int k) {
    if (vw.raw) return tap<BF16>(vw.p, (rw.row0 + c.x0) * vw.ips + k);
    float p00, p01, p10, p11;
    if constexpr (LDS) {
        const float* r0 = rows + vw.lds_off;
        const float* r1 = r0 + vw.ax.in * K;
        p00 = r0[c.x0 * K + k]; p01 = r0[c.x1 * K + k];
        p10 = r1[c.x0 * K + k]; p11 = r1[c.x1 * K + k];
    } else {
        p00 = tap<BF16>(vw.p, (rw.row0 + c.x0) * vw.ips + k); p01 = tap<BF16>(vw.p, (rw.row0 + c.x1) * vw.ips + k);
        p10 = tap<BF16>(vw.p, (rw.row1 + c.x0) * vw.ips + k); p11 = tap<BF16>(vw.p, (rw.row1 + c.x1) * vw.ips + k);
    }
    return rw.hy * (c.hx * p00 + c.wx * p01) + rw.wy * (c.hx * p10 + c.wx * p11);          // resize_fwd_kernel's association
}

template <bool BF16, bool LDS>
__global__ __launch_bounds__(THREADS) void ensemble_render_kernel(Views vs, int K, int H, int W, Render r) {
    extern __shared__ __attribute__((aligned(16))) float rows[];            // LDS: per resized view [2][w_v][K]
    __shared__ Stage st;
    const int oy = blockIdx.x % H;
    const int64_t b = blockIdx.x / H;
    const int64_t opix = (b * H + oy) * (int64_t)W;                         // first output pixel of this row
    load_palette(st, r, K);
    Rows rw[MAX_VIEWS];
#pragma unroll
    for (int v = 0; v < MAX_VIEWS; ++v) {
        rw[v].row0 = rw[v].row1 = 0; rw[v].hy = 1.f; rw[v].wy = 0.f;
        if (v < vs.V) {
            const View& vw = vs.v[v];
            int y0 = oy, y1 = oy; float wy = 0.f;
            if (!vw.raw) src_index(vw.ay, oy, y0, y1, wy);
            rw[v].row0 = (b * vw.ay.in + y0) * vw.ax.in; rw[v].row1 = (b * vw.ay.in + y1) * vw.ax.in;
            rw[v].wy = wy; rw[v].hy = 1.f - wy;
            if constexpr (LDS) {
                if (!vw.raw) {
                    const int n = vw.ax.in * K;
                    float* r0 = rows + vw.lds_off;
                    for (int j = threadIdx.x; j < n; j += THREADS) {
                        const int x = j / K, k = j - x * K;
                        r0[j] = tap<BF16>(vw.p, (rw[v].row0 + x) * vw.ips + k);
                        r0[n + j] = tap<BF16>(vw.p, (rw[v].row1 + x) * vw.ips + k);
                    }
                }
            }
        }
    }
    __syncthreads();                                                        // pal and rows
    const int lphase = r.labels ? (int)((uintptr_t)(r.labels + opix) & 3) : 0;
    const int cphase = r.rgb ? (int)((uintptr_t)(r.rgb + 3 * opix) & 3) : 0;
    for (int base = 0; base < W; base += THREADS) {                         // uniform trip count: barriers inside
        const int ox = base + threadIdx.x;
        if (ox < W) {
            Cols c[MAX_VIEWS];
            float m[MAX_VIEWS], inv[MAX_VIEWS];
            // walk A: every view's maximum and 1 / sum
#pragma unroll
            for (int v = 0; v < MAX_VIEWS; ++v) {
                c[v].x0 = c[v].x1 = 0; c[v].hx = 1.f; c[v].wx = 0.f; m[v] = 0.f; inv[v] = 0.f;
                if (v < vs.V) {
                    const View& vw = vs.v[v];
                    const int oxv = vw.flip ? W - 1 - ox : ox;
                    if (vw.raw) {
                        c[v].x0 = c[v].x1 = oxv;
                    } else {
                        src_index(vw.ax, oxv, c[v].x0, c[v].x1, c[v].wx);
                        c[v].hx = 1.f - c[v].wx;
                    }
                    float best = view_value<BF16, LDS>(vw, rows, K, rw[v], c[v], 0), sum = 1.f;
                    int unused = 0;
                    for (int k = 1; k < K; ++k) take(view_value<BF16, LDS>(vw, rows, K, rw[v], c[v], k), k, best, unused, sum);
                    m[v] = best;
                    // best - best is 0 for a finite maximum and NaN otherwise (NaN, +inf: the sum alone would miss it; -inf)
                    inv[v] = (best - best == 0.f) ? 1.f / sum : __builtin_nanf("");
                }
            }
            // walk B: the mean probability class by class, running first-argmax
            float pbest = 0.f;
            int idx = 0;
            for (int k = 0; k < K; ++k) {
                float p = 0.f;
#pragma unroll
                for (int v = 0; v < MAX_VIEWS; ++v) {
                    if (v < vs.V) {
                        const float q = __expf(view_value<BF16, LDS>(vs.v[v], rows, K, rw[v], c[v], k) - m[v]) * inv[v];
                        p = v == 0 ? q : p + q;
                    }
                }
                p = p * vs.inv_v;
                if (k == 0 || p > pbest || (p != p && pbest == pbest)) { pbest = p; idx = k; }
            }
            emit_conf(st, r, K, opix + ox, lphase, cphase, idx, pbest);
        }
        flush_chunk(st, r, opix + base, lphase, cphase, W - base < THREADS ? W - base : THREADS);
    }
}

}  // namespace

extern "C" {

int oess_segment_render_ensemble(const void* const* logits, const long long* pix_strides, const int* hs, const int* ws,
                                 const int* flips, int V, int is_bf16, int B, int K, int H, int W, int align_corners,
                                 const uint8_t* palette, const uint8_t* grey, int alpha256, float min_conf, int ignore_label,
                                 uint8_t* labels, float* conf, uint8_t* rgb, oess_stream_t stream) {
    if (!logits || !pix_strides || !hs || !ws || !flips || V < 1 || V > MAX_VIEWS ||
        bad_render_args(palette, labels, conf, rgb, K, alpha256, min_conf, ignore_label) || B <= 0 || H <= 0 || W <= 0)
        return OESS_EINVAL;
    int64_t out_elems;
    if ((int64_t)B * H > INT32_MAX || __builtin_mul_overflow((int64_t)B * H, (int64_t)W, &out_elems) || out_elems > INT64_MAX / 4)
        return OESS_EINVAL;
    Views vs;
    vs.V = V; vs.inv_v = 1.0f / (float)V;
    size_t lds_floats = 0;
    for (int v = 0; v < MAX_VIEWS; ++v) {
        View& vw = vs.v[v];
        vw.p = nullptr; vw.ips = 0; vw.ay = vw.ax = make_axis(1, 1, 0); vw.flip = 0; vw.raw = 1; vw.lds_off = 0; vw.pad = 0;
        if (v >= V) continue;
        const int h = hs[v], w = ws[v];
        const long long ps = pix_strides[v];
        int64_t in_elems;
        if (!logits[v] || (flips[v] != 0 && flips[v] != 1) || h <= 0 || w <= 0 || ps < K || (int64_t)B * h > INT32_MAX ||
            (int64_t)w * K > INT32_MAX || __builtin_mul_overflow((int64_t)B * h * w, (int64_t)ps, &in_elems) ||
            in_elems > INT64_MAX / 4)
            return OESS_EINVAL;
        vw.p = logits[v]; vw.ips = (int64_t)ps; vw.flip = flips[v]; vw.raw = (h == H && w == W);
        vw.ay = make_axis(h, H, align_corners); vw.ax = make_axis(w, W, align_corners);
        if (!vw.raw) {
            // read only while the total stays within the budget; capped so that it fits an int whatever the sizes are
            vw.lds_off = (int)(lds_floats < LDS_BUDGET / sizeof(float) ? lds_floats : LDS_BUDGET / sizeof(float));
            lds_floats += (size_t)2 * w * K;
        }
    }
    Render r;
    r.palette = palette; r.grey = grey; r.labels = labels; r.conf = conf; r.rgb = rgb;
    r.alpha256 = alpha256; r.ignore_label = ignore_label; r.min_conf = min_conf;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((int64_t)B * H)), block(THREADS);
    const size_t lds = lds_floats * sizeof(float);
#define OESS_ER(BF, LDS, SH) hipLaunchKernelGGL((ensemble_render_kernel<BF, LDS>), grid, block, SH, st, vs, K, H, W, r)
    if (lds <= LDS_BUDGET) { if (is_bf16) OESS_ER(true, true, lds); else OESS_ER(false, true, lds); }
    else { if (is_bf16) OESS_ER(true, false, 0); else OESS_ER(false, false, 0); }
#undef OESS_ER
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
