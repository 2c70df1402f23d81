// ConvGRU (e2vid/model/submodules.py:217-253 of the reference) for gfx950 (K28 of DESIGN.md).
//   bf16: two launches per step, each the LDS-DMA MFMA convolution of conv_dma.h with a fused epilogue (convgru_epilogue.h):
//         oess_convgru_gates_bf16 (u, r * h) and oess_convgru_out_bf16 (tanh + blend, fp32 master of h + bf16 copy).
//   fp32: the two pointwise kernels behind oess_conv2d_fwd_f32's pre-activations: oess_convgru_gates_f32, oess_convgru_blend_f32.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"

namespace {
#include <type_traits>
#include <utility>
using namespace oess;

#include "conv_args.h"
#include "convgru_epilogue.h"
#include "conv_frag.h"
#include "conv_dma.h"

constexpr size_t GRU_LDS = (size_t)2 * (BM + 128) * 8 * 16;          // the 2-stage operand ring; both epilogues' images fit it
static_assert((size_t)128 * 65 * 4 + (size_t)128 * 66 * 2 <= GRU_LDS, "gates epilogue images");
static_assert((size_t)64 * 129 * 4 + (size_t)64 * 130 * 2 <= GRU_LDS, "output epilogue images");

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// A strided window: `pixels` runs of `width` bytes, `stride` bytes apart.
struct Window { const char* p; long long width, stride, pixels; };
Window win_bf16(const void* p, int C, long long pix_stride, long long pixels) { return Window{(const char*)p, 2ll * C, 2 * pix_stride, pixels}; }
Window win_f32(const void* p, int C, long long pixels) { return Window{(const char*)p, 4ll * C * pixels, 4ll * C * pixels, 1}; }
// True when two windows share a byte.  Channel windows of ONE buffer (same stride, same pixel count) interleave without
// touching; anything else is compared by its byte range.
bool overlap(const Window& x, const Window& y) {
    if (!x.p || !y.p) return false;
    const char *x1 = x.p + (x.pixels - 1) * x.stride + x.width, *y1 = y.p + (y.pixels - 1) * y.stride + y.width;
    if (!(x.p < y1 && y.p < x1)) return false;
    if (x.stride == y.stride && x.pixels == y.pixels && x.width <= x.stride && y.width <= y.stride) {
        const long long d = ((y.p - x.p) % x.stride + x.stride) % x.stride;        // y's offset inside x's pixel period
        if (d >= x.width && d + y.width <= x.stride) return false;
    }
    return true;
}

// Geometry both bf16 entries take (include/oess.h) -> the ConvArgs of conv_fwd_dma_kernel, pointers left null.
int gru_plan(int B, int H, int W, int Cin, long long in_pix_stride, int C, int rows, int R, int S, int pad, long long out_pix_stride,
             ConvArgs* ap) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 31) || R != 3 || S != 3 || pad != 1) return OESS_EINVAL;
    if (Cin != C && Cin != 2 * C) return OESS_EINVAL;                 // x alone (zero state) or cat(.., ..): input_size == hidden_size
    if ((in_pix_stride & 7) || in_pix_stride < Cin || (out_pix_stride & 7) || out_pix_stride < C) return OESS_EINVAL;
    const long long M = (long long)B * H * W;
    if (M > 0x7fffffffll) return OESS_EINVAL;
    // 32-bit buffer offsets of the LDS-DMA gather; the outputs are addressed with 64-bit arithmetic
    if (((M - 1) * in_pix_stride + Cin) * 2 >= 0x7ffffff0ll) return OESS_EINVAL;
    ConvArgs& a = *ap;
    a = ConvArgs{};
    a.in_pix_stride = in_pix_stride;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = rows;
    a.R = 3; a.S = 3; a.stride = 1; a.pad = 1; a.dil = 1;
    a.Ho = H; a.Wo = W;
    a.Kpad = (9 * Cin + BK - 1) / BK * BK;
    a.M = (int)M;
    a.lstm_C = C; a.lstm_h_stride = out_pix_stride;
    a.tiles_m = (a.M + BM - 1) / BM; a.tiles_n = (rows + 127) / 128;
    a.ksplit = 1;
    if ((long long)a.tiles_m * a.tiles_n > 0x7fffffffll || (long long)a.tiles_n * 128 * a.Kpad * 2 >= 0x7ffffff0ll) return OESS_EINVAL;
    // exact small-range reciprocals of the tap decode (conv_dma.h), verified over the whole range
    const unsigned cpt = (unsigned)(Cin >> 3), nkc = (unsigned)(a.Kpad / 8);
    a.inv_cpt = ((1u << 20) + cpt - 1) / cpt;
    a.inv_s = ((1u << 16) + 3u - 1) / 3u;
    if (nkc >= 4096) return OESS_EINVAL;
    for (unsigned kc = 0; kc < nkc; ++kc) if (((kc * a.inv_cpt) >> 20) != kc / cpt) return OESS_EINVAL;
    for (unsigned t = 0; t <= nkc / cpt + 1; ++t) if (((t * a.inv_s) >> 16) != t / 3u) return OESS_EINVAL;
    return OESS_OK;
}

template <int EPI>
int gru_launch(const ConvArgs& a, oess_stream_t stream) {
    const dim3 grid(a.tiles_m * a.tiles_n), block(CONV_THREADS);
    if (a.Cin % 64 == 0) hipLaunchKernelGGL((conv_fwd_dma_kernel<128, 128, 2, true, EPI>), grid, block, GRU_LDS, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((conv_fwd_dma_kernel<128, 128, 2, false, EPI>), grid, block, GRU_LDS, (hipStream_t)stream, a);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

// ---- fp32 pointwise kernels (sigmoid / tanh as the fp32 ConvLSTM cell kernel has them: library expf / tanhf, IEEE division)
constexpr int PW_THREADS = 256;
struct V32 { float* p; long long sb, sy, sx, sc; };
V32 to_v32(const oess_f32_view_t* v) { return v ? V32{(float*)v->data, v->sb, v->sy, v->sx, v->sc} : V32{nullptr, 0, 0, 0, 0}; }
__device__ __forceinline__ long long v32_off(const V32& v, long long p, int c, int H, int W) {
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const long long b = p / ((long long)W * H);
    return b * v.sb + y * v.sy + x * v.sx + c * v.sc;
}

__global__ __launch_bounds__(PW_THREADS) void gru_gates_f32_kernel(const float* __restrict__ pre, V32 h, int C, long long npix, int H, int W,
                                                                   float* __restrict__ u, V32 rh) {
    const long long e = (long long)blockIdx.x * PW_THREADS + threadIdx.x;
    if (e >= npix * C) return;
    const long long p = e / C;
    const int c = (int)(e - p * C);
    const float* g = pre + p * 2 * C;
    const float ug = 1.0f / (1.0f + expf(-g[c]));
    const float rg = 1.0f / (1.0f + expf(-g[C + c]));
    const float hv = h.p ? h.p[v32_off(h, p, c, H, W)] : 0.0f;
    u[e] = ug;
    rh.p[v32_off(rh, p, c, H, W)] = rg * hv;
}

__global__ __launch_bounds__(PW_THREADS) void gru_blend_f32_kernel(const float* __restrict__ pre, const float* __restrict__ u, V32 h,
                                                                   int C, long long npix, int H, int W, V32 out) {
    const long long e = (long long)blockIdx.x * PW_THREADS + threadIdx.x;
    if (e >= npix * C) return;
    const long long p = e / C;
    const int c = (int)(e - p * C);
    const float hv = h.p ? h.p[v32_off(h, p, c, H, W)] : 0.0f;
    const float ug = u[e];
    out.p[v32_off(out, p, c, H, W)] = hv * (1.0f - ug) + tanhf(pre[e]) * ug;
}

// The window of a view: an NHWC channel window with uniformly strided pixels keeps its interleaving (the h, x and r * h windows
// of one state buffer do not touch), any other view is its byte range.  Negative strides are refused.
bool win_view(const oess_f32_view_t* v, int B, int H, int W, int C, Window* w) {
    if (v->sb < 0 || v->sy < 0 || v->sx < 0 || v->sc < 0) return false;
    const long long px = (long long)B * H * W;
    if (v->sc == 1 && v->sx >= C && (H == 1 || v->sy == W * v->sx) && (B == 1 || v->sb == H * W * v->sx)) { *w = Window{(const char*)v->data, 4ll * C, 4 * v->sx, px}; return true; }
    const long long bytes = 4 * ((B - 1) * v->sb + (H - 1) * v->sy + (W - 1) * v->sx + (C - 1) * v->sc + 1);
    *w = Window{(const char*)v->data, bytes, bytes, 1};
    return true;
}
bool same_view(const oess_f32_view_t* x, const oess_f32_view_t* y) {
    return x->data == y->data && x->sb == y->sb && x->sy == y->sy && x->sx == y->sx && x->sc == y->sc;
}
// one thread per element on a one-dimensional grid of PW_THREADS-wide workgroups: at most 2^31 - 1 workgroups
constexpr long long PW_MAX_ELEMS = 0x7fffffffLL * PW_THREADS;
bool f32_geom_ok(int B, int H, int W, int C) {
    return B >= 1 && H >= 1 && W >= 1 && C >= 1 && (long long)B * H * W <= PW_MAX_ELEMS / C;
}

}  // namespace

extern "C" {

int oess_convgru_gates_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int Cin, const void* w_packed_gates,
                            const float* bias, int C_hidden, int R, int S, int pad, const float* h_prev, float* u, void* rh,
                            long long rh_pix_stride, float* rh_f32, oess_stream_t stream) {
    if (!in || !w_packed_gates || !u || !rh) return OESS_EINVAL;
    ConvArgs a;
    const int rc = gru_plan(B, H, W, Cin, in_pix_stride, C_hidden, 2 * C_hidden, R, S, pad, rh_pix_stride, &a);
    if (rc != OESS_OK) return rc;
    if (Cin == C_hidden && h_prev) return OESS_EINVAL;               // x alone is the step from a zero state
    if (!aligned16(in) || !aligned16(w_packed_gates) || !aligned16(u) || !aligned16(rh) || !aligned16(h_prev) || !aligned16(rh_f32) ||
        (bias && ((uintptr_t)bias & 3)))
        return OESS_EINVAL;
    const long long px = a.M;
    const Window wi = win_bf16(in, Cin, in_pix_stride, px), wr = win_bf16(rh, C_hidden, rh_pix_stride, px);
    const Window wu = win_f32(u, C_hidden, px), wh = win_f32(h_prev, C_hidden, px), wd = win_f32(rh_f32, C_hidden, px);
    // no output may touch the convolved window (neighbouring tiles still read it), h_prev or another output
    if (overlap(wr, wi) || overlap(wu, wi) || overlap(wd, wi) || overlap(wr, wh) || overlap(wu, wh) || overlap(wd, wh) ||
        overlap(wr, wu) || overlap(wr, wd) || overlap(wu, wd))
        return OESS_EINVAL;
    a.in = (const uint16_t*)in; a.w = (const uint16_t*)w_packed_gates; a.bias = bias;
    a.lstm_prev = h_prev; a.lstm_cell = u; a.lstm_h = (uint16_t*)rh; a.gru_rh32 = rh_f32;
    return gru_launch<2>(a, stream);
}

int oess_convgru_out_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int Cin, const void* w_packed,
                          const float* bias, int C_hidden, int R, int S, int pad, const float* u, const float* h_prev, float* h,
                          void* h_bf16, long long h_bf16_pix_stride, oess_stream_t stream) {
    if (!in || !w_packed || !u || !h || !h_bf16) return OESS_EINVAL;
    ConvArgs a;
    const int rc = gru_plan(B, H, W, Cin, in_pix_stride, C_hidden, C_hidden, R, S, pad, h_bf16_pix_stride, &a);
    if (rc != OESS_OK) return rc;
    if (Cin == C_hidden && h_prev) return OESS_EINVAL;
    if (!aligned16(in) || !aligned16(w_packed) || !aligned16(u) || !aligned16(h) || !aligned16(h_prev) || !aligned16(h_bf16) ||
        (bias && ((uintptr_t)bias & 3)))
        return OESS_EINVAL;
    const long long px = a.M;
    const Window wi = win_bf16(in, Cin, in_pix_stride, px), wb = win_bf16(h_bf16, C_hidden, h_bf16_pix_stride, px);
    const Window wu = win_f32(u, C_hidden, px), wp = win_f32(h_prev, C_hidden, px), wh = win_f32(h, C_hidden, px);
    // h may BE h_prev (a value is read and written by the lane that owns it); otherwise outputs touch no input and not each other
    if (overlap(wb, wi) || overlap(wh, wi) || overlap(wb, wu) || overlap(wh, wu) || overlap(wb, wh) || overlap(wb, wp) ||
        (h != h_prev && overlap(wh, wp)))
        return OESS_EINVAL;
    a.in = (const uint16_t*)in; a.w = (const uint16_t*)w_packed; a.bias = bias;
    a.gru_u = u; a.lstm_prev = h_prev; a.lstm_cell = h; a.lstm_h = (uint16_t*)h_bf16;
    return gru_launch<3>(a, stream);
}

size_t oess_convgru_f32_workspace_bytes(long long pixels, int C_hidden) {
    if (pixels < 1 || C_hidden < 1 || pixels > PW_MAX_ELEMS / C_hidden) return 0;
    return (size_t)pixels * 4 * C_hidden * sizeof(float);
}

int oess_convgru_gates_f32(const float* pre, const oess_f32_view_t* h_prev, int B, int H, int W, int C_hidden, float* u,
                           const oess_f32_view_t* rh, oess_stream_t stream) {
    if (!pre || !u || !rh || !rh->data || (h_prev && !h_prev->data) || !f32_geom_ok(B, H, W, C_hidden)) return OESS_EINVAL;
    if ((((uintptr_t)pre | (uintptr_t)u | (uintptr_t)rh->data | (uintptr_t)(h_prev ? h_prev->data : nullptr)) & 3) != 0) return OESS_EINVAL;
    const long long npix = (long long)B * H * W, n = npix * C_hidden;
    const Window wp = win_f32(pre, 2 * C_hidden, npix), wu = win_f32(u, C_hidden, npix);
    Window wr, wh{nullptr, 0, 0, 0};
    if (!win_view(rh, B, H, W, C_hidden, &wr) || (h_prev && !win_view(h_prev, B, H, W, C_hidden, &wh))) return OESS_EINVAL;
    // u and rh are written while pre and h_prev are read by other threads: no output meets an input or the other output
    // (rh may BE h_prev: element-wise in place)
    if (overlap(wu, wp) || overlap(wr, wp) || overlap(wu, wr) || overlap(wu, wh) || (overlap(wr, wh) && !same_view(rh, h_prev)))
        return OESS_EINVAL;
    hipLaunchKernelGGL(gru_gates_f32_kernel, dim3((unsigned)((n + PW_THREADS - 1) / PW_THREADS)), dim3(PW_THREADS), 0, (hipStream_t)stream,
                       pre, to_v32(h_prev), C_hidden, npix, H, W, u, to_v32(rh));
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_convgru_blend_f32(const float* pre, const float* u, const oess_f32_view_t* h_prev, int B, int H, int W, int C_hidden,
                           const oess_f32_view_t* h, oess_stream_t stream) {
    if (!pre || !u || !h || !h->data || (h_prev && !h_prev->data) || !f32_geom_ok(B, H, W, C_hidden)) return OESS_EINVAL;
    if ((((uintptr_t)pre | (uintptr_t)u | (uintptr_t)h->data | (uintptr_t)(h_prev ? h_prev->data : nullptr)) & 3) != 0) return OESS_EINVAL;
    const long long npix = (long long)B * H * W, n = npix * C_hidden;
    const Window wp = win_f32(pre, C_hidden, npix), wu = win_f32(u, C_hidden, npix);
    Window wo, wh{nullptr, 0, 0, 0};
    if (!win_view(h, B, H, W, C_hidden, &wo) || (h_prev && !win_view(h_prev, B, H, W, C_hidden, &wh))) return OESS_EINVAL;
    // h may BE h_prev (element-wise in place); otherwise it meets no input
    if (overlap(wo, wp) || overlap(wo, wu) || (overlap(wo, wh) && !same_view(h, h_prev))) return OESS_EINVAL;
    hipLaunchKernelGGL(gru_blend_f32_kernel, dim3((unsigned)((n + PW_THREADS - 1) / PW_THREADS)), dim3(PW_THREADS), 0, (hipStream_t)stream,
                       pre, u, to_v32(h_prev), C_hidden, npix, H, W, to_v32(h));
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
