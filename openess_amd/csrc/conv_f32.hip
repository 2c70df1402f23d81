// K14 fp32 E2VID inference: implicit-GEMM convolutions on the f32-input MFMA of gfx950 (v_mfma_f32_32x32x2_f32).
//
// One kernel template covers every layer of UNetRecurrent (e2vid/model/unet.py of the reference) in fp32:
//   M = output pixels of one phase, N = Cout, K = taps x Cin, K ordered (tap, ci).
// A tap table (dy, dx per tap, per phase) describes the geometry:
//   ordinary conv:      one phase, input row = q * stride - pad + r, output row = q;
//   transposed conv:    ConvTranspose2d(k 5, stride 2, pad 2, output_padding 1) as four stride-1 phase sub-convolutions
//                       (output parity py, px; 3 / 2 taps per axis), input row = q + 1 - t, output row = 2 q + py;
//   upsample conv:      the operand loader reads the bilinear x2 (align_corners=False) map of its input on the fly.
//   dilated conv (K16): tap (r, s) at (r d, s d); 7 x 7 taps for the ResNet stem; a workgroup skips the taps it cannot reach.
//   stride-2 dgrad (K21): the data gradient of a stride-2 conv as four stride-1 phase sub-convolutions of dY (input parity py,
//                       px; the taps of matching parity), output row = 2 q + py; a phase without taps writes zeros.
// A second input may be summed on load (skip_sum); the epilogue adds bias, an optional residual, then ReLU or sigmoid.
//
// Tiling: 256 threads = 4 waves; a wave owns 64 pixels x 32 output channels (two 32 x 32 accumulators, 16 registers each);
// block tile BM x BN with BN = 32 (BM = 256) or 64 (BM = 128); K steps of 16 staged through LDS, the next step's global
// loads held in registers while the current one runs on the matrix cores.  Every output element is a k-ordered fmaf chain
// (the MFMA's own numerics), written once: no atomics, results repeat bit for bit.
#include <hip/hip_runtime.h>

#include "oess.h"
#include "oess_common.h"

namespace {

#include "f32_view.h"

constexpr int NT = 256;
constexpr int BK = 16;
constexpr int MAXTAP = 49;             // tap table: up to the 7 x 7 stem of ResNet (oess_conv2d_dilated_fwd_f32)
constexpr int MAXTAP_V1 = 25;          // what oess_conv2d_fwd_f32 / oess_convlstm_step_f32 take
constexpr int ACT_GELU = 3;            // internal epilogue code, reached through oess_linear_tokens_f32 only
constexpr int ACT_QUICK_GELU = 4;      // internal epilogue code, reached through oess_linear_tokens_quick_gelu_f32 only (K29)

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Phase {
    int ntap, py, px, kp;            // kp: K rows of this phase's packed block (multiple of BK)
    long long w_off;                 // first float of the block
    signed char dy[MAXTAP], dx[MAXTAP];
};

struct Params {
    View in, in2;
    int has_in2;
    int B, H, W, Cin, up;            // source map; up: the conv sees its bilinear x2 ((2H) x (2W))
    int Hl, Wl;                      // logical input extent seen by the taps
    int Hq, Wq;                      // GEMM grid of one phase: M = B * Hq * Wq
    int stride, off_y, off_x, ostride;
    int oh, ow;                      // output extent: a phase pixel beyond it is not written (odd maps under ostride 2)
    int skip;                        // dilated convs: a workgroup walks only the taps that reach the map from one of its pixels
    const float* w;
    int CoutP;
    const float* bias;
    int Cout, act;                   // act: 0 none, 1 ReLU, 2 sigmoid; ACT_GELU, ACT_QUICK_GELU: instances of their own (launch)
    View res;
    int has_res;
    float* out;
    long long ob, oy, ox, oc;
    Phase ph[4];
};
static_assert(sizeof(Params) <= 1024, "Params travels as a kernel argument");
static_assert(MAXTAP <= 64, "the tap mask of a workgroup is one 64-bit word");

// area_pixel_compute_source_index(scale 0.5, align_corners=False) + the clamp of upsample_bilinear2d
__device__ __forceinline__ void bil_axis(int d, int n, int& i0, int& i1, float& l0, float& l1) {
    float s = 0.5f * ((float)d + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l1 = s - (float)i0;
    l0 = 1.f - l1;
}

__device__ __forceinline__ float ld1(const Params& P, int b, int y, int x, int c) {
    float v = P.in.p[b * P.in.sb + y * P.in.sy + x * P.in.sx + c * P.in.sc];
    if (P.has_in2) v = v + P.in2.p[b * P.in2.sb + y * P.in2.sy + x * P.in2.sx + c * P.in2.sc];
    return v;
}

__device__ __forceinline__ float4 ld4(const Params& P, int b, int y, int x, int c) {
    float4 v = *(const float4*)(P.in.p + (b * P.in.sb + y * P.in.sy + x * P.in.sx + c));
    if (P.has_in2) {
        const float4 u = *(const float4*)(P.in2.p + (b * P.in2.sb + y * P.in2.sy + x * P.in2.sx + c));
        v.x = v.x + u.x; v.y = v.y + u.y; v.z = v.z + u.z; v.w = v.w + u.w;
    }
    return v;
}

__device__ __forceinline__ float blend(float a, float b, float c, float d, float ly0, float ly1, float lx0, float lx1) {
    return ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d);
}

// element (b, y, x, c) of the map the taps read; (y, x) already inside [0, Hl) x [0, Wl)
__device__ __forceinline__ float fetch1(const Params& P, int b, int y, int x, int c) {
    if (!P.up) return ld1(P, b, y, x, c);
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    bil_axis(y, P.H, y0, y1, ly0, ly1);
    bil_axis(x, P.W, x0, x1, lx0, lx1);
    return blend(ld1(P, b, y0, x0, c), ld1(P, b, y0, x1, c), ld1(P, b, y1, x0, c), ld1(P, b, y1, x1, c), ly0, ly1, lx0, lx1);
}

__device__ __forceinline__ float4 fetch4(const Params& P, int b, int y, int x, int c) {
    if (!P.up) return ld4(P, b, y, x, c);
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    bil_axis(y, P.H, y0, y1, ly0, ly1);
    bil_axis(x, P.W, x0, x1, lx0, lx1);
    const float4 a = ld4(P, b, y0, x0, c), bb = ld4(P, b, y0, x1, c), cc = ld4(P, b, y1, x0, c), d = ld4(P, b, y1, x1, c);
    return make_float4(blend(a.x, bb.x, cc.x, d.x, ly0, ly1, lx0, lx1), blend(a.y, bb.y, cc.y, d.y, ly0, ly1, lx0, lx1),
                       blend(a.z, bb.z, cc.z, d.z, ly0, ly1, lx0, lx1), blend(a.w, bb.w, cc.w, d.w, ly0, ly1, lx0, lx1));
}

// VEC: Cin % 16 == 0 and dense, 16-byte aligned channels in both inputs -> a K step lies inside one tap, float4 loads
// GELU (K25): the token GEMM's exact-GELU epilogue (oess_linear_tokens_f32, act 1) is an instance of its own, so the instances
// the convolutions run are unchanged by it.  EPI: 0 the runtime act, 1 that GELU, 2 QuickGELU v sigmoid(1.702 v) with the accurate
// expf (K29: the FFN of CLIP's text tower, oess_linear_tokens_quick_gelu_f32)
template <int BN, bool VEC, int EPI = 0>
__global__ __launch_bounds__(NT) void conv_f32_kernel(const Params P) {
    constexpr int WN = BN / 32, WM = 4 / WN, BM = WM * 64;
    constexpr int LDA = BM + 32, LDB = BN + 32;          // +32 floats: the two k rows of one MFMA operand read hit disjoint banks
    constexpr int NA = VEC ? BM * BK / 4 / NT : BM * BK / NT;
    constexpr int AROW = NT / BM;                         // k rows (VEC: k quads) a thread advances per staged element
    constexpr int NB4 = BN * BK / 4;                      // float4s of one B step
    __shared__ float As[BK * LDA];
    __shared__ float Bs[BK * LDB];
    __shared__ unsigned long long s_mask;
    __shared__ unsigned char s_tap[MAXTAP];
    __shared__ int s_ntap;

    const Phase& ph = P.ph[blockIdx.z];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const long long M = (long long)P.B * P.Hq * P.Wq;
    const long long m0 = (long long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int K = ph.ntap * P.Cin;
    const float* wp = P.w + ph.w_off;

    // the pixel this thread stages for the A operand
    const int am = tid % BM, arow = tid / BM;
    const long long mg = m0 + am;
    const bool mvalid = mg < M;
    int ab = 0, ay0 = 0, ax0 = 0;
    if (mvalid) {
        long long r = mg;
        const int qx = (int)(r % P.Wq);
        r /= P.Wq;
        const int qy = (int)(r % P.Hq);
        ab = (int)(r / P.Hq);
        ay0 = qy * P.stride + P.off_y;
        ax0 = qx * P.stride + P.off_x;
    }

    // K steps of this workgroup.  skip (VEC only): at dilation d most taps of a tile near the border, and on a map smaller than
    // d all but the centre tap, read nothing but padding; their products are exact zeros, so the K steps of a tap that no pixel
    // of the tile reaches are left out whole (no operand loads, no MFMAs).  The taps kept stay in (r, s) order.
    const int spt = VEC ? P.Cin / BK : 1;                 // K steps per tap
    const bool skip = VEC && P.skip;
    int nstep = ph.kp / BK;
    if (skip) {
        if (tid == 0) s_mask = 0ull;
        __syncthreads();
        unsigned long long mine = 0ull;
        if (mvalid) {
            for (int t = 0; t < ph.ntap; ++t) {
                const int y = ay0 + ph.dy[t], x = ax0 + ph.dx[t];
                if (y >= 0 && y < P.Hl && x >= 0 && x < P.Wl) mine |= 1ull << t;
            }
        }
        if (mine) atomicOr(&s_mask, mine);                // integer OR in LDS: order-free
        __syncthreads();
        if (tid == 0) {
            int n = 0;
            for (int t = 0; t < ph.ntap; ++t)
                if ((s_mask >> t) & 1ull) s_tap[n++] = (unsigned char)t;
            s_ntap = n;
        }
        __syncthreads();
        nstep = s_ntap * spt;
    }

    float ra[VEC ? NA * 4 : NA];
    float4 rb = make_float4(0.f, 0.f, 0.f, 0.f);
    const int bidx = tid, brow = bidx / (BN / 4), bcol = (bidx % (BN / 4)) * 4;

    auto load = [&](int step) {
        int k0 = step * BK;                               // first weight row of the step
        if (VEC) {
            const int ti = step / spt;
            const int tap = skip ? __builtin_amdgcn_readfirstlane((int)s_tap[ti]) : ti;
            const int cbase = (step - ti * spt) * BK;
            k0 = tap * P.Cin + cbase;
            const int y = ay0 + ph.dy[tap], x = ax0 + ph.dx[tap];
            const bool ok = mvalid && y >= 0 && y < P.Hl && x >= 0 && x < P.Wl;
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const int kq = arow + j * AROW;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) v = fetch4(P, ab, y, x, cbase + kq * 4);
                ra[4 * j] = v.x; ra[4 * j + 1] = v.y; ra[4 * j + 2] = v.z; ra[4 * j + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const int k = k0 + arow + j * AROW;
                float v = 0.f;
                if (mvalid && k < K) {
                    const int tap = k / P.Cin, c = k - tap * P.Cin;
                    const int y = ay0 + ph.dy[tap], x = ax0 + ph.dx[tap];
                    if (y >= 0 && y < P.Hl && x >= 0 && x < P.Wl) v = fetch1(P, ab, y, x, c);
                }
                ra[j] = v;
            }
        }
        if (bidx < NB4) rb = *(const float4*)(wp + (long long)(k0 + brow) * P.CoutP + n0 + bcol);
    };
    auto store = [&]() {
        if (VEC) {
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const int kq = arow + j * AROW;
#pragma unroll
                for (int i = 0; i < 4; ++i) As[(kq * 4 + i) * LDA + am] = ra[4 * j + i];
            }
        } else {
#pragma unroll
            for (int j = 0; j < NA; ++j) As[(arow + j * AROW) * LDA + am] = ra[j];
        }
        if (bidx < NB4) *(float4*)(Bs + brow * LDB + bcol) = rb;
    };

    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }

    const int l31 = lane & 31, lk = lane >> 5;
    if (nstep > 0) {
        load(0);
        store();
    }
    __syncthreads();
    for (int step = 0; step < nstep; ++step) {
        const bool more = step + 1 < nstep;
        if (more) load(step + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const int kr = 2 * kk + lk;
            const float b = Bs[kr * LDB + wn * 32 + l31];
            const float a0 = As[kr * LDA + wm * 64 + l31];
            const float a1 = As[kr * LDA + wm * 64 + 32 + l31];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            store();
            __syncthreads();
        }
    }

    // epilogue: D[i][j], j = lane & 31 (output channel), i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (pixel)
    const int n = n0 + wn * 32 + l31;
    if (n >= P.Cout) return;
    const float bias = P.bias ? P.bias[n] : 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long m = m0 + wm * 64 + s * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (m >= M) continue;
            long long t = m;
            const int qx = (int)(t % P.Wq);
            t /= P.Wq;
            const int qy = (int)(t % P.Hq);
            const int b = (int)(t / P.Hq);
            const int oy = qy * P.ostride + ph.py, ox = qx * P.ostride + ph.px;
            if (oy >= P.oh || ox >= P.ow) continue;
            float v = (s ? acc1[r] : acc0[r]) + bias;
            if (P.has_res) v = v + P.res.p[b * P.res.sb + oy * P.res.sy + ox * P.res.sx + n * P.res.sc];
            if (EPI == 1) v = 0.5f * v * (1.0f + erff(v * 0.70710678f));
            else if (EPI == 2) v = v / (1.0f + expf(-1.702f * v));
            else if (P.act == 1) v = v > 0.f ? v : 0.f;
            else if (P.act == 2) v = 1.0f / (1.0f + expf(-v));
            P.out[b * P.ob + oy * P.oy + ox * P.ox + n * P.oc] = v;
        }
    }
}

// ConvLSTM cell update (e2vid/model/submodules.py:200-212 of the reference) on the gates [P][4C] = (in, remember, out, cell)
__global__ __launch_bounds__(NT) void lstm_cell_f32_kernel(const float* __restrict__ gates, int C, long long npix, int H, int W,
                                                           float* __restrict__ cell, int prev_zero, float* hid, long long hb,
                                                           long long hy, long long hx, long long hc) {
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e >= npix * C) return;
    const long long p = e / C;
    const int c = (int)(e - p * C);
    const float* g = gates + p * 4 * C;
    const float ig = 1.0f / (1.0f + expf(-g[c]));
    const float fg = 1.0f / (1.0f + expf(-g[C + c]));
    const float og = 1.0f / (1.0f + expf(-g[2 * C + c]));
    const float cg = tanhf(g[3 * C + c]);
    const float cn = prev_zero ? ig * cg : fg * cell[e] + ig * cg;
    cell[e] = cn;
    const int x = (int)(p % W), y = (int)((p / W) % H), b = (int)(p / ((long long)W * H));
    hid[b * hb + y * hy + x * hx + c * hc] = og * tanhf(cn);
}

int ceil_to(int v, int a) { return (v + a - 1) / a * a; }

// common checks of the input side (in, in2, geometry)
bool inputs_ok(const oess_f32_view_t* in, const oess_f32_view_t* in2, int B, int H, int W, int Cin) {
    if (!view_ok(in) || (in2 && !in2->data)) return false;
    if (B < 1 || H < 1 || W < 1 || Cin < 1) return false;
    return (long long)B * H * W * Cin < (1LL << 40);
}

int launch(Params& P, int nphase, hipStream_t stream) {
    const long long M = (long long)P.B * P.Hq * P.Wq;
    if (M < 1 || M >= (1LL << 31) || P.Cin > (1 << 20)) return OESS_EINVAL;
    bool vec = P.Cin % BK == 0 && P.in.sc == 1 && ((uintptr_t)P.in.p & 15) == 0 && P.in.sb % 4 == 0 && P.in.sy % 4 == 0 &&
               P.in.sx % 4 == 0;
    if (P.has_in2)
        vec = vec && P.in2.sc == 1 && ((uintptr_t)P.in2.p & 15) == 0 && P.in2.sb % 4 == 0 && P.in2.sy % 4 == 0 && P.in2.sx % 4 == 0;
    const bool bn64 = P.CoutP % 64 == 0;
    const int BM = bn64 ? 128 : 256;
    dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)(P.CoutP / (bn64 ? 64 : 32)), (unsigned)nphase);
    if (P.act == ACT_GELU) {
        if (bn64) {
            if (vec) hipLaunchKernelGGL((conv_f32_kernel<64, true, 1>), grid, dim3(NT), 0, stream, P);
            else hipLaunchKernelGGL((conv_f32_kernel<64, false, 1>), grid, dim3(NT), 0, stream, P);
        } else {
            if (vec) hipLaunchKernelGGL((conv_f32_kernel<32, true, 1>), grid, dim3(NT), 0, stream, P);
            else hipLaunchKernelGGL((conv_f32_kernel<32, false, 1>), grid, dim3(NT), 0, stream, P);
        }
    } else if (P.act == ACT_QUICK_GELU) {
        if (bn64) {
            if (vec) hipLaunchKernelGGL((conv_f32_kernel<64, true, 2>), grid, dim3(NT), 0, stream, P);
            else hipLaunchKernelGGL((conv_f32_kernel<64, false, 2>), grid, dim3(NT), 0, stream, P);
        } else {
            if (vec) hipLaunchKernelGGL((conv_f32_kernel<32, true, 2>), grid, dim3(NT), 0, stream, P);
            else hipLaunchKernelGGL((conv_f32_kernel<32, false, 2>), grid, dim3(NT), 0, stream, P);
        }
    } else if (bn64) {
        if (vec) hipLaunchKernelGGL((conv_f32_kernel<64, true>), grid, dim3(NT), 0, stream, P);
        else hipLaunchKernelGGL((conv_f32_kernel<64, false>), grid, dim3(NT), 0, stream, P);
    } else {
        if (vec) hipLaunchKernelGGL((conv_f32_kernel<32, true>), grid, dim3(NT), 0, stream, P);
        else hipLaunchKernelGGL((conv_f32_kernel<32, false>), grid, dim3(NT), 0, stream, P);
    }
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

void set_inputs(Params& P, const oess_f32_view_t* in, const oess_f32_view_t* in2, int B, int H, int W, int Cin) {
    P.in = to_view(in);
    P.has_in2 = in2 != nullptr;
    P.in2 = in2 ? to_view(in2) : View{nullptr, 0, 0, 0, 0};
    P.B = B; P.H = H; P.W = W; P.Cin = Cin;
}

void set_output(Params& P, const oess_f32_view_t* out) {
    P.out = (float*)out->data;
    P.ob = out->sb; P.oy = out->sy; P.ox = out->sx; P.oc = out->sc;
}

bool weights_ok(const float* w, const float* bias) {
    return w && ((uintptr_t)w & 15) == 0 && (!bias || ((uintptr_t)bias & 3) == 0);
}

}  // namespace

extern "C" {

size_t oess_conv2d_f32_packed_floats(int Cout, int Cin, int R, int S) {
    if (Cout < 1 || Cin < 1 || R < 1 || S < 1 || R * S > MAXTAP) return 0;
    if (R * S > MAXTAP_V1 && (R != 7 || S != 7)) return 0;        // beyond 25 taps: the 7 x 7 stem only (oess.h, K16)
    return (size_t)ceil_to(R * S * Cin, BK) * ceil_to(Cout, 32);
}

size_t oess_conv_transpose2d_f32_packed_floats(int Cout, int Cin) {
    if (Cout < 1 || Cin < 1) return 0;
    size_t rows = 0;
    for (int p = 0; p < 4; ++p) rows += ceil_to((p >> 1 ? 2 : 3) * (p & 1 ? 2 : 3) * Cin, BK);
    return rows * ceil_to(Cout, 32);
}

int oess_conv2d_dilated_fwd_f32(const oess_f32_view_t* in, const oess_f32_view_t* in2, int B, int H, int W, int Cin, int upsample2x,
                                const float* w_packed, const float* bias, int Cout, int R, int S, int stride, int pad, int dilation,
                                int act, const oess_f32_view_t* residual, const oess_f32_view_t* out, oess_stream_t stream) {
    if (!inputs_ok(in, in2, B, H, W, Cin) || !weights_ok(w_packed, bias) || !view_ok(out)) return OESS_EINVAL;
    if (Cout < 1 || oess_conv2d_f32_packed_floats(Cout, Cin, R, S) == 0 || (stride != 1 && stride != 2)) return OESS_EINVAL;
    if (pad < 0 || pad > (1 << 20) || dilation < 1 || (long long)(R - 1) * dilation > 127 || (long long)(S - 1) * dilation > 127)
        return OESS_EINVAL;                                       // tap offsets r * dilation, s * dilation live in signed char
    if (act < 0 || act > 2 || (upsample2x != 0 && upsample2x != 1) || (residual && !residual->data)) return OESS_EINVAL;
    const int Hl = upsample2x ? 2 * H : H, Wl = upsample2x ? 2 * W : W;
    const int ny = Hl + 2 * pad - dilation * (R - 1) - 1, nx = Wl + 2 * pad - dilation * (S - 1) - 1;
    if (ny < 0 || nx < 0) return OESS_EINVAL;                     // Ho, Wo >= 1
    const int Ho = ny / stride + 1, Wo = nx / stride + 1;
    Params P{};
    set_inputs(P, in, in2, B, H, W, Cin);
    P.up = upsample2x;
    P.Hl = Hl; P.Wl = Wl; P.Hq = Ho; P.Wq = Wo;
    P.stride = stride; P.off_y = -pad; P.off_x = -pad; P.ostride = 1;
    P.oh = Ho; P.ow = Wo;
    P.skip = dilation > 1;
    P.w = w_packed; P.CoutP = ceil_to(Cout, 32); P.bias = bias; P.Cout = Cout; P.act = act;
    P.has_res = residual != nullptr;
    P.res = residual ? to_view(residual) : View{nullptr, 0, 0, 0, 0};
    set_output(P, out);
    Phase& ph = P.ph[0];
    ph.ntap = R * S; ph.py = 0; ph.px = 0; ph.w_off = 0; ph.kp = ceil_to(R * S * Cin, BK);
    for (int r = 0; r < R; ++r)
        for (int s = 0; s < S; ++s) { ph.dy[r * S + s] = (signed char)(r * dilation); ph.dx[r * S + s] = (signed char)(s * dilation); }
    return launch(P, 1, (hipStream_t)stream);
}

int oess_conv2d_fwd_f32(const oess_f32_view_t* in, const oess_f32_view_t* in2, int B, int H, int W, int Cin, int upsample2x,
                        const float* w_packed, const float* bias, int Cout, int R, int S, int stride, int pad, int act,
                        const oess_f32_view_t* residual, const oess_f32_view_t* out, oess_stream_t stream) {
    if (R < 1 || S < 1 || R * S > MAXTAP_V1 || pad < 0 || pad >= R || pad >= S) return OESS_EINVAL;
    return oess_conv2d_dilated_fwd_f32(in, in2, B, H, W, Cin, upsample2x, w_packed, bias, Cout, R, S, stride, pad, 1, act, residual, out,
                                       stream);
}

int oess_conv_transpose2d_fwd_f32(const oess_f32_view_t* in, const oess_f32_view_t* in2, int B, int H, int W, int Cin,
                                  const float* w_packed, const float* bias, int Cout, int act, const oess_f32_view_t* out,
                                  oess_stream_t stream) {
    if (!inputs_ok(in, in2, B, H, W, Cin) || !weights_ok(w_packed, bias) || !view_ok(out)) return OESS_EINVAL;
    if (Cout < 1 || act < 0 || act > 2) return OESS_EINVAL;
    Params P{};
    set_inputs(P, in, in2, B, H, W, Cin);
    P.up = 0;
    P.Hl = H; P.Wl = W; P.Hq = H; P.Wq = W;
    P.stride = 1; P.off_y = 1; P.off_x = 1; P.ostride = 2;
    P.oh = 2 * H; P.ow = 2 * W;
    P.w = w_packed; P.CoutP = ceil_to(Cout, 32); P.bias = bias; P.Cout = Cout; P.act = act;
    P.has_res = 0;
    set_output(P, out);
    long long off = 0;
    for (int p = 0; p < 4; ++p) {
        Phase& ph = P.ph[p];
        ph.py = p >> 1; ph.px = p & 1;
        const int ny = ph.py ? 2 : 3, nx = ph.px ? 2 : 3;
        ph.ntap = ny * nx; ph.w_off = off; ph.kp = ceil_to(ny * nx * Cin, BK);
        for (int ty = 0; ty < ny; ++ty)
            for (int tx = 0; tx < nx; ++tx) { ph.dy[ty * nx + tx] = (signed char)-ty; ph.dx[ty * nx + tx] = (signed char)-tx; }
        off += (long long)ph.kp * P.CoutP;
    }
    return launch(P, 4, (hipStream_t)stream);
}

// K25: a token GEMM as the 1 x 1 convolution of a [1, C, 1, rows] map (the Params oess_conv2d_fwd_f32 builds at R = S = 1)
static int linear_tokens(const float* x, long long x_row_stride, int64_t rows, int Cin, const float* w_packed, const float* bias,
                         int Cout, int act, const float* residual, long long res_row_stride, float* out, long long out_row_stride,
                         oess_stream_t stream) {
    if (!x || !out || !weights_ok(w_packed, bias) || (residual && ((uintptr_t)residual & 3) != 0)) return OESS_EINVAL;
    if (rows < 1 || rows >= (1LL << 31) || Cin < 1 || Cin > (1 << 20) || Cout < 1 || Cout > (1 << 20)) return OESS_EINVAL;
    if (x_row_stride < Cin || out_row_stride < Cout || (residual && res_row_stride < Cout)) return OESS_EINVAL;
    if (x_row_stride >= (1LL << 31) || out_row_stride >= (1LL << 31) || (residual && res_row_stride >= (1LL << 31)))
        return OESS_EINVAL;                                       // rows x stride stays inside the 64-bit index arithmetic
    Params P{};
    P.in = View{x, 0, 0, x_row_stride, 1};
    P.has_in2 = 0;
    P.in2 = View{nullptr, 0, 0, 0, 0};
    P.B = 1; P.H = 1; P.W = (int)rows; P.Cin = Cin;
    P.up = 0;
    P.Hl = 1; P.Wl = (int)rows; P.Hq = 1; P.Wq = (int)rows;
    P.stride = 1; P.off_y = 0; P.off_x = 0; P.ostride = 1;
    P.oh = 1; P.ow = (int)rows;
    P.skip = 0;
    P.w = w_packed; P.CoutP = ceil_to(Cout, 32); P.bias = bias; P.Cout = Cout; P.act = act;
    P.has_res = residual != nullptr;
    P.res = View{residual, 0, 0, res_row_stride, 1};
    P.out = out;
    P.ob = 0; P.oy = 0; P.ox = out_row_stride; P.oc = 1;
    Phase& ph = P.ph[0];
    ph.ntap = 1; ph.py = 0; ph.px = 0; ph.w_off = 0; ph.kp = ceil_to(Cin, BK);
    ph.dy[0] = 0; ph.dx[0] = 0;
    return launch(P, 1, (hipStream_t)stream);
}

int oess_linear_tokens_f32(const float* x, long long x_row_stride, int64_t rows, int Cin, const float* w_packed, const float* bias,
                           int Cout, int act, const float* residual, long long res_row_stride, float* out, long long out_row_stride,
                           oess_stream_t stream) {
    if (act != 0 && act != 1) return OESS_EINVAL;
    return linear_tokens(x, x_row_stride, rows, Cin, w_packed, bias, Cout, act ? ACT_GELU : 0, residual, res_row_stride, out,
                         out_row_stride, stream);
}

// K29: the same GEMM with QuickGELU as its epilogue (an entry of its own: act 2 of oess_linear_tokens_f32 stays refused)
int oess_linear_tokens_quick_gelu_f32(const float* x, long long x_row_stride, int64_t rows, int Cin, const float* w_packed,
                                      const float* bias, int Cout, const float* residual, long long res_row_stride, float* out,
                                      long long out_row_stride, oess_stream_t stream) {
    return linear_tokens(x, x_row_stride, rows, Cin, w_packed, bias, Cout, ACT_QUICK_GELU, residual, res_row_stride, out, out_row_stride,
                         stream);
}

size_t oess_conv2d_dgrad_s2_f32_packed_floats(int Cout, int Cin, int R) {
    if (Cout < 1 || Cin < 1 || (R != 1 && R != 3)) return 0;
    size_t rows = 0;
    for (int c = 0; c < 4; ++c) rows += ceil_to(((R - (c >> 1) + 1) / 2) * ((R - (c & 1) + 1) / 2) * Cout, BK);
    return rows * ceil_to(Cin, 32);
}

int oess_conv2d_dgrad_s2_f32(const oess_f32_view_t* dy, int B, int H, int W, int Cin, const float* w_packed, int Cout, int R, int S,
                             int pad, const oess_f32_view_t* dx, oess_stream_t stream) {
    if (!view_ok(dy) || !view_ok(dx) || !weights_ok(w_packed, nullptr)) return OESS_EINVAL;
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (long long)B * H * W * Cin >= (1LL << 40)) return OESS_EINVAL;
    if (R != S || (R != 1 && R != 3) || pad < 0 || pad >= R || H + 2 * pad < R || W + 2 * pad < R) return OESS_EINVAL;
    const int Ho = (H + 2 * pad - R) / 2 + 1, Wo = (W + 2 * pad - R) / 2 + 1;
    if ((long long)B * Ho * Wo * Cout >= (1LL << 40)) return OESS_EINVAL;
    Params P{};
    set_inputs(P, dy, nullptr, B, Ho, Wo, Cout);
    P.up = 0;
    P.Hl = Ho; P.Wl = Wo; P.Hq = (H + 1) / 2; P.Wq = (W + 1) / 2;
    P.stride = 1; P.off_y = 0; P.off_x = 0; P.ostride = 2;
    P.oh = H; P.ow = W;
    P.w = w_packed; P.CoutP = ceil_to(Cin, 32); P.bias = nullptr; P.Cout = Cin; P.act = 0;
    P.has_res = 0;
    set_output(P, dx);
    // the packed blocks, by tap parity class c = 2 ry + rx: taps r = ry + 2 ty, s = rx + 2 tx
    long long off[4], o = 0;
    for (int c = 0; c < 4; ++c) {
        off[c] = o;
        o += (long long)ceil_to(((R - (c >> 1) + 1) / 2) * ((R - (c & 1) + 1) / 2) * Cout, BK) * P.CoutP;
    }
    for (int p = 0; p < 4; ++p) {
        Phase& ph = P.ph[p];
        ph.py = p >> 1; ph.px = p & 1;
        // input row 2 q + py is read by tap r of window oy when 2 oy - pad + r == 2 q + py: r of the parity of py + pad
        const int ry = (ph.py + pad) & 1, rx = (ph.px + pad) & 1;
        const int ny = (R - ry + 1) / 2, nx = (R - rx + 1) / 2;
        ph.ntap = ny * nx; ph.w_off = off[2 * ry + rx]; ph.kp = ceil_to(ny * nx * Cout, BK);
        for (int ty = 0; ty < ny; ++ty)
            for (int tx = 0; tx < nx; ++tx) {
                ph.dy[ty * nx + tx] = (signed char)((ph.py + pad - ry) / 2 - ty);
                ph.dx[ty * nx + tx] = (signed char)((ph.px + pad - rx) / 2 - tx);
            }
    }
    return launch(P, 4, (hipStream_t)stream);
}

size_t oess_convlstm_f32_workspace_bytes(long long pixels, int C_hidden) {
    if (pixels < 1 || C_hidden < 1) return 0;
    return (size_t)pixels * 4 * C_hidden * sizeof(float);
}

int oess_convlstm_step_f32(const oess_f32_view_t* xh, int B, int H, int W, int Cin, const float* w_packed, const float* bias,
                           int C_hidden, int R, int S, int pad, int prev_cell_is_zero, float* cell, const oess_f32_view_t* hidden,
                           void* ws, size_t ws_bytes, oess_stream_t stream) {
    if (!inputs_ok(xh, nullptr, B, H, W, Cin) || !weights_ok(w_packed, bias) || !cell || !view_ok(hidden) || !ws) return OESS_EINVAL;
    if (C_hidden < 1 || R < 1 || S < 1 || R * S > MAXTAP_V1 || 2 * pad != R - 1 || 2 * pad != S - 1) return OESS_EINVAL;
    if ((prev_cell_is_zero != 0 && prev_cell_is_zero != 1) || ((uintptr_t)ws & 15) != 0) return OESS_EINVAL;
    const long long npix = (long long)B * H * W;
    if (ws_bytes < oess_convlstm_f32_workspace_bytes(npix, C_hidden)) return OESS_ENOMEM;
    if (npix * 4 * C_hidden >= (1LL << 40)) return OESS_EINVAL;
    float* gates = (float*)ws;
    const oess_f32_view_t gv = {gates, (long long)H * W * 4 * C_hidden, (long long)W * 4 * C_hidden, 4LL * C_hidden, 1};
    const int e = oess_conv2d_fwd_f32(xh, nullptr, B, H, W, Cin, 0, w_packed, bias, 4 * C_hidden, R, S, 1, pad, 0, nullptr, &gv, stream);
    if (e) return e;
    const long long n = npix * C_hidden;
    hipLaunchKernelGGL(lstm_cell_f32_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, gates, C_hidden,
                       npix, H, W, cell, prev_cell_is_zero, (float*)hidden->data, hidden->sb, hidden->sy, hidden->sx, hidden->sc);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
