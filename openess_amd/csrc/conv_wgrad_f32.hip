// K18 fp32 SemSegE2VID training, K21 fp32 ResNet-50 training: weight and bias gradient of a convolution on the f32-input MFMA
// of gfx950 (v_mfma_f32_32x32x2_f32).
//
//   dW[co][ci][r][s] = sum over (b, oy, ox) of dY[b, oy, ox, co] * X[b, oy stride - pad + r dilation, ox stride - pad + s dilation, ci]
//   db[co] = sum of dY
// as one GEMM per tap, D[ci][co] reduced over the OUTPUT pixels: with NHWC operands both LDS tiles are [k = pixel][channel], the
// k-major layout conv_f32_kernel feeds its MFMAs from (no transpose); a tap that leaves the map is a row of zeros.
// oess_conv2d_wgrad_f32 (K18) is the stride-1, dilation-1, "same"-pad form; oess_conv2d_dilated_wgrad_f32 (K21) takes stride 1 or
// 2, any dilation and pad and the 7 x 7 stem, and leaves out the K loop of a tap that reaches the map from no output pixel at all
// (dilation 12 on a 3 x 4 map: eight of nine taps): such a tile is exact zeros.  The 7 x 7 stem folds its taps into M (folds()).
//
// Tiling: 256 threads = 4 waves in 2 x 2; a wave owns (32 NACC) input channels x 32 output channels (NACC 32 x 32 accumulators);
// block tile BM x 64 with BM = 64 or 128 input channels; K steps of 16 pixels staged through LDS, the next step's global loads
// held in registers while the current one runs on the matrix cores.
// The pixel range is split over blockIdx.z into ranges whose count depends on the shapes alone; a workgroup writes its partial
// tile with plain stores into the workspace, and a second launch adds the partials in range order and writes dW in OIHW and db.
// Every element is a fixed chain of fmaf / add: no atomics, results repeat bit for bit on any device.
#include <hip/hip_runtime.h>

#include "oess.h"
#include "oess_common.h"

namespace {

#include "f32_view.h"

constexpr int NT = 256;
constexpr int BK = 16;                 // pixels per K step
constexpr int BN = 64;                 // output channels per workgroup
constexpr int LDB = BN + 32;           // +32 floats: the two k rows of one MFMA operand read hit disjoint banks
constexpr int TARGET_WG = 1024;        // workgroups wanted (4 per CU on 256 CUs); a constant, not the device's CU count
constexpr int MIN_RANGE_PIX = 256;     // a range shorter than this is not worth its partial tile
constexpr int MAX_RANGE_PIX = 8192;    // bounds the length of one fp32 chain, whatever the map size
constexpr int MAX_SPLIT = 1024;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Params {
    View x, dy;
    int B, H, W, Cin, Cout, R, pad;
    int Ho, Wo, stride, dil;             // dy is B x Ho x Wo x Cout
    unsigned long long tap_mask;         // bit (r R + s): the tap reaches the map from some output pixel
    int fold;                            // element path only: the taps are folded into M, row m = tap Cin + ci (the 7 x 7 stem)
    int P;                               // B * Ho * Wo
    int range_pix, nsplit;
    int ntile_n;                         // output-channel tiles; blockIdx.y = tap * ntile_n + tile
    int want_db;
    float* part;                         // [nsplit][R R Cin][Cout], then [nsplit][Cout] (db)
};

struct Pix {
    int b, y, x;
};

__device__ __forceinline__ Pix pix_of(int p, int H, int W) {
    Pix r;
    r.x = p % W;
    const int t = p / W;
    r.y = t % H;
    r.b = t / H;
    return r;
}

// VEC: dense, 16-byte aligned channels in x and dy, Cin % 4 == 0 and Cout % 4 == 0 -> float4 loads
template <int NACC, bool VEC>
__global__ __launch_bounds__(NT) void conv_wgrad_f32_kernel(const Params P) {
    constexpr int BM = 64 * NACC, LDA = BM + 32;
    constexpr int NA = VEC ? BM * BK / 4 / NT : BM * BK / NT;       // staged A elements (VEC: float4s) per thread
    constexpr int NB = VEC ? 1 : BN * BK / NT;
    constexpr int AQ = VEC ? BM / 4 : BM, BQ = VEC ? BN / 4 : BN;   // columns (VEC: column quads) of one staged row
    constexpr int AROW = NT / AQ, BROW = NT / BQ;                   // rows a thread advances per staged element
    __shared__ float As[BK * LDA];
    __shared__ float Bs[BK * LDB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const bool fold = !VEC && P.fold;
    const int tap = blockIdx.y / P.ntile_n;                   // fold: 0, the rows of a tile carry their own taps
    const int m0 = blockIdx.x * BM, n0 = (blockIdx.y - tap * P.ntile_n) * BN;
    const int p0 = blockIdx.z * P.range_pix, p1 = min(p0 + P.range_pix, P.P);
    const bool do_db = P.want_db && blockIdx.x == 0 && tap == 0;
    // a tap no output pixel reaches the map through: zeros without a K loop (the db workgroup still walks dy)
    const int nstep = ((P.tap_mask >> tap) & 1ull) || do_db || fold ? (p1 - p0 + BK - 1) / BK : 0;

    const int acol = tid % AQ, arow = tid / AQ, bcol = tid % BQ, brow = tid / BQ;
    int ac = m0 + acol * (VEC ? 4 : 1);
    const int bc = n0 + bcol * (VEC ? 4 : 1);
    int my_tap = tap;
    bool a_on = ac < P.Cin;
    if (fold) {                                               // this thread's column of the A tile: row tap Cin + ci of dW
        a_on = ac < P.R * P.R * P.Cin;
        my_tap = a_on ? ac / P.Cin : 0;
        ac -= my_tap * P.Cin;
    }
    const bool b_on = bc < P.Cout;
    const int dy_tap = (my_tap / P.R) * P.dil - P.pad, dx_tap = (my_tap % P.R) * P.dil - P.pad;

    float ra[VEC ? NA * 4 : NA], rb[VEC ? NB * 4 : NB];

    auto load = [&](int step) {
        const int pk = p0 + step * BK;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int p = pk + arow + j * AROW;
            bool ok = a_on && p < p1;
            long long off = 0;
            if (ok) {
                const Pix q = pix_of(p, P.Ho, P.Wo);
                const int y = q.y * P.stride + dy_tap, x = q.x * P.stride + dx_tap;
                ok = y >= 0 && y < P.H && x >= 0 && x < P.W;
                off = q.b * P.x.sb + y * P.x.sy + x * P.x.sx + ac * P.x.sc;
            }
            if (VEC) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) v = *(const float4*)(P.x.p + off);
                ra[4 * j] = v.x; ra[4 * j + 1] = v.y; ra[4 * j + 2] = v.z; ra[4 * j + 3] = v.w;
            } else {
                ra[j] = ok ? P.x.p[off] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int p = pk + brow + j * BROW;
            const bool ok = b_on && p < p1;
            long long off = 0;
            if (ok) {
                const Pix q = pix_of(p, P.Ho, P.Wo);
                off = q.b * P.dy.sb + q.y * P.dy.sy + q.x * P.dy.sx + bc * P.dy.sc;
            }
            if (VEC) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) v = *(const float4*)(P.dy.p + off);
                rb[4 * j] = v.x; rb[4 * j + 1] = v.y; rb[4 * j + 2] = v.z; rb[4 * j + 3] = v.w;
            } else {
                rb[j] = ok ? P.dy.p[off] : 0.f;
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int row = arow + j * AROW;
            if (VEC) *(float4*)(As + row * LDA + acol * 4) = make_float4(ra[4 * j], ra[4 * j + 1], ra[4 * j + 2], ra[4 * j + 3]);
            else As[row * LDA + acol] = ra[j];
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int row = brow + j * BROW;
            if (VEC) *(float4*)(Bs + row * LDB + bcol * 4) = make_float4(rb[4 * j], rb[4 * j + 1], rb[4 * j + 2], rb[4 * j + 3]);
            else Bs[row * LDB + bcol] = rb[j];
        }
    };

    f32x16 acc[NACC];
#pragma unroll
    for (int s = 0; s < NACC; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
    float dbsum = 0.f;

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
#pragma unroll
            for (int s = 0; s < NACC; ++s) {
                const float a = As[kr * LDA + wm * 32 * NACC + s * 32 + l31];
                acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[s], 0, 0, 0);
            }
        }
        if (do_db && tid < BN) {                            // db: one chain per output channel, pixels in order
#pragma unroll
            for (int k = 0; k < BK; ++k) dbsum = dbsum + Bs[k * LDB + tid];
        }
        __syncthreads();
        if (more) {
            store();
            __syncthreads();
        }
    }

    // epilogue: D[i][j], j = lane & 31 (output channel), i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (input channel)
    const long long K = (long long)P.R * P.R * P.Cin;
    if (do_db && tid < BN && n0 + tid < P.Cout)
        P.part[(long long)P.nsplit * K * P.Cout + (long long)blockIdx.z * P.Cout + n0 + tid] = dbsum;
    const int n = n0 + wn * 32 + l31;
    if (n >= P.Cout) return;
    float* o = P.part + ((long long)blockIdx.z * K + (long long)tap * P.Cin) * P.Cout + n;
    const int rows = fold ? (int)K : P.Cin;                   // fold: row m of the tile is row m of [R R Cin][Cout]
#pragma unroll
    for (int s = 0; s < NACC; ++s) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = m0 + wm * 32 * NACC + s * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (ci < rows) o[(long long)ci * P.Cout] = acc[s][r];
        }
    }
}

// dW[co][ci][r][s] (OIHW) and db[co]: the ranges' partials added in range order
__global__ __launch_bounds__(NT) void conv_wgrad_f32_reduce_kernel(const float* __restrict__ part, int nsplit, int Cin, int Cout, int ntap,
                                                                   float* __restrict__ dw, float* __restrict__ db) {
    const long long KC = (long long)ntap * Cin * Cout;
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e < KC) {
        float s = 0.f;
        for (int i = 0; i < nsplit; ++i) s = s + part[i * KC + e];
        const int co = (int)(e % Cout);
        const long long k = e / Cout;
        const int ci = (int)(k % Cin), tap = (int)(k / Cin);
        dw[((long long)co * Cin + ci) * ntap + tap] = s;
    } else if (db && e < KC + Cout) {
        const int co = (int)(e - KC);
        const float* q = part + (long long)nsplit * KC + co;
        float s = 0.f;
        for (int i = 0; i < nsplit; ++i) s = s + q[(long long)i * Cout];
        db[co] = s;
    }
}

// Ho, Wo of the forward (oess_conv2d_dilated_fwd_f32's formula); false when there is no output
bool out_extent(int H, int W, int R, int stride, int pad, int dilation, int& Ho, int& Wo) {
    const long long ny = (long long)H + 2LL * pad - (long long)dilation * (R - 1) - 1, nx = (long long)W + 2LL * pad - (long long)dilation * (R - 1) - 1;
    if (ny < 0 || nx < 0) return false;
    Ho = (int)(ny / stride) + 1;
    Wo = (int)(nx / stride) + 1;
    return true;
}

// K21 geometry: R == S in {1, 3, 7}, stride 1 or 2, dilation >= 1 with (R - 1) dilation <= 127, pad >= 0, Ho, Wo >= 1
bool dilated_geometry_ok(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dilation) {
    if (!geometry_ok(B, H, W, Cin) || Cout < 1 || Cout > (1 << 20)) return false;
    if (R != S || (R != 1 && R != 3 && R != 7) || (stride != 1 && stride != 2)) return false;
    if (pad < 0 || pad > (1 << 20) || dilation < 1 || (long long)(R - 1) * dilation > 127) return false;
    int Ho, Wo;
    if (!out_extent(H, W, R, stride, pad, dilation, Ho, Wo) || !geometry_ok(B, Ho, Wo, Cout)) return false;
    if ((long long)B * Ho * Wo >= (1LL << 31) - MAX_RANGE_PIX) return false;
    return (long long)R * S * Cin * Cout < (1LL << 31);
}

// K18 geometry: the stride-1, "same"-pad subset of the above (Ho == H, Wo == W)
bool wgrad_geometry_ok(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dilation) {
    if (R != S || (R != 1 && R != 3) || stride != 1 || dilation != 1 || 2 * pad != R - 1) return false;
    return dilated_geometry_ok(B, H, W, Cin, Cout, R, S, stride, pad, dilation);
}

// the split of the OUTPUT pixel range: a function of the shapes alone
// The 7 x 7 stem (Cin = 3): one tap per tile would run 49 tiles of 64 rows with 3 rows of data each and read dy 49 times; its
// taps are folded into M instead (147 rows = two tiles of 128).  Cin % 4 != 0 is always the element path: a function of the shapes.
bool folds(int Cin, int R) { return R == 7 && Cin % 4 != 0 && Cin < 64; }

void split_of(int B, int Ho, int Wo, int Cin, int Cout, int R, int& nsplit, int& range_pix) {
    const long long P = (long long)B * Ho * Wo;
    const int M = folds(Cin, R) ? R * R * Cin : Cin, BM = M > 64 ? 128 : 64;
    const long long tiles = (long long)(folds(Cin, R) ? 1 : R * R) * ((M + BM - 1) / BM) * ((Cout + BN - 1) / BN);
    long long n = (TARGET_WG + tiles - 1) / tiles;
    const long long by_size = (P + MIN_RANGE_PIX - 1) / MIN_RANGE_PIX, by_chain = (P + MAX_RANGE_PIX - 1) / MAX_RANGE_PIX;
    n = n < by_size ? n : by_size;
    n = n > by_chain ? n : by_chain;
    n = n < MAX_SPLIT ? n : MAX_SPLIT;
    long long rp = (P + n - 1) / n;
    rp = (rp + BK - 1) / BK * BK;
    range_pix = (int)rp;
    nsplit = (int)((P + rp - 1) / rp);
}

// does tap offset t (= r dilation - pad) reach [0, n) from some output index in [0, no)?
bool tap_reaches(int t, int n, int no, int stride) {
    const int lo = t >= 0 ? 0 : (-t + stride - 1) / stride;
    if (n - 1 - t < 0) return false;
    const int hi = (n - 1 - t) / stride < no - 1 ? (n - 1 - t) / stride : no - 1;
    return lo <= hi;
}

size_t workspace_bytes(int B, int H, int W, int Cin, int Cout, int R, int stride, int pad, int dilation) {
    int Ho, Wo, nsplit, range_pix;
    out_extent(H, W, R, stride, pad, dilation, Ho, Wo);
    split_of(B, Ho, Wo, Cin, Cout, R, nsplit, range_pix);
    return (size_t)nsplit * ((size_t)R * R * Cin * Cout + Cout) * sizeof(float);
}

// geometry already checked.  skip_taps: leave out the K loop of the taps that read nothing but padding
int run(const oess_f32_view_t* x, const oess_f32_view_t* dy, int B, int H, int W, int Cin, int Cout, int R, int stride, int pad,
        int dilation, bool skip_taps, float* dw, float* db, void* ws, oess_stream_t stream) {
    Params P{};
    P.x = to_view(x);
    P.dy = to_view(dy);
    P.B = B; P.H = H; P.W = W; P.Cin = Cin; P.Cout = Cout; P.R = R; P.pad = pad;
    P.stride = stride; P.dil = dilation;
    out_extent(H, W, R, stride, pad, dilation, P.Ho, P.Wo);
    P.P = B * P.Ho * P.Wo;
    P.tap_mask = ~0ull;
    if (skip_taps) {
        P.tap_mask = 0ull;
        for (int r = 0; r < R; ++r)
            for (int s = 0; s < R; ++s)
                if (tap_reaches(r * dilation - pad, H, P.Ho, stride) && tap_reaches(s * dilation - pad, W, P.Wo, stride))
                    P.tap_mask |= 1ull << (r * R + s);
    }
    split_of(B, P.Ho, P.Wo, Cin, Cout, R, P.nsplit, P.range_pix);
    P.ntile_n = (Cout + BN - 1) / BN;
    P.want_db = db != nullptr;
    P.part = (float*)ws;
    P.fold = folds(Cin, R);
    const int M = P.fold ? R * R * Cin : Cin;
    const bool big = M > 64;
    const int BM = big ? 128 : 64;
    const long long gy = (long long)(P.fold ? 1 : R * R) * P.ntile_n;
    if (gy > 65535 || (M + BM - 1) / BM > 65535) return OESS_EINVAL;
    const bool vec = Cin % 4 == 0 && Cout % 4 == 0 && vec_ok(x) && vec_ok(dy);
    const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)gy, (unsigned)P.nsplit);
    hipStream_t st = (hipStream_t)stream;
    if (big) {
        if (vec) hipLaunchKernelGGL((conv_wgrad_f32_kernel<2, true>), grid, dim3(NT), 0, st, P);
        else hipLaunchKernelGGL((conv_wgrad_f32_kernel<2, false>), grid, dim3(NT), 0, st, P);
    } else {
        if (vec) hipLaunchKernelGGL((conv_wgrad_f32_kernel<1, true>), grid, dim3(NT), 0, st, P);
        else hipLaunchKernelGGL((conv_wgrad_f32_kernel<1, false>), grid, dim3(NT), 0, st, P);
    }
    OESS_HIP(hipGetLastError());
    const long long total = (long long)R * R * Cin * Cout + Cout;
    hipLaunchKernelGGL(conv_wgrad_f32_reduce_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st, (const float*)ws, P.nsplit,
                       Cin, Cout, R * R, dw, db);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // namespace

extern "C" {

size_t oess_conv2d_wgrad_f32_workspace_bytes(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dilation) {
    if (!wgrad_geometry_ok(B, H, W, Cin, Cout, R, S, stride, pad, dilation)) return 0;
    return workspace_bytes(B, H, W, Cin, Cout, R, stride, pad, dilation);
}

int oess_conv2d_wgrad_f32(const oess_f32_view_t* x, const oess_f32_view_t* dy, int B, int H, int W, int Cin, int Cout, int R, int S,
                          int stride, int pad, int dilation, float* dw, float* db, void* ws, size_t ws_bytes, oess_stream_t stream) {
    if (!view_ok(x) || !view_ok(dy) || !dw || !ws || ((uintptr_t)ws & 15) != 0) return OESS_EINVAL;
    if (!wgrad_geometry_ok(B, H, W, Cin, Cout, R, S, stride, pad, dilation)) return OESS_EINVAL;
    if (ws_bytes < workspace_bytes(B, H, W, Cin, Cout, R, stride, pad, dilation)) return OESS_ENOMEM;
    return run(x, dy, B, H, W, Cin, Cout, R, stride, pad, dilation, false, dw, db, ws, stream);
}

size_t oess_conv2d_dilated_wgrad_f32_workspace_bytes(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                                                     int dilation) {
    if (!dilated_geometry_ok(B, H, W, Cin, Cout, R, S, stride, pad, dilation)) return 0;
    return workspace_bytes(B, H, W, Cin, Cout, R, stride, pad, dilation);
}

int oess_conv2d_dilated_wgrad_f32(const oess_f32_view_t* x, const oess_f32_view_t* dy, int B, int H, int W, int Cin, int Cout, int R,
                                  int S, int stride, int pad, int dilation, float* dw, float* db, void* ws, size_t ws_bytes,
                                  oess_stream_t stream) {
    if (!view_ok(x) || !view_ok(dy) || !dw || !ws || ((uintptr_t)ws & 15) != 0) return OESS_EINVAL;
    if (!dilated_geometry_ok(B, H, W, Cin, Cout, R, S, stride, pad, dilation)) return OESS_EINVAL;
    if (ws_bytes < workspace_bytes(B, H, W, Cin, Cout, R, stride, pad, dilation)) return OESS_ENOMEM;
    return run(x, dy, B, H, W, Cin, Cout, R, stride, pad, dilation, true, dw, db, ws, stream);
}

}  // extern "C"
