// K20: the image teacher's head under the contrastive loss in fp32, as one forward and one backward node:
//   k = scatter_mean(F.normalize(nn.Upsample(scale, bilinear, align_corners)(x), dim=C, eps), superpixels)
//                                                     models/image_model.py:121-143 + training/pretrain_trainer.py:445-465
// x is the head's 1x1-conv output (fp32 NHWC, 144 MB at 8 x 110 x 160 x 256); its x4 upsampled, normalised form is 2.31 GB in
// fp32 and is NEVER written: forward and backward recompute the four-corner blend of an output pixel from x.
//
// Forward (headpool_fwd_kernel): a workgroup owns HP_TW input columns (+ 1 halo column) x HP_ROWS output rows of one sample.  Per
// output row the two source rows are blended vertically ONCE into an fp32 LDS tile V[x][c] (as resize_up_rows_bf16_kernel does;
// a whole row at C = 256, W = 160 would be 160 KiB, the entire LDS of a CU, hence the column tile), every output pixel is then
// u = hx V[x0] + wx V[x1], y = u / max(|u|, eps) with the norm as a butterfly over the C / 4 lanes that hold the pixel.  The y
// rows are summed exactly as K7 sums them: a lane group walks a contiguous run of the row's pixels with an fp32 register
// accumulator, converts the run sum to 2^-32 fixed point when the superpixel id changes and adds it to an LDS table (integer
// atomics), the table leaves through the 96-bit global accumulators and segmean_fx_finalize_kernel.  The partition of pixels into
// fp32 runs depends on the shapes alone (constants HP_TW, HP_ROWS, HP_THREADS), everything that meets another partial sum is an
// integer: bit-repeatable.  The LDS table is a small open-addressed map raw id -> row (tags claimed with atomicCAS); which row an
// id lands in, or whether it overflows to the global accumulators, can differ from run to run but only re-routes integer sums.
//
// Backward (headpool_bwd_x_kernel): l2pool_bwd_x_kernel's structure -- one workgroup per output row, the C / 4 lanes of an input
// column visit the output pixels whose LEFT corner it is, take the gradient row from the S x C quotient table, form
// inv (g - y <y, g>) and split it (1 - lam) : lam between their own column and the right neighbour's LDS slot -- with y and inv
// recomputed from x by the forward's own blend (same operations in the same order: -ffp-contract=off) instead of loaded from a
// saved map.  The y pass is resize_bwd_y_kernel<false, 4>.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"
#include "bilinear_axis.h"
#include "resize_shared.h"
#include "seg_fixed.h"

namespace {
using namespace oess;

constexpr int HP_THREADS = 512;                   // forward: 8 waves
constexpr int HP_TW = 32;                         // input columns per workgroup (+ 1 halo column in LDS)
constexpr int HP_ROWS = 32;                       // output rows per workgroup
constexpr int HP_TABLE_U64 = 4096;                // LDS table: 32 KiB = (4096 / C) rows of C fixed-point sums
constexpr int HP_RAW_IDS = 256;                   // raw ids at or above go straight to the global accumulators (as K7)

constexpr size_t hp_lds_bytes(int C) {
    return (size_t)(HP_TW + 1) * C * 4 + (size_t)HP_TABLE_U64 * 8 + (size_t)(HP_TABLE_U64 / C) * 8;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 blend4(float h, const float4& a, float w, const float4& d) {
    return make_float4(h * a.x + w * d.x, h * a.y + w * d.y, h * a.z + w * d.z, h * a.w + w * d.w);
}
template <int LPP>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = LPP / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// first output index whose left source index is >= i (the left index is monotonic in the output index)
__device__ __forceinline__ int first_out_at(const Axis& ax, int i) {
    if (i <= 0) return 0;
    if (i >= ax.in) return ax.out;
    int lo, hi;
    candidates(ax, i, lo, hi);
    int o = lo;
    for (; o < ax.out; ++o) {
        int i0, i1; float lam;
        src_index(ax, o, i0, i1, lam);
        if (i0 >= i) break;
    }
    return o;
}

template <int LPP>
__global__ __launch_bounds__(HP_THREADS) void headpool_fwd_kernel(const float* __restrict__ x, int64_t xps, const int64_t* __restrict__ ids,
                                                                  int sps, int S, float eps, Axis ay, Axis ax, int ntx, int nband,
                                                                  u64_t* __restrict__ acc_lo, u64_t* __restrict__ acc_hi,
                                                                  int* __restrict__ gcnt, int* __restrict__ err) {
    constexpr int C = LPP * 4, G = HP_THREADS / LPP, NID = HP_TABLE_U64 / C;
    extern __shared__ __attribute__((aligned(16))) unsigned char hp_smem[];
    float* vrow = reinterpret_cast<float*>(hp_smem);                                     // [HP_TW + 1][C]
    u64_t* tab = reinterpret_cast<u64_t*>(hp_smem + (size_t)(HP_TW + 1) * C * 4);        // [NID][C]; channel sub*4+c at c*LPP+sub
    int* tag = reinterpret_cast<int*>(tab + HP_TABLE_U64);                               // [NID] raw id of the row, -1 = free
    int* cnt = tag + NID;                                                                // [NID]
    const int tile = blockIdx.x % ntx;
    const int lin = blockIdx.x / ntx;
    const int band = lin % nband;
    const int64_t b = lin / nband;
    const int x_beg = tile * HP_TW;
    const int ncol = min(HP_TW + 1, ax.in - x_beg);
    const int oy_beg = band * HP_ROWS, oy_end = min(oy_beg + HP_ROWS, ay.out);
    const int ox_lo = first_out_at(ax, x_beg), ox_hi = first_out_at(ax, x_beg + HP_TW);
    const int sub = threadIdx.x % LPP, grp = threadIdx.x / LPP, c = sub * 4;
    const int64_t id_off = b * (int64_t)sps;
    for (int i = threadIdx.x; i < HP_TABLE_U64; i += HP_THREADS) tab[i] = 0ull;
    for (int i = threadIdx.x; i < NID; i += HP_THREADS) { tag[i] = -1; cnt[i] = 0; }
    // this lane group's pixels of every row: a contiguous share of [ox_lo, ox_hi)
    const int n = ox_hi - ox_lo, q = (n + G - 1) / G;
    const int g_beg = min(ox_lo + grp * q, ox_hi), g_end = min(g_beg + q, ox_hi);
    int64_t cur = -1;
    float run[4] = {0.f, 0.f, 0.f, 0.f};
    int run_n = 0;
    uint32_t amax = 0;
    auto flush = [&]() {
        if (run_n == 0) return;
        int row = -1;
        if (cur >= 0 && cur < HP_RAW_IDS) {
            for (int j = 0; j < NID; ++j) {                   // open addressing; a tag never changes once claimed
                const int s = ((int)cur + j) & (NID - 1);
                const int o = atomicCAS(&tag[s], -1, (int)cur);
                if (o == -1 || o == (int)cur) { row = s; break; }
            }
        }
        if (row >= 0) {
            u64_t* r = tab + row * C + sub;
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(&r[k * LPP], (u64_t)seg_to_fixed(run[k]));
            if (sub == 0) atomicAdd(&cnt[row], run_n);
        } else {
            const int64_t gid = cur + id_off;
            if (gid >= 0 && gid < S) {
#pragma unroll
                for (int k = 0; k < 4; ++k) seg_global_add(acc_lo, acc_hi, gid * C + c + k, seg_to_fixed(run[k]));
                if (sub == 0) atomicAdd(&gcnt[gid], run_n);
            }
        }
    };
    for (int oy = oy_beg; oy < oy_end; ++oy) {
        int y0, y1; float wy;
        src_index(ay, oy, y0, y1, wy);
        const float hy = 1.f - wy;
        const int64_t row0 = (b * ay.in + y0) * ax.in + x_beg, row1 = (b * ay.in + y1) * ax.in + x_beg;
        __syncthreads();                                      // table initialised / previous row's tile consumed
        for (int j = threadIdx.x; j < ncol * LPP; j += HP_THREADS) {
            const int xl = j / LPP, cc = (j - xl * LPP) * 4;
            const float4 a = ld4(x + (row0 + xl) * xps + cc), d = ld4(x + (row1 + xl) * xps + cc);
            *reinterpret_cast<float4*>(vrow + xl * C + cc) = blend4(hy, a, wy, d);
        }
        __syncthreads();
        const int64_t prow = (b * ay.out + oy) * (int64_t)ax.out;
        cur = -1; run_n = 0;
        for (int ox = g_beg; ox < g_end; ++ox) {
            int x0, x1; float wx;
            src_index(ax, ox, x0, x1, wx);
            const float hx = 1.f - wx;
            const float4 u = blend4(hx, *reinterpret_cast<const float4*>(vrow + (x0 - x_beg) * C + c), wx,
                                    *reinterpret_cast<const float4*>(vrow + (x1 - x_beg) * C + c));
            const float ss = group_sum<LPP>(u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w);
            const float inv = 1.0f / fmaxf(sqrtf(ss), eps);
            const float yv[4] = {u.x * inv, u.y * inv, u.z * inv, u.w * inv};
            const int64_t id = ids[prow + ox];
            if (id != cur) {
                flush();
                cur = id; run_n = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) run[k] = 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                amax = max(amax, __float_as_uint(yv[k]) & 0x7fffffffu);
                run[k] += yv[k];
            }
            run_n += 1;
        }
        flush();
        run_n = 0;
    }
    if (amax >= SEG_RANGE_BITS) atomicOr(err, 1);           // a non-finite input: the whole of k becomes NaN (K7's contract)
    __syncthreads();
    for (int i = threadIdx.x; i < HP_TABLE_U64; i += HP_THREADS) {
        const int row = i / C, pos = i - row * C;
        const int raw = tag[row];
        if (raw < 0) continue;
        const int64_t gid = raw + id_off;
        if (gid < 0 || gid >= S) continue;
        const int ch = (pos % LPP) * 4 + pos / LPP;
        seg_global_add(acc_lo, acc_hi, gid * C + ch, (long long)tab[i]);
        if (pos == 0 && cnt[row] != 0) atomicAdd(&gcnt[gid], cnt[row]);
    }
}

// tmp[b, oy, ix, c] = sum over the output pixels ox of row (b, oy) of w(ox -> ix) * (adjoint row of pixel ox)
template <int LPP>
__global__ __launch_bounds__(RESIZE_THREADS) void headpool_bwd_x_kernel(const float* __restrict__ x, int64_t xps,
                                                                        const int64_t* __restrict__ ids, const float* __restrict__ table,
                                                                        int sps, int S, float eps, Axis ay, Axis ax,
                                                                        float* __restrict__ tmp) {
    constexpr int C = LPP * 4, G = RESIZE_THREADS / LPP;      // G input columns per iteration
    __shared__ __attribute__((aligned(16))) float share[(G + 1) * C];   // slot g + 1 = column (base + g)'s B; slot 0 = carry
    const int64_t t = blockIdx.x;                             // t = b * Ho + oy
    const int64_t b = t / ay.out;
    const int oy = (int)(t - b * ay.out);
    const int64_t id_off = b * (int64_t)sps;
    int y0, y1; float wy;
    src_index(ay, oy, y0, y1, wy);
    const float hy = 1.f - wy;
    const int64_t row0 = (b * ay.in + y0) * ax.in, row1 = (b * ay.in + y1) * ax.in;
    const int sub = threadIdx.x % LPP, grp = threadIdx.x / LPP, c = sub * 4;
    const float clamp_at = 1.0f / eps;
    int64_t held = -1;                                        // table row in g: neighbouring pixels mostly share their superpixel
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (grp == 0) *reinterpret_cast<float4*>(share + c) = g;
    for (int base = 0; base < ax.in; base += G) {
        const int ix = base + grp;
        float4 A = make_float4(0.f, 0.f, 0.f, 0.f), Bq = A;
        if (ix < ax.in) {
            const int ixr = min(ix + 1, ax.in - 1);
            const float4 v0 = blend4(hy, ld4(x + (row0 + ix) * xps + c), wy, ld4(x + (row1 + ix) * xps + c));
            const float4 v1 = blend4(hy, ld4(x + (row0 + ixr) * xps + c), wy, ld4(x + (row1 + ixr) * xps + c));
            int lo, hi;
            candidates(ax, ix, lo, hi);
            for (int ox = lo; ox <= hi; ++ox) {               // (everything below is uniform over the LPP lanes of this column)
                int x0, x1; float lam;
                src_index(ax, ox, x0, x1, lam);
                if (x0 != ix) continue;
                const int64_t p = t * ax.out + ox;
                const int64_t gid = ids[p] + id_off;
                if (gid < 0 || gid >= S) continue;            // rows outside the table received no gradient
                const float hx = 1.f - lam;
                const float4 u = blend4(hx, v0, lam, v1);     // the forward's blend, bit for bit
                const float ss = group_sum<LPP>(u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w);
                const float iv = 1.0f / fmaxf(sqrtf(ss), eps);
                const float4 f = make_float4(u.x * iv, u.y * iv, u.z * iv, u.w * iv);
                if (gid != held) { g = ld4(table + gid * C + c); held = gid; }
                float dot = group_sum<LPP>(f.x * g.x + f.y * g.y + f.z * g.z + f.w * g.w);
                if (iv >= clamp_at) dot = 0.f;                // |u| <= eps: y = u / eps, no projection term
                const float wa = (x1 == x0) ? iv : iv * hx, wb = (x1 == x0) ? 0.f : iv * lam;
                const float4 r = make_float4(g.x - f.x * dot, g.y - f.y * dot, g.z - f.z * dot, g.w - f.w * dot);
                A.x += wa * r.x; A.y += wa * r.y; A.z += wa * r.z; A.w += wa * r.w;
                Bq.x += wb * r.x; Bq.y += wb * r.y; Bq.z += wb * r.z; Bq.w += wb * r.w;
            }
        }
        *reinterpret_cast<float4*>(share + (grp + 1) * C + c) = Bq;
        __syncthreads();
        const float4 r0 = *reinterpret_cast<const float4*>(share + grp * C + c);
        if (ix < ax.in)
            *reinterpret_cast<float4*>(tmp + (t * ax.in + ix) * (int64_t)C + c) = make_float4(A.x + r0.x, A.y + r0.y, A.z + r0.z, A.w + r0.w);
        __syncthreads();
        if (grp == G - 1) *reinterpret_cast<float4*>(share + c) = Bq;   // carry into the next iteration's first column
    }
}

bool hp_channels_ok(int C) { return C == 64 || C == 128 || C == 256; }
}  // namespace

extern "C" {

int oess_bilinear_l2norm_pool_fwd_f32(const float* x, long long x_pix_stride, const int64_t* ids, int superpixel_size, int S, int B, int H,
                                      int W, int C, int scale, int align_corners, float eps, float* k, float* count, void* workspace,
                                      size_t workspace_bytes, oess_stream_t stream) {
    if (!x || !ids || !k || !count || !workspace || B <= 0 || H <= 0 || W <= 0 || S <= 0 || superpixel_size <= 0 || scale < 1 ||
        !hp_channels_ok(C) || x_pix_stride < C || eps <= 0.f)
        return OESS_EINVAL;
    if (!vec_ok(x, x_pix_stride, C, 0) || ((uintptr_t)workspace & 15)) return OESS_EINVAL;
    if ((int64_t)H * scale > 0x7fffffffLL || (int64_t)W * scale > 0x7fffffffLL) return OESS_EINVAL;
    const size_t need = seg_workspace_bytes(S, C);
    if (workspace_bytes < need) return OESS_ENOMEM;
    const int Ho = H * scale, Wo = W * scale;
    const Axis ay = make_axis(H, Ho, align_corners), ax = make_axis(W, Wo, align_corners);
    const int ntx = (W + HP_TW - 1) / HP_TW, nband = (Ho + HP_ROWS - 1) / HP_ROWS;
    const int64_t nwg = (int64_t)B * nband * ntx;
    if (nwg > 0x7fffffffLL) return OESS_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    OESS_HIP(hipMemsetAsync(workspace, 0, need, st));
    u64_t* acc_lo = (u64_t*)workspace;
    u64_t* acc_hi = acc_lo + (size_t)S * C;
    int* gcnt = (int*)(acc_hi + (size_t)S * C);
    int* err = gcnt + S;
#define OESS_HPF(L)                                                                                                                  \
    {                                                                                                                                \
        (void)hipFuncSetAttribute((const void*)&headpool_fwd_kernel<L>, hipFuncAttributeMaxDynamicSharedMemorySize,                  \
                                  (int)hp_lds_bytes(L * 4));                                                                         \
        hipLaunchKernelGGL((headpool_fwd_kernel<L>), dim3((unsigned)nwg), dim3(HP_THREADS), hp_lds_bytes(L * 4), st, x,              \
                           (int64_t)x_pix_stride, ids, superpixel_size, S, eps, ay, ax, ntx, nband, acc_lo, acc_hi, gcnt, err);      \
    }
    if (C == 64) OESS_HPF(16) else if (C == 128) OESS_HPF(32) else OESS_HPF(64)
#undef OESS_HPF
    hipLaunchKernelGGL(segmean_fx_finalize_kernel, dim3(grid_for((int64_t)S * C)), dim3(SEG_FIN_THREADS), 0, st, acc_lo, acc_hi, gcnt, err,
                       k, count, S, C);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_bilinear_l2norm_pool_bwd_f32(const float* x, long long x_pix_stride, const int64_t* ids, const float* grad_k, const float* count,
                                      int superpixel_size, int S, int B, int H, int W, int C, int scale, int align_corners, float eps,
                                      void* workspace, size_t workspace_bytes, float* grad_x, long long gx_pix_stride,
                                      oess_stream_t stream) {
    if (!x || !ids || !grad_k || !count || !workspace || !grad_x || B <= 0 || H <= 0 || W <= 0 || S <= 0 || superpixel_size <= 0 ||
        scale < 1 || !hp_channels_ok(C) || x_pix_stride < C || gx_pix_stride < C || eps <= 0.f)
        return OESS_EINVAL;
    if (!vec_ok(x, x_pix_stride, C, 0) || !vec_ok(grad_x, gx_pix_stride, C, 0)) return OESS_EINVAL;
    if ((int64_t)H * scale > 0x7fffffffLL || (int64_t)W * scale > 0x7fffffffLL || (int64_t)B * H * scale > 0x7fffffffLL) return OESS_EINVAL;
    const int Ho = H * scale, Wo = W * scale;
    if (workspace_bytes < oess_bilinear_l2norm_pool_bwd_workspace_bytes(B, W, C, Ho, S) || ((uintptr_t)workspace & 15)) return OESS_ENOMEM;
    const Axis ay = make_axis(H, Ho, align_corners), ax = make_axis(W, Wo, align_corners);
    hipStream_t st = (hipStream_t)stream;
    float* tmp = (float*)workspace;
    float* table = tmp + (size_t)B * Ho * W * C;
    hipLaunchKernelGGL(pool_table_kernel, dim3(grid_for((int64_t)S * C)), dim3(RESIZE_THREADS), 0, st, grad_k, count, S, C, table);
    const dim3 gx((unsigned)((int64_t)B * Ho));
#define OESS_HPB(L) hipLaunchKernelGGL((headpool_bwd_x_kernel<L>), gx, dim3(RESIZE_THREADS), 0, st, x, (int64_t)x_pix_stride, ids,      \
                                       (const float*)table, superpixel_size, S, eps, ay, ax, tmp)
    if (C == 64) OESS_HPB(16); else if (C == 128) OESS_HPB(32); else OESS_HPB(64);
#undef OESS_HPB
    hipLaunchKernelGGL((resize_bwd_y_kernel<false, 4>), dim3((unsigned)((int64_t)B * H)), dim3(RESIZE_THREADS), 0, st, (const float*)tmp, B,
                       C, ay, ax, (void*)grad_x, (int64_t)gx_pix_stride);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
