// bf16 implicit-GEMM 2-D convolutions for gfx950: the host half (ConvCall / conv_plan / conv_launch, the grouped launches,
// the w128 tile schedule, the fused head launch, every extern "C" entry).  The kernels live in headers included below, inside
// this file's anonymous namespace, one family each:
//   conv_args.h        operand layout, ConvArgs, LDS swizzle, output store, activation, conv_epilogue, ConvLSTM epilogue
//   convgru_epilogue.h the fused ConvGRU epilogues conv_fwd_dma_kernel names (instantiated by convgru.hip)
//   conv_frag.h        the fragment macros the K loops share (MFMA block, counted LDS wait, w128 fragment reads)
//   conv_general.h     conv_fwd_kernel: register-staged general route
//   conv_dma.h         conv_fwd_dma_kernel (LDS-DMA routes, split-K slices, 256 x 256 tile), splitk_reduce_kernel
//   conv3x3_halo.h     conv3x3_halo_kernel, ConvGroup and the two grouped ConvLSTM kernels (row-halo reuse)
//   conv_lstm_w128.h   conv3x3_lstm_w128_kernel: persistent w128 ConvLSTM gates
//   conv_w128_gemm.h   conv1x1_w128_kernel: persistent w128 1x1 / GEMM
//   conv3x3_w128.h     conv3x3_w128_kernel: persistent w128 3x3
//   conv5x5s2_halo.h   conv5x5s2_halo_kernel, S2Head (fused E2VID head), S2Group and the grouped kernel, S2Pre and
//                      conv5x5s2_halo_pre_kernel (fused head with EventPreprocessor's hot-pixel mask and flip)
//   conv_dma32.h       conv_fwd_dma32_kernel: 32-wide K slabs in a deeper ring
//   conv_smallcin.h    conv_smallcin_kernel: Cin == 8
//   conv_pack.h        pack_weight_kernel, pack_fwd_multi_kernel, pack_flip_multi_kernel
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include <map>
#include <mutex>
#include <vector>
#include "oess.h"
#include "oess_common.h"

namespace {
#include <type_traits>
#include <utility>
using namespace oess;

#include "conv_args.h"
#include "convgru_epilogue.h"
#include "conv_frag.h"
#include "conv_general.h"
#include "conv_dma.h"
#include "conv3x3_halo.h"
// The frag_read / mma lambdas of the three w128 kernels name their captures: hipcc does not count an asm operand inside a
// generic lambda as a use, so it calls those captures unused, and with a capture default the same lambdas do not compile.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-lambda-capture"
#include "conv_lstm_w128.h"
#include "conv_w128_gemm.h"
#include "conv3x3_w128.h"
#pragma clang diagnostic pop
#include "conv5x5s2_halo.h"
#include "conv_dma32.h"
#include "conv_smallcin.h"
#include "conv_pack.h"

}  // namespace

extern "C" {

long long oess_conv2d_pack_multi_blocks(int Cout, int Cin, int R, int S, int flip_from_packed) {
    if (Cout <= 0 || Cin <= 0 || R <= 0 || S <= 0 || (Cout & 7) || (Cin & 7)) return 0;
    if (flip_from_packed) return (long long)R * S * ((Cout + 63) / 64) * ((Cin + 63) / 64);
    const long long groups = (long long)Cout * (R * S * Cin / 8);
    return (groups + PACK_CHUNK / 8 - 1) / (PACK_CHUNK / 8);
}

int oess_conv2d_pack_weight_multi(const long long* table_dev, int n, long long total_blocks, int flip_from_packed,
                                  oess_stream_t stream) {
    if (!table_dev || n <= 0 || total_blocks <= 0 || total_blocks > 0x7fffffffll) return OESS_EINVAL;
    if (flip_from_packed)
        hipLaunchKernelGGL(pack_flip_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, table_dev, n);
    else
        hipLaunchKernelGGL(pack_fwd_multi_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, table_dev, n);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_conv2d_pack_weight(const float* w_oihw, int Cout, int Cin, int R, int S, int flip_for_dgrad, void* packed,
                            size_t packed_bytes, oess_stream_t stream) {
    if (!w_oihw || !packed || Cout <= 0 || Cin <= 0 || R <= 0 || S <= 0) return OESS_EINVAL;
    if (flip_for_dgrad == 2 && (Cout & 3)) return OESS_EINVAL;
    const int n_log = flip_for_dgrad == 1 ? Cin : Cout, c_log = flip_for_dgrad == 1 ? Cout : Cin;
    const int cin_pad = (c_log + 7) / 8 * 8;
    const int kpad = (R * S * cin_pad + BK - 1) / BK * BK;
    const int npad = (n_log + 127) / 128 * 128;
    if (packed_bytes < (size_t)npad * kpad * 2) return OESS_ENOMEM;
    const long long total = (long long)npad * kpad;
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(pack_weight_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w_oihw, (uint16_t*)packed, Cout,
                       Cin, R, S, cin_pad, kpad, npad, flip_for_dgrad);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

size_t oess_conv2d_packed_bytes(int Cout, int Cin, int R, int S, int flip_for_dgrad) {
    if (Cout <= 0 || Cin <= 0 || R <= 0 || S <= 0) return 0;
    const int n_log = flip_for_dgrad == 1 ? Cin : Cout, c_log = flip_for_dgrad == 1 ? Cout : Cin;
    const int cin_pad = (c_log + 7) / 8 * 8;
    const int kpad = (R * S * cin_pad + BK - 1) / BK * BK;
    const int npad = (n_log + 127) / 128 * 128;
    return (size_t)npad * kpad * 2;
}

}  // extern "C"

namespace {
void conv_set_attrs() {
    static bool set_on[64] = {false};     // the attribute is per device
    int dev = 0;
    (void)hipGetDevice(&dev);
    const bool attrs_set = dev >= 0 && dev < 64 && set_on[dev];
    if (!attrs_set) {       // > 64 KiB of dynamic LDS needs an explicit opt-in
        const void* fns[] = {(const void*)&conv_fwd_kernel<128>, (const void*)&conv_fwd_kernel<64>, (const void*)&conv_fwd_kernel<32>,
                             (const void*)&conv_fwd_dma_kernel<128, 128, 2, false>, (const void*)&conv_fwd_dma_kernel<128, 64, 2, false>, (const void*)&conv_fwd_dma_kernel<128, 32, 2, false>,
                             (const void*)&conv_fwd_dma_kernel<128, 128, 2, true>, (const void*)&conv_fwd_dma_kernel<128, 64, 2, true>, (const void*)&conv_fwd_dma_kernel<128, 32, 2, true>,
                             (const void*)&conv_fwd_dma_kernel<64, 128, 2, false>, (const void*)&conv_fwd_dma_kernel<64, 128, 2, true>,
                             (const void*)&conv_fwd_dma_kernel<128, 128, 2, false, 1>, (const void*)&conv_fwd_dma_kernel<128, 128, 2, true, 1>,
                             (const void*)&conv3x3_halo_kernel<0>, (const void*)&conv3x3_halo_kernel<1>, (const void*)&conv3x3_halo_group_kernel<1>,
                             (const void*)&conv3x3_halo256_group_kernel, (const void*)&conv3x3_lstm_w128_kernel, (const void*)&conv1x1_w128_kernel<true>, (const void*)&conv1x1_w128_kernel<false>, (const void*)&conv3x3_w128_kernel,
                             (const void*)&conv_fwd_dma_kernel<256, 256, 2, true>,
                             (const void*)&conv_fwd_dma_kernel<128, 128, 4, true, 0, 512>,
                             (const void*)&conv_fwd_dma32_kernel<128, true, 0, 3>, (const void*)&conv5x5s2_halo_kernel<false>,
                             (const void*)&conv5x5s2_halo_kernel<true>, (const void*)&conv5x5s2_halo_group_kernel,
                             (const void*)&conv5x5s2_halo_pre_kernel};
        for (const void* f : fns) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (dev >= 0 && dev < 64) set_on[dev] = true;
    }
}

// One bf16 convolution (or fused ConvLSTM step) without its pointers: everything the dispatch rules look at.
struct ConvCall {
    int B, H, W, Cin, Cout, R, S, stride, pad, dil, relu;
    bool has_bias, has_residual, out_is_f32, with_tile_stats, out_aligned16;    // (the bf16 output pointer's 16-byte alignment)
    long long in_pix_stride, out_pix_stride, res_pix_stride;
    int C_hidden; long long hidden_pix_stride;      // C_hidden != 0: fused ConvLSTM step (Cout = 4 * C_hidden; the out_* / res_* fields are unused)
    size_t workspace_bytes;                 // split-K workspace on offer (0 = none)
};
// What conv_plan decides: the kernel (OESS_ROUTE_*, split-K with its slice count), its launch shape and the ConvArgs it gets,
// pointers left null.  want_workspace = the split-K workspace the call takes if offered that much (0: no split-K for it).
struct ConvPlan {
    int route;
    ConvArgs args;                          // (conv_bind puts the pointers in)
    dim3 grid, block;
    size_t lds, want_workspace;
};
struct ConvPtrs {                           // ConvLSTM calls: lstm_prev / lstm_cell / lstm_h = previous cell (or null), new cell, hidden output
    const void *in, *w; const float* bias; const void* residual; void* out_bf16; float *out_f32, *tile_stats;
    const float* lstm_prev; float* lstm_cell; void* lstm_h; void* workspace;
};

inline int s2_tiles_m(int B, int Ho, int Wo) { return B * ((Ho + S2_PH - 1) / S2_PH) * ((Wo + S2_PW - 1) / S2_PW); }

// The dispatch rules as a pure host function: validates the call, walks the rules in order and fills *p for the first one that
// takes it.  No launch, no attribute call, no allocation; the one runtime call is num_cus() behind the w128 rules.  One value
// of OESS_ROUTE_* per template instantiation (include/oess.h), each pinned by a row of tests/conv_route_cases.py.
int conv_plan(const ConvCall& c, ConvPlan* p) {
    const int B = c.B, H = c.H, W = c.W, Cin = c.Cin, Cout = c.Cout, R = c.R, S = c.S, stride = c.stride, pad = c.pad, dil = c.dil, relu = c.relu;
    const bool bias = c.has_bias, residual = c.has_residual, out_f32 = c.out_is_f32, tile_stats = c.with_tile_stats, lstm = c.C_hidden != 0;
    // (a ConvLSTM call's output stride satisfies the generic output checks below; the conv epilogue is not used)
    const long long in_pix_stride = c.in_pix_stride, res_pix_stride = c.res_pix_stride, out_pix_stride = lstm ? Cout : c.out_pix_stride;
    p->want_workspace = 0;
    if (lstm) {
        if (c.C_hidden <= 0 || (c.C_hidden & 31) || Cout != 4 * c.C_hidden || (c.hidden_pix_stride & 1) ||
            c.hidden_pix_stride < c.C_hidden || residual || relu || tile_stats || out_f32 || stride != 1)
            return OESS_EINVAL;
    }
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || (Cin & 7) || Cout <= 0 || R <= 0 || S <= 0 || stride <= 0 || pad < 0 || dil <= 0)
        return OESS_EINVAL;
    if ((in_pix_stride & 7) || in_pix_stride < Cin || out_pix_stride < Cout) return OESS_EINVAL;
    if (!out_f32 && (out_pix_stride & 7) && (Cout & 7) == 0) return OESS_EINVAL;
    if (residual && ((res_pix_stride & 7) || out_f32)) return OESS_EINVAL;
    ConvArgs& a = p->args;
    a = ConvArgs{};                         // (all pointers null)
    if (tile_stats && (bias || out_f32 || residual || relu)) return OESS_EINVAL;
    a.in_pix_stride = in_pix_stride; a.out_pix_stride = out_pix_stride; a.res_pix_stride = res_pix_stride;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
    a.R = R; a.S = S; a.stride = stride; a.pad = pad; a.dil = dil;
    a.Ho = (H + 2 * pad - dil * (R - 1) - 1) / stride + 1;
    a.Wo = (W + 2 * pad - dil * (S - 1) - 1) / stride + 1;
    if (a.Ho <= 0 || a.Wo <= 0) return OESS_EINVAL;
    a.Kpad = (R * S * Cin + BK - 1) / BK * BK;
    const long long M = (long long)B * a.Ho * a.Wo;
    if (M > 0x7fffffffll) return OESS_EINVAL;
    a.M = (int)M;
    a.relu = relu;
    a.lstm_h_stride = lstm ? c.hidden_pix_stride : 0; a.lstm_C = c.C_hidden;
    a.tiles_m = (a.M + BM - 1) / BM;
    a.ksplit = 1; a.kt_per = 0;
    a.mg_w = (W >= 2 && 256ll * W < 0x100000000ll) ? (unsigned)(0x100000000ull / (unsigned)W) + 1u : 0u;
    a.mg_wd = (256ll * (W + dil) < 0x100000000ll) ? (unsigned)(0x100000000ull / (unsigned)(W + dil)) + 1u : 0u;
    // The LDS-DMA kernels address the input with 32-bit buffer offsets and decode filter taps with exact small-range
    // reciprocals (verified here over the whole range); anything outside takes the register-staged generic kernel.
    const long long in_extent = (((long long)B * H * W - 1) * in_pix_stride + Cin) * 2;
    bool dma_ok = in_extent < 0x7ffffff0ll;
    {
        const unsigned cpt = (unsigned)(Cin >> 3), nkc = (unsigned)(a.Kpad / 8);
        a.inv_cpt = ((1u << 20) + cpt - 1) / cpt;
        a.inv_s = ((1u << 16) + (unsigned)S - 1) / (unsigned)S;
        bool exact = nkc < 4096;
        for (unsigned kc = 0; exact && kc < nkc; ++kc) exact = ((kc * a.inv_cpt) >> 20) == kc / cpt;
        const unsigned maxtap = nkc / cpt + 1;
        for (unsigned t = 0; exact && t <= maxtap; ++t) exact = ((t * a.inv_s) >> 16) == t / (unsigned)S;
        if (!exact) dma_ok = false;
    }
    // the packed weight has Npad = multiple of 128 rows, so any BN <= 128 tiles it safely
    const int bn = Cout > 64 ? 128 : (Cout > 32 ? 64 : 32);
    a.tiles_n = (Cout + bn - 1) / bn;
    const dim3 grid(a.tiles_m * a.tiles_n), block(CONV_THREADS);
    const bool fastk = (Cin % 64) == 0, fastk32 = (Cin % 32) == 0;
    const size_t epi = (size_t)BM * (bn + 8) * 2 + 4096;     // output image + BatchNorm partials
    // tile-quantisation model shared by the rules below: 128-row tiles run two workgroups per CU (512 slots), 64-row tiles
    // three (768 slots) at 0.88 of the per-tile efficiency (measured)
    const long long t128 = (long long)a.tiles_m * a.tiles_n;
    const long long t64 = (long long)((a.M + 63) / 64) * a.tiles_n;
    const double e128 = (double)t128 / (double)(((t128 + 511) / 512) * 512);
    const double e64 = 0.88 * (double)t64 / (double)(((t64 + 767) / 768) * 768);
    const bool want64 = bn == 128 && !tile_stats && !lstm && e64 > e128 * 1.04;
    auto take = [p](int route, dim3 g, dim3 b, size_t lds) { p->route = route; p->grid = g; p->block = b; p->lds = lds; return OESS_OK; };

    // (1) Cin == 8 stencil layers (E2VID head): LDS halo tile instead of the im2col gather
    if (!lstm && Cin == 8 && stride == 1 && dil == 1 && R == 5 && S == 5 && Cout <= 32 && (Cout & 3) == 0 && !residual && !out_f32 &&
        !tile_stats && (out_pix_stride & 3) == 0 && a.Kpad == 256 && dma_ok) {
        const int tiles = B * ((a.Ho + 7) / 8) * ((a.Wo + 63) / 64);
        return take(OESS_ROUTE_SMALLCIN, dim3(tiles < 512 ? tiles : 512), dim3(256), 0);   // persistent: 2 workgroups per CU
    }
    if (!dma_ok) {
        if (lstm) return OESS_EINVAL;       // the fused ConvLSTM epilogue exists only in the LDS-DMA kernels
        const size_t tab = (size_t)(a.Kpad / 8) * 8;
        size_t lds = (size_t)2 * (BM + bn) * 8 * 16 + tab;
        if (lds < epi) lds = epi;
        return take(bn == 128 ? OESS_ROUTE_FALLBACK_128 : (bn == 64 ? OESS_ROUTE_FALLBACK_64 : OESS_ROUTE_FALLBACK_32), grid, block, lds);
    }
    // (1b) 5x5 stride-2 pad-2 layers (E2VID's encoder ConvLayers): 2-D input halo in LDS, 8 x 16-pixel x 64-channel tiles
    if (!lstm && R == 5 && S == 5 && stride == 2 && pad == 2 && dil == 1 && (Cin & 31) == 0 && (Cout & 63) == 0 && !tile_stats &&
        !residual && !out_f32 && relu != 2 && (out_pix_stride & 7) == 0 && c.out_aligned16 && a.Kpad >= 25 * Cin) {
        a.tiles_n = Cout / 64;
        a.tiles_m = s2_tiles_m(B, a.Ho, a.Wo);
        return take(OESS_ROUTE_S2_HALO, dim3(a.tiles_m * a.tiles_n), dim3(256), S2_LDS);
    }
    // (1c) SMALL MAPS (at most one 128 x 128 tile per CU: DeepLabv3's OS16 half, M = 8 960), K >= 16 slabs, not a row-halo 3x3:
    //      with a single workgroup on a CU nothing is lost by giving it the whole LDS, so the ring is 4 deep (three slabs in
    //      flight).  Measured on the DeepLabv3 forward (round 5, same box, ring 2 / 3 / 4): 1024->256 36.1 / 31.6 / 31.4 us,
    //      2048->256 42.1 / 36.2 / 35.4, 1280->256 30.6-43.8 / 26.3 / 26.7, 256->1024 25.1 / 21.1 / 23.8; the 3x3 layers of the
    //      same maps do not move (45 / 64 / 73 us either way: they stay on the row-halo kernel) -- the small-map K loop is not
    //      waiting for the operand round trip alone (profiles/r05_deep_ring_ab.txt).  EIGHT waves (32 x 64 wave tiles, two waves
    //      per SIMD: one wave's DMA issue runs under the other's MFMAs, which a lone 4-wave workgroup cannot do): 1024->256
    //      32.3 -> 29.4 us, 2048->256 36.0 -> 30.1, 1280->256 28.7 -> 23.1, 256->1024 22.5 -> 20.4 (same box, alternating).
    {
        const bool is3x3halo = R == 3 && S == 3 && stride == 1 && pad == dil;
        if (!lstm && bn == 128 && fastk && t128 <= 256 && a.Kpad / BK >= 16 && a.Kpad / BK < 200 && !is3x3halo) {
            size_t lds = (size_t)4 * (BM + 128) * 8 * 16;
            if (lds < epi) lds = epi;
            return take(OESS_ROUTE_SMALLMAP_RING, grid, dim3(512), lds);
        }
    }
    // (2a) the same layers in front of a BatchNorm (raw bf16 result + tile statistics: conv2 of the frozen teacher's dilated
    //      bottlenecks), Cout % 256 == 0, >= 2 tiles of 256 x 256 per CU: persistent workgroups on 128 x 128 wave tiles
    //      (conv3x3_w128.h).  OESS_W128_CONV3=0 keeps rule (2) (A/B).
    if (!lstm && R == 3 && S == 3 && stride == 1 && pad == dil && fastk && (Cout % 256) == 0 && a.Kpad == 9 * Cin && a.Ho == H && a.Wo == W &&
        !bias && !relu && !residual && !out_f32 && (out_pix_stride & 7) == 0 && c.out_aligned16 && a.mg_w && a.mg_wd) {
        const int use3 = [] { const char* e = getenv("OESS_W128_CONV3"); return e ? atoi(e) : 1; }();
        const long long t256 = (long long)((a.M + 255) / 256) * (Cout / 256);
        const long long out_extent = ((long long)a.M - 1) * out_pix_stride * 2 + (long long)Cout * 2;
        const int breaks = (256 + W - 2) / W;
        if (use3 && t256 >= 2ll * num_cus() && dil + 255 + dil * breaks + dil + 1 <= W128_HROWS && breaks + 1 + 2 * dil <= H &&
            out_extent < 0x7ffffff0ll && (long long)Cout * a.Kpad * 2 < 0x7ffffff0ll && (long long)H * W * W < 0x100000000ll) {
            a.tiles_m = (a.M + 255) / 256; a.tiles_n = Cout / 256;
            return take(OESS_ROUTE_CONV3X3_W128, dim3(num_cus() / 8 * 8), dim3(256), (size_t)W128_OPER);
        }
    }
    // (2) 3x3 stride-1 'same' convolutions with Cin % 64 == 0: row-halo reuse of the pixel operand, unless the 64-row tiling
    //     is what the layer wants (tile quantisation of small maps)
    if (R == 3 && S == 3 && stride == 1 && pad == dil && fastk && bn == 128 && a.Kpad == 9 * Cin && a.Ho == H && a.Wo == W &&
        (dil + 127 + dil * ((BM + W - 2) / W) + dil + 1) <= HALO_ROWS && !want64)
        return take(lstm ? OESS_ROUTE_HALO3X3_LSTM : OESS_ROUTE_HALO3X3, grid, block, (size_t)2 * HALO_ROWS * 128 + (size_t)2 * 128 * 128);
    // (3) fused ConvLSTM cell update on geometries the halo kernel does not take
    if (lstm) return take(fastk ? OESS_ROUTE_LSTM_FASTK : OESS_ROUTE_LSTM_SLOWK, grid, block, (size_t)2 * (BM + 128) * 8 * 16);
    // (3a) split-K for small-M / long-K layers (DeepLabv3's ASPP at output stride 16: M = 8 960 = 70 row tiles x 2 column
    //      tiles = 140 workgroups for 512 slots, K = 18 432 = 288 slabs each: 272 us at 311 TFLOP/s).  Model (us): a workgroup
    //      spends 1.1 per slab + 6 fixed; the fp32 slices cost a write and a read of ks * M * Cout * 4 bytes at ~3 TB/s plus
    //      one launch.  Taken when it beats both the one-pass 128-row tiling and the 64-row tiling by 15 %.
    if (bn == 128 && (Cout & 3) == 0 && a.Kpad / BK >= 32 && t128 <= 384 && (!out_f32 || (out_pix_stride & 3) == 0)) {
        const int KTall = a.Kpad / BK;
        auto rounds = [](long long wg, long long slots) { return (double)((wg + slots - 1) / slots); };
        const double t_one = rounds(t128, 512) * (KTall * 1.1 + 6.0);
        const double t_64 = rounds(t64, 768) * (KTall * 0.62 + 6.0);
        int best = 1;
        double tbest = (tile_stats ? t_one : (t_one < t_64 ? t_one : t_64)) / 1.15;
        for (int ks = 2; ks <= 8; ++ks) {
            const int per = (KTall + ks - 1) / ks;
            if (per < 8 || (long long)per * (ks - 1) >= KTall) continue;       // every slice non-empty
            const double tk = rounds(t128 * ks, 512) * (per * 1.1 + 6.0) + 2.0 * ks * (double)a.M * Cout * 4.0 / 3.0e6 + 5.0;
            if (tk < tbest) { tbest = tk; best = ks; }
        }
        if (best > 1) {
            p->want_workspace = (size_t)best * (size_t)a.M * Cout * sizeof(float);
            if (c.workspace_bytes >= p->want_workspace) {        // (conv_launch points a.partial at the workspace)
                a.ksplit = best; a.kt_per = (KTall + best - 1) / best;
                return take((fastk ? OESS_ROUTE_SPLITK_FASTK : OESS_ROUTE_SPLITK_SLOWK) | best << 8, dim3(a.tiles_m * a.tiles_n, best), block,
                            (size_t)2 * (BM + 128) * 8 * 16);
            }
        }
    }
    // (3b) large plain-GEMM layers (1x1, Cin % 64 == 0, Cout % 256 == 0, K >= 256): 256 x 256 tiles on ONE 8-wave workgroup per
    //      CU, wave tile 64 x 128 (24 fragment reads per 32 MFMAs instead of 16 per 16, half the L2 -> LDS bytes per FLOP).
    //      Same template as rule (6).  Measured against the 128 x 128 tiling on the teacher's layers at M = 140 800:
    //      512->2048 556 -> 451 us, 1024->2048 831 -> 680, 2048->512 396 -> 362, 256->1024 179 -> 169; ViT fc1 (M = 8 968,
    //      432 tiles) 65.8 -> 62.5 without its GELU epilogue (with it, round 5: 88 us on either tiling).  Below ~1.5 rounds of 256 tiles the coarser quantisation loses (324 tiles: 51.7 -> 59.5 us).
    //      (Round 5: under the concurrent step schedule these 128 KB / 512-thread workgroups wait for a CU free of ConvLSTM
    //      workgroups and run 2.2 x longer than alone; the 128 x 128 tiling, which co-resides, was measured there as well:
    //      193.0 vs 194.8 event-frames/s, 318 vs 324 on frame2recon_full -- the big tile stays.)
    if (bn == 128 && fastk && (Cout % 256) == 0 && a.Kpad >= 256 && R == 1 && S == 1 && stride == 1) {
        const long long t256 = (long long)((a.M + 255) / 256) * (Cout / 256);
        // (3a) the same layers in front of a BatchNorm (raw bf16 result + tile statistics; the frozen teacher's conv1 / conv3 /
        //      downsample layers) or with a bias / ReLU (its 2048 -> 256 decoder layer), >= 2 tiles per CU: persistent workgroups on
        //      128 x 128 wave tiles (conv_w128_gemm.h).
        //      OESS_W128_GEMM=0 keeps rule (3b) (A/B).
        const int use_w128 = [] { const char* e = getenv("OESS_W128_GEMM"); return e ? atoi(e) : 1; }();
        const long long out_extent = ((long long)a.M - 1) * out_pix_stride * 2 + (long long)Cout * 2;
        static const long long min_t = [] { const char* e = getenv("OESS_W128_MIN_TILES"); return e ? atoll(e) : 0ll; }();      // A/B knob
        if (use_w128 && t256 >= (min_t > 0 ? min_t : 2ll * num_cus()) && (relu == 0 || relu == 1) && !residual && !out_f32 && a.Kpad == Cin && (out_pix_stride & 7) == 0 &&
            c.out_aligned16 && out_extent < 0x7ffffff0ll && (long long)Cout * a.Kpad * 2 < 0x7ffffff0ll) {
            a.tiles_m = (a.M + 255) / 256; a.tiles_n = Cout / 256;
            // non-temporal result stores where the result is >= 4 x the input (256 -> 1024 168 -> 150 us, 512 -> 2048 402 -> 376;
            // 2 x and reducing layers lose 2-10 % with them: EXPERIMENTS R6-8).  OESS_W128_NT = 0 / 1 forces (A/B).
            static const int nt_env = [] { const char* e = getenv("OESS_W128_NT"); return e ? atoi(e) : -1; }();
            a.ksplit = nt_env >= 0 ? nt_env : (Cout >= 4 * Cin);
            return take(OESS_ROUTE_CONV1X1_W128, dim3(num_cus() / 8 * 8), dim3(256), (size_t)G128_LDS);
        }
        if (getenv("OESS_W128_WHY"))
            fprintf(stderr, "[oess] 1x1 %d -> %d M %d not on conv1x1_w128_kernel: t256 %lld bias %d relu %d residual %d out_f32 %d Kpad %d ops %lld align %d\n", Cin, Cout, a.M,
                    t256, bias, relu, residual, out_f32, a.Kpad, (long long)out_pix_stride, c.out_aligned16 ? 0 : 1);
        if (t256 >= 400) {
            a.tiles_m = (a.M + 255) / 256; a.tiles_n = Cout / 256;
            size_t lds = (size_t)2 * 512 * 128;                                          // 2 stages x (256 + 256) rows x 128 B
            const size_t epi256 = (size_t)256 * (256 + 8) * 2 + (size_t)4 * 256 * 2 * 4 + 256;   // output image + BatchNorm partials
            if (lds < epi256) lds = epi256;
            return take(OESS_ROUTE_TILE256, dim3(a.tiles_m * a.tiles_n), dim3(512), lds);
        }
    }
    // (4) short reductions (K <= 256, the 1x1 bottleneck convs): a workgroup lives ~6 us of which the K loop is a fraction, so
    //     residency matters more than the main loop: BK = 32 slabs in a 3-deep ring = 48 KB -> 3 workgroups per CU
    //     (K = 64: 0.121 -> 0.096 ms, K = 256: 0.0414 -> 0.0369 ms; from K = 512 up the BK = 64 kernel wins again)
    if (bn == 128 && fastk32 && a.Kpad <= 256) {
        size_t lds3 = (size_t)3 * (BM + 128) * 64;
        if (lds3 < epi) lds3 = epi;
        return take(OESS_ROUTE_RING32, grid, block, lds3);
    }
    // (5) 64 x 128 tiles (48 KB of LDS: 3 workgroups per CU) when the 128-row tiling leaves most of its last round of
    //     workgroups empty: e.g. 550 tiles over 512 slots run as two rounds at 54 % - 1100 half tiles over 768 slots do not
    if (want64) {
        a.tiles_m = (a.M + 63) / 64;
        size_t lds = (size_t)2 * (64 + 128) * 8 * 16;
        const size_t epi64 = (size_t)64 * (128 + 8) * 2 + 4096;
        if (lds < epi64) lds = epi64;
        return take(fastk ? OESS_ROUTE_TILE64_FASTK : OESS_ROUTE_TILE64_SLOWK, dim3(a.tiles_m * a.tiles_n), block, lds);
    }
    // (6) the general LDS-DMA kernel: 128 x {128, 64, 32} tiles, 2-stage ring, 2 workgroups per CU
    size_t lds = (size_t)2 * (BM + bn) * 8 * 16;
    if (lds < epi) lds = epi;
    return take((bn == 128 ? OESS_ROUTE_DMA128_FASTK : (bn == 64 ? OESS_ROUTE_DMA64_FASTK : OESS_ROUTE_DMA32_FASTK)) + (fastk ? 0 : 1), grid, block, lds);
}

// plan.args with the call's pointers in place (a ConvLSTM call's a.out is its hidden output; the conv epilogue is not used)
ConvArgs conv_bind(const ConvPlan& p, const ConvPtrs& q) {
    ConvArgs a = p.args;
    a.in = (const uint16_t*)q.in; a.w = (const uint16_t*)q.w; a.bias = q.bias;
    a.out = q.out_f32 ? nullptr : (uint16_t*)(a.lstm_C ? q.lstm_h : q.out_bf16); a.out_f32 = q.out_f32;
    a.residual = (const uint16_t*)q.residual;
    a.stats = q.tile_stats;
    a.lstm_prev = q.lstm_prev; a.lstm_cell = q.lstm_cell; a.lstm_h = (uint16_t*)q.lstm_h;
    a.partial = OESS_ROUTE_KSPLIT(p.route) ? (float*)q.workspace : nullptr;
    return a;
}

// The one place that names the kernels for launching: one case per OESS_ROUTE_* value.
int conv_launch(const ConvPlan& p, const ConvPtrs& q, oess_stream_t stream) {
    conv_set_attrs();
    const ConvArgs a = conv_bind(p, q);
    hipStream_t st = (hipStream_t)stream;
#define OESS_CASE(route_, ...) case route_: hipLaunchKernelGGL((__VA_ARGS__), p.grid, p.block, p.lds, st, a); break;
    switch (OESS_ROUTE_KERNEL(p.route)) {
        OESS_CASE(OESS_ROUTE_SMALLCIN, conv_smallcin_kernel<5, 5>)
        OESS_CASE(OESS_ROUTE_FALLBACK_128, conv_fwd_kernel<128>)
        OESS_CASE(OESS_ROUTE_FALLBACK_64, conv_fwd_kernel<64>)
        OESS_CASE(OESS_ROUTE_FALLBACK_32, conv_fwd_kernel<32>)
        case OESS_ROUTE_S2_HALO: hipLaunchKernelGGL((conv5x5s2_halo_kernel<false>), p.grid, p.block, p.lds, st, a, S2Head{}); break;
        OESS_CASE(OESS_ROUTE_SMALLMAP_RING, conv_fwd_dma_kernel<128, 128, 4, true, 0, 512>)
        OESS_CASE(OESS_ROUTE_CONV3X3_W128, conv3x3_w128_kernel)
        OESS_CASE(OESS_ROUTE_HALO3X3, conv3x3_halo_kernel<0>)
        OESS_CASE(OESS_ROUTE_HALO3X3_LSTM, conv3x3_halo_kernel<1>)
        OESS_CASE(OESS_ROUTE_LSTM_FASTK, conv_fwd_dma_kernel<128, 128, 2, true, 1>)
        OESS_CASE(OESS_ROUTE_LSTM_SLOWK, conv_fwd_dma_kernel<128, 128, 2, false, 1>)
        OESS_CASE(OESS_ROUTE_SPLITK_FASTK, conv_fwd_dma_kernel<128, 128, 2, true>)        // (+ the reduce below)
        OESS_CASE(OESS_ROUTE_SPLITK_SLOWK, conv_fwd_dma_kernel<128, 128, 2, false>)
        OESS_CASE(OESS_ROUTE_CONV1X1_W128, conv1x1_w128_kernel<true>)
        OESS_CASE(OESS_ROUTE_TILE256, conv_fwd_dma_kernel<256, 256, 2, true>)
        OESS_CASE(OESS_ROUTE_RING32, conv_fwd_dma32_kernel<128, true, 0, 3>)
        OESS_CASE(OESS_ROUTE_TILE64_FASTK, conv_fwd_dma_kernel<64, 128, 2, true>)
        OESS_CASE(OESS_ROUTE_TILE64_SLOWK, conv_fwd_dma_kernel<64, 128, 2, false>)
        OESS_CASE(OESS_ROUTE_DMA128_FASTK, conv_fwd_dma_kernel<128, 128, 2, true>)
        OESS_CASE(OESS_ROUTE_DMA128_SLOWK, conv_fwd_dma_kernel<128, 128, 2, false>)
        OESS_CASE(OESS_ROUTE_DMA64_FASTK, conv_fwd_dma_kernel<128, 64, 2, true>)
        OESS_CASE(OESS_ROUTE_DMA64_SLOWK, conv_fwd_dma_kernel<128, 64, 2, false>)
        OESS_CASE(OESS_ROUTE_DMA32_FASTK, conv_fwd_dma_kernel<128, 32, 2, true>)
        OESS_CASE(OESS_ROUTE_DMA32_SLOWK, conv_fwd_dma_kernel<128, 32, 2, false>)
        default: return OESS_EINVAL;
    }
#undef OESS_CASE
    if (OESS_ROUTE_KSPLIT(p.route)) hipLaunchKernelGGL(splitk_reduce_kernel, dim3(a.tiles_m, (a.Cout + 63) / 64), dim3(256), 0, st, a);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

ConvCall conv_call(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dil, int relu, bool has_bias, bool has_residual, bool out_is_f32,
                   bool with_tile_stats, bool out_aligned16, long long in_pix_stride, long long out_pix_stride, long long res_pix_stride, size_t workspace_bytes) {
    return ConvCall{B, H, W, Cin, Cout, R, S, stride, pad, dil, relu, has_bias, has_residual, out_is_f32, with_tile_stats, out_aligned16,
                    in_pix_stride, out_pix_stride, res_pix_stride, 0, 0, workspace_bytes};
}
ConvCall lstm_call(int B, int H, int W, int Cin, long long in_pix_stride, int C_hidden, int R, int S, int pad, long long hidden_pix_stride) {
    ConvCall c = conv_call(B, H, W, Cin, 4 * C_hidden, R, S, 1, pad, 1, 0, false, false, false, false, true, in_pix_stride, 0, 0, 0);
    c.C_hidden = C_hidden; c.hidden_pix_stride = hidden_pix_stride;
    return c;
}
// Grouped ConvLSTM launches run their problems concurrently: true when an output of one problem (hidden state, cell state)
// overlaps an input or an output of another, or a problem's hidden output its own input (the single-problem rule).  tiled_cell:
// the cell is in the w128 kernel's padded layout (oess_convlstm_w128_cell_bytes), and must not overlap its own input either.
bool lstm_group_overlap(const oess_convlstm_desc_t* d, int n, bool tiled_cell) {
    auto span = [](const void* p, long long pixels, long long stride, int c, const char** lo, const char** hi) {
        *lo = (const char*)p; *hi = *lo + (pixels - 1) * stride * 2 + (long long)c * 2;
    };
    auto cell_bytes = [tiled_cell](long long px, int C) { return tiled_cell ? (long long)oess_convlstm_w128_cell_bytes(px, C) : px * C * 4; };
    for (int i = 0; i < n; ++i) {
        const long long px = (long long)d[i].B * d[i].H * d[i].W;
        const char *h0, *h1, *c0 = (const char*)d[i].cell, *c1 = c0 + cell_bytes(px, d[i].C_hidden);
        span(d[i].hidden, px, d[i].hidden_pix_stride, d[i].C_hidden, &h0, &h1);
        for (int j = 0; j < n; ++j) {
            const long long pj = (long long)d[j].B * d[j].H * d[j].W;
            const char *i0, *i1, *g0, *g1, *e0 = (const char*)d[j].cell, *e1 = e0 + cell_bytes(pj, d[j].C_hidden);
            span(d[j].in, pj, d[j].in_pix_stride, d[j].Cin, &i0, &i1);
            span(d[j].hidden, pj, d[j].hidden_pix_stride, d[j].C_hidden, &g0, &g1);
            if (h0 < i1 && i0 < h1) return true;
            if ((j != i || tiled_cell) && c0 < i1 && i0 < c1) return true;
            if (j != i && ((h0 < g1 && g0 < h1) || (c0 < e1 && e0 < c1))) return true;
        }
    }
    return false;
}
// the row-halo ConvLSTM kernel's arguments for one problem of a grouped launch; false when the problem's plan is another kernel
bool lstm_group_args(const oess_convlstm_desc_t& d, ConvArgs* a) {
    ConvPlan p;
    if (!d.w_packed_gates ||            // (the callers have checked the other pointers)
        conv_plan(lstm_call(d.B, d.H, d.W, d.Cin, d.in_pix_stride, d.C_hidden, d.R, d.S, d.pad, d.hidden_pix_stride), &p) != OESS_OK ||
        p.route != OESS_ROUTE_HALO3X3_LSTM)
        return false;
    *a = conv_bind(p, ConvPtrs{d.in, d.w_packed_gates, d.bias, nullptr, nullptr, nullptr, nullptr, d.prev_cell, d.cell, d.hidden, nullptr});
    return true;
}
bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
}  // namespace

extern "C" {

int oess_conv2d_fwd_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int Cin, const void* w_packed,
                         const float* bias, int Cout, int R, int S, int stride, int pad, int dil, int relu,
                         const void* residual, long long res_pix_stride, void* out_bf16, float* out_f32,
                         long long out_pix_stride, float* tile_stats, void* workspace, size_t workspace_bytes,
                         oess_stream_t stream) {
    if (!in || !w_packed || (!out_bf16 && !out_f32)) return OESS_EINVAL;
    ConvPlan p;
    const int rc = conv_plan(conv_call(B, H, W, Cin, Cout, R, S, stride, pad, dil, relu, bias, residual, out_f32, tile_stats, aligned16(out_bf16),
                                       in_pix_stride, out_pix_stride, res_pix_stride, workspace ? workspace_bytes : 0), &p);
    if (rc != OESS_OK) return rc;
    return conv_launch(p, ConvPtrs{in, w_packed, bias, residual, out_bf16, out_f32, tile_stats, nullptr, nullptr, nullptr, workspace}, stream);
}

int oess_conv2d_stats_only_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int Cin, const void* w_packed, int Cout,
                                float* tile_stats, oess_stream_t stream) {
    if (!in || !w_packed || !tile_stats) return OESS_EINVAL;
    // the plan of the storing call with a dense, aligned output: only where that is the w128 GEMM does the store-free form exist
    ConvPlan p;
    const int rc = conv_plan(conv_call(B, H, W, Cin, Cout, 1, 1, 1, 0, 1, 0, false, false, false, true, true, in_pix_stride, Cout, 0, 0), &p);
    if (rc != OESS_OK) return rc;
    if (p.route != OESS_ROUTE_CONV1X1_W128) return OESS_EINVAL;
    conv_set_attrs();
    const ConvArgs a = conv_bind(p, ConvPtrs{in, w_packed, nullptr, nullptr, nullptr, nullptr, tile_stats, nullptr, nullptr, nullptr, nullptr});
    hipLaunchKernelGGL((conv1x1_w128_kernel<false>), p.grid, p.block, p.lds, (hipStream_t)stream, a);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

size_t oess_conv2d_fwd_workspace_bytes(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dil,
                                       int with_tile_stats, int out_is_f32) {
    // the plan of oess_conv2d_fwd_bf16 with any workspace on offer.  The query has no strides, pointers or epilogue flags, so it
    // assumes a dense input, an output of pixel stride ceil8(Cout) at a 16-byte aligned address, and no bias / ReLU / residual
    // (what the dummy call of the earlier implementation amounted to)
    ConvPlan p;
    const int rc = conv_plan(conv_call(B, H, W, Cin, Cout, R, S, stride, pad, dil, 0, false, false, out_is_f32, with_tile_stats, true, Cin,
                                       (Cout + 7) / 8 * 8, 0, ~(size_t)0), &p);
    return rc == OESS_OK ? p.want_workspace : 0;
}

int oess_conv2d_fwd_route(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dil, int has_bias,
                          int relu, int has_residual, int out_is_f32, int with_tile_stats, long long in_pix_stride,
                          long long out_pix_stride, long long res_pix_stride, int out_aligned16, size_t workspace_bytes) {
    ConvPlan p;         // the plan the launch itself executes
    const int rc = conv_plan(conv_call(B, H, W, Cin, Cout, R, S, stride, pad, dil, relu, has_bias, has_residual, out_is_f32, with_tile_stats,
                                       out_aligned16, in_pix_stride, out_pix_stride, res_pix_stride, workspace_bytes), &p);
    return rc == OESS_OK ? p.route : rc;
}

int oess_convlstm_fused_route(int B, int H, int W, int Cin, long long in_pix_stride, int C_hidden, int R, int S, int pad,
                              long long hidden_pix_stride) {
    ConvPlan p;
    const int rc = conv_plan(lstm_call(B, H, W, Cin, in_pix_stride, C_hidden, R, S, pad, hidden_pix_stride), &p);
    return rc == OESS_OK ? p.route : rc;
}

int oess_conv2d_route_count(void) { return OESS_ROUTE_COUNT; }

const char* oess_conv2d_route_name(int route) {
    static const char* const names[OESS_ROUTE_COUNT + 1] = {
        "?", "conv_smallcin_kernel<5, 5>", "conv_fwd_kernel<128>", "conv_fwd_kernel<64>", "conv_fwd_kernel<32>",
        "conv5x5s2_halo_kernel<false>", "conv_fwd_dma_kernel<128, 128, 4, true, 0, 512>", "conv3x3_w128_kernel",
        "conv3x3_halo_kernel<0>", "conv3x3_halo_kernel<1>", "conv_fwd_dma_kernel<128, 128, 2, true, 1>",
        "conv_fwd_dma_kernel<128, 128, 2, false, 1>", "split-K conv_fwd_dma_kernel<128, 128, 2, true> + splitk_reduce_kernel",
        "split-K conv_fwd_dma_kernel<128, 128, 2, false> + splitk_reduce_kernel", "conv1x1_w128_kernel",
        "conv_fwd_dma_kernel<256, 256, 2, true>", "conv_fwd_dma32_kernel<128, true, 0, 3>", "conv_fwd_dma_kernel<64, 128, 2, true>",
        "conv_fwd_dma_kernel<64, 128, 2, false>", "conv_fwd_dma_kernel<128, 128, 2, true>", "conv_fwd_dma_kernel<128, 128, 2, false>",
        "conv_fwd_dma_kernel<128, 64, 2, true>", "conv_fwd_dma_kernel<128, 64, 2, false>", "conv_fwd_dma_kernel<128, 32, 2, true>",
        "conv_fwd_dma_kernel<128, 32, 2, false>"};
    const int k = OESS_ROUTE_KERNEL(route);        // a split-K slice count in the upper bits does not change the name
    return route > 0 && k >= 1 && k <= OESS_ROUTE_COUNT ? names[k] : names[0];
}

int oess_convlstm_fused_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int Cin, const void* w_packed_gates,
                             const float* bias, int C_hidden, int R, int S, int pad, const float* prev_cell, float* cell,
                             void* hidden, long long hidden_pix_stride, oess_stream_t stream) {
    if (!in || !hidden || !w_packed_gates || !cell) return OESS_EINVAL;
    {   // the hidden output must not alias the convolution input (neighbouring tiles still read the old state)
        const char* i0 = (const char*)in; const char* i1 = i0 + ((long long)B * H * W - 1) * in_pix_stride * 2 + (long long)Cin * 2;
        const char* h0 = (const char*)hidden; const char* h1 = h0 + ((long long)B * H * W - 1) * hidden_pix_stride * 2 + (long long)C_hidden * 2;
        if (h0 < i1 && i0 < h1) return OESS_EINVAL;
    }
    ConvPlan p;
    const int rc = conv_plan(lstm_call(B, H, W, Cin, in_pix_stride, C_hidden, R, S, pad, hidden_pix_stride), &p);
    if (rc != OESS_OK) return rc;
    return conv_launch(p, ConvPtrs{in, w_packed_gates, bias, nullptr, nullptr, nullptr, nullptr, prev_cell, cell, hidden, nullptr}, stream);
}

int oess_convlstm_fused_group_bf16(const oess_convlstm_desc_t* d, int n, oess_stream_t stream) {
    if (!d || n <= 0 || n > 3) return OESS_EINVAL;
    for (int i = 0; i < n; ++i)
        if (!d[i].in || !d[i].hidden || !d[i].cell || d[i].B <= 0 || d[i].H <= 0 || d[i].W <= 0) return OESS_EINVAL;
    if (lstm_group_overlap(d, n, false)) return OESS_EINVAL;
    // one launch iff every problem's own plan is the row-halo kernel; otherwise the problems go one by one, each on its plan's route
    ConvArgs args[3];
    bool grouped = n >= 2;
    for (int i = 0; i < n && grouped; ++i) grouped = lstm_group_args(d[i], &args[i]);
    if (!grouped) {
        for (int i = 0; i < n; ++i) {
            const int rc = oess_convlstm_fused_bf16(d[i].in, d[i].in_pix_stride, d[i].B, d[i].H, d[i].W, d[i].Cin, d[i].w_packed_gates,
                                                    d[i].bias, d[i].C_hidden, d[i].R, d[i].S, d[i].pad, d[i].prev_cell, d[i].cell,
                                                    d[i].hidden, d[i].hidden_pix_stride, stream);
            if (rc != OESS_OK) return rc;
        }
        return OESS_OK;
    }
    conv_set_attrs();
    int order[3] = {0, 1, 2};                  // longest K first: the launch ends on the short tiles
    for (int i = 1; i < n; ++i)
        for (int j = i; j > 0 && args[order[j]].Kpad > args[order[j - 1]].Kpad; --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
    ConvGroup g;
    memset(&g, 0, sizeof(g));
    int at = 0;
    for (int i = 0; i < 3; ++i) {
        g.start8[i] = at;
        if (i < n) {
            g.a[i] = args[order[i]];
            at += (g.a[i].tiles_m * g.a[i].tiles_n + 7) / 8;
        }
    }
    g.start8[3] = at;
    // 256 x 128 tiles on ONE 8-wave workgroup per CU (default since round 5).  Alone the grouped launch is 2-3 % slower on them
    // than on two 128 x 128 workgroups per CU (one workgroup per CU exposes the cell-update epilogue; fewer operand bytes per FLOP
    // buy nothing), but the product schedule runs it next to the teacher's and the decoder's kernels, and one 112 KB workgroup
    // leaves them 48 KB of LDS and 24 wave slots per CU where two 72 KB workgroups leave 16 KB: +1.4-1.6 % on the step on three
    // boxes (EXPERIMENTS R5-3b).  OESS_LSTM256 = 0 restores the 128 x 128 tiles (A/B), 2 = only the problems with >= 30 K-slabs.
    static const int use256 = [] { const char* e = getenv("OESS_LSTM256"); return e ? atoi(e) : 1; }();
    if (use256) {
        ConvGroup big, small;
        memset(&big, 0, sizeof(big)); memset(&small, 0, sizeof(small));
        int nb = 0, ns = 0;
        for (int i = 0; i < n; ++i) {
            const ConvArgs& a = g.a[i];
            const bool fits = a.R == 3 && a.dil == 1 && (a.dil + 255 + a.dil * ((256 + a.W - 2) / a.W) + a.dil + 1) <= HALO_ROWS_256 &&
                              a.tiles_n * 128 == a.Cout;
            if (fits && (use256 == 1 || a.Kpad / BK >= 30)) big.a[nb++] = a; else small.a[ns++] = a;
        }
        auto layout = [](ConvGroup& q, int cnt, int rows) {
            int at_ = 0;
            for (int i = 0; i < 3; ++i) {
                q.start8[i] = at_;
                if (i < cnt) {
                    q.a[i].tiles_m = (q.a[i].M + rows - 1) / rows;
                    at_ += (q.a[i].tiles_m * q.a[i].tiles_n + 7) / 8;
                }
            }
            q.start8[3] = at_;
            return at_;
        };
        if (nb) {
            const int atb = layout(big, nb, 256);
            const size_t lds256 = (size_t)2 * HALO_ROWS_256 * 128 + (size_t)2 * 128 * 128;
            hipLaunchKernelGGL(conv3x3_halo256_group_kernel, dim3(8 * atb), dim3(512), lds256, (hipStream_t)stream, big);
        }
        if (ns) {
            const int ats = layout(small, ns, 128);
            const size_t lds128 = (size_t)2 * HALO_ROWS * 128 + (size_t)2 * 128 * 128;
            hipLaunchKernelGGL((conv3x3_halo_group_kernel<1>), dim3(8 * ats), dim3(CONV_THREADS), lds128, (hipStream_t)stream, small);
        }
        OESS_HIP(hipGetLastError());
        return OESS_OK;
    }
    const size_t lds = (size_t)2 * HALO_ROWS * 128 + (size_t)2 * 128 * 128;
    hipLaunchKernelGGL((conv3x3_halo_group_kernel<1>), dim3(8 * at), dim3(CONV_THREADS), lds, (hipStream_t)stream, g);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"

// ---- ConvLSTM on 128 x 128 wave tiles with the cell state in the kernel's own layout (conv_lstm_w128.h)
namespace {
struct W128Sched { int* dev; int stride; int grid; };
// Static tile lists: workgroup b (one per CU; XCD b % 8 by the dispatch order, used for locality only) takes tiles of "its" XCD's
// contiguous chunk of every problem -- neighbouring tiles share halo rows and weight slabs in that XCD's L2, as in the one-tile
// kernels -- dealt longest-K first onto the least loaded of the XCD's workgroups (cost = slabs x measured cycles per slab + a
// per-tile constant), i.e. what a dynamic queue would do, without an atomic and a reset per launch.
// pure host part: flat[grid][stride] tile lists ((problem << 24) | tile, -1 = end), every tile of every problem exactly once
static int w128_tile_lists(const ConvArgs* a, int n, int grid, std::vector<int>* flat, int* stride_out) {
    if (grid < 8 || grid % 8) return OESS_EINVAL;
    const int per = grid / 8;
    std::vector<std::vector<int>> lists(grid);
    std::vector<long long> load(grid, 0);
    for (int x = 0; x < 8; ++x)
        for (int p = 0; p < n; ++p) {
            const int nwg = a[p].tiles_m * a[p].tiles_n, q = nwg >> 3, r = nwg & 7;
            const int cnt = q + (x < r ? 1 : 0), base = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
            const long long cost = (long long)(a[p].Cin / 64) * 9 * 2330 + 20000;     // measured: cycles per K-slab, per-tile set-up + cell update (profiles/r06_w128_v2_stamps.txt)
            for (int li = 0; li < cnt; ++li) {
                int best = 0;
                for (int c = 1; c < per; ++c) if (load[c * 8 + x] < load[best * 8 + x]) best = c;
                lists[best * 8 + x].push_back((p << 24) | (base + li));
                load[best * 8 + x] += cost;
            }
        }
    size_t longest = 0;
    for (auto& l : lists) longest = l.size() > longest ? l.size() : longest;
    if (longest > (size_t)W128_MAX_LIST) return OESS_EINVAL;
    const int stride = (int)longest + 1;
    flat->assign((size_t)grid * stride, -1);
    for (int b = 0; b < grid; ++b) for (size_t k = 0; k < lists[b].size(); ++k) (*flat)[(size_t)b * stride + k] = lists[b][k];
    *stride_out = stride;
    return OESS_OK;
}
static int w128_schedule(const ConvArgs* a, int n, W128Sched* out) {
    static std::mutex mu;
    static std::map<std::vector<int>, W128Sched> cache;
    std::vector<int> key;
    // OESS_W128_GRID (A/B): fewer persistent workgroups than CUs leaves whole CUs to the kernels of the other streams of the product
    // schedule (a 152 KB / 512-register workgroup shares its CU with nothing)
    static const int grid_env = [] { const char* e = getenv("OESS_W128_GRID"); return e ? atoi(e) : 0; }();
    const int grid = (grid_env >= 8 && grid_env <= num_cus()) ? grid_env / 8 * 8 : num_cus();
    int dev = 0;
    (void)hipGetDevice(&dev);
    key.push_back(dev);                        // the list lives in this device's memory
    key.push_back(grid);
    for (int i = 0; i < n; ++i) { key.push_back(a[i].tiles_m); key.push_back(a[i].tiles_n); key.push_back(a[i].Cin); }
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) { *out = it->second; return OESS_OK; }
    std::vector<int> flat;
    int stride = 0;
    if (w128_tile_lists(a, n, grid, &flat, &stride) != OESS_OK) return OESS_EINVAL;
    W128Sched sc{nullptr, stride, grid};
    if (hipMalloc((void**)&sc.dev, flat.size() * sizeof(int) + (size_t)grid * 4 * 16 * sizeof(float)) != hipSuccess) return OESS_ELAUNCH;
    if (hipMemcpy(sc.dev, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return OESS_ELAUNCH;
    cache[key] = sc;
    *out = sc;
    return OESS_OK;
}
}  // namespace

extern "C" {
int oess_convlstm_w128_tile_lists(const int* tiles_m, const int* tiles_n, const int* cin, int n, int grid, int* lists, int capacity, int* stride) {
    if (!tiles_m || !tiles_n || !cin || !stride || n <= 0 || n > 3) return OESS_EINVAL;
    ConvArgs a[3];
    memset(a, 0, sizeof(a));
    for (int i = 0; i < n; ++i) { a[i].tiles_m = tiles_m[i]; a[i].tiles_n = tiles_n[i]; a[i].Cin = cin[i]; }
    std::vector<int> flat;
    const int rc = w128_tile_lists(a, n, grid, &flat, stride);
    if (rc != OESS_OK) return rc;
    if (lists) {
        if ((size_t)capacity < flat.size()) return OESS_ENOMEM;
        memcpy(lists, flat.data(), flat.size() * sizeof(int));
    }
    return OESS_OK;
}

size_t oess_convlstm_w128_cell_bytes(long long pixels, int C_hidden) {
    if (pixels <= 0 || C_hidden <= 0 || (C_hidden & 63)) return 0;
    return (size_t)((pixels + 255) / 256 * 256) * (size_t)C_hidden * 4;
}

int oess_convlstm_w128_cell_relayout(const float* src, float* dst, long long pixels, int C_hidden, int to_tiled, oess_stream_t stream) {
    if (!src || !dst || src == dst || pixels <= 0 || C_hidden <= 0 || (C_hidden & 63)) return OESS_EINVAL;
    const long long total = (pixels + 255) / 256 * 256 * C_hidden;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(w128_cell_relayout_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, dst, pixels, C_hidden, to_tiled);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_convlstm_w128_group_bf16(const oess_convlstm_desc_t* d, int n, oess_stream_t stream) {
    if (!d || n <= 0 || n > 3) return OESS_EINVAL;
    int ctot = 0;
    for (int i = 0; i < n; ++i) {
        if (!d[i].in || !d[i].hidden || !d[i].cell || d[i].B <= 0 || d[i].H < 8 || d[i].W <= 0 || d[i].R != 3 || d[i].S != 3 || d[i].pad != 1 ||
            d[i].C_hidden <= 0 || (d[i].C_hidden & 63) || d[i].Cin <= 0 || (d[i].Cin & 63))
            return OESS_EINVAL;
        ctot += 4 * d[i].C_hidden;
        const long long px = (long long)d[i].B * d[i].H * d[i].W;
        const size_t cb = oess_convlstm_w128_cell_bytes(px, d[i].C_hidden);
        if (cb >= 0x7fffffffull || px * d[i].W >= 0x100000000ll) return OESS_EINVAL;
        if (d[i].prev_cell && d[i].prev_cell != d[i].cell) {
            const char *p0 = (const char*)d[i].prev_cell, *c0 = (const char*)d[i].cell;
            if (p0 < c0 + cb && c0 < p0 + cb) return OESS_EINVAL;         // a tile updates its own block in place or elsewhere, not a shifted copy
        }
        if ((px - 1) * d[i].hidden_pix_stride * 2 + (long long)d[i].C_hidden * 2 >= 0x7fffffffll) return OESS_EINVAL;
    }
    if (lstm_group_overlap(d, n, true)) return OESS_EINVAL;
    if (ctot > W128_BIAS_FLOATS) return OESS_EINVAL;
    ConvArgs args[3];
    for (int i = 0; i < n; ++i) {
        if (!lstm_group_args(d[i], &args[i])) return OESS_EINVAL;
        ConvArgs& a = args[i];
        // halo rows of a 256-pixel tile; a tile may wrap into the next image at most once (rows per tile <= H)
        if (a.Kpad != 9 * a.Cin || (1 + 255 + ((256 + a.W - 2) / a.W) + 1 + 1) > W128_HROWS || ((256 + a.W - 2) / a.W + 1) > a.H || !a.mg_w || !a.mg_wd)
            return OESS_EINVAL;
        a.tiles_m = (a.M + 255) / 256;
        a.tiles_n = a.Cout / 256;
    }
    conv_set_attrs();
    int order[3] = {0, 1, 2};                  // longest K first
    for (int i = 1; i < n; ++i)
        for (int j = i; j > 0 && args[order[j]].Kpad > args[order[j - 1]].Kpad; --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
    W128Group g;
    memset(&g, 0, sizeof(g));
    for (int i = 0; i < n; ++i) g.a[i] = args[order[i]];
    g.n = n;
    W128Sched sc;
    const int rc = w128_schedule(g.a, n, &sc);
    if (rc != OESS_OK) return rc;
    g.sched = sc.dev; g.sched_stride = sc.stride;
    hipLaunchKernelGGL(conv3x3_lstm_w128_kernel, dim3(sc.grid), dim3(256), (size_t)W128_LDS, (hipStream_t)stream, g);
    OESS_HIP(hipGetLastError());
#if (W128_ABL & 8192)
    {
        std::vector<float> st((size_t)sc.grid * 64);
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(st.data(), sc.dev + (size_t)sc.grid * sc.stride, st.size() * 4, hipMemcpyDeviceToHost);
        double sum[16] = {0};
        for (int b = 0; b < sc.grid; ++b) for (int k = 0; k < 16; ++k) sum[k] += st[((size_t)b * 4) * 16 + k];
        fprintf(stderr, "w128 stamps (wave 0, cycles per workgroup, mean of %d): dx0 G0..G3 | dx1 | dx2 | setup+fill-issue  first-operand-wait  cell-update  tiles\n  ", sc.grid);
        double loop = 0;
        for (int k = 0; k < 12; ++k) { fprintf(stderr, "%9.0f%s", sum[k] / sc.grid, (k & 3) == 3 ? " |" : ""); loop += sum[k] / sc.grid; }
        fprintf(stderr, " %9.0f %9.0f %9.0f %5.1f   loop %9.0f\n", sum[12] / sc.grid, sum[13] / sc.grid, sum[14] / sc.grid, sum[15] / sc.grid, loop);
        double mn = 1e30, mx = 0, mean = 0;
        for (int b = 0; b < sc.grid; ++b) {
            double t = 0;
            for (int k = 0; k < 15; ++k) t += st[((size_t)b * 4) * 16 + k];
            mn = t < mn ? t : mn; mx = t > mx ? t : mx; mean += t / sc.grid;
        }
        fprintf(stderr, "  stamped cycles per workgroup: min %.0f mean %.0f max %.0f\n", mn, mean, mx);
    }
#endif
    return OESS_OK;
}
}  // extern "C"

extern "C" {
int oess_conv5x5s2_group_bf16(const oess_conv_s2_desc_t* d, int n, oess_stream_t stream) {
    if (!d || n <= 0 || n > 2) return OESS_EINVAL;
    for (int i = 0; i < n; ++i)
        if (!d[i].in || !d[i].w_packed || !d[i].out || d[i].B <= 0 || d[i].H <= 0 || d[i].W <= 0) return OESS_EINVAL;
    if (n == 2) {       // the problems run concurrently: neither output may overlap the other's input or output
        const char *lo[2][2], *hi[2][2];
        long long st[2][2], cb[2][2];                      // pixel stride and channel bytes of {in, out}
        for (int i = 0; i < 2; ++i) {
            const long long pin = (long long)d[i].B * d[i].H * d[i].W;
            const long long pout = (long long)d[i].B * ((d[i].H - 1) / 2 + 1) * ((d[i].W - 1) / 2 + 1);
            st[i][0] = d[i].in_pix_stride * 2; cb[i][0] = (long long)d[i].Cin * 2;
            st[i][1] = d[i].out_pix_stride * 2; cb[i][1] = (long long)d[i].Cout * 2;
            lo[i][0] = (const char*)d[i].in; hi[i][0] = lo[i][0] + (pin - 1) * st[i][0] + cb[i][0];
            lo[i][1] = (const char*)d[i].out; hi[i][1] = lo[i][1] + (pout - 1) * st[i][1] + cb[i][1];
        }
        for (int i = 0; i < 2; ++i)
            for (int k = 0; k < 2; ++k) {
                if (!(lo[i][1] < hi[1 - i][k] && lo[1 - i][k] < hi[i][1])) continue;
                // overlapping spans are fine when the two views are disjoint CHANNEL SLICES of one pixel grid (the x half and
                // the h half of a ConvLSTM cat(x, h) buffer): same pixel stride S, offsets differing by delta (mod S) with
                // delta >= bytes of the first and delta + bytes of the second <= S
                const long long S = st[i][1];
                if (S != st[1 - i][k] || S <= 0) return OESS_EINVAL;
                const long long diff = (long long)(lo[1 - i][k] - lo[i][1]);
                const long long delta = ((diff % S) + S) % S;
                if (!(delta >= cb[i][1] && delta + cb[1 - i][k] <= S)) return OESS_EINVAL;
            }
    }
    // one launch iff both problems' own plans are the stride-2 halo kernel; otherwise each goes alone on its plan's route
    ConvPlan plan[2];
    ConvPtrs q[2];
    int rc[2];
    bool grouped = n == 2;
    for (int i = 0; i < n; ++i) {
        q[i] = ConvPtrs{d[i].in, d[i].w_packed, d[i].bias, nullptr, d[i].out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        rc[i] = conv_plan(conv_call(d[i].B, d[i].H, d[i].W, d[i].Cin, d[i].Cout, 5, 5, 2, 2, 1, d[i].relu, d[i].bias, false, false, false,
                                    aligned16(d[i].out), d[i].in_pix_stride, d[i].out_pix_stride, 0, 0), &plan[i]);
        grouped = grouped && rc[i] == OESS_OK && plan[i].route == OESS_ROUTE_S2_HALO;
    }
    if (!grouped) {
        for (int i = 0; i < n; ++i) {
            const int r = rc[i] != OESS_OK ? rc[i] : conv_launch(plan[i], q[i], stream);
            if (r != OESS_OK) return r;
        }
        return OESS_OK;
    }
    conv_set_attrs();
    S2Group g;
    memset(&g, 0, sizeof(g));
    const int first = plan[1].args.Cin > plan[0].args.Cin ? 1 : 0;           // longest K first
    g.a[0] = conv_bind(plan[first], q[first]); g.a[1] = conv_bind(plan[1 - first], q[1 - first]);
    g.start8[0] = 0;
    g.start8[1] = (g.a[0].tiles_m * g.a[0].tiles_n + 7) / 8;
    g.start8[2] = g.start8[1] + (g.a[1].tiles_m * g.a[1].tiles_n + 7) / 8;
    hipLaunchKernelGGL(conv5x5s2_halo_group_kernel, dim3(8 * g.start8[2]), dim3(256), S2_LDS, (hipStream_t)stream, g);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

static int e2vid_head_enc0_launch(const S2Head& hd, int B, int H, int W, const void* enc_w_packed, const float* enc_bias, int enc_relu,
                                  void* out, long long out_pix_stride, oess_stream_t stream, const S2Pre* pre = nullptr) {
    conv_set_attrs();
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.w = (const uint16_t*)enc_w_packed; a.bias = enc_bias; a.out = (uint16_t*)out; a.out_pix_stride = out_pix_stride;
    a.B = B; a.H = H; a.W = W; a.Cin = 32; a.Cout = 64; a.R = 5; a.S = 5; a.stride = 2; a.pad = 2; a.dil = 1;
    a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1;
    a.Kpad = (25 * 32 + BK - 1) / BK * BK;
    a.M = B * a.Ho * a.Wo; a.relu = enc_relu;
    a.tiles_n = 1;
    a.tiles_m = s2_tiles_m(B, a.Ho, a.Wo);
    if (pre) hipLaunchKernelGGL(conv5x5s2_halo_pre_kernel, dim3(a.tiles_m), dim3(256), S2_LDS_FUSED, (hipStream_t)stream, a, hd, *pre);
    else hipLaunchKernelGGL((conv5x5s2_halo_kernel<true>), dim3(a.tiles_m), dim3(256), S2_LDS_FUSED, (hipStream_t)stream, a, hd);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

int oess_e2vid_events_head_enc0_bf16(const float* events, int B, int Ctot, int c0, int Cs, int H, int W, const double* stats,
                                     int normalize, const void* head_w_packed, const float* head_bias, int head_relu,
                                     const void* enc_w_packed, const float* enc_bias, int enc_relu, void* out,
                                     long long out_pix_stride, oess_stream_t stream) {
    if (!events || !head_w_packed || !enc_w_packed || !out || B <= 0 || H <= 0 || W <= 0 || Ctot <= 0 || c0 < 0 || Cs <= 0 ||
        Cs > 5 || c0 + Cs > Ctot || (normalize && !stats) || (out_pix_stride & 7) || out_pix_stride < 64 || (((uintptr_t)out) & 15) ||
        (unsigned)head_relu > 1u || (unsigned)enc_relu > 1u)
        return OESS_EINVAL;
    S2Head hd{nullptr, 8, (const uint16_t*)head_w_packed, head_bias, head_relu, events, Ctot, c0, Cs, normalize, stats};
    return e2vid_head_enc0_launch(hd, B, H, W, enc_w_packed, enc_bias, enc_relu, out, out_pix_stride, stream);
}

int oess_e2vid_events_head_enc0_pre_bf16(const float* events, int B, int Ctot, int c0, int Cs, int H, int W,
                                         const oess_event_pre_t* pre, const double* stats, int normalize,
                                         const void* head_w_packed, const float* head_bias, int head_relu,
                                         const void* enc_w_packed, const float* enc_bias, int enc_relu, void* out,
                                         long long out_pix_stride, oess_stream_t stream) {
    if (!events || !pre || !head_w_packed || !enc_w_packed || !out || B <= 0 || H <= 0 || W <= 0 || Ctot <= 0 || c0 < 0 || Cs <= 0 ||
        Cs > 5 || c0 + Cs > Ctot || (normalize && !stats) || (out_pix_stride & 7) || out_pix_stride < 64 || (((uintptr_t)out) & 15) ||
        (unsigned)head_relu > 1u || (unsigned)enc_relu > 1u)
        return OESS_EINVAL;
    S2Head hd{nullptr, 8, (const uint16_t*)head_w_packed, head_bias, head_relu, events, Ctot, c0, Cs, normalize, stats};
    const S2Pre sp{pre->hot_mask, pre->flip ? 1 : 0};
    return e2vid_head_enc0_launch(hd, B, H, W, enc_w_packed, enc_bias, enc_relu, out, out_pix_stride, stream, &sp);
}

int oess_e2vid_head_enc0_bf16(const void* x8, long long x8_pix_stride, int B, int H, int W, const void* head_w_packed,
                              const float* head_bias, int head_relu, const void* enc_w_packed, const float* enc_bias, int enc_relu,
                              void* out, long long out_pix_stride, oess_stream_t stream) {
    if (!x8 || !head_w_packed || !enc_w_packed || !out || B <= 0 || H <= 0 || W <= 0 || (x8_pix_stride & 7) || x8_pix_stride < 8 ||
        (out_pix_stride & 7) || out_pix_stride < 64 || (((uintptr_t)out) & 15) || (unsigned)head_relu > 1u || (unsigned)enc_relu > 1u)
        return OESS_EINVAL;
    if ((((long long)B * H * W - 1) * x8_pix_stride + 8) * 2 >= 0x7ffffff0ll) return OESS_EINVAL;     // 32-bit buffer offsets
    S2Head hd{(const uint16_t*)x8, x8_pix_stride, (const uint16_t*)head_w_packed, head_bias, head_relu, nullptr, 0, 0, 0, 0, nullptr};
    return e2vid_head_enc0_launch(hd, B, H, W, enc_w_packed, enc_bias, enc_relu, out, out_pix_stride, stream);
}

}  // extern "C"
