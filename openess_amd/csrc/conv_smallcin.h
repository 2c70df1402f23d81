// =================================================================================================
// Small-Cin convolution (Cin == 8: one 16-byte chunk per pixel, e.g. the E2VID head on the 5-bin voxel grid padded
// to 8 channels; stride 1, dilation 1, R*S <= 32 taps, Cout <= 32).
// As an implicit GEMM this layer is an im2col blow-up: every output pixel pulls R*S x 16 B through L2 -> LDS (400 B for
// 16 B of unique input at 5x5), and the generic kernel runs at the L2 gather rate.  Here a workgroup stages the input
// HALO tile ((8+R-1) x (64+S-1) pixels x 16 B, ~13 KB) in LDS once and the MFMA B-operand (pixels) is read straight
// out of it: lane p of k-step ks reads the chunk of pixel (ty + r, tx + s), (r, s) = tap ks*2 + (lane>>5).  Consecutive
// lanes read consecutive 16-byte chunks: conflict free.  The whole packed weight (32 x 256 bf16) lives in 64 VGPRs.
// The product is computed transposed (weights = MFMA A operand), so a lane owns 4 consecutive output channels of one
// pixel per register quad and stores them as 8-byte pieces.
// =================================================================================================
template <int R, int S>
__global__ __launch_bounds__(256, 2) void conv_smallcin_kernel(ConvArgs a) {
    // PERSISTENT over tiles: the weights are fetched once per workgroup, and the halo of the NEXT tile travels
    // HBM -> registers while the current tile is multiplied and stored, so a tile costs its LDS / MFMA / store work and
    // not a load round trip on top (one tile per workgroup measured 111 us for 180 MB of traffic: 3x the HBM time).
    constexpr int TH = 8, TW = 64, HW_ = TW + S - 1, HH_ = TH + R - 1, NTAP = R * S;
    constexpr int KS = (NTAP + 1) / 2;                       // k-steps of 16 = 2 taps; taps >= NTAP carry zero weights
    constexpr int OP = 36;                                   // output image pitch in elements (32 ch + 4: conflict-free 8-byte writes)
    constexpr int HALO_N = HH_ * HW_, HALO_BYTES = HALO_N * 16, IMG_BYTES = TH * TW * OP * 2;
    constexpr int HPT = (HALO_N + 255) / 256;                // halo chunks per thread
    __shared__ __attribute__((aligned(16))) unsigned char sm[HALO_BYTES + IMG_BYTES];
    u32x4_t* halo = reinterpret_cast<u32x4_t*>(sm);
    uint16_t* img = reinterpret_cast<uint16_t*>(sm + HALO_BYTES);
    const int tiles_x = (a.Wo + TW - 1) / TW, tiles_y = (a.Ho + TH - 1) / TH;
    const int ntiles = a.B * tiles_y * tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = lane & 31, hi = lane >> 5;

    // weights: lane (n = p, k-half = hi) keeps its fragments for the whole kernel
    bf16x8_t wf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
        wf[ks] = *reinterpret_cast<const bf16x8_t*>(a.w + (size_t)p * a.Kpad + (ks * 2 + hi) * 8);

    const u32x4_t zero4 = {0u, 0u, 0u, 0u};
    // halo of tile t -> registers (zero outside the image / beyond the tile list)
    auto fetch = [&](int t, u32x4_t (&h)[HPT]) {
        int bid = t;
        const int tx0 = (bid % tiles_x) * TW; bid /= tiles_x;
        const int ty0 = (bid % tiles_y) * TH;
        const int b = bid / tiles_y;
#pragma unroll
        for (int k = 0; k < HPT; ++k) {
            const int i = tid + k * 256;
            const int hy = i / HW_, hx = i - hy * HW_;
            const int iy = ty0 - a.pad + hy, ix = tx0 - a.pad + hx;
            h[k] = zero4;
            if (t < ntiles && i < HALO_N && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                h[k] = *reinterpret_cast<const u32x4_t*>(a.in + (((long long)b * a.H + iy) * a.W + ix) * a.in_pix_stride);
        }
    };
    const int cchunks = (a.Cout + 7) >> 3;
    const bool al16 = (((uintptr_t)a.out) & 15) == 0 && (a.out_pix_stride & 7) == 0;
    float bq[4][4];                                          // this lane's 16 output-channel biases
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ch = 8 * q + 4 * hi + k;
            bq[q][k] = (a.bias && ch < a.Cout) ? a.bias[ch] : 0.0f;
        }

    u32x4_t hreg[HPT];
    fetch((int)blockIdx.x, hreg);
    auto park = [&]() {
#pragma unroll
        for (int k = 0; k < HPT; ++k) {
            const int i = tid + k * 256;
            if (i < HALO_N) halo[i] = hreg[k];
        }
    };
    park();
    for (int t = (int)blockIdx.x; t < ntiles; t += (int)gridDim.x) {
        int bid = t;
        const int tx0 = (bid % tiles_x) * TW; bid /= tiles_x;
        const int ty0 = (bid % tiles_y) * TH;
        const int b = bid / tiles_y;
        // LDS-only barriers: __syncthreads() would also drain vmcnt, i.e. wait for the previous tile's stores to be acknowledged
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                        // halo complete; the previous tile's image reads are done too
        fetch(t + (int)gridDim.x, hreg);                     // next tile's halo, in flight under the MFMA phase

        // wave w: output rows 2w, 2w+1 of the tile, two 32-pixel halves each
        f32x16_t acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[u][e] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            int tap = ks * 2 + hi;
            tap = tap < NTAP ? tap : 0;                      // zero weights there: any in-range address will do
            const int r = tap / S, sx = tap - r * S;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ty = wave * 2 + (u >> 1), tx = (u & 1) * 32 + p;
                const u32x4_t q = halo[(ty + r) * HW_ + tx + sx];
                bf16x8_t af;
                __builtin_memcpy(&af, &q, 16);
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[ks], af, acc[u], 0, 0, 0);
            }
        }
        // epilogue: lane (pixel p of the m-tile, hi) holds channels (e&3) + 8*(e>>2) + 4*hi -> 8-byte pieces into the image
        // the activation mode is wave-uniform: branch ONCE around the whole block (per-value mode tests inlined erff 64 times)
        auto to_image = [&](auto act) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pl = (wave * 2 + (u >> 1)) * TW + (u & 1) * 32 + p;      // pixel index inside the tile
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ch = 8 * q + 4 * hi;
                    float v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = act(acc[u][q * 4 + k] + bq[q][k]);
                    uint2 o;
                    o.x = pack_bf16x2(v[0], v[1]);
                    o.y = pack_bf16x2(v[2], v[3]);
                    *reinterpret_cast<uint2*>(img + pl * OP + ch) = o;
                }
            }
        };
        if (a.relu == 1) to_image([](float x) { return fmaxf(x, 0.0f); });
        else if (a.relu == 2) to_image([](float x) { return conv_act(x, 2); });
        else to_image([](float x) { return x; });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                        // image complete (and every halo read of this tile retired)
        // Park the next halo BEFORE this tile's stores: vmcnt is one in-order counter for loads and stores, so waiting for
        // the halo registers after the stores would wait for their acknowledgement too (a store round trip per tile).
        park();
        // coalesced stores: 4 lanes x 16 bytes per pixel row (Cout <= 32), consecutive lanes = consecutive pixels
#pragma unroll 2
        for (int i = tid; i < TH * TW * 4; i += 256) {
            const int pl = i >> 2, cc = i & 3;
            if (cc >= cchunks) continue;
            const int oy = ty0 + pl / TW, ox = tx0 + (pl % TW);
            if (oy >= a.Ho || ox >= a.Wo) continue;
            uint16_t* dst = a.out + (((long long)b * a.Ho + oy) * a.Wo + ox) * a.out_pix_stride + cc * 8;
            const uint2 lo = *reinterpret_cast<const uint2*>(img + pl * OP + cc * 8);
            const uint2 hi2 = *reinterpret_cast<const uint2*>(img + pl * OP + cc * 8 + 4);
            if (cc * 8 + 8 <= a.Cout && al16) {
                *reinterpret_cast<uint4*>(dst) = make_uint4(lo.x, lo.y, hi2.x, hi2.y);
            } else {                                         // ragged channel tail (Cout % 8 == 4) or 8-byte aligned rows
                *reinterpret_cast<uint2*>(dst) = lo;
                if (cc * 8 + 4 < a.Cout) *reinterpret_cast<uint2*>(dst + 4) = hi2;
            }
        }
        // no barrier here: the image is only rewritten after the next iteration's first barrier
    }
}
