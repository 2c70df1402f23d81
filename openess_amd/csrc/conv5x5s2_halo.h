// =================================================================================================
// 5x5 / stride-2 / pad-2 convolutions with a 2-D INPUT HALO in LDS (conv5x5s2_halo_kernel): E2VID's three encoder
// ConvLayers (e2vid/model/unet.py: 32->64 @440x640, 64->128 @220x320, 128->256 @110x160, 20 launches each per step).
//
// In the implicit GEMM every (tap, channel chunk) K-slab fetches its own im2col block, so an input pixel travels L2 -> LDS
// 25 / 4 = 6.25 times per output-channel tile.  Here a workgroup owns an 8 x 16 patch of output pixels x 64 output channels
// and keeps the 19 x 35 input pixels under it (32 channels = 64 bytes each) in LDS for all 25 taps: 5.2 input pixels per
// output pixel instead of 25, and tiles of 128 x 64 instead of 128 x 128 (4 400 / 2 200 / 1 120 workgroups on the three
// layers instead of 550-1 100 tiles that quantise badly over the 512 slots).
// Stride 2 would make the 16 lanes of a fragment-read phase touch only every second 64-byte block (half the banks), so the
// halo is stored as TWO COLUMN-PARITY PLANES: plane p holds input columns 2 xi + p, and tap column s reads plane s & 1 at
// xi = px + (s >> 1) -- consecutive output pixels are consecutive blocks again.  Block (p, hy, xi) keeps its four 16-byte
// chunks at slot = chunk ^ (((xi >> 2) & 1) | (((hy >> 1) & 1) << 1)); a fragment row r of an M-tile is the pixel
// (py = 2 i + ((r >> 3) & 1), px = (r & 7) + 8 (r >> 4)), so a phase (16 lanes) = 8 pixels x 2 patch rows = 4 lanes in each
// of the 4 bank quarters with 4 different slots: conflict-free.  Weights: one (tap, 32-channel) slab of 64 rows x 64 bytes
// per tap in a 6-deep LDS-DMA ring (5 slabs = ~1.5 us of taps in flight), slot = chunk ^ ((row >> 2) & 3).
// Four waves, each a 64-pixel x 32-channel wave tile (fragments of the next k-step in flight under the current MFMAs); LDS 44 KB
// halo + 24 KB ring = 68 KB -> two workgroups per CU = two waves per SIMD from DIFFERENT workgroups, so one workgroup's halo
// fetch and epilogue run under the other's K loop (with two-wave workgroups, one wave per SIMD, the three phases of a tile
// simply added up: 130 us on the 32->64 layer, 92 us with the epilogue compiled out, against 118 us for the im2col kernel).
// Channel chunks (Cin = 64 / 128) reload the halo; the weight ring runs on across the chunk boundary.
// =================================================================================================
constexpr int S2_PH = 8, S2_PW = 16;                                 // output patch
constexpr int S2_HH = 2 * S2_PH + 3, S2_XW = 18;                     // 19 halo rows; 18 blocks per plane row (35 columns)
constexpr int S2_BLOCKS = 2 * S2_HH * S2_XW;                         // 684 blocks of 64 bytes
constexpr int S2_HINSTR = (S2_BLOCKS + 63) / 64;                     // 11 wave-level DMA instructions (16 blocks each) per wave, 4 waves
constexpr int S2_HALO_BYTES = S2_HINSTR * 4 * 1024;                  // 45 056
constexpr int S2_SLAB = 64 * 64;
constexpr int S2_RING_PLAIN = 6, S2_RING_FUSED = 5;                  // weight slabs in the ring
constexpr int S2_LDS = S2_HALO_BYTES + S2_RING_PLAIN * S2_SLAB;      // 69 632
// fused E2VID head (5x5 stride 1, 8 -> 32 channels) in front of the 32 -> 64 encoder: the voxel patch under the halo
constexpr int S2_VH = S2_HH + 4, S2_VW = 2 * S2_PW + 3 + 4;          // 23 x 39 voxel pixels of 16 bytes (8 channels)
constexpr int S2_VINSTR = (S2_VH * S2_VW + 255) / 256;               // 4 wave-level DMA instructions per wave (64 pixels each)
constexpr int S2_VTOTAL = (S2_VH * S2_VW + 63) / 64;                 // 15 instructions in all
constexpr int S2_VOX_BYTES = S2_VTOTAL * 1024;                       // 15 360
constexpr int S2_LDS_FUSED = S2_HALO_BYTES + S2_RING_FUSED * S2_SLAB + S2_VOX_BYTES;    // 80 896: two workgroups per CU
struct S2Head {              // FUSED: the encoder's input is relu(conv5x5(x8, hw) + hb), computed per patch into the LDS halo
    const uint16_t* x8;      // NHWC bf16, 8 channels (event bins zero-padded), pixel stride x8_stride elements
    long long x8_stride;
    const uint16_t* hw;      // packed head weight [128][256] (rows 0..31 used, k = tap * 8 + channel)
    const float* hb;         // [32] or null
    int relu;
    // ev != null: the 8-channel input is formed on the fly from the fp32 NCHW event tensor (EventPreprocessor apply + NHWC8
    // bf16 re-layout of oess_event_slice_to_nhwc8_bf16, same arithmetic): x8 is not read
    const float* ev;         // [B][Ctot][H][W] fp32
    int Ctot, c0, Cs, normalize;
    const double* stats;     // {sum, sumsq, nnz} of the slice
};
// K32: EventPreprocessor's hot-pixel mask and flip (inference_utils.py:71-75) in the ev loader of the fused kernel (PRE
// instantiation only: the option-less kernels do not see this struct)
struct S2Pre {
    const unsigned char* mask;   // [H][W] bytes in source coordinates, non-zero = hot; may be null
    int flip;                    // voxel pixel (iy, ix) reads source pixel (H - 1 - iy, W - 1 - ix)
};
constexpr int S2_IMG_PITCH = 72;                                     // bf16 output image [128 pixels][64 + 8]

template <typename F, int... Is>
__device__ __forceinline__ void s2_for_taps(F&& f, std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }

// one 8 x 16-pixel x 64-channel tile (`bid` = tile index after the XCD remap)
template <bool FUSED, bool PRE = false>
__device__ __forceinline__ void conv5x5s2_halo_tile(const ConvArgs& a, const S2Head& hd, const int bid, unsigned char* smem,
                                                    const S2Pre& pre = S2Pre{}) {
    static_assert(FUSED || !PRE, "the event options live in the fused kernel's ev loader");
    constexpr int S2_RING = FUSED ? S2_RING_FUSED : S2_RING_PLAIN;
    const int tile_n = bid % a.tiles_n;
    int patch = bid / a.tiles_n;
    const int tiles_x = (a.Wo + S2_PW - 1) / S2_PW, tiles_y = (a.Ho + S2_PH - 1) / S2_PH;
    const int ox0 = (patch % tiles_x) * S2_PW; patch /= tiles_x;
    const int oy0 = (patch % tiles_y) * S2_PH;
    const int b = patch / tiles_y;
    const int n0 = tile_n * 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;                         // wave tile: patch rows 4 wm .. 4 wm + 3 (64 pixels) x channels 32 wn .. + 31
    constexpr int MT = 2, NT = 1;                                    // ... in 32 x 32 fragments (OESS_FRAG_WAIT)
    const int nchunks = a.Cin >> 5;
    const int NS = nchunks * 25;                                     // weight slabs of this tile

    const long long in_bytes = FUSED ? (((long long)a.B * a.H * a.W - 1) * hd.x8_stride + 8) * 2
                                     : (((long long)a.B * a.H * a.W - 1) * a.in_pix_stride + a.Cin) * 2;
    __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(FUSED ? (void*)hd.x8 : (void*)a.in, 0, (FUSED && !hd.x8) ? 0 : (int)in_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x7ffffff0, 0x00020000);

    // ---- halo DMA geometry: lane (block lb = lane >> 2, slot = lane & 3) of instruction i writes block u = (wave*11 + i)*16 + lb
    unsigned hoff[FUSED ? 1 : S2_HINSTR];
#pragma unroll
    for (int i = 0; i < (FUSED ? 0 : S2_HINSTR); ++i) {
        const int u = (wave * S2_HINSTR + i) * 16 + (lane >> 2), slot = lane & 3;
        const int p = u / (S2_HH * S2_XW), rem = u - p * (S2_HH * S2_XW);
        const int hy = rem / S2_XW, xi = rem - hy * S2_XW;
        const int hx = 2 * xi + p;
        const int f = ((xi >> 2) & 1) | (((hy >> 1) & 1) << 1);
        const int iy = 2 * oy0 - 2 + hy, ix = 2 * ox0 - 2 + hx;
        const bool ok = u < S2_BLOCKS && hx < 2 * S2_PW + 3 && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        hoff[i] = ok ? (unsigned)((((long long)b * a.H + iy) * a.W + ix) * a.in_pix_stride * 2 + ((slot ^ f) << 4)) : 0x80000000u;
    }
    // ---- weight DMA geometry: this wave writes rows wave*16 + (lane >> 2) of every slab
    unsigned boff;
    {
        const int row = wave * 16 + (lane >> 2), slot = lane & 3;
        boff = (unsigned)(((n0 + row) * a.Kpad + ((slot ^ ((row >> 2) & 3)) << 3)) * 2);
    }
    auto issue_halo = [&](int cc) {
#pragma unroll
        for (int i = 0; i < (FUSED ? 0 : S2_HINSTR); ++i) {
            const unsigned voff = hoff[i] == 0x80000000u ? 0x80000000u : hoff[i] + (unsigned)(cc * 64);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(smem + (wave * S2_HINSTR + i) * 1024),
                                                     16, voff, 0, 0, 0);
        }
    };
    // slab s = (chunk, tap) -> ring buffer `buf`; slabs beyond the tile are dummy (out-of-range source = zero fill) so that
    // the number of DMA instructions in flight is the same at every tap
    auto issue_w = [&](int s, int buf) {
        const int cc = s / 25, tap = s - cc * 25;
        const unsigned voff = s < NS ? boff + (unsigned)((tap * a.Cin + cc * 32) * 2) : 0x80000000u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(smem + S2_HALO_BYTES + buf * S2_SLAB + wave * 1024),
                                                 16, voff, 0, 0, 0);
    };

    // accumulators: acc[i] = channels (rows) x pixels (columns) of M-tile i -- operands swapped, so that a lane holds four
    // CONSECUTIVE channels of one pixel and the epilogue writes 8-byte pieces
    f32x16_t acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;

    // ---- fragment addresses.  slot << 4 = (ks << 5) ^ ((half ^ f) << 4): the lane part ((half ^ f) << 4) is folded into one base
    //      register per (M-tile, s >> 1, parity of r >> 1) -- 12 registers -- the tap's block offset is an instruction immediate
    //      and k-step 1 flips bit 5 (bases are multiples of 64 bytes + the slot bits, so the XOR never carries)
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    const int r31 = lane & 31, half = lane >> 5;
    const int a_px = (r31 & 7) + 8 * (r31 >> 4);
    uint32_t va[2][3][2], vb;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int py = 4 * wm + 2 * i + ((r31 >> 3) & 1);
#pragma unroll
        for (int sv = 0; sv < 3; ++sv)
#pragma unroll
            for (int rp = 0; rp < 2; ++rp) {
                const int f = (((a_px + sv) >> 2) & 1) | (((py + rp) & 1) << 1);
                va[i][sv][rp] = lds0 + (uint32_t)((2 * py * S2_XW + a_px) * 64 + ((half ^ f) << 4));
            }
    }
    {
        const int n = wn * 32 + r31;
        vb = lds0 + (uint32_t)(S2_HALO_BYTES + n * 64 + ((half ^ ((n >> 2) & 3)) << 4));
    }

#define S2_READ(FA, FB, R_, S_, KS_, BUF_)                                                                              \
    {                                                                                                                   \
        constexpr int blk_ = ((((S_) & 1) * S2_HH + (R_)) * S2_XW + ((S_) >> 1)) * 64;                                   \
        _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                                   \
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(FA[i]) : "v"(va[i][(S_) >> 1][((R_) >> 1) & 1] ^ (uint32_t)((KS_) << 5)), "n"(blk_) : "memory"); \
        asm volatile("ds_read_b128 %0, %1" : "=v"(FB[0]) : "v"((vb ^ (uint32_t)((KS_) << 5)) + (uint32_t)((BUF_) * S2_SLAB)) : "memory");  \
    }
#define S2_MMA(FA, FB)                                                                                                  \
    {                                                                                                                   \
        _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                                   \
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FB[0], FA[i], acc[i], 0, 0, 0);                            \
    }

    if constexpr (FUSED) {
        // ---- E2VID head in front of the encoder: relu(conv5x5(x8) + hb) for the 19 x 35 halo pixels, written straight into the
        //      halo planes (zeros outside the image = the encoder's own padding).  Head weights: 13 k-steps of two taps x 8
        //      channels, kept in registers (MFMA A operand: rows = 32 head channels); pixels are the B operand, read from the
        //      23 x 39 voxel patch in LDS; a lane ends up with four consecutive channels of one halo pixel -> 8-byte LDS writes.
        unsigned char* vox = smem + S2_HALO_BYTES + S2_RING_FUSED * S2_SLAB;
        bf16x8_t wf[13];
        {
            const int p32 = lane & 31, hi = lane >> 5;
#pragma unroll
            for (int ks = 0; ks < 13; ++ks) wf[ks] = *reinterpret_cast<const bf16x8_t*>(hd.hw + (size_t)p32 * 256 + (ks * 2 + hi) * 8);
        }
        if (hd.ev) {
            // voxel patch straight from the fp32 event tensor: the slice's EventPreprocessor normalisation (inference_utils.py:80-85,
            // the float32 operation order of norm_to_nhwc8_kernel) and the 8-channel bf16 packing happen here, per patch
#pragma unroll
            for (int s = 0; s < S2_RING - 1; ++s) issue_w(s, s);
            const double nnz = hd.stats ? hd.stats[2] : 0.0;
            const bool active = hd.normalize && nnz > 0.0;
            float mean = 0.f, stdv = 1.f;
            if (active) {
                const float nf = (float)nnz;
                mean = (float)hd.stats[0] / nf;
                stdv = sqrtf(__fsub_rn((float)hd.stats[1] / nf, __fmul_rn(mean, mean)));
            }
            const long long hw_ = (long long)a.H * a.W;
            float raw[4][5];
            bool okv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int v = tid + 256 * i;
                const int vy = v / S2_VW, vx = v - vy * S2_VW;
                const int iy = 2 * oy0 - 4 + vy, ix = 2 * ox0 - 4 + vx;
                okv[i] = v < S2_VH * S2_VW && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                const float* src = hd.ev + ((long long)b * hd.Ctot + hd.c0) * hw_ + (long long)iy * a.W + ix;
                bool hot = false;
                if constexpr (PRE) {
                    // the border test above is on the mirrored (output) coordinates: the zero padding stays where it was.  The
                    // mask byte is loaded beside the events (no load waits for it); a hot pixel enters the normalisation below
                    // as a zero, as in the reference's zeroed tensor
                    const long long spix = pre.flip ? (long long)(a.H - 1 - iy) * a.W + (a.W - 1 - ix) : (long long)iy * a.W + ix;
                    src = hd.ev + ((long long)b * hd.Ctot + hd.c0) * hw_ + spix;
                    if (pre.mask) hot = pre.mask[okv[i] ? spix : 0] != 0;
                }
#pragma unroll
                for (int c = 0; c < 5; ++c) raw[i][c] = (okv[i] && c < hd.Cs) ? src[c * hw_] : 0.0f;
                if constexpr (PRE) {
#pragma unroll
                    for (int c = 0; c < 5; ++c) raw[i][c] = hot ? 0.0f : raw[i][c];
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int v = tid + 256 * i;
                float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    float q = raw[i][c];
                    if (active) q = __fmul_rn((q != 0.0f) ? 1.0f : 0.0f, __fsub_rn(q, mean)) / stdv;
                    f[c] = (okv[i] && c < hd.Cs) ? q : 0.0f;
                }
                const u32x4_t o = {pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])};
                if (v < S2_VTOTAL * 64)
                    asm volatile("ds_write_b128 %0, %1" :: "v"((uint32_t)(uintptr_t)vox + (uint32_t)(v * 16)), "v"(o) : "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        } else {
#pragma unroll
            for (int i = 0; i < S2_VINSTR; ++i) {
                const int v = (wave * S2_VINSTR + i) * 64 + lane;
                const int vy = v / S2_VW, vx = v - vy * S2_VW;
                const int iy = 2 * oy0 - 4 + vy, ix = 2 * ox0 - 4 + vx;
                const bool ok = v < S2_VH * S2_VW && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                const unsigned voff = ok ? (unsigned)((((long long)b * a.H + iy) * a.W + ix) * hd.x8_stride * 2) : 0x80000000u;
                if (wave * S2_VINSTR + i < S2_VTOTAL)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(vox + (wave * S2_VINSTR + i) * 1024), 16, voff, 0, 0, 0);
            }
#pragma unroll
            for (int s = 0; s < S2_RING - 1; ++s) issue_w(s, s);
        }
        float bq[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) bq[q][k] = hd.hb ? hd.hb[8 * q + 4 * (lane >> 5) + k] : 0.0f;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                // voxel patch (and the first weight slabs) are in LDS
        const uint32_t vox0 = (uint32_t)(uintptr_t)vox, pl0 = (uint32_t)(uintptr_t)smem;
        const int hi = lane >> 5;
        // two M-tiles (64 halo pixels) per pass: two independent accumulators, two reads in flight under two MFMAs
        static_assert(((S2_BLOCKS + 31) / 32) % 2 == 0, "M-tiles are taken in pairs");
        for (int pr = wave; pr < (S2_BLOCKS + 31) / 64; pr += 4) {
            int uu_[2], hy_[2], xi_[2];
            bool inside_[2];
            uint32_t vbase[2];
#pragma unroll
            for (int z = 0; z < 2; ++z) {
                const int u = (2 * pr + z) * 32 + (lane & 31);
                uu_[z] = u;
                const int uu = u < S2_BLOCKS ? u : 0;
                const int p = uu / (S2_HH * S2_XW), rem = uu - p * (S2_HH * S2_XW);
                const int hy = rem / S2_XW, xi = rem - hy * S2_XW;
                int hx = 2 * xi + p;
                inside_[z] = u < S2_BLOCKS && hx < 2 * S2_PW + 3 && (unsigned)(2 * oy0 - 2 + hy) < (unsigned)a.H &&
                             (unsigned)(2 * ox0 - 2 + hx) < (unsigned)a.W;
                hx = hx < 2 * S2_PW + 3 ? hx : 0;
                hy_[z] = hy; xi_[z] = xi;
                vbase[z] = vox0 + (uint32_t)((hy * S2_VW + hx) * 16);
            }
            f32x16_t hacc[2];
#pragma unroll
            for (int z = 0; z < 2; ++z)
#pragma unroll
                for (int e = 0; e < 16; ++e) hacc[z][e] = 0.0f;
            bf16x8_t pa[2], pb[2];
            // k-step ks: this half wave's tap = 2 ks + hi (tap 25 carries zero weights: any address)
#define S2_HREAD(DST, KS_)                                                                                             \
            {                                                                                                         \
                constexpr int t0_ = 2 * (KS_), t1_ = 2 * (KS_) + 1 < 25 ? 2 * (KS_) + 1 : 0;                            \
                const uint32_t off_ = hi ? (uint32_t)(((t1_ / 5) * S2_VW + t1_ % 5) * 16) : (uint32_t)(((t0_ / 5) * S2_VW + t0_ % 5) * 16); \
                asm volatile("ds_read_b128 %0, %1" : "=v"(DST[0]) : "v"(vbase[0] + off_) : "memory");                  \
                asm volatile("ds_read_b128 %0, %1" : "=v"(DST[1]) : "v"(vbase[1] + off_) : "memory");                  \
            }
            S2_HREAD(pa, 0)
            s2_for_taps([&](auto kc) __attribute__((always_inline)) {
                constexpr int ks = decltype(kc)::value;
                if constexpr (ks + 1 < 13) {
                    if constexpr (ks & 1) { S2_HREAD(pa, ks + 1) } else { S2_HREAD(pb, ks + 1) }
                    if constexpr (ks & 1) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(pb[0]), "+v"(pb[1]) :: "memory");
                    else asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(pa[0]), "+v"(pa[1]) :: "memory");
                } else {
                    if constexpr (ks & 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pb[0]), "+v"(pb[1]) :: "memory");
                    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pa[0]), "+v"(pa[1]) :: "memory");
                }
#pragma unroll
                for (int z = 0; z < 2; ++z)
                    hacc[z] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[ks], (ks & 1) ? pb[z] : pa[z], hacc[z], 0, 0, 0);
            }, std::make_integer_sequence<int, 13>{});
#undef S2_HREAD
#pragma unroll
            for (int z = 0; z < 2; ++z) {
                if (uu_[z] >= S2_BLOCKS) continue;
                const uint32_t f = (uint32_t)(((xi_[z] >> 2) & 1) | (((hy_[z] >> 1) & 1) << 1));
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v[k] = hacc[z][q * 4 + k] + bq[q][k];
                        if (hd.relu) v[k] = fmaxf(v[k], 0.0f);
                        v[k] = inside_[z] ? v[k] : 0.0f;
                    }
                    const uint2 o = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
                    asm volatile("ds_write_b64 %0, %1" :: "v"(pl0 + (uint32_t)(uu_[z] * 64) + (((uint32_t)q ^ f) << 4) + (uint32_t)(8 * hi)), "v"(o) : "memory");
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    } else {
#pragma unroll
        for (int s = 0; s < S2_RING - 1; ++s) issue_w(s, s);
    }
    int sg = 0, buf = 0;                                             // global slab index and its ring buffer
    for (int cc = 0; cc < nchunks; ++cc) {
        if (cc > 0) __builtin_amdgcn_s_barrier();                    // every wave is done with the previous chunk's halo
        issue_halo(cc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                // halo and every slab issued so far are in LDS
        bf16x8_t fa0[MT], fb0[NT], fa1[MT], fb1[NT];
        S2_READ(fa0, fb0, 0, 0, 0, buf)
        // the 25 taps, unrolled with compile-time (r, s): tap offsets are instruction immediates
        s2_for_taps([&](auto tc) __attribute__((always_inline)) {
            constexpr int t = decltype(tc)::value, r = t / 5, s = t - r * 5;
            if (t > 0) {
                asm volatile("s_waitcnt vmcnt(%0)" :: "n"(S2_RING - 3) : "memory");     // slab sg + 1 has landed (RING - 3 younger slabs may be in flight)
                __builtin_amdgcn_s_barrier();                        // ... for every wave; the buffer of slab sg - 1 is free
            }
            const int nb = buf + 1 == S2_RING ? 0 : buf + 1;         // buffer of slab sg + 1
            issue_w(sg + S2_RING - 1, buf == 0 ? S2_RING - 1 : buf - 1);
            __builtin_amdgcn_s_setprio(3);
            S2_READ(fa1, fb1, r, s, 1, buf)
            OESS_FRAG_WAIT(3, fa0, fb0)
            S2_MMA(fa0, fb0)
            if constexpr (t < 24) {
                constexpr int r2 = (t + 1) / 5, s2 = (t + 1) - r2 * 5;
                S2_READ(fa0, fb0, r2, s2, 0, nb)
                OESS_FRAG_WAIT(3, fa1, fb1)
            } else {
                OESS_FRAG_WAIT(0, fa1, fb1)
            }
            S2_MMA(fa1, fb1)
            __builtin_amdgcn_s_setprio(0);
            ++sg; buf = nb;
        }, std::make_integer_sequence<int, 25>{});
    }
#undef S2_READ
#undef S2_MMA
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // dummy tail slabs have been written (ring region only)
    __syncthreads();

    // ---- epilogue: bias + activation -> bf16 image [128 pixels][64 channels] in LDS (8-byte pieces: a lane holds channels
    //      32 wn + 8 q + 4 half + {0..3} of pixel r31 of each M-tile) -> 16-byte row stores
    uint16_t* img = reinterpret_cast<uint16_t*>(smem);
    {
        float bq[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) bq[q][k] = a.bias ? a.bias[n0 + wn * 32 + 8 * q + 4 * half + k] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int py = 4 * wm + 2 * i + ((r31 >> 3) & 1);
            uint16_t* dst = img + (py * S2_PW + a_px) * S2_IMG_PITCH + wn * 32 + 4 * half;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[k] = acc[i][q * 4 + k] + bq[q][k];
                    if (a.relu) v[k] = fmaxf(v[k], 0.0f);
                }
                uint2 o;
                o.x = pack_bf16x2(v[0], v[1]);
                o.y = pack_bf16x2(v[2], v[3]);
                *reinterpret_cast<uint2*>(dst + 8 * q) = o;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = tid + k * 256, pl = idx >> 3, c = idx & 7;
        const int oy = oy0 + (pl >> 4), ox = ox0 + (pl & 15);
        if (oy < a.Ho && ox < a.Wo)
            out_store16(a.out + (((long long)b * a.Ho + oy) * a.Wo + ox) * a.out_pix_stride + n0 + c * 8,
                        *reinterpret_cast<const uint4*>(img + pl * S2_IMG_PITCH + c * 8));
    }
}

template <bool FUSED>
__global__ __launch_bounds__(256, 2) void conv5x5s2_halo_kernel(ConvArgs a, S2Head hd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nwg = a.tiles_m * a.tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    conv5x5s2_halo_tile<FUSED>(a, hd, bid, smem);
}

// K32: the fused kernel with the event options (hd.ev != null)
__global__ __launch_bounds__(256, 2) void conv5x5s2_halo_pre_kernel(ConvArgs a, S2Head hd, S2Pre pre) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nwg = a.tiles_m * a.tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    conv5x5s2_halo_tile<true, true>(a, hd, bid, smem, pre);
}

// Two independent problems of the plain kernel in one launch (encoder convs of levels 1 and 2 on the skewed schedule of the
// recurrent encoder: 2 240 + 1 120 workgroups = 4.4 + 2.2 rounds over the 512 slots alone, 6.6 together); mapping as in
// conv3x3_halo_group_kernel, longest K first.
struct S2Group {
    ConvArgs a[2];
    int start8[3];
};
__global__ __launch_bounds__(256, 2) void conv5x5s2_halo_group_kernel(S2Group g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int p = idx >= g.start8[1] ? 1 : 0;
    const int li = idx - g.start8[p];
    const ConvArgs& a = g.a[p];
    const int nwg = a.tiles_m * a.tiles_n;
    const int q = nwg >> 3, r = nwg & 7;
    if (li >= q + (xcd < r ? 1 : 0)) return;
    conv5x5s2_halo_tile<false>(a, S2Head{}, (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + li, smem);
}
