// =================================================================================================
// 3x3 / stride-1 / "same" convolutions with ROW-HALO REUSE of the pixel operand (conv3x3_halo_kernel).
//
// In the implicit GEMM above, every K-slab = (filter tap, 64 input channels) fetches its own 128 x 64 im2col block, yet the
// blocks of the three taps of one filter ROW (dx = 0, 1, 2) are the same 128 pixels shifted by `dil` pixels.  Here the
// K loop runs in (dy, channel chunk, dx) order -- the standard packed weight already holds each (tap, chunk) as 64
// contiguous k, so no new packing -- and the pixel operand of the three dx taps is ONE halo buffer in LDS:
//   halo rows = [dil lead pixels][segment 0][dil gap][segment 1][dil gap] ... [last segment][dil trail pixels]
// where a segment is a run of tile pixels inside one image row; the gap rows are written as zeros by out-of-range DMA
// offsets, so a side tap that crosses an image-row (or image) boundary lands on zeros exactly like the im2col padding.
// Tile pixel i sits at halo row hrow(i); tap dx reads row hrow(i) + (dx - 1) * dil.  Per K-slab the workgroup now moves
// 16 KB of weights + a third of a <= 20 KB halo instead of 32 KB: ~30 % fewer L2->LDS bytes and LDS-DMA writes on the
// layers that make up most of the step (ConvLSTM gates, decoder and teacher 3x3 convs).
// LDS: 2 halo buffers (2 x 20 KB) + 2 weight stages (2 x 16 KB) = 72 KB -> still two workgroups per CU.
// =================================================================================================
constexpr int HALO_ROWS = 160;

// one 128 x 128 tile (`bid` = tile index after the XCD remap); smem = [halo 0][halo 1][weights 0][weights 1]
// BMX = 256 (EPI = 1 only; round 5): an 8-wave workgroup owns 256 pixels x 128 gate columns -- the weight slab is
// fetched once per 256 pixels (150 instead of 92 FLOP per L2 -> LDS byte, 3.7 instead of 5.7 DMA instructions per wave and slab),
// one workgroup per CU (2 x 40 KB halo + 2 x 16 KB weights), the wave tile stays 64 x 64.
constexpr int HALO_ROWS_256 = 320;
constexpr int LSTM_EPI_HALF = 26624;                     // LDS of one 128-row half of the ConvLSTM epilogue (25 600 B used)
template <int EPI, int BMX = 128>
__device__ __forceinline__ void conv3x3_halo_tile(const ConvArgs& a, const int bid, unsigned char* smem) {
    constexpr int BN = 128, NWAVES = BMX / 32, WAVES_N = 2, WM = 64, WN = 64, MT = 2, NT = 2;
    constexpr int HROWS = (BMX == 128) ? HALO_ROWS : HALO_ROWS_256;
    constexpr int H_INSTR = HROWS / 8 / NWAVES;          // 5 DMA instructions per thread per halo
    constexpr int B_INSTR = BN * 8 / 64 / NWAVES;        // 4 (2 with eight waves)
    constexpr int HALO_BYTES = HROWS * 128, BST_BYTES = BN * 128;
    static_assert(BMX == 128 || EPI == 1, "the 256-row tile exists for the fused ConvLSTM only");
    constexpr int NFRAG = MT + NT;

    const int tile_n = bid % a.tiles_n, tile_m = bid / a.tiles_n;
    const int m0 = tile_m * BMX, n0 = tile_n * BN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    // Loop-invariant scalars of the K loop, pinned in SGPRs.  In the grouped kernel `a` is g.a[p] with a run-time p, i.e. kernel-
    // argument MEMORY: hipcc treats such loads as free to rematerialise and re-issued s_load_dword a.Cin / a.H / a.in_pix_stride
    // + s_waitcnt lgkmcnt(0) in front of every slab's barrier (round-5 disassembly: three scalar-cache round trips per macro step
    // on the kernel that owns 41 % of the step).  The empty asm makes the values opaque, so they stay in registers.
    int Cin_s = a.Cin, H_s = a.H, ips_s = (int)a.in_pix_stride;
    asm volatile("" : "+s"(Cin_s), "+s"(H_s), "+s"(ips_s));
    const int nch = Cin_s >> 6;                          // 64-channel chunks
    const int NJ = 3 * nch;                              // macro steps (dy, chunk); 3 K-slabs each
    const int W = a.W, dil = a.dil, wd = W + dil;

    const long long in_bytes = (((long long)a.B * a.H * a.W - 1) * a.in_pix_stride + a.Cin) * 2;
    __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, (int)in_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x7ffffff0, 0x00020000);

    // tile origin (wave-uniform)
    const int hw = a.H * W;
    const int b0 = m0 / hw, rem0 = m0 - b0 * hw;
    const int oy0 = rem0 / W, ox0 = rem0 - oy0 * W;
    const int L0 = (W - ox0 < BMX) ? W - ox0 : BMX;      // tile pixels in the first image row

    // ---- halo DMA geometry: lane (lrow, slot) of instruction q writes halo row h = q*8 + lrow, 16-byte slot `slot`
    const int lrow = lane >> 3, slot = lane & 7;
    int hy[H_INSTR], hoff[H_INSTR];
#pragma unroll
    for (int i = 0; i < H_INSTR; ++i) {
        const int h = (wave * H_INSTR + i) * 8 + lrow;
        const int hp = h - dil;
        int m_seg, px, drow;                             // first tile pixel of the row's segment, x coordinate of this halo row, image rows below the tile's first
        if (hp < L0 + dil) { m_seg = m0; px = ox0 + hp; drow = 0; }
        else {
            const int h2 = hp - (L0 + dil);
            const int q = a.mg_wd ? (int)__umulhi((unsigned)h2, a.mg_wd) : h2 / wd, r = h2 - q * wd;
            m_seg = m0 + L0 + q * W; px = r; drow = q + 1;
        }
        const bool valid = m_seg < a.M && (m_seg == m0 || m_seg - m0 < BMX) && (unsigned)px < (unsigned)W;
        // segment q starts an image row: its row is the tile's first row + drow, carried into the next image(s) -- no division
        int oy = oy0 + drow;
        const long long grow = (long long)b0 * a.H + oy;  // row index over the whole batch
        while (oy >= a.H) oy -= a.H;
        hy[i] = valid ? oy : -0x4000;
        hoff[i] = valid ? (int)((grow * W + px) * a.in_pix_stride * 2) + (slot ^ ((h >> 1) & 7)) * 16 : 0;
    }
    int boff[B_INSTR];
#pragma unroll
    for (int i = 0; i < B_INSTR; ++i) {
        const int r = (wave * B_INSTR + i) * 8 + lrow;
        boff[i] = ((n0 + r) * a.Kpad + (slot ^ ((r >> 1) & 7)) * 8) * 2;
    }
    // halo part `part` (instructions [i0, i1)) of macro step j -> halo buffer j & 1
    auto issue_halo = [&](int j, int dy, int cc, int i0, int i1) {        // (dy, cc) = (j / nch, j % nch), kept by the caller
        const int ddy = (dy - 1) * dil;
        const int tapoff = (ddy * W * ips_s + cc * 64) * 2;
        unsigned char* st = smem + (j & 1) * HALO_BYTES;
#pragma unroll
        for (int i = 0; i < H_INSTR; ++i) {
            if (i < i0 || i >= i1) continue;
            const bool ok = (unsigned)(hy[i] + ddy) < (unsigned)H_s;
            const unsigned voff = ok ? (unsigned)(hoff[i] + tapoff) : 0x80000000u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(st + (wave * H_INSTR + i) * 1024),
                                                     16, voff, 0, 0, 0);
        }
    };
    // weight slab of (macro step j, dx) -> weight stage kt & 1, kt = 3*j + dx
    auto issue_w = [&](int j, int dy, int cc, int dx) {
        const int koff = ((dy * 3 + dx) * Cin_s + cc * 64) * 2;
        unsigned char* st = smem + 2 * HALO_BYTES + ((3 * j + dx) & 1) * BST_BYTES;
#pragma unroll
        for (int i = 0; i < B_INSTR; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(st + (wave * B_INSTR + i) * 1024),
                                                     16, (unsigned)(boff[i] + koff), 0, 0, 0);
    };

    f32x16_t acc[MT][NT];
    if constexpr (EPI == 1) {
        lstm_bias_init<MT, NT>(a, acc, n0, wn, lane);
    } else {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    }

    // ---- fragment addresses.  Pixel fragments: halo row of tile pixel (wm*64 + i*32 + lane&31), shifted per dx tap
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    uint32_t fa_row[MT][3], fa_sw[MT][3], fb_off[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int r = wm * WM + i * 32 + (lane & 31);
        int hr;
        if (r < L0) hr = r;                              // (+ dil lead rows, - dil for the dx = 0 tap)
        else {
            const int t = r - L0, q = a.mg_w ? (int)__umulhi((unsigned)t, a.mg_w) : t / W, rr = t - q * W;
            hr = L0 + dil + q * wd + rr;
        }
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int h = hr + dx * dil;
            fa_row[i][dx] = (uint32_t)h * 128;
            fa_sw[i][dx] = (uint32_t)((h >> 1) & 7);
        }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) fb_off[j] = (uint32_t)(2 * HALO_BYTES + (wn * WN + j * 32 + (lane & 31)) * 128);
    const uint32_t half = (uint32_t)(lane >> 5);
    const uint32_t rswb = (uint32_t)(((lane & 31) >> 1) & 7);

    // Fragment addresses, complete: one VGPR per (tile row block, dx tap, k-step) for the pixel operand and per (column block,
    // k-step) for the weights; the halo buffer (j & 1) and the weight stage ((j + dx) & 1) enter as the ds_read's IMMEDIATE offset
    // (the macro-step loop is unrolled by the parity of j), so a fragment read costs no VALU instruction.  Round-5 PMC: the
    // kernel issues ~80 non-MFMA instructions per 16 MFMAs per wave, the most an in-order wave hides (MI355X_MICROARCH.md, "one
    // wave per SIMD: <= 5 single-issue instructions hidden per MFMA gap"); 30 of them were the v_add_u32 of these addresses.
    uint32_t fa_addr[MT][3][4], fb_addr[NT][4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const uint32_t c_ = (uint32_t)(ks * 2) + half;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                fa_addr[i][dx][ks] = lds0 + fa_row[i][dx] + ((c_ ^ fa_sw[i][dx]) << 4);
                asm volatile("" : "+v"(fa_addr[i][dx][ks]));       // keep it in its register (not recomputed in the loop)
            }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            fb_addr[j][ks] = lds0 + fb_off[j] + ((c_ ^ rswb) << 4);
            asm volatile("" : "+v"(fb_addr[j][ks]));
        }
    }

    issue_halo(0, 0, 0, 0, H_INSTR);
    issue_w(0, 0, 0, 0);
    constexpr bool LSTM_PREF = (EPI == 1);
    LstmPrefetch pref;
    const int ehalf = (BMX == 256) ? (wm >> 1) : 0;      // 256-row tile: the epilogue runs as two independent 128-row halves
    if constexpr (LSTM_PREF) lstm_prefetch(a, pref, m0 + ehalf * 128, n0, tid & 255);

#define OESS_HFRAG_READ(DST_A, DST_B, KS, DX)                                                                    \
    {                                                                                                            \
        _Pragma("unroll") for (int i = 0; i < MT; ++i)                                                           \
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(DST_A[i]) : "v"(fa_addr[i][DX][KS]), "n"(HOFF) : "memory"); \
        _Pragma("unroll") for (int j = 0; j < NT; ++j)                                                           \
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(DST_B[j]) : "v"(fb_addr[j][KS]), "n"(WOFF) : "memory"); \
    }

    int dy_c = 0, cc_c = 0;                              // (dy, chunk) of macro step j, carried instead of divided out
    int dy_n = 0, cc_n = 0;
    // one K-slab (macro step j of parity PAR, tap dx): barrier, next operands on their way, 16 MFMAs
    auto slab = [&](auto par_c, auto dx_c, int j) __attribute__((always_inline)) {
        constexpr int PAR = decltype(par_c)::value, dx = decltype(dx_c)::value;
        constexpr int HOFF = PAR * HALO_BYTES, WOFF = ((PAR + dx) & 1) * BST_BYTES;       // (3 j + dx) & 1 == (j + dx) & 1
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                   // slab (j, dx) complete for every wave; the other buffers are free
        // next weight slab, and a third of the next macro step's halo, travel under this slab's MFMAs
        if (dx < 2) issue_w(j, dy_c, cc_c, dx + 1);
        else if (j + 1 < NJ) issue_w(j + 1, dy_n, cc_n, 0);
        if (j + 1 < NJ) {
            if (dx == 0) issue_halo(j + 1, dy_n, cc_n, 0, 2);
            else if (dx == 1) issue_halo(j + 1, dy_n, cc_n, 2, 4);
            else issue_halo(j + 1, dy_n, cc_n, 4, H_INSTR);
        }
        bf16x8_t fa0[MT], fb0[NT], fa1[MT], fb1[NT];
        __builtin_amdgcn_s_setprio(3);
        OESS_HFRAG_READ(fa0, fb0, 0, dx)
        OESS_HFRAG_READ(fa1, fb1, 1, dx)
        OESS_FRAG_WAIT(NFRAG, fa0, fb0)
        OESS_FRAG_MMA(fa0, fb0)
        OESS_HFRAG_READ(fa0, fb0, 2, dx)
        OESS_FRAG_WAIT(NFRAG, fa1, fb1)
        OESS_FRAG_MMA(fa1, fb1)
        OESS_HFRAG_READ(fa1, fb1, 3, dx)
        OESS_FRAG_WAIT(NFRAG, fa0, fb0)
        OESS_FRAG_MMA(fa0, fb0)
        OESS_FRAG_WAIT(0, fa1, fb1)
        OESS_FRAG_MMA(fa1, fb1)
        __builtin_amdgcn_s_setprio(0);
    };
    auto macro_step = [&](auto par_c, int j) __attribute__((always_inline)) {
        dy_n = dy_c; cc_n = cc_c + 1;                    // macro step j + 1
        if (cc_n == nch) { cc_n = 0; ++dy_n; }
        slab(par_c, std::integral_constant<int, 0>{}, j);
        slab(par_c, std::integral_constant<int, 1>{}, j);
        slab(par_c, std::integral_constant<int, 2>{}, j);
        dy_c = dy_n; cc_c = cc_n;
    };
    for (int j = 0; j < NJ; j += 2) {
        macro_step(std::integral_constant<int, 0>{}, j);
        if (j + 1 < NJ) macro_step(std::integral_constant<int, 1>{}, j + 1);
    }
#undef OESS_HFRAG_READ
    __syncthreads();

    if constexpr (EPI == 1) lstm_epilogue<MT, NT, true, false>(a, acc, smem + ehalf * LSTM_EPI_HALF, m0 + ehalf * 128, n0, wm & 1, wn, lane,
                                                                 tid & 255, &pref);
    else conv_epilogue<BMX, BN, BN + 8, 256, WAVES_N>(a, acc, smem, m0, n0, wm, wn, lane, tid);
}

template <int EPI>
__global__ __launch_bounds__(256) void conv3x3_halo_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nwg = a.tiles_m * a.tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    conv3x3_halo_tile<EPI>(a, bid, smem);
}

// Up to three INDEPENDENT problems of the kernel above in one launch (the three ConvLSTM levels of E2VID's recurrent encoder
// on the skewed schedule: level l works on sub-window s - l, e2vid/model/unet.py mirror).  Alone, the levels are 17.2 /
// 8.6 / 4.3 rounds of tiles over the 512 workgroup slots and each pays its own partial last round and launch gap; together
// they are 30.1 rounds.  The host orders the problems by K, longest tiles first, so that the launch ends on the short ones.
// Workgroup blockIdx = 8 * idx + xcd: problem p owns idx in [start8[p], start8[p + 1]) on every XCD, and inside it the tiles
// are dealt to the XCDs in contiguous chunks exactly as the single-problem kernel does (neighbouring tiles share halo rows
// and weight slabs in that XCD's L2).
struct ConvGroup {
    ConvArgs a[3];
    int start8[4];           // problem p owns idx in [start8[p], start8[p + 1]); absent problems: empty ranges at the end
};
template <int EPI>
__global__ __launch_bounds__(256) void conv3x3_halo_group_kernel(ConvGroup g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    // (alternating the short-K tiles with the long-K ones, so that a CU's two workgroups differ in kind, was measured: -2.8 %
    //  against this problem-after-problem order -- the problems' weight slabs and halos evict each other from the XCD's L2)
    const int p = (idx >= g.start8[1] ? 1 : 0) + (idx >= g.start8[2] ? 1 : 0);
    const int li = idx - g.start8[p];
    const ConvArgs& a = g.a[p];
    const int nwg = a.tiles_m * a.tiles_n;
    const int q = nwg >> 3, r = nwg & 7;
    if (li >= q + (xcd < r ? 1 : 0)) return;             // padding of a problem whose tile count is not a multiple of 8
    conv3x3_halo_tile<EPI>(a, (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + li, smem);
}

// the same grouped launch on 256 x 128 tiles (8 waves, one workgroup per CU): tiles_m of every problem counts 256-row tiles
__global__ __launch_bounds__(512) void conv3x3_halo256_group_kernel(ConvGroup g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int p = (idx >= g.start8[1] ? 1 : 0) + (idx >= g.start8[2] ? 1 : 0);
    const int li = idx - g.start8[p];
    const ConvArgs& a = g.a[p];
    const int nwg = a.tiles_m * a.tiles_n;
    const int q = nwg >> 3, r = nwg & 7;
    if (li >= q + (xcd < r ? 1 : 0)) return;
    conv3x3_halo_tile<1, 256>(a, (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + li, smem);
}
