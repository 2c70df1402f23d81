// Register-staged general kernel (conv_fwd_kernel): any R x S, stride, padding, dilation and Cin % 8 == 0.
//
// Kernel: 128 x BN output tile per 256-thread workgroup (4 waves), BK = 64.
//   - A and B K-slabs are gathered with 16-byte loads (8 channels of one filter tap) into registers
//     and written to an XOR-swizzled LDS image (16-byte chunk c of row r lives at c ^ ((r>>1)&7):
//     conflict-free ds_read_b128 for the 32x32x16 fragment pattern);
//   - next slab's global loads are issued before the MFMA block of the current slab (register
//     staging: the zero fill of padded taps needs per-lane predication, which LDS-DMA cannot do);
//   - v_mfma_f32_32x32x16_bf16, each wave owns a 64 x 64 (BN=128), 32 x 64 (BN=64) or 32 x 32
//     (BN=32) accumulator block;
//   - epilogue: bias + optional ReLU in fp32, convert to bf16, transpose through LDS and store
//     whole NHWC rows with 16-byte stores (or fp32 direct stores for the small logits heads).
//   - workgroup ids are remapped so that the n-tiles of one m-tile land on the same XCD (shared L2).

template <int BN>
__global__ __launch_bounds__(CONV_THREADS) void conv_fwd_kernel(ConvArgs a) {
    // wave layout: BN=128 -> 2x2 waves of 64x64; BN=64 -> 4x1 waves of 32x64; BN=32 -> 4x1 waves of 32x32
    constexpr int WAVES_N = (BN == 128) ? 2 : 1;
    constexpr int WAVES_M = 4 / WAVES_N;
    constexpr int WM = BM / WAVES_M;          // 64 or 32
    constexpr int WN = BN / WAVES_N;          // 64, 64 or 32
    constexpr int MT = WM / 32, NT = WN / 32;
    constexpr int B_ROWS_PER_THREAD = BN / 32;   // 16-byte chunks of the B slab per thread

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // LDS: 2 x { A slab [BM][8] chunks, B slab [BN][8] chunks } (double buffered), then the tap table
    constexpr int STAGE_CHUNKS = (BM + BN) * 8;
    u32x4_t* lbase = reinterpret_cast<u32x4_t*>(smem);
    int2* ltab = reinterpret_cast<int2*>(smem + 2 * STAGE_CHUNKS * 16);      // [Kpad/8] {element offset, dy | dx<<16}

    // ---- XCD-aware tile mapping (bijective): consecutive logical tiles share an XCD's L2
    const int nwg = a.tiles_m * a.tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tile_n = bid % a.tiles_n, tile_m = bid / a.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int KT = a.Kpad / BK;

    // ---- tap table, built once per workgroup: chunk kc -> (r, s, channel chunk).  Keeps the two integer
    //      divisions out of the K loop (they were ~40 % of its VALU work).
    {
        const int cpt = a.Cin >> 3, ntaps = a.R * a.S;
        for (int kc = tid; kc < KT * 8; kc += CONV_THREADS) {
            const int tap = kc / cpt, cc = kc - tap * cpt;
            const int r = tap / a.S, s = tap - r * a.S;
            int2 e;
            if (tap < ntaps) {
                const int dy = r * a.dil, dx = s * a.dil;
                e.x = (dy * a.W + dx) * (int)a.in_pix_stride + cc * 8;
                e.y = (dy & 0xffff) | (dx << 16);
            } else {
                e.x = 0;
                e.y = 0x7fff | (0x7fff << 16);                  // far outside: fails every bounds test
            }
            ltab[kc] = e;
        }
    }

    // ---- per-thread gather state: chunk column c (fixed), rows (tid>>3) + 32*i
    const int c = tid & 7;
    const int row0 = tid >> 3;
    int iy0[4], ix0[4];
    const uint16_t* rowptr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + row0 + 32 * i;
        const bool valid = m < a.M;
        const int mm = valid ? m : 0;
        const int hw = a.Ho * a.Wo;
        const int b = mm / hw, rem = mm - b * hw;
        const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
        iy0[i] = valid ? oy * a.stride - a.pad : -0x4000;       // invalid rows fail the bounds test
        ix0[i] = ox * a.stride - a.pad;
        rowptr[i] = a.in + (((long long)b * a.H + (oy * a.stride - a.pad)) * a.W + ix0[i]) * a.in_pix_stride;
    }
    const uint16_t* wrow = a.w + (size_t)(n0 + row0) * a.Kpad + c * 8;

    u32x4_t ra[4], rb[B_ROWS_PER_THREAD];
    const u32x4_t zero4 = {0u, 0u, 0u, 0u};
    // global -> registers for K-slab KT_IDX.  Loads are unconditional (clamped to the tensor base) and
    // zeroed by select afterwards, so the four gathers issue back to back without exec-mask branches.
#define OESS_GLOAD(KT_IDX)                                                                                          \
    {                                                                                                               \
        const int2 e_ = ltab[(KT_IDX) * 8 + c];                                                                     \
        const int dy_ = (int)(short)(e_.y & 0xffff), dx_ = e_.y >> 16;                                              \
        bool ok_[4];                                                                                                \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                             \
            ok_[i] = (unsigned)(iy0[i] + dy_) < (unsigned)a.H && (unsigned)(ix0[i] + dx_) < (unsigned)a.W;          \
            const uint16_t* src_ = ok_[i] ? rowptr[i] + e_.x : a.in;                                                \
            ra[i] = *reinterpret_cast<const u32x4_t*>(src_);                                                        \
        }                                                                                                           \
        _Pragma("unroll") for (int i = 0; i < B_ROWS_PER_THREAD; ++i)                                               \
            rb[i] = *reinterpret_cast<const u32x4_t*>(wrow + (size_t)(32 * i) * a.Kpad + (size_t)(KT_IDX) * BK);    \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) ra[i] = ok_[i] ? ra[i] : zero4;                               \
    }
#define OESS_LSTORE(BUF)                                                                               \
    {                                                                                                  \
        u32x4_t* lA_ = lbase + (BUF) * STAGE_CHUNKS;                                                   \
        u32x4_t* lB_ = lA_ + BM * 8;                                                                   \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                \
            const int r_ = row0 + 32 * i;                                                              \
            lA_[r_ * 8 + swz(r_, c)] = ra[i];                                                          \
        }                                                                                              \
        _Pragma("unroll") for (int i = 0; i < B_ROWS_PER_THREAD; ++i) {                                \
            const int r_ = row0 + 32 * i;                                                              \
            lB_[r_ * 8 + swz(r_, c)] = rb[i];                                                          \
        }                                                                                              \
    }

    f32x16_t acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    __syncthreads();                                   // tap table visible
    OESS_GLOAD(0)
    OESS_LSTORE(0)
    __syncthreads();
    if (KT > 1) OESS_GLOAD(1)
    // double-buffered LDS: ONE barrier per K-slab.  compute(buf) -> store next slab into the other buffer ->
    // barrier -> issue the global loads two slabs ahead (they fly under the next compute).
    for (int kt = 0; kt < KT; ++kt) {
        const u32x4_t* lA = lbase + (kt & 1) * STAGE_CHUNKS;
        const u32x4_t* lB = lA + BM * 8;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            bf16x8_t fa[MT], fb[NT];
            const int chunk = ks * 2 + (lane >> 5);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int r = wm * WM + i * 32 + (lane & 31);
                fa[i] = *reinterpret_cast<const bf16x8_t*>(&lA[r * 8 + swz(r, chunk)]);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int r = wn * WN + j * 32 + (lane & 31);
                fb[j] = *reinterpret_cast<const bf16x8_t*>(&lB[r * 8 + swz(r, chunk)]);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < KT) {
            OESS_LSTORE((kt + 1) & 1)
            __syncthreads();
            if (kt + 2 < KT) OESS_GLOAD(kt + 2)
        }
    }
    __syncthreads();                                   // all LDS reads done before the epilogue reuses smem

    conv_epilogue<BM, BN>(a, acc, smem, m0, n0, wm, wn, lane, tid);
}
