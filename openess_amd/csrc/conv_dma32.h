// =================================================================================================
// v4: BK = 32 slabs in a 4-deep LDS ring (same 64 KB per workgroup, still 2 workgroups per CU).
// The 2-stage BK = 64 kernel has ONE slab in flight per workgroup and must hide the whole L2 -> LDS round trip
// (~1.0-1.3 us under load) behind one slab of MFMAs (0.54 us when two workgroups share the CU): it is latency bound
// (tools/conv_ablate.py).  Here three 32-wide slabs are in flight (48 KB instead of 32 KB per workgroup) and a slab
// is issued three compute phases before it is needed.  64-byte LDS rows: chunk c of row r lives at
// c ^ ((r >> 2) & 3) (conflict free for the ds_read_b128 lane groups), one wave DMA instruction covers 16 rows.
// =================================================================================================
template <int BN, bool FASTK, int EPI = 0, int NST = 4>
__global__ __launch_bounds__(256) void conv_fwd_dma32_kernel(ConvArgs a) {
    constexpr int BMX = 128, BKS = 32, NWAVES = 4;
    constexpr int WAVES_N = (BN == 128) ? 2 : 1;
    constexpr int WAVES_M = NWAVES / WAVES_N;
    constexpr int WM = BMX / WAVES_M;
    constexpr int WN = BN / WAVES_N;
    constexpr int MT = WM / 32, NT = WN / 32;
    constexpr int A_INSTR = BMX / 16 / NWAVES;        // 2: 16 rows x 64 B per wave instruction
    constexpr int B_INSTR = BN / 16 / NWAVES;         // 2 (BN = 128) or 1 (BN = 64)
    constexpr int IPS = A_INSTR + B_INSTR;
    constexpr int A_BYTES = BMX * 64;
    constexpr int STAGE_BYTES = (BMX + BN) * 64;
    constexpr int NFRAG = MT + NT;
    static_assert(BN == 128 || BN == 64, "BN");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nwg = a.tiles_m * a.tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tile_n = bid % a.tiles_n, tile_m = bid / a.tiles_n;
    const int m0 = tile_m * BMX, n0 = tile_n * BN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int KT = a.Kpad / BKS;
    const int cpt = a.Cin >> 3, ntaps = a.R * a.S;

    const long long in_bytes = (((long long)a.B * a.H * a.W - 1) * a.in_pix_stride + a.Cin) * 2;
    __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, (int)in_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x7ffffff0, 0x00020000);

    const int lrow = lane >> 2, slot = lane & 3;       // 16 rows x 4 chunk slots per wave instruction
    int iy0[A_INSTR], ix0[A_INSTR], rowoff[A_INSTR], csrc[A_INSTR];
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i) {
        const int r = (wave * A_INSTR + i) * 16 + lrow;
        const int m = m0 + r;
        const bool valid = m < a.M;
        const int mm = valid ? m : 0;
        const int hw = a.Ho * a.Wo;
        const int b = mm / hw, rem = mm - b * hw;
        const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
        iy0[i] = valid ? oy * a.stride - a.pad : -0x4000;
        ix0[i] = ox * a.stride - a.pad;
        rowoff[i] = (int)((((long long)b * a.H + (oy * a.stride - a.pad)) * a.W + ix0[i]) * a.in_pix_stride * 2);
        csrc[i] = slot ^ ((r >> 2) & 3);
    }
    int boff[B_INSTR];
#pragma unroll
    for (int i = 0; i < B_INSTR; ++i) {
        const int r = (wave * B_INSTR + i) * 16 + lrow;
        boff[i] = ((n0 + r) * a.Kpad + (slot ^ ((r >> 2) & 3)) * 8) * 2;
    }

    auto issue = [&](int kt) {
        unsigned char* st = smem + (kt % NST) * STAGE_BYTES;
        if constexpr (FASTK) {
            const unsigned kc0 = (unsigned)(kt * 4);
            const unsigned tap = (kc0 * a.inv_cpt) >> 20;
            const int cc0 = (int)(kc0 - tap * cpt);
            const unsigned r = (tap * a.inv_s) >> 16;
            const int sx = (int)(tap - r * a.S);
            const int dy = (int)r * a.dil, dx = sx * a.dil;
            const int tapoff = ((dy * a.W + dx) * (int)a.in_pix_stride + cc0 * 8) * 2;
            const bool tap_ok = (int)tap < ntaps;
#pragma unroll
            for (int i = 0; i < A_INSTR; ++i) {
                const bool ok = tap_ok && (unsigned)(iy0[i] + dy) < (unsigned)a.H && (unsigned)(ix0[i] + dx) < (unsigned)a.W;
                const unsigned voff = ok ? (unsigned)(rowoff[i] + csrc[i] * 16 + tapoff) : 0x80000000u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(st + (wave * A_INSTR + i) * 1024),
                                                         16, voff, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < A_INSTR; ++i) {
                const unsigned kc = (unsigned)(kt * 4 + csrc[i]);
                const unsigned tap = (kc * a.inv_cpt) >> 20;
                const int cc = (int)(kc - tap * cpt);
                const unsigned r = (tap * a.inv_s) >> 16;
                const int sx = (int)(tap - r * a.S);
                const int dy = (int)r * a.dil, dx = sx * a.dil;
                const bool ok = (int)tap < ntaps && (unsigned)(iy0[i] + dy) < (unsigned)a.H && (unsigned)(ix0[i] + dx) < (unsigned)a.W;
                const unsigned voff = ok ? (unsigned)(rowoff[i] + ((dy * a.W + dx) * (int)a.in_pix_stride + cc * 8) * 2) : 0x80000000u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(st + (wave * A_INSTR + i) * 1024),
                                                         16, voff, 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < B_INSTR; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(st + A_BYTES + (wave * B_INSTR + i) * 1024),
                                                     16, (unsigned)(boff[i] + kt * BKS * 2), 0, 0, 0);
    };

    f32x16_t acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    uint32_t fa_off[MT], fb_off[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) fa_off[i] = (uint32_t)(wm * WM + i * 32 + (lane & 31)) * 64;
#pragma unroll
    for (int j = 0; j < NT; ++j) fb_off[j] = (uint32_t)(A_BYTES + (wn * WN + j * 32 + (lane & 31)) * 64);
    const int half = lane >> 5;
    const int rsw = ((lane & 31) >> 2) & 3;
    const uint32_t sl0 = (uint32_t)(((0 + half) ^ rsw) * 16), sl1 = (uint32_t)(((2 + half) ^ rsw) * 16);

#pragma unroll
    for (int s = 0; s < NST - 1; ++s)
        if (s < KT) issue(s);

#define OESS_FR32(DST_A, DST_B, SL)                                                                              \
    {                                                                                                            \
        _Pragma("unroll") for (int i = 0; i < MT; ++i)                                                           \
            asm volatile("ds_read_b128 %0, %1" : "=v"(DST_A[i]) : "v"(stage_ + fa_off[i] + SL) : "memory");     \
        _Pragma("unroll") for (int j = 0; j < NT; ++j)                                                           \
            asm volatile("ds_read_b128 %0, %1" : "=v"(DST_B[j]) : "v"(stage_ + fb_off[j] + SL) : "memory");     \
    }

    for (int kt = 0; kt < KT; ++kt) {
        // retire slab kt; up to two younger slabs stay in flight across the barrier
        if (NST == 4 && kt + 2 < KT) {
            if constexpr (IPS == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        } else if (kt + 1 < KT) {
            if constexpr (IPS == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();                   // slab kt visible to every wave; the stage of slab kt-1 is free
        if (kt + NST - 1 < KT) issue(kt + NST - 1);
        const uint32_t stage_ = lds0 + (uint32_t)((kt % NST) * STAGE_BYTES);
        bf16x8_t fa0[MT], fb0[NT], fa1[MT], fb1[NT];
        OESS_FR32(fa0, fb0, sl0)
        OESS_FR32(fa1, fb1, sl1)
        OESS_FRAG_WAIT(NFRAG, fa0, fb0)
        OESS_FRAG_MMA(fa0, fb0)
        OESS_FRAG_WAIT(0, fa1, fb1)
        OESS_FRAG_MMA(fa1, fb1)
    }
#undef OESS_FR32
    __syncthreads();

    if constexpr (EPI == 1) lstm_epilogue(a, acc, smem, m0, n0, wm, wn, lane, tid);
    else conv_epilogue<BMX, BN>(a, acc, smem, m0, n0, wm, wn, lane, tid);
}
