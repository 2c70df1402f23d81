// =================================================================================================
// v2: LDS-DMA pipeline.  Both operand slabs are moved HBM -> LDS by `buffer_load_dwordx4 ... lds`
// (no staging VGPRs, no ds_write pass, fully asynchronous).  Probed on MI355X
// (tools/probes/lds_dma_probe.hip): the destination is M0-base + lane*16 (lane-linear per wave) and an
// out-of-range voffset WRITES ZEROS, which is exactly the zero padding an implicit GEMM needs: padded
// taps and rows beyond M simply get voffset = 0x80000000.  The XOR swizzle is applied on the SOURCE
// side (lane p of a wave instruction fetches the chunk that belongs at LDS slot p), reads are unchanged.
// NSTAGE-deep LDS ring, ONE raw s_barrier per K-slab, counted vmcnt so that NSTAGE-2 slabs stay in
// flight across the barrier (a __syncthreads would drain them: cdna_hip_programming.md section 5).
// =================================================================================================
// FASTK: Cin % 64 == 0, i.e. every 64-wide K-slab lies inside ONE filter tap -> the tap decode is wave-uniform
// (scalar) and the per-lane part of a gather address is a constant.
// NTHREADS = 256 with a 256 x 256 tile gives the vendor-GEMM shape: 4 waves, each a 128 x 128 wave tile (16 MFMAs per
// 8 fragment reads instead of 4 per 4 -> half the LDS read bytes per FLOP), 2 x 64 KB ring, 1 workgroup per CU.
template <int BMX, int BN, int NSTAGE, bool FASTK, int EPI = 0, int NTHREADS = conv_tile_threads(BMX)>
__global__ __launch_bounds__(NTHREADS) void conv_fwd_dma_kernel(ConvArgs a) {
    constexpr int NWAVES = NTHREADS / 64;            // 64 / 128-row tile: 4 waves, 256 x 128 tile: 8 waves
    constexpr int WAVES_N = (BN >= 128) ? 2 : 1;
    constexpr int WAVES_M = NWAVES / WAVES_N;
    constexpr int WM = BMX / WAVES_M;
    constexpr int WN = BN / WAVES_N;
    constexpr int MT = WM / 32, NT = WN / 32;
    constexpr int A_INSTR = BMX * 8 / 64 / NWAVES;   // = 4: BMX rows x 8 chunks / 64 lanes / waves
    constexpr int B_INSTR = BN * 8 / 64 / NWAVES;    // BN rows x 8 chunks / 64 lanes / waves
    constexpr int IPS = A_INSTR + B_INSTR;           // DMA instructions per thread per stage
    constexpr int STAGE_BYTES = (BMX + BN) * 8 * 16;
    constexpr int NFRAG = MT + NT;                   // ds_read_b128 per k-step

    // ONE LDS array (a second __shared__ object makes hipcc drain vmcnt before every ds_read)
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
    // K-slab range of this workgroup: everything, or slice blockIdx.y of a split-K launch
    const int kbeg = (EPI == 0 && a.partial) ? (int)blockIdx.y * a.kt_per : 0;
    const int KT = (EPI == 0 && a.partial) ? ((kbeg + a.kt_per < a.Kpad / BK) ? kbeg + a.kt_per : a.Kpad / BK) : a.Kpad / BK;
    const int cpt = a.Cin >> 3, ntaps = a.R * a.S;

    // buffer descriptors (wave-uniform kernel arguments only)
    const long long in_bytes = (((long long)a.B * a.H * a.W - 1) * a.in_pix_stride + a.Cin) * 2;
    __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, (int)in_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x7ffffff0, 0x00020000);

    // lane geometry of one wave-level DMA instruction: 8 rows x 8 chunk slots
    const int lrow = lane >> 3, slot = lane & 7;
    int iy0[A_INSTR], ix0[A_INSTR], rowoff[A_INSTR], csrc[A_INSTR];
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i) {
        const int r = (wave * A_INSTR + i) * 8 + lrow;           // row of the tile this lane fetches
        const int m = m0 + r;
        const bool valid = m < a.M;
        const int mm = valid ? m : 0;
        const int hw = a.Ho * a.Wo;
        const int b = mm / hw, rem = mm - b * hw;
        const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
        iy0[i] = valid ? oy * a.stride - a.pad : -0x4000;
        ix0[i] = ox * a.stride - a.pad;
        rowoff[i] = (int)((((long long)b * a.H + (oy * a.stride - a.pad)) * a.W + ix0[i]) * a.in_pix_stride * 2);
        csrc[i] = slot ^ ((r >> 1) & 7);                           // source chunk that lives at this LDS slot
    }
    int boff[B_INSTR];
#pragma unroll
    for (int i = 0; i < B_INSTR; ++i) {
        const int r = (wave * B_INSTR + i) * 8 + lrow;
        boff[i] = ((n0 + r) * a.Kpad + (slot ^ ((r >> 1) & 7)) * 8) * 2;
    }

    // DMA issue for K-slab kt.  Tap arithmetic uses exact reciprocals (host-verified): no LDS table reads here,
    // because hipcc drains vmcnt(0) in front of any compiler-visible LDS read while an LDS-DMA is in flight.
    auto issue = [&](int kt) {
        unsigned char* st = smem + (kt % NSTAGE) * STAGE_BYTES;
        if constexpr (FASTK) {
            // scalar tap decode for the whole slab
            const unsigned kc0 = (unsigned)(kt * 8);
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
                const unsigned kc = (unsigned)(kt * 8 + csrc[i]);
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
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(st + BMX * 128 + (wave * B_INSTR + i) * 1024),
                                                     16, (unsigned)(boff[i] + kt * BK * 2), 0, 0, 0);
    };

    f32x16_t acc[MT][NT];
    if constexpr (EPI == 1) {
        lstm_bias_init<MT, NT>(a, acc, n0, wn, lane);
    } else if constexpr (EPI == 2 || EPI == 3) {
        gru_bias_init<EPI, MT, NT>(a, acc, n0, wn, lane);
    } else {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    }

    // fragment addresses (bytes from the stage base), fixed over the K loop: row r, chunk slot swz(r, ks*2 + half)
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
    uint32_t fa_off[MT], fb_off[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) fa_off[i] = (uint32_t)(wm * WM + i * 32 + (lane & 31)) * 128;
#pragma unroll
    for (int j = 0; j < NT; ++j) fb_off[j] = (uint32_t)(BMX * 128 + (wn * WN + j * 32 + (lane & 31)) * 128);
    const int half = lane >> 5;
    // slot of chunk (ks*2+half) in row r: (ks*2+half) ^ ((r>>1)&7); (r>>1)&7 == ((lane&31)>>1)&7 for every tile row here
    const int rsw = ((lane & 31) >> 1) & 7;

#pragma unroll
    for (int s = 0; s < NSTAGE - 1; ++s)
        if (kbeg + s < KT) issue(kbeg + s);
    constexpr bool LSTM_PREF = (EPI == 1 && MT == 2 && NT == 2);
    LstmPrefetch pref;
    if constexpr (LSTM_PREF) lstm_prefetch(a, pref, m0, n0, tid);

#define OESS_FRAG_READ(DST_A, DST_B, KS)                                                                         \
    {                                                                                                            \
        const uint32_t sl_ = (uint32_t)((((KS) * 2 + half) ^ rsw) * 16);                                         \
        _Pragma("unroll") for (int i = 0; i < MT; ++i)                                                           \
            asm volatile("ds_read_b128 %0, %1" : "=v"(DST_A[i]) : "v"(stage_ + fa_off[i] + sl_) : "memory");   \
        _Pragma("unroll") for (int j = 0; j < NT; ++j)                                                           \
            asm volatile("ds_read_b128 %0, %1" : "=v"(DST_B[j]) : "v"(stage_ + fb_off[j] + sl_) : "memory");   \
    }

    for (int kt = kbeg; kt < KT; ++kt) {
        // retire slab kt: at most NSTAGE-2 younger slabs may stay in flight (fewer at the tail)
        if (kt + NSTAGE - 2 < KT) {
            if constexpr (NSTAGE == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if constexpr ((NSTAGE - 2) * IPS == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
            else if constexpr ((NSTAGE - 2) * IPS == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else if constexpr ((NSTAGE - 2) * IPS == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else if constexpr ((NSTAGE - 2) * IPS == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
            else if constexpr ((NSTAGE - 2) * IPS == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
            else if constexpr ((NSTAGE - 2) * IPS == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();                   // slab kt complete for every wave; buffer of slab kt-1 is free
        if (kt + NSTAGE - 1 < KT) issue(kt + NSTAGE - 1);
        const uint32_t stage_ = lds0 + (uint32_t)((kt % NSTAGE) * STAGE_BYTES);
        bf16x8_t fa0[MT], fb0[NT], fa1[MT], fb1[NT];
        // register double-buffered fragments: reads of k-step ks+1 are in flight under the MFMAs of k-step ks
        __builtin_amdgcn_s_setprio(3);
        OESS_FRAG_READ(fa0, fb0, 0)
        OESS_FRAG_READ(fa1, fb1, 1)
        OESS_FRAG_WAIT(NFRAG, fa0, fb0)
        OESS_FRAG_MMA(fa0, fb0)
        OESS_FRAG_READ(fa0, fb0, 2)
        OESS_FRAG_WAIT(NFRAG, fa1, fb1)
        OESS_FRAG_MMA(fa1, fb1)
        OESS_FRAG_READ(fa1, fb1, 3)
        OESS_FRAG_WAIT(NFRAG, fa0, fb0)
        OESS_FRAG_MMA(fa0, fb0)
        OESS_FRAG_WAIT(0, fa1, fb1)
        OESS_FRAG_MMA(fa1, fb1)
        __builtin_amdgcn_s_setprio(0);
    }
#undef OESS_FRAG_READ
    __syncthreads();

    if constexpr (LSTM_PREF) lstm_epilogue<MT, NT, true, false>(a, acc, smem, m0, n0, wm, wn, lane, tid, &pref);
    else if constexpr (EPI == 1) lstm_epilogue<MT, NT, false, false>(a, acc, smem, m0, n0, wm, wn, lane, tid);
    else if constexpr (EPI == 2) gru_gates_epilogue<MT, NT>(a, acc, smem, m0, n0, wm, wn, lane, tid);       // convgru_epilogue.h
    else if constexpr (EPI == 3) gru_out_epilogue<MT, NT>(a, acc, smem, m0, n0, wm, wn, lane, tid);
    else {
        if (a.partial) {        // split-K slice: raw fp32 accumulators, 128-byte row segments per half wave
            float* dst = a.partial + (size_t)blockIdx.y * (size_t)a.M * a.Cout;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int n = n0 + wn * WN + j * 32 + (lane & 31);
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int m = m0 + wm * WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                        if (m < a.M && n < a.Cout) dst[(size_t)m * a.Cout + n] = acc[i][j][e];
                    }
                }
            return;
        }
        conv_epilogue<BMX, BN, BN + 8, NTHREADS, WAVES_N>(a, acc, smem, m0, n0, wm, wn, lane, tid);
    }
}

// Split-K tail: out[m][n] = act(sum_z partial[z][m][n] + bias[n] [+ residual]) as bf16 NHWC, slices added in z order
// (deterministic), plus the per-128-row-tile column sums / sums of squares of the fp32 result that the conv epilogue
// provides for BatchNorm (same [tiles_m][2][Cout] layout).  grid = (tiles_m, ceil(Cout / 64)); thread = (row lane, 4 columns).
__global__ __launch_bounds__(256) void splitk_reduce_kernel(ConvArgs a) {
    __shared__ float red[16][64][2];
    const int tile = blockIdx.x, n = blockIdx.y * 64 + (threadIdx.x & 15) * 4, rl = threadIdx.x >> 4;
    const size_t MN = (size_t)a.M * a.Cout;
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    const bool n_ok = n < a.Cout;               // Cout % 4 == 0 (host-checked): a float4 is inside the row or not at all
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.bias && n_ok) { bv[0] = a.bias[n]; bv[1] = a.bias[n + 1]; bv[2] = a.bias[n + 2]; bv[3] = a.bias[n + 3]; }
    for (int r = rl; r < 128; r += 16) {
        const int m = tile * 128 + r;
        if (m >= a.M || !n_ok) continue;
        const float* p = a.partial + (size_t)m * a.Cout + n;
        float4 v = *reinterpret_cast<const float4*>(p);
        for (int z = 1; z < a.ksplit; ++z) {
            const float4 w = *reinterpret_cast<const float4*>(p + (size_t)z * MN);
            v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
        }
        float f[4] = {v.x + bv[0], v.y + bv[1], v.z + bv[2], v.w + bv[3]};
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float q = bf16_to_f32(f32_to_bf16(f[k])); s1[k] += q; s2[k] += q * q; }   // statistics of the stored values
        if (a.out_f32) {
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = conv_act(f[k], a.relu);
            *reinterpret_cast<float4*>(a.out_f32 + (long long)m * a.out_pix_stride + n) = make_float4(f[0], f[1], f[2], f[3]);
            continue;
        }
        if (a.residual || a.relu) {
            // the one-pass epilogue rounds the conv result to bf16 BEFORE the residual add: keep that rounding point
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float t = bf16_to_f32(f32_to_bf16(f[k]));
                if (a.residual) t += bf16_to_f32(a.residual[(long long)m * a.res_pix_stride + n + k]);
                f[k] = conv_act(t, a.relu);
            }
        }
        uint2 o;
        o.x = pack_bf16x2(f[0], f[1]);
        o.y = pack_bf16x2(f[2], f[3]);
        *reinterpret_cast<uint2*>(a.out + (long long)m * a.out_pix_stride + n) = o;
    }
    if (!a.stats) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) { red[rl][(threadIdx.x & 15) * 4 + k][0] = s1[k]; red[rl][(threadIdx.x & 15) * 4 + k][1] = s2[k]; }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int nn = blockIdx.y * 64 + threadIdx.x;
        if (nn < a.Cout) {
            float t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { t1 += red[r][threadIdx.x][0]; t2 += red[r][threadIdx.x][1]; }
            a.stats[((size_t)tile * 2 + 0) * a.Cout + nn] = t1;
            a.stats[((size_t)tile * 2 + 1) * a.Cout + nn] = t2;
        }
    }
}
