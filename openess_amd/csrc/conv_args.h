// Shared by every bf16 convolution family (included by conv_fwd.hip inside its anonymous namespace): operand typedefs,
// ConvArgs, the LDS swizzle, the output store, the activation, the common epilogue and the fused ConvLSTM epilogue.
//
// Implicit-GEMM 2-D convolution for gfx950 (bf16 in, fp32 MFMA accumulate).
//
//   out[m, n] = act( sum_k A[m, k] * Wp[n, k] + bias[n] ),   m = (b, oy, ox),  k = (r, s, ci)
//   A[m, k]  = in[b, oy*stride - pad + r*dil, ox*stride - pad + s*dil, ci]   (0 outside the image)
//
// Layout: activations are NHWC bf16 with an explicit pixel stride (so a conv can read or write a
// channel slice of a wider concat buffer: skip connections and ConvLSTM cat(x, h) need no copy).
// Weights are pre-packed once to Wp[Npad][Kpad] bf16, K ordered (r, s, ci), zero padded to the
// tile sizes, so the B operand is a plain row-major panel.

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;     // 8 bf16 = 4 VGPRs (MFMA A/B operand)
typedef __attribute__((ext_vector_type(16))) float f32x16_t;    // 32x32 accumulator fragment
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t; // 16-byte staging register (native vector: stays in VGPRs)

constexpr int BM = 128;
constexpr int BK = 64;
constexpr int CONV_THREADS = 256;

struct ConvArgs {
    const uint16_t* in;      // NHWC bf16
    const uint16_t* w;       // packed [Npad][Kpad]
    const float* bias;       // [Cout] or null
    uint16_t* out;           // NHWC bf16 (or null when out_f32 is set)
    float* out_f32;          // NHWC fp32 alternative output
    const uint16_t* residual;  // optional NHWC bf16 tensor added before the activation (same pixel stride as out)
    float* stats;              // optional [tiles_m][2][Cout] per-tile column sums / sums of squares of the fp32 result
    long long in_pix_stride, out_pix_stride, res_pix_stride;
    int B, H, W, Cin;        // input geometry; Cin % 8 == 0
    int Ho, Wo, Cout;
    int R, S, stride, pad, dil;
    int Kpad;                // multiple of BK
    int M;                   // B*Ho*Wo
    int relu;
    int tiles_m, tiles_n;
    // fused ConvLSTM epilogue (EPI == 1): Cout = 4*lstm_C gate-interleaved rows (n' = 4*hc + gate)
    const float* lstm_prev;    // [M][C] fp32 previous cell state or null (= zero state)
    float* lstm_cell;          // [M][C] fp32 new cell state (may alias lstm_prev: a tile only touches its own block)
    uint16_t* lstm_h;          // hidden output, bf16, pixel stride lstm_h_stride (must NOT alias the conv input)
    long long lstm_h_stride;
    int lstm_C;
    unsigned inv_cpt, inv_s;   // exact small-range reciprocals: kc / cpt == (kc * inv_cpt) >> 20, tap / S == (tap * inv_s) >> 16
    // split-K (small-M, long-K layers: DeepLab's ASPP at output stride 16): grid.y = ksplit, workgroup (tile, z) reduces
    // K-slabs [z * kt_per, (z + 1) * kt_per) and writes its fp32 accumulators to partial[z][M][Cout]; splitk_reduce_kernel
    // adds the slices in a fixed order and does what the epilogue would have done (bias / residual / activation / tile stats)
    float* partial;
    int ksplit, kt_per;
    // row-halo kernel: exact reciprocals of W and W + dil for the small per-lane quotients of its prologue (x < 256:
    // x / d == umulhi(x, floor(2^32 / d) + 1) whenever x * d < 2^32); 0 = divide
    unsigned mg_w, mg_wd;
    // fused ConvGRU epilogues (EPI == 2 gates, EPI == 3 output: convgru_epilogue.h).  They reuse lstm_prev (fp32 master of
    // h_prev or null = zero state), lstm_cell (EPI 2: u out; EPI 3: the new fp32 master), lstm_h / lstm_h_stride (EPI 2: the
    // r*h window; EPI 3: the bf16 copy of the master) and lstm_C.
    const float* gru_u;        // EPI 3: [M][C] fp32 update gate written by the gates launch
    float* gru_rh32;           // EPI 2: optional [M][C] fp32 r*h before its bf16 rounding (tests), or null
};

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

// 16-byte store of a finished output row piece.  OESS_OUT_STORE: 0 = plain (write-back in the XCD's L2), 1 = non-temporal,
// 2 = agent scope (write-through).  The end of a kernel writes the XCD L2s' dirty lines back before the next kernel of the
// stream may start (8 non-coherent L2s): the fewer dirty lines a kernel leaves, the shorter the gap behind it.
#define OESS_OUT_STORE 0
__device__ __forceinline__ void out_store16(void* p, uint4 v) {
#if OESS_OUT_STORE == 1
    __builtin_nontemporal_store(u32x4_t{v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4_t*>(p));
#elif OESS_OUT_STORE == 2
    asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(p), "v"(u32x4_t{v.x, v.y, v.z, v.w}) : "memory");
#else
    *reinterpret_cast<uint4*>(p) = v;
#endif
}

// threads per workgroup of the LDS-DMA kernel by tile height: 64- and 128-row tiles 4 waves, 256-row tiles 8 waves
constexpr int conv_tile_threads(int bmx) { return bmx == 256 ? 512 : 256; }

// epilogue activation: 0 none, 1 ReLU, 2 GELU (exact erf form = nn.GELU(), the ViT FFN of models/maskclip_model.py)
// erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, i.e. 2^-15 of the bf16 result's ulp): one exp, one rcp, five FMAs instead
// of the ~50-instruction library erff.  The GELU epilogue of the ViT's fc1 (256 x 256 tiles, one workgroup per CU, nothing to
// hide an epilogue behind) spent a third of its workgroup lifetime in erff: 128 calls per thread.
__device__ __forceinline__ float fast_erf(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * ax);
    const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    const float r = 1.0f - poly * __expf(-ax * ax);
    return copysignf(r, x);
}
__device__ __forceinline__ float conv_act(float v, int mode) {
    if (mode == 1) return fmaxf(v, 0.0f);
    if (mode == 2) return 0.5f * v * (1.0f + fast_erf(v * 0.70710678118654752f));
    return v;
}

// PITCH: row pitch (elements) of the bf16 LDS image (BN + 8: padded, conflict-free 16-byte row reads).
template <int BMX, int BN, int PITCH = BN + 8, int NTHREADS = conv_tile_threads(BMX), int WAVES_N = (BN == 128) ? 2 : 1>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a,
                                              f32x16_t (&acc)[BMX / ((NTHREADS / 64) / WAVES_N) / 32][(BN / WAVES_N) / 32],
                                              unsigned char* smem, int m0, int n0, int wm, int wn, int lane, int tid,
                                              float* red_override = nullptr) {
    constexpr int WAVES_M = (NTHREADS / 64) / WAVES_N;
    constexpr int WM = BMX / WAVES_M;
    constexpr int WN = BN / WAVES_N;
    constexpr int MT = WM / 32, NT = WN / 32;
    // ---- epilogue.  C/D layout of 32x32 MFMA: col = lane & 31, row = (e & 3) + 8*(e >> 2) + 4*(lane >> 5)
    const int ncol_l = lane & 31;
    if (a.out_f32) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = n0 + wn * WN + j * 32 + ncol_l;
                const float bv = (a.bias && n < a.Cout) ? a.bias[n] : 0.0f;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = m0 + wm * WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                    if (m < a.M && n < a.Cout) {
                        float v = acc[i][j][e] + bv;
                        v = conv_act(v, a.relu);
                        a.out_f32[(long long)m * a.out_pix_stride + n] = v;
                    }
                }
            }
        return;
    }
    // bf16 path: stage the tile as [BM][BN] bf16 in LDS (row pitch BN*2 + 16 bytes against bank conflicts)
    uint16_t* lC = reinterpret_cast<uint16_t*>(smem);
    float* red = red_override ? red_override : reinterpret_cast<float*>(smem + BMX * PITCH * 2);   // [WAVES_M][BN][2] (BatchNorm partials)
    // bf16 image + (optionally) per-column sum / sum of squares over this tile's rows of the values AS STORED (rounded to bf16): the
    // statistics then describe exactly the tensor that BatchNorm normalises afterwards (sum of xhat == 0 over the stored values),
    // which the backward needs -- with statistics of the un-rounded accumulators the residual mean of the rounding errors times
    // d(beta) leaks into d(gamma), a second noise term as large as the rounding noise itself on common-mode gradients (measured:
    // BatchNorm weight-gradient cosine 0.74 -> 0.51 on the DeepLab test).  Rows >= M are exact zeros (their A rows were zero
    // filled; stats are only requested for bias-free convs).  One rounding per value serves both the image and the sums.
    auto stage = [&](auto with_stats) __attribute__((always_inline)) {
        constexpr bool WS = decltype(with_stats)::value;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int nl = wn * WN + j * 32 + ncol_l;
            const int n = n0 + nl;
            const float bv = (a.bias && n < a.Cout) ? a.bias[n] : 0.0f;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int ml = wm * WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                    const uint32_t pk = pack_bf16x2(acc[i][j][e] + bv, 0.0f);      // activation applied after the residual
                    lC[ml * PITCH + nl] = (uint16_t)pk;
                    if constexpr (WS) {
                        const float v = __uint_as_float(pk << 16);
                        s1 += v; s2 += v * v;
                    }
                }
            if constexpr (WS) {
                s1 += __shfl_xor(s1, 32, 64);
                s2 += __shfl_xor(s2, 32, 64);
                if (lane < 32) {
                    const int col = wn * WN + j * 32 + lane;
                    red[(wm * BN + col) * 2 + 0] = s1;
                    red[(wm * BN + col) * 2 + 1] = s2;
                }
            }
        }
    };
    // Residual rows of this thread's output pieces are requested all at once between the staging writes and the barrier (the
    // accumulators are dead there, so the ITERS 16-byte pieces -- 16 on the 256 x 256 tile, 8 / 4 on the 128- / 64-row tiles --
    // reuse their registers): one L2 / HBM latency under the barrier instead of one per store-loop iteration (the 512 -> 2048
    // layer at M = 140 800 ran 657 us with a residual against 417 us without one: a workgroup that owns its CU has no other
    // wave to hide the loads).  Requested before the staging they would cost the 128-row kernels their third wave per SIMD.
    constexpr int CHUNKS_N = BN / 8;                       // 16-byte chunks per tile row
    constexpr int ITERS = (BMX * CHUNKS_N + NTHREADS - 1) / NTHREADS;
    if (a.stats) stage(std::true_type{});
    else stage(std::false_type{});
    uint4 rsv[ITERS];
    if (a.residual) {
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int idx = tid + it * NTHREADS;
            const int ml = idx / CHUNKS_N, cn = idx - ml * CHUNKS_N;
            const int m = m0 + ml, n = n0 + cn * 8;
            rsv[it] = make_uint4(0u, 0u, 0u, 0u);
            if (idx < BMX * CHUNKS_N && m < a.M && n + 8 <= a.Cout)
                rsv[it] = *reinterpret_cast<const uint4*>(a.residual + (long long)m * a.res_pix_stride + n);
        }
    }
    __syncthreads();
    if (a.stats && tid < BN) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES_M; ++w) { s1 += red[(w * BN + tid) * 2]; s2 += red[(w * BN + tid) * 2 + 1]; }
        const int n = n0 + tid;
        if (n < a.Cout) {
            // tile_stats rows are per 128 output rows; a 256-row tile fills row 2t and zeroes row 2t+1
            const int trow = (m0 / BMX) * (BMX / 128);
            a.stats[((size_t)trow * 2 + 0) * a.Cout + n] = s1;
            a.stats[((size_t)trow * 2 + 1) * a.Cout + n] = s2;
            if (BMX == 256 && m0 + 128 < a.M) {
                a.stats[((size_t)(trow + 1) * 2 + 0) * a.Cout + n] = 0.f;
                a.stats[((size_t)(trow + 1) * 2 + 1) * a.Cout + n] = 0.f;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int idx = tid + it * NTHREADS;
        if (idx >= BMX * CHUNKS_N) break;
        const int ml = idx / CHUNKS_N, cn = idx - ml * CHUNKS_N;
        const int m = m0 + ml, n = n0 + cn * 8;
        if (m >= a.M || n >= a.Cout) continue;
        uint4 v = *reinterpret_cast<const uint4*>(&lC[ml * PITCH + cn * 8]);
        uint16_t* dst = a.out + (long long)m * a.out_pix_stride + n;
        union { uint4 q4; uint16_t h[8]; } u, rs;
        u.q4 = v;
        rs.q4 = make_uint4(0u, 0u, 0u, 0u);
        const bool full = n + 8 <= a.Cout;
        if (a.residual) {
            if (full) rs.q4 = rsv[it];
            else {
#pragma unroll
                for (int q = 0; q < 8; ++q) if (n + q < a.Cout) rs.h[q] = a.residual[(long long)m * a.res_pix_stride + n + q];
            }
        }
        if (a.residual || a.relu) {
            float f[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                f[q] = bf16_to_f32(u.h[q]);
                if (a.residual) f[q] += bf16_to_f32(rs.h[q]);
                f[q] = conv_act(f[q], a.relu);
            }
            u.q4 = pack_bf16x8(f);
        }
        if (full) {
            out_store16(dst, u.q4);
        } else {                                   // ragged channel tail (Cout % 8 != 0)
#pragma unroll
            for (int q = 0; q < 8; ++q) if (n + q < a.Cout) dst[q] = u.h[q];
        }
    }
}


// ---- fused ConvLSTM cell update (e2vid/model/submodules.py:205-212) straight from the accumulators.
// The gate convolution is run TRANSPOSED (D^T = W * A^T: the packed weight is the MFMA A operand), so a lane
// holds, for ONE pixel (col = lane & 31), rows (e&3) + 8*(e>>2) + 4*(lane>>5) of the 32-row n block; with the
// weight rows packed gate-interleaved (n' = 4*hc + gate) the four registers e = 4*q .. 4*q+3 are exactly the
// (in, remember, out, cell) pre-activations of hidden channel 2*q + (lane>>5): the LSTM algebra is lane local,
// the 4C-channel gate tensor never exists in memory, and c / h leave through padded LDS images as full rows.
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float fast_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

// Previous cell state of a 128-row x 32-hidden-channel tile, fetched COALESCED (whole 128-byte rows, float4 per lane)
// at kernel start so the loads retire under the K loop; the epilogue redistributes it through LDS.  (Read in place by
// the lanes that own the gates it would be 16 loads per lane touching 32 different lines each, issued after the K loop.)
struct LstmPrefetch { float4 v[4]; };
__device__ __forceinline__ void lstm_prefetch(const ConvArgs& a, LstmPrefetch& p, int m0, int n0, int tid) {
    const int hc0 = n0 >> 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = tid + 256 * k, row = idx >> 3, c4 = idx & 7;
        const int m = m0 + row;
        p.v[k] = (a.lstm_prev && m < a.M) ? *reinterpret_cast<const float4*>(a.lstm_prev + (long long)m * a.lstm_C + hc0 + c4 * 4)
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// accumulator start values = the gate biases (EPI == 1 kernels that pass ADD_BIAS = false to the epilogue): the 64 bias
// loads per lane leave the epilogue and hide under the first operand fetch
template <int MT, int NT>
__device__ __forceinline__ void lstm_bias_init(const ConvArgs& a, f32x16_t (&acc)[MT][NT], int n0, int wn, int lane) {
    const int hi = lane >> 5, hc0 = n0 >> 2, C = a.lstm_C;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int hc = hc0 + wn * 8 * NT + j * 8 + 2 * q + hi;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float b = a.bias ? a.bias[g * C + hc] : 0.0f;
#pragma unroll
                for (int i = 0; i < MT; ++i) acc[i][j][q * 4 + g] = b;
            }
        }
}

template <int MT = 2, int NT = 2, bool PREF = false, bool ADD_BIAS = true>
__device__ __forceinline__ void lstm_epilogue(const ConvArgs& a, f32x16_t (&acc)[MT][NT], unsigned char* smem, int m0, int n0,
                                              int wm, int wn, int lane, int tid, const LstmPrefetch* pref = nullptr) {
    // 2 x 2 waves; workgroup tile = 64*MT rows x 64*NT gate columns = 16*NT hidden channels
    constexpr int ROWS = 64 * MT, HC = 16 * NT;
    constexpr int CP = HC + 1, HP = HC + 2;                // LDS pitches: fp32 cell image, bf16 hidden image
    static_assert(!PREF || (MT == 2 && NT == 2), "prefetch layout is the 128 x 128 tile's");
    float* lc = reinterpret_cast<float*>(smem);            // [ROWS][CP]
    uint16_t* lh = reinterpret_cast<uint16_t*>(smem + ROWS * CP * 4);    // [ROWS][HP]
    const int C = a.lstm_C;
    const int hc0 = n0 >> 2;                               // first hidden channel of this tile
    const int p = lane & 31, hi = lane >> 5;
    if constexpr (PREF) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = tid + 256 * k, row = idx >> 3, c4 = idx & 7;
            float* d = lc + row * CP + c4 * 4;
            d[0] = pref->v[k].x; d[1] = pref->v[k].y; d[2] = pref->v[k].z; d[3] = pref->v[k].w;
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int ml = wm * 32 * MT + i * 32 + p;
        const int m = m0 + ml;
        const bool valid = m < a.M;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int hcl = wn * 8 * NT + j * 8 + 2 * q + hi;
                const int hc = hc0 + hcl;
                float gi = acc[i][j][q * 4 + 0], gr = acc[i][j][q * 4 + 1], go = acc[i][j][q * 4 + 2], gc = acc[i][j][q * 4 + 3];
                if (ADD_BIAS && a.bias) { gi += a.bias[hc]; gr += a.bias[C + hc]; go += a.bias[2 * C + hc]; gc += a.bias[3 * C + hc]; }
                float pc;
                if constexpr (PREF) pc = lc[ml * CP + hcl];              // this lane is the slot's only reader and writer
                else pc = (a.lstm_prev && valid) ? a.lstm_prev[(long long)m * C + hc] : 0.0f;
                const float nc = fast_sigmoid(gr) * pc + fast_sigmoid(gi) * fast_tanh(gc);     // submodules.py:211
                const float hv = fast_sigmoid(go) * fast_tanh(nc);                              // submodules.py:212
                lc[ml * CP + hcl] = nc;
                lh[ml * HP + hcl] = (uint16_t)pack_bf16x2(hv, 0.0f);
            }
    }
    __syncthreads();
    // 16-byte stores when rows are 16-byte aligned (always for the E2VID state buffers); LDS pitches are odd -> dword reads
    const bool vec_ok = (C & 3) == 0 && (a.lstm_h_stride & 7) == 0 && (((uintptr_t)a.lstm_h | (uintptr_t)a.lstm_cell) & 15) == 0;
    if (vec_ok) {
#pragma unroll
        for (int idx = tid; idx < ROWS * (HC / 4); idx += 256) {       // cell: float4 per lane, HC/4 lanes per row
            const int row = idx / (HC / 4), c4 = idx - row * (HC / 4);
            const int m = m0 + row;
            const float* sp = lc + row * CP + c4 * 4;
            if (m < a.M) out_store16(a.lstm_cell + (long long)m * C + hc0 + c4 * 4, make_uint4(__float_as_uint(sp[0]), __float_as_uint(sp[1]), __float_as_uint(sp[2]), __float_as_uint(sp[3])));
        }
        const uint32_t* lhv = reinterpret_cast<const uint32_t*>(lh);
#pragma unroll
        for (int idx = tid; idx < ROWS * (HC / 8); idx += 256) {       // hidden: 8 bf16 per lane
            const int row = idx / (HC / 8), c8 = idx - row * (HC / 8);
            const int m = m0 + row;
            const uint32_t* sp = lhv + row * (HP / 2) + c8 * 4;
            if (m < a.M) out_store16(a.lstm_h + (long long)m * a.lstm_h_stride + hc0 + c8 * 8, make_uint4(sp[0], sp[1], sp[2], sp[3]));
        }
        return;
    }
#pragma unroll 4
    for (int idx = tid; idx < ROWS * HC; idx += 256) {     // cell: ROWS x HC fp32, whole rows per lane group
        const int row = idx / HC, col = idx - row * HC;
        const int m = m0 + row;
        if (m < a.M) a.lstm_cell[(long long)m * C + hc0 + col] = lc[row * CP + col];
    }
    const uint32_t* lh32 = reinterpret_cast<const uint32_t*>(lh);
#pragma unroll 4
    for (int idx = tid; idx < ROWS * (HC / 2); idx += 256) {   // hidden: ROWS x HC/2 dwords (2 bf16 each)
        const int row = idx / (HC / 2), col = idx - row * (HC / 2);
        const int m = m0 + row;
        if (m < a.M) *reinterpret_cast<uint32_t*>(a.lstm_h + (long long)m * a.lstm_h_stride + hc0 + col * 2) = lh32[row * (HP / 2) + col];
    }
}
