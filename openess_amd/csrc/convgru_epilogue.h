// Fused ConvGRU epilogues of conv_fwd_dma_kernel (included after conv_args.h, inside the including file's anonymous namespace).
//
// One ConvGRU step (e2vid/model/submodules.py:217-253 of the reference) is two dependent 3 x 3 convolutions:
//   gates  (EPI == 2): u = sigmoid(conv(cat(x, h), Wu) + bu), r = sigmoid(conv(cat(x, h), Wr) + br)  -> u (fp32), r * h (bf16)
//   output (EPI == 3): o = tanh(conv(cat(x, r * h), Wo) + bo), h' = h * (1 - u) + o * u              -> h' (fp32 master + bf16 copy)
// Both run the product transposed (D^T = W * A^T, as the fused ConvLSTM does): a lane holds, for ONE pixel (col = lane & 31),
// rows (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5) of a 32-row block of weight rows.
//   gates:  rows are packed gate-interleaved (n' = 2 * hc + gate, gate 0 = u, 1 = r): registers 4q .. 4q + 3 are (u, r) of the
//           two adjacent hidden channels 4q + 2 * (lane >> 5) + {0, 1} of the block's 16.
//   output: rows are hidden channels: registers 4q .. 4q + 3 are o of channels 8q + 4 * (lane >> 5) + {0 .. 3} of the block's 32.
// The gate algebra is lane local; u, r and o never exist as tensors of pre-activations.  Results leave through padded LDS
// images as whole rows (16-byte stores).  h is kept in fp32 (lstm_prev -> lstm_cell, in place is fine: a value is read and
// written by the lane that owns it, before and after the tile's barrier) next to the bf16 copy the next gates launch convolves.

// accumulator start values = the biases (Conv2d order: [bu | br] for the gates, bo for the output)
template <int EPI, int MT, int NT>
__device__ __forceinline__ void gru_bias_init(const ConvArgs& a, f32x16_t (&acc)[MT][NT], int n0, int wn, int lane) {
    const int hi = lane >> 5, C = a.lstm_C;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int q = e >> 2, t = e & 3;
            float b = 0.0f;
            if constexpr (EPI == 2) {
                const int hc = (n0 >> 1) + wn * 16 * NT + j * 16 + 4 * q + 2 * hi + (t >> 1);
                if (a.bias && hc < C) b = a.bias[(t & 1) * C + hc];
            } else {
                const int hc = n0 + wn * 32 * NT + j * 32 + 8 * q + 4 * hi + t;
                if (a.bias && hc < C) b = a.bias[hc];
            }
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[i][j][e] = b;
        }
}

// Rows [0, ROWS) x HC channels of an fp32 image (pitch CP) and a bf16 image (pitch HP) in LDS -> global rows m0 + rowmap(row),
// channels hc0 + [0, HC), 16 bytes per lane.  Pitches are odd in dwords (conflict-free lane-per-row writes): dword reads.
template <int ROWS, int HC, typename RowMap>
__device__ __forceinline__ void gru_store_images(const ConvArgs& a, const float* lc, const uint16_t* lh, int m0, int hc0, int tid, RowMap rowmap) {
    constexpr int CP = HC + 1, HP = HC + 2;
    const int C = a.lstm_C;
#pragma unroll
    for (int idx = tid; idx < ROWS * (HC / 4); idx += 256) {
        const int row = idx / (HC / 4), c4 = idx - row * (HC / 4);
        const int m = m0 + rowmap(row);
        const float* sp = lc + row * CP + c4 * 4;
        if (m < a.M && hc0 + c4 * 4 < C)
            out_store16(a.lstm_cell + (long long)m * C + hc0 + c4 * 4,
                        make_uint4(__float_as_uint(sp[0]), __float_as_uint(sp[1]), __float_as_uint(sp[2]), __float_as_uint(sp[3])));
    }
    const uint32_t* lhv = reinterpret_cast<const uint32_t*>(lh);
#pragma unroll
    for (int idx = tid; idx < ROWS * (HC / 8); idx += 256) {
        const int row = idx / (HC / 8), c8 = idx - row * (HC / 8);
        const int m = m0 + rowmap(row);
        const uint32_t* sp = lhv + row * (HP / 2) + c8 * 4;
        if (m < a.M && hc0 + c8 * 8 < C)
            out_store16(a.lstm_h + (long long)m * a.lstm_h_stride + hc0 + c8 * 8, make_uint4(sp[0], sp[1], sp[2], sp[3]));
    }
}

// gates: 128 pixels x 128 gate rows = 64 hidden channels per workgroup (2 x 2 waves, MT = NT = 2)
template <int MT, int NT>
__device__ __forceinline__ void gru_gates_epilogue(const ConvArgs& a, f32x16_t (&acc)[MT][NT], unsigned char* smem, int m0, int n0,
                                                   int wm, int wn, int lane, int tid) {
    constexpr int ROWS = 64 * MT, HC = 32 * NT;
    constexpr int CP = HC + 1, HP = HC + 2;
    float* lc = reinterpret_cast<float*>(smem);                          // [ROWS][CP]  u
    uint16_t* lh = reinterpret_cast<uint16_t*>(smem + ROWS * CP * 4);    // [ROWS][HP]  r * h
    const int C = a.lstm_C;
    const int hc0 = n0 >> 1;
    const int p = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int ml = wm * 32 * MT + i * 32 + p;
        const int m = m0 + ml;
        const bool valid = m < a.M;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int hcl = wn * 16 * NT + j * 16 + 4 * q + 2 * hi;      // even: this lane owns hcl and hcl + 1
                const int hc = hc0 + hcl;
                float2 h = make_float2(0.f, 0.f);
                if (a.lstm_prev && valid && hc < C) h = *reinterpret_cast<const float2*>(a.lstm_prev + (long long)m * C + hc);
                const float u0 = fast_sigmoid(acc[i][j][q * 4 + 0]), r0 = fast_sigmoid(acc[i][j][q * 4 + 1]);
                const float u1 = fast_sigmoid(acc[i][j][q * 4 + 2]), r1 = fast_sigmoid(acc[i][j][q * 4 + 3]);
                const float rh0 = r0 * h.x, rh1 = r1 * h.y;                  // submodules.py:250 (prev_state * reset)
                lc[ml * CP + hcl] = u0;
                lc[ml * CP + hcl + 1] = u1;
                *reinterpret_cast<uint32_t*>(lh + ml * HP + hcl) = pack_bf16x2(rh0, rh1);
                if (a.gru_rh32 && valid && hc < C) *reinterpret_cast<float2*>(a.gru_rh32 + (long long)m * C + hc) = make_float2(rh0, rh1);
            }
    }
    __syncthreads();
    gru_store_images<ROWS, HC>(a, lc, lh, m0, hc0, tid, [](int row) { return row; });
}

// output: 128 pixels x 128 hidden channels per workgroup; the images of 64 pixels fit the operand ring, so the tile leaves in
// MT passes (pass i: rows wm * 32 * MT + i * 32 + [0, 32) of both wave rows)
template <int MT, int NT>
__device__ __forceinline__ void gru_out_epilogue(const ConvArgs& a, f32x16_t (&acc)[MT][NT], unsigned char* smem, int m0, int n0,
                                                 int wm, int wn, int lane, int tid) {
    constexpr int ROWS = 64, HC = 64 * NT;
    constexpr int CP = HC + 1, HP = HC + 2;
    float* lc = reinterpret_cast<float*>(smem);                          // [ROWS][CP]  h' (fp32 master)
    uint16_t* lh = reinterpret_cast<uint16_t*>(smem + ROWS * CP * 4);    // [ROWS][HP]  h' (bf16 copy)
    const int C = a.lstm_C;
    const int p = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int lr = wm * 32 + p;                                       // row of this pass's images
        const int m = m0 + wm * 32 * MT + i * 32 + p;
        const bool valid = m < a.M;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int hcl = wn * 32 * NT + j * 32 + 8 * q + 4 * hi;      // this lane owns hcl .. hcl + 3
                const int hc = n0 + hcl;
                float4 h = make_float4(0.f, 0.f, 0.f, 0.f), u = make_float4(0.f, 0.f, 0.f, 0.f);
                if (valid && hc < C) {
                    u = *reinterpret_cast<const float4*>(a.gru_u + (long long)m * C + hc);
                    if (a.lstm_prev) h = *reinterpret_cast<const float4*>(a.lstm_prev + (long long)m * C + hc);
                }
                // submodules.py:252: new_state = prev_state * (1 - update) + out_inputs * update
                const float n0_ = h.x * (1.0f - u.x) + fast_tanh(acc[i][j][q * 4 + 0]) * u.x;
                const float n1_ = h.y * (1.0f - u.y) + fast_tanh(acc[i][j][q * 4 + 1]) * u.y;
                const float n2_ = h.z * (1.0f - u.z) + fast_tanh(acc[i][j][q * 4 + 2]) * u.z;
                const float n3_ = h.w * (1.0f - u.w) + fast_tanh(acc[i][j][q * 4 + 3]) * u.w;
                float* d = lc + lr * CP + hcl;
                d[0] = n0_; d[1] = n1_; d[2] = n2_; d[3] = n3_;
                uint32_t* dh = reinterpret_cast<uint32_t*>(lh + lr * HP + hcl);
                dh[0] = pack_bf16x2(n0_, n1_);
                dh[1] = pack_bf16x2(n2_, n3_);
            }
        __syncthreads();
        gru_store_images<ROWS, HC>(a, lc, lh, m0, n0, tid, [i](int row) { return (row >> 5) * 32 * MT + i * 32 + (row & 31); });
        if (i + 1 < MT) __syncthreads();
    }
}
