// Fragment macros shared by the hand-scheduled K loops of the bf16 convolution kernels (included by conv_fwd.hip after
// conv_args.h).  They are macros on purpose: the same text as an inline function template compiles to different register
// allocation and a different ds_read / v_mfma interleave in those loops (EXPERIMENTS.md, "fragment macros as functions").
//
// The using scope provides constexpr MT, NT (32 x 32 fragments of the wave tile along pixels / channels), EPI and
// f32x16_t acc[MT][NT].

// acc += A * B for every fragment pair; EPI != 0 (fused ConvLSTM, fused ConvGRU) runs the product transposed: weights are the MFMA A operand
#define OESS_FRAG_MMA(SRC_A, SRC_B)                                                                              \
    {                                                                                                            \
        _Pragma("unroll") for (int i = 0; i < MT; ++i)                                                           \
            _Pragma("unroll") for (int j = 0; j < NT; ++j)                                                       \
                acc[i][j] = (EPI != 0) ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(SRC_B[j], SRC_A[i], acc[i][j], 0, 0, 0)     \
                                       : __builtin_amdgcn_mfma_f32_32x32x16_bf16(SRC_A[i], SRC_B[j], acc[i][j], 0, 0, 0);   \
    }

// wait until only N_ LDS reads remain outstanding; the "+v" operands tie later uses of the fragments FA_[MT], FB_[NT] to the wait
#define OESS_FRAG_WAIT(N_, FA_, FB_)                                                                             \
    {                                                                                                            \
        if constexpr (MT == 4 && NT == 4)                                                                        \
            asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(FA_[0]), "+v"(FA_[1]), "+v"(FA_[2]), "+v"(FA_[3]),       \
                         "+v"(FB_[0]), "+v"(FB_[1]), "+v"(FB_[2]), "+v"(FB_[3]) : "n"(N_) : "memory");           \
        else if constexpr (MT == 2 && NT == 4)                                                                   \
            asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(FA_[0]), "+v"(FA_[1]), "+v"(FB_[0]), "+v"(FB_[1]), "+v"(FB_[2]), "+v"(FB_[3]) : "n"(N_) : "memory"); \
        else if constexpr (MT == 2 && NT == 2)                                                                   \
            asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(FA_[0]), "+v"(FA_[1]), "+v"(FB_[0]), "+v"(FB_[1]) : "n"(N_) : "memory"); \
        else if constexpr (MT == 2 && NT == 1)                                                                   \
            asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(FA_[0]), "+v"(FA_[1]), "+v"(FB_[0]) : "n"(N_) : "memory"); \
        else if constexpr (MT == 1 && NT == 2)                                                                   \
            asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(FA_[0]), "+v"(FB_[0]), "+v"(FB_[1]) : "n"(N_) : "memory"); \
        else                                                                                                     \
            asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(FA_[0]), "+v"(FB_[0]) : "n"(N_) : "memory");             \
    }

// Fragment reads of the three persistent w128 kernels (conv_lstm_w128.h, conv_w128_gemm.h, conv3x3_w128.h) into their
// fp[2][4] / fw[2][4] register double buffers; wa[J][KS] holds the weight fragment addresses.  ADDR is the pixel fragment's
// k-step-0 address register; k-step KS flips bits of it (the XOR never carries), k-step 0 needs no XOR.
#define W128_RD_P(BUF, I, ADDR, KS, OFF) { uint32_t t_; asm volatile("v_xor_b32 %1, %4, %2\n\tds_read_b128 %0, %1 offset:%3" : "=v"(fp[BUF][I]), "=&v"(t_) : "v"(ADDR), "n"(OFF), "n"((KS) << 5) : "memory"); }
#define W128_RD_P0(BUF, I, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fp[BUF][I]) : "v"(ADDR), "n"(OFF) : "memory")
#define W128_RD_W(BUF, J, KS, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fw[BUF][J]) : "v"(wa[J][KS]), "n"(OFF) : "memory")
