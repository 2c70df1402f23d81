// GPU-side PNG encode of 8-bit grey / RGB maps: the label, colour and superpixel maps that segment_render and SLIC
// leave on the device become PNG files there, so the host only copies file bytes (png_ops.hip is the decoding half).
// The format is a fixed subset of PNG, stated in include/oess.h: Paeth on every scanline, the filtered stream cut into segments of
// OESS_PNG_ENCODE_SEGMENT bytes, each segment one byte-aligned DEFLATE block in its own IDAT chunk -- fixed Huffman code with
// distance-1 matches over runs of equal bytes, or stored where that is not shorter.
//   K1  png_encode_segment_kernel  one workgroup per (image, segment): Paeth filter into LDS (pointwise: it reads source pixels
//                                  only), run heads as a 64-bit mask per thread (64 consecutive bytes each), block scans for the
//                                  run start / end that cross threads and for the token bit offsets, bits packed into a zeroed LDS
//                                  buffer by OR, coded-or-stored decision, the chunk's CRC-32 by slices (CRC is linear over GF(2):
//                                  every thread walks its slice from a zero state and multiplies by x^(8 bytes behind it) mod P),
//                                  the segment's Adler pair; the whole chunk (length, type, payload, CRC) goes to scratch.
//   K2  png_encode_layout_kernel   one workgroup per image: prefix sum of the chunk sizes -> file offsets, Adler-32 combined from
//                                  the per-segment (a, b, len), signature / IHDR / zlib-header IDAT / Adler IDAT / IEND, sizes[i].
//   K3  png_encode_gather_kernel   one workgroup per (image, segment): the chunk moves to its offset in the file slot (dword
//                                  stores on the destination's alignment).
// Integer work only; the bytes are a function of the input alone (OR / XOR / integer sums commute), so two calls agree bit for bit.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"

namespace {

constexpr int SEG = OESS_PNG_ENCODE_SEGMENT;
constexpr int NT = 256;                       // threads per workgroup
constexpr int PER = SEG / NT;                 // consecutive filtered bytes per thread
static_assert(PER == 64, "a thread's run heads are one 64-bit mask");
static_assert(SEG <= 65535, "a stored block holds at most 65535 bytes");
constexpr int OB_WORDS = (5 + SEG + 4 + 3) / 4 + 1;          // payload (at most 5 + SEG) and its CRC, in dwords
constexpr int CHUNK_STRIDE = (8 + 4 * OB_WORDS + 15) / 16 * 16;   // scratch bytes per chunk: length, type, payload, CRC
constexpr int HEAD_BYTES = 8 + 25 + 14;       // signature, IHDR chunk, the IDAT chunk holding 78 01
constexpr int TAIL_BYTES = 16 + 12;           // the IDAT chunk holding Adler-32, IEND
constexpr uint32_t POLY = 0xedb88320u;        // CRC-32, reflected
constexpr uint32_t ADLER = 65521u;

// a * b mod P over GF(2) in the reflected representation (x^0 = 0x80000000); 32 steps
__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ POLY : b >> 1;
    }
    return p;
}

struct CrcTables { uint32_t byte[256]; uint32_t pow8[16]; };       // pow8[k] = x^(8 2^k) mod P: a state moved over 2^k zero bytes
constexpr CrcTables make_tables() {
    CrcTables t{};
    for (uint32_t n = 0; n < 256; ++n) {
        uint32_t c = n;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? POLY ^ (c >> 1) : c >> 1;
        t.byte[n] = c;
    }
    uint32_t p = 1u << 30;                                          // x^1
    for (int k = 0; k < 3; ++k) p = gf_mul(p, p);                   // x^8
    for (int k = 0; k < 16; ++k) { t.pow8[k] = p; p = gf_mul(p, p); }
    return t;
}
constexpr CrcTables H_TABLES = make_tables();
__constant__ CrcTables TABLES = H_TABLES;

// CRC state `c` after `n` more zero bytes (n < 65536)
__device__ __forceinline__ uint32_t crc_shift(uint32_t c, int n) {
    for (int k = 0; n; ++k, n >>= 1)
        if (n & 1) c = gf_mul(c, TABLES.pow8[k]);
    return c;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// inclusive scan over the NT threads of a workgroup; buf holds 2 NT values and ends with the results in buf[0 ... NT)
template <class T, class Op>
__device__ __forceinline__ T block_scan(T v, T* buf, int t, Op op) {
    __syncthreads();                           // readers of the previous scan's results are done
    buf[t] = v;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < NT; d <<= 1) {
        T x = buf[cur * NT + t];
        if (t >= d) x = op(buf[cur * NT + t - d], x);
        cur ^= 1;
        buf[cur * NT + t] = x;
        __syncthreads();
    }
    static_assert(NT == 256, "8 steps leave the results in the first half");
    return buf[t];
}

// The token that position p (value v) of a run [s, e) puts out, as (bits, count), LSB first; count 0 inside a match.
// A run is one literal, then matches at distance 1 of at most 258 bytes while at least 3 remain, then 0 ... 2 literals.
// adv = the distance to the next position that can put out a token (the bytes a match covers put out none).
__device__ __forceinline__ int token(int p, int s, int e, int v, uint32_t& bits, int& adv) {
    const int k = p - s;
    adv = 1;
    if (k > 0) {
        const int j = k - 1, q = j / 258, r = j - q * 258, rem = (e - s - 1) - q * 258;
        if (rem >= 3) {
            const int m = min(rem, 258);
            adv = m - r;
            if (r != 0) return 0;
            int idx, eb = 0, ev = 0;
            if (m == 258) idx = 28;
            else {
                const int m3 = m - 3;
                if (m3 < 8) idx = m3;
                else { eb = 29 - __clz(m3); idx = 4 * eb + 4 + ((m3 >> eb) & 3); ev = m3 & ((1 << eb) - 1); }
            }
            int n;
            uint32_t code;
            if (idx < 23) { code = (uint32_t)(idx + 1); n = 7; }           // symbols 257 ... 279: 7 bits from 0000001
            else { code = 0xc0u + (uint32_t)(idx - 23); n = 8; }           // symbols 280 ... 285: 8 bits from 11000000
            bits = (__brev(code) >> (32 - n)) | ((uint32_t)ev << n);       // Huffman codes go MSB first, extra bits LSB first
            return n + eb + 5;                                             // distance 1: five zero bits
        }
    }
    if (v < 144) { bits = __brev(0x30u + (uint32_t)v) >> 24; return 8; }
    bits = __brev(0x190u + (uint32_t)(v - 144)) >> 23;
    return 9;
}

// every token of a thread's 64 positions, in order; the bytes inside a match are stepped over
template <class F>
__device__ __forceinline__ void walk_tokens(const uint8_t* fb, int p0, int len, uint64_t heads, int carry_s, int carry_e, F f) {
    const int n_mine = min(PER, len - p0);
    for (int i = 0; i < n_mine;) {
        const int p = p0 + i;
        const uint64_t below = heads & (~0ull >> (63 - i));               // heads at or before i
        const int s = below ? p0 + 63 - __builtin_clzll(below) : carry_s;
        const uint64_t rest = i < 63 ? heads >> (i + 1) : 0;
        const int e = rest ? p + 1 + __builtin_ctzll(rest) : carry_e;
        uint32_t bits = 0;
        int adv;
        const int n = token(p, s, e, (int)fb[p], bits, adv);
        if (n) f(bits, n);
        i += adv;
    }
}

__global__ __launch_bounds__(NT) void png_encode_segment_kernel(const uint8_t* __restrict__ images, int H, int W, int ch, int nseg,
                                                                uint8_t* __restrict__ chunks, int4* __restrict__ meta) {
    __shared__ uint32_t fb32[SEG / 4];         // the segment's filtered bytes
    __shared__ uint32_t ob32[OB_WORDS];        // the chunk's payload, then its CRC
    __shared__ uint32_t crc_tbl[256];
    __shared__ uint32_t scan[2 * NT];
    __shared__ uint32_t red[3];                // Adler a, Adler b, CRC
    uint8_t* fb = (uint8_t*)fb32;
    uint8_t* ob = (uint8_t*)ob32;
    const int t = threadIdx.x;
    const int img = blockIdx.x / nseg, seg = blockIdx.x - img * nseg;
    const int pixbytes = W * ch, rowbytes = 1 + pixbytes;
    const int S = H * rowbytes;                // < 2^31 (H, W <= 16384)
    const int g0 = seg * SEG, len = min(SEG, S - g0);
    const bool last = seg == nseg - 1;
    const uint8_t* im = images + (long long)img * H * pixbytes;

    crc_tbl[t] = TABLES.byte[t];
    if (t < 3) red[t] = 0;
    for (int k = t; k < OB_WORDS; k += NT) ob32[k] = 0;
    // ---- Paeth filter, pointwise from the source pixels: four stream bytes per thread and pass, every load unconditional (a
    // neighbour outside the image reads the pixel itself and is zeroed afterwards) so that the loads of a pass are in flight together
#pragma unroll 4
    for (int it = 0; it < SEG / (4 * NT); ++it) {
        const int q = t + NT * it, g = g0 + 4 * q;
        int y = g / rowbytes, c = g - y * rowbytes;
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = y < H;                                         // g0 + p < S
            const int yy = in ? y : H - 1, cs = in ? c : rowbytes - 1;
            const int x = max(cs - 1, 0);
            const bool ha = x >= ch, hb = yy > 0;
            const uint8_t* r = im + (long long)yy * pixbytes + x;
            const int v = r[0];
            int a = r[ha ? -ch : 0], b = r[hb ? -pixbytes : 0], d = r[(ha && hb) ? -ch - pixbytes : 0];
            a = ha ? a : 0; b = hb ? b : 0; d = (ha && hb) ? d : 0;
            int f = (v - paeth(a, b, d)) & 255;
            f = cs == 0 ? 4 : f;
            word |= (uint32_t)(in ? f : 0) << (8 * j);
            if (++c == rowbytes) { c = 0; ++y; }
        }
        fb32[q] = word;
    }
    __syncthreads();

    // ---- run heads of this thread's 64 bytes, Adler partial sums
    const int p0 = t * PER;
    uint64_t heads = 0;
    {
        uint32_t sa = 0, sb = 0;
        int prev = p0 > 0 ? (int)fb[p0 - 1] : -1;
        for (int w = 0; w < PER / 4; ++w) {
            if (p0 + 4 * w >= len) break;
            const uint32_t word = fb32[(p0 >> 2) + w];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * w + j, p = p0 + i;
                const int v = (int)((word >> (8 * j)) & 255u);
                if (p < len) {
                    if (v != prev) heads |= 1ull << i;
                    sa += (uint32_t)v;
                    sb += (uint32_t)(len - p) * (uint32_t)v;          // at most 64 * 16384 * 255 per thread
                }
                prev = v;
            }
        }
        if (sa) { atomicAdd(&red[0], sa); atomicAdd(&red[1], sb % ADLER); }
    }
    // run start before this thread's first head: the last head of the threads below; run end after its last: the first head above
    int* iscan = (int*)scan;
    const int last_head = heads ? p0 + 63 - __builtin_clzll(heads) : -1;
    const int first_head = heads ? p0 + __builtin_ctzll(heads) : len;
    block_scan(last_head, iscan, t, [](int a, int b) { return max(a, b); });
    const int carry_s = t > 0 ? iscan[t - 1] : 0;
    block_scan(first_head, iscan, NT - 1 - t, [](int a, int b) { return min(a, b); });
    const int carry_e = t < NT - 1 ? iscan[NT - 2 - t] : len;

    // ---- bit offsets of the tokens
    uint32_t my_bits = 0;
    walk_tokens(fb, p0, len, heads, carry_s, carry_e, [&](uint32_t, int n) { my_bits += (uint32_t)n; });
    const uint32_t incl = block_scan(my_bits, scan, t, [](uint32_t a, uint32_t b) { return a + b; });
    const uint32_t total_bits = scan[NT - 1];
    // header (3 bits), tokens, end-of-block (7 zero bits); a segment that is not the last is closed by an empty stored block
    const uint32_t tb = 3 + total_bits + 7;
    const int coded = last ? (int)((tb + 7) >> 3) : (int)((tb + 3 + 7) >> 3) + 4;
    const bool stored = coded >= 5 + len;
    const int plen = stored ? 5 + len : coded;
    if (!stored) {
        uint32_t off = 3 + incl - my_bits;
        uint32_t wi = off >> 5;
        int fill = (int)(off & 31u);
        uint64_t acc = 0;
        if (t == 0) { acc = (last ? 1u : 0u) | 2u; wi = 0; fill = 3; }     // BFINAL, BTYPE = 01
        walk_tokens(fb, p0, len, heads, carry_s, carry_e, [&](uint32_t bits, int n) {
            acc |= (uint64_t)bits << fill;
            fill += n;
            if (fill >= 32) { atomicOr(&ob32[wi++], (uint32_t)acc); acc >>= 32; fill -= 32; }
        });
        if (acc) atomicOr(&ob32[wi], (uint32_t)acc);
        __syncthreads();
        if (t == 0 && !last) { ob[coded - 2] = 0xff; ob[coded - 1] = 0xff; }   // LEN = 0000 is already there, NLEN = ffff
    } else {
        if (t == 0) {
            ob[0] = last ? 1 : 0;
            ob[1] = (uint8_t)(len & 255); ob[2] = (uint8_t)(len >> 8);
            ob[3] = (uint8_t)(~len & 255); ob[4] = (uint8_t)((~len >> 8) & 255);
        }
        for (int p = t; p < len; p += NT) ob[5 + p] = fb[p];
    }
    __syncthreads();

    // ---- CRC-32 of "IDAT" + payload: slices from a zero state, moved over the bytes behind them, XORed
    {
        const int B = (plen + NT - 1) / NT;
        const int b0 = min(plen, t * B), b1 = min(plen, b0 + B);
        uint32_t c = 0;
        for (int i = b0; i < b1; ++i) c = crc_tbl[(c ^ ob[i]) & 255u] ^ (c >> 8);
        if (c) c = crc_shift(c, plen - b1);
        if (t == NT - 1) {                       // the state after the type bytes from the all-ones start, moved over the payload
            uint32_t k = 0xffffffffu;
            const uint8_t type[4] = {'I', 'D', 'A', 'T'};
            for (int i = 0; i < 4; ++i) k = crc_tbl[(k ^ type[i]) & 255u] ^ (k >> 8);
            c ^= crc_shift(k, plen);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o, 64);
        if ((t & 63) == 0) atomicXor(&red[2], c);
    }
    __syncthreads();
    if (t == 0) {
        const uint32_t crc = red[2] ^ 0xffffffffu;
        ob[plen] = (uint8_t)(crc >> 24); ob[plen + 1] = (uint8_t)(crc >> 16); ob[plen + 2] = (uint8_t)(crc >> 8); ob[plen + 3] = (uint8_t)crc;
        meta[blockIdx.x] = make_int4(plen, (int)(red[0] % ADLER), (int)(red[1] % ADLER), len);
    }
    __syncthreads();
    uint32_t* dst = (uint32_t*)(chunks + (size_t)blockIdx.x * CHUNK_STRIDE);
    if (t == 0) {
        dst[0] = __builtin_bswap32((uint32_t)plen);
        dst[1] = 0x54414449u;                    // "IDAT" as a little-endian dword
    }
    const int nw = (plen + 4 + 3) >> 2;
    for (int k = t; k < nw; k += NT) dst[2 + k] = ob32[k];
}

__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// CRC of the chunk whose type starts at p (n bytes of type + data), written behind it; one thread
__device__ void seal_chunk(uint8_t* p, int n) {
    uint32_t c = 0xffffffffu;
    for (int i = 0; i < n; ++i) c = TABLES.byte[(c ^ p[i]) & 255u] ^ (c >> 8);
    put_be32(p + n, c ^ 0xffffffffu);
}

__global__ __launch_bounds__(NT) void png_encode_layout_kernel(int H, int W, int ch, int nseg, const int4* __restrict__ meta,
                                                               int* __restrict__ offs, uint8_t* __restrict__ files, long long slot_bytes,
                                                               int* __restrict__ sizes) {
    __shared__ uint32_t scan[2 * NT];
    __shared__ uint32_t bsum;
    const int t = threadIdx.x, img = blockIdx.x;
    const int4* m = meta + (size_t)img * nseg;
    int* o = offs + (size_t)img * nseg;
    if (t == 0) bsum = 0;
    uint32_t off = HEAD_BYTES, a_run = 1, b_mine = 0;          // Adler-32 starts at a = 1, b = 0
    for (int base = 0; base < nseg; base += NT) {
        const int k = base + t;
        const int4 e = k < nseg ? m[k] : make_int4(-12, 0, 0, 0);
        const uint32_t sz = (uint32_t)(12 + e.x);
        const uint32_t o_incl = block_scan(sz, scan, t, [](uint32_t a, uint32_t b) { return a + b; });
        const uint32_t o_all = scan[NT - 1];
        const uint32_t a_incl = block_scan((uint32_t)e.y, scan, t, [](uint32_t a, uint32_t b) { return a + b; });
        const uint32_t a_all = scan[NT - 1];
        if (k < nseg) {
            o[k] = (int)(off + o_incl - sz);
            // a segment of `len` bytes met at (a0, b0) leaves b = b0 + len a0 + its own b
            const uint32_t a0 = (a_run + a_incl - (uint32_t)e.y) % ADLER;
            b_mine = (b_mine + ((uint32_t)e.w * a0 + (uint32_t)e.z) % ADLER) % ADLER;
        }
        off += o_all;
        a_run = (a_run + a_all) % ADLER;
    }
    __syncthreads();
    atomicAdd(&bsum, b_mine);
    __syncthreads();
    if (t == 0) {
        uint8_t* f = files + (long long)img * slot_bytes;
        const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
        for (int i = 0; i < 8; ++i) f[i] = sig[i];
        put_be32(f + 8, 13);
        f[12] = 'I'; f[13] = 'H'; f[14] = 'D'; f[15] = 'R';
        put_be32(f + 16, (uint32_t)W); put_be32(f + 20, (uint32_t)H);
        f[24] = 8; f[25] = ch == 3 ? 2 : 0; f[26] = 0; f[27] = 0; f[28] = 0;
        seal_chunk(f + 12, 17);
        put_be32(f + 33, 2);
        f[37] = 'I'; f[38] = 'D'; f[39] = 'A'; f[40] = 'T'; f[41] = 0x78; f[42] = 0x01;
        seal_chunk(f + 37, 6);
        uint8_t* z = f + off;
        put_be32(z, 4);
        z[4] = 'I'; z[5] = 'D'; z[6] = 'A'; z[7] = 'T';
        put_be32(z + 8, ((bsum % ADLER) << 16) | a_run);
        seal_chunk(z + 4, 8);
        put_be32(z + 16, 0);
        z[20] = 'I'; z[21] = 'E'; z[22] = 'N'; z[23] = 'D';
        seal_chunk(z + 20, 4);
        sizes[img] = (int)off + TAIL_BYTES;
    }
}

__global__ __launch_bounds__(NT) void png_encode_gather_kernel(int nseg, const uint8_t* __restrict__ chunks, const int4* __restrict__ meta,
                                                               const int* __restrict__ offs, uint8_t* __restrict__ files, long long slot_bytes) {
    const int t = threadIdx.x, img = blockIdx.x / nseg;
    const uint8_t* src = chunks + (size_t)blockIdx.x * CHUNK_STRIDE;
    const uint32_t* s32 = (const uint32_t*)src;
    const int nbytes = 12 + meta[blockIdx.x].x;
    uint8_t* dst = files + (long long)img * slot_bytes + offs[blockIdx.x];
    const int head = min(nbytes, (int)((4 - ((uintptr_t)dst & 3)) & 3));
    if (t < head) dst[t] = src[t];
    const int nw = (nbytes - head) >> 2;
    uint32_t* d32 = (uint32_t*)(dst + head);
    const int sh = head * 8;                   // source byte of destination dword k: head + 4 k
    for (int k = t; k < nw; k += NT) {
        uint32_t v = s32[k];
        if (sh) v = (v >> sh) | (s32[k + 1] << (32 - sh));
        d32[k] = v;
    }
    const int done = head + 4 * nw;
    if (t < nbytes - done) dst[done + t] = src[done + t];
}

// stream bytes, segments; false for what the encoder refuses
bool geometry(int H, int W, int channels, long long* S, long long* nseg) {
    if ((channels != 1 && channels != 3) || H < 1 || H > 16384 || W < 1 || W > 16384) return false;
    *S = (long long)H * (1 + (long long)W * channels);
    *nseg = (*S + SEG - 1) / SEG;
    return true;
}

}  // namespace

extern "C" {

long long oess_png_encode_bound(int H, int W, int channels) {
    long long S, nseg;
    if (!geometry(H, W, channels, &S, &nseg)) return 0;
    return HEAD_BYTES + TAIL_BYTES + S + 17 * nseg;
}

size_t oess_png_encode_scratch_bytes(int n_images, int H, int W, int channels) {
    long long S, nseg;
    if (n_images < 1 || !geometry(H, W, channels, &S, &nseg) || (long long)n_images * nseg > INT_MAX) return 0;
    return (size_t)n_images * (size_t)nseg * (CHUNK_STRIDE + sizeof(int4) + sizeof(int)) + 256;
}

int oess_png_encode_batch(const uint8_t* images, int n_images, int H, int W, int channels, uint8_t* files, long long slot_bytes,
                          int* sizes, void* scratch, size_t scratch_bytes, oess_stream_t stream) {
    long long S, nseg;
    if (!images || !files || !sizes || !scratch || n_images < 1 || !geometry(H, W, channels, &S, &nseg)) return OESS_EINVAL;
    if ((long long)n_images * nseg > INT_MAX || slot_bytes < oess_png_encode_bound(H, W, channels)) return OESS_EINVAL;
    if (scratch_bytes < oess_png_encode_scratch_bytes(n_images, H, W, channels) || ((uintptr_t)scratch & 15)) return OESS_EINVAL;
    const size_t nchunks = (size_t)n_images * (size_t)nseg;
    uint8_t* chunks = (uint8_t*)scratch;
    int4* meta = (int4*)(chunks + nchunks * CHUNK_STRIDE);
    int* offs = (int*)(meta + nchunks);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(png_encode_segment_kernel, dim3((unsigned)nchunks), dim3(NT), 0, st, images, H, W, channels, (int)nseg, chunks, meta);
    hipLaunchKernelGGL(png_encode_layout_kernel, dim3(n_images), dim3(NT), 0, st, H, W, channels, (int)nseg, (const int4*)meta, offs, files,
                       slot_bytes, sizes);
    hipLaunchKernelGGL(png_encode_gather_kernel, dim3((unsigned)nchunks), dim3(NT), 0, st, (int)nseg, (const uint8_t*)chunks,
                       (const int4*)meta, (const int*)offs, files, slot_bytes);
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}

}  // extern "C"
