// Output stage: the entropy-coded scan of a baseline JPEG frame, written on the device (include/lwg_hip.h 'lwg_jpeg_scan_u8' gives the format;
// tests/jpegdev_emu.py is its definition, which these kernels equal byte for byte).  Integers only - no fp32 arithmetic.
//
// Launch 1, one 256-thread workgroup per segment (mcus_per_segment <= 64 consecutive MCUs of one frame, raster order):
//   the MCUs' 8 x 24 pixel bytes -> LDS in words, coalesced along the MCU row (edge MCUs replicate the last row / column byte by byte);
//   wave c = component c, lane m = MCU m of the segment: colour conversion, the two DCT passes and the quantiser with the 64 values in
//   registers, the coefficients -> LDS in zigzag order (int16, [position][thread]: no bank conflicts); DC differences from LDS; bits per
//   block, a workgroup scan in MCU-major order for the bit offsets; every thread ORs its block's codes MSB-first into zeroed LDS words
//   (over the dead pixel bytes); the last block pads with 1-bits; every thread counts the FF bytes of a fixed run of words, a second scan,
//   and the stuffed bytes go to the segment's slot of the workspace, its size to the table in front of the slots.
// Launch 2, one workgroup per segment: prefix sum of the frame's segment sizes, the slot's bytes packed behind each other with FF D0+(k mod 8)
//   between them, and - the last segment's workgroup - nbytes[b].
// Every loop bound is an argument the host validated.
// 4:2:0 ('lwg_jpeg420_scan_u8', tests/jpeg420_emu.py) has a launch 1 of its own further down - 384 threads, one wave per block of a 16 x 16 MCU -
// and shares launch 2, the tables and the bit writer.
#include "lwg_common.h"
#include "lwg_jpeg_code.h"
#include "../../include/lwg_hip.h"

namespace {

__device__ const JpgCodes jpg_codes = jpg_make_codes();

struct JpgQuant { unsigned char q[128]; };     // luminance then chrominance, natural order (a kernel argument)

// natural index -> zigzag position
struct JpgUnzig { unsigned char pos[64]; };
constexpr JpgUnzig jpg_make_unzig() {
    JpgUnzig u{};
    for (int i = 0; i < 64; ++i) u.pos[JPG_ZIGZAG[i]] = (unsigned char)i;
    return u;
}
constexpr JpgUnzig JPG_UNZIG = jpg_make_unzig();

// tables of launch 1 in front of the coefficients and the pixel / bit buffer of the dynamic LDS block (a 16-byte multiple)
struct JpgTables {
    unsigned dc[2][16];
    unsigned ac[2][256];
    int q[128];
    int dcv[3][JPG_MAX_MCUS];
    unsigned bits[JPG_NT];       // bits of block 3 m + c, then its bit offset in the segment
    unsigned scan[4];
    unsigned ffs[4];
};
static_assert(sizeof(JpgTables) % 16 == 0, "the LDS carve-up keeps 16-byte offsets");
constexpr unsigned JPG_COEF_BYTES = 64u * JPG_COEF_STRIDE * 2u;

__device__ __forceinline__ unsigned jpg_size(int v) { return 32u - (unsigned)__clz(v < 0 ? -v : v); }      // bits of |v|; 0 for 0
__device__ __forceinline__ unsigned jpg_amp(int v, unsigned s) { return (unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u); }

// inclusive sum over the 64 NW threads' v; part: NW words of LDS.  -> (exclusive prefix of this thread, total)
template <int NW = JPG_NT / 64>
__device__ __forceinline__ void jpg_block_scan(unsigned v, unsigned* part, int wave, int lane, unsigned& excl, unsigned& total) {
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    excl = inc - v;
    for (int w = 0; w < wave; ++w) excl += part[w];
    total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) total += part[w];
}

// bits MSB-first behind each other: acc holds the nb < 32 pending bits in its top; whole words are ORed into the shared buffer
struct JpgBits {
    unsigned* out;
    unsigned wi, nb;
    unsigned long long acc;
    __device__ __forceinline__ void put(unsigned value, unsigned n) {       // n <= 27
        acc |= (unsigned long long)value << (64u - nb - n);
        nb += n;
        if (nb >= 32u) {
            atomicOr(&out[wi], (unsigned)(acc >> 32));
            ++wi;
            acc <<= 32;
            nb -= 32u;
        }
    }
    __device__ __forceinline__ void flush() {
        if (nb) atomicOr(&out[wi], (unsigned)(acc >> 32));
    }
};

__global__ void __launch_bounds__(JPG_NT) lwg_jpeg_segment_kernel(const unsigned char* __restrict__ u8, JpgGeom g, JpgQuant qt, int words_ok,
                                                                  unsigned* __restrict__ sizes, unsigned char* __restrict__ slots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jpg_lds[];
    JpgTables& t = *reinterpret_cast<JpgTables*>(jpg_lds);
    short* coef = reinterpret_cast<short*>(jpg_lds + sizeof(JpgTables));                         // [64][JPG_COEF_STRIDE]
    unsigned char* pix = jpg_lds + sizeof(JpgTables) + JPG_COEF_BYTES;                           // [nm][JPG_PIX_STRIDE]
    unsigned* out = reinterpret_cast<unsigned*>(pix);                                            // [jpg_out_words(ri)], once the pixels are dead
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int sid = blockIdx.x, b = sid / g.nseg, seg = sid - b * g.nseg;
    const int g0 = seg * g.ri, nm = min(g.ri, g.nmcu - g0);
    const unsigned char* img = u8 + (size_t)b * g.H * g.W * 3u;
    const size_t rowb = (size_t)g.W * 3u;

    for (int i = tid; i < 2 * 16 + 2 * 256; i += JPG_NT) (&t.dc[0][0])[i] = (&jpg_codes.dc[0][0])[i];
    if (tid < 128) t.q[tid] = qt.q[tid];
    t.bits[tid] = 0u;

    // ---- pixels: word d of row r of MCU m, in the order (r, m, d): the MCUs of an MCU row are neighbours in memory
    const int per_row = nm * 6;
    for (int i = tid; i < 8 * per_row; i += JPG_NT) {
        const int r = i / per_row, rem = i - r * per_row, m = rem / 6, d = rem - m * 6;
        const int gm = g0 + m, my = gm / g.mcux, mx = gm - my * g.mcux;
        const int y = min(my * 8 + r, g.H - 1), x0 = mx * 8;
        const unsigned char* row = img + (size_t)y * rowb;
        unsigned v;
        if (words_ok && x0 + 8 <= g.W) {
            v = *reinterpret_cast<const unsigned*>(row + (size_t)x0 * 3u + 4u * (unsigned)d);
        } else {
            v = 0u;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int j = 4 * d + h, px = min(x0 + j / 3, g.W - 1);
                v |= (unsigned)row[(size_t)px * 3u + (unsigned)(j % 3)] << (8 * h);
            }
        }
        *reinterpret_cast<unsigned*>(pix + (unsigned)m * JPG_PIX_STRIDE + (unsigned)r * 24u + 4u * (unsigned)d) = v;
    }
    __syncthreads();

    // ---- wave c, lane m: block (m, c)
    const int c = wave, m = lane;
    const bool active = c < 3 && m < nm;
    const int tc = c ? 1 : 0;
    if (active) {
        const int kr = c == 0 ? 19595 : c == 1 ? -11059 : 32768;
        const int kg = c == 0 ? 38470 : c == 1 ? -21709 : -27439;
        const int kb = c == 0 ? 7471 : c == 1 ? 32768 : -5329;
        const int add = c == 0 ? 32768 : (128 << 16) + 32767;
        const unsigned* p = reinterpret_cast<const unsigned*>(pix + (unsigned)m * JPG_PIX_STRIDE);
        int X[8][8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            unsigned w[6];
#pragma unroll
            for (int d = 0; d < 6; ++d) w[d] = p[r * 6 + d];
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int R = (int)((w[(3 * x) >> 2] >> (8 * ((3 * x) & 3))) & 255u);
                const int G = (int)((w[(3 * x + 1) >> 2] >> (8 * ((3 * x + 1) & 3))) & 255u);
                const int Bv = (int)((w[(3 * x + 2) >> 2] >> (8 * ((3 * x + 2) & 3))) & 255u);
                const int v = (kr * R + kg * G + kb * Bv + add) >> 16;
                X[r][x] = min(max(v, 0), 255) - 128;
            }
        }
        // columns: T = (M X + 1024) >> 11 (|X| <= 128, |M| <= 4017, |T| <= 1449: every product is a 24-bit one)
        int T[8][8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                int s = 1024;
#pragma unroll
                for (int n = 0; n < 8; ++n) s += __mul24(JPG_DCT[k][n], X[n][x]);
                T[k][x] = s >> 11;
            }
        }
        // rows: F = T M^T, the quantiser, zigzag
        const int* q = t.q + 64 * tc;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int l = 0; l < 8; ++l) {
                int f = 0;
#pragma unroll
                for (int x = 0; x < 8; ++x) f += __mul24(T[k][x], JPG_DCT[l][x]);
                const unsigned Q = (unsigned)q[k * 8 + l];
                const unsigned a = (unsigned)(f < 0 ? -f : f);
                int v = (int)((a + (Q << 14)) / (Q << 15));
                if (k + l) v = min(v, 1023);
                v = f < 0 ? -v : v;
                coef[(unsigned)JPG_UNZIG.pos[k * 8 + l] * JPG_COEF_STRIDE + (unsigned)tid] = (short)v;
                if (k + l == 0) t.dcv[c][m] = v;
            }
        }
    }
    __syncthreads();                                    // the pixels are dead: their bytes become the bit buffer
    const unsigned out_words = jpg_out_words(g.ri);
    for (unsigned i = tid; i < out_words; i += JPG_NT) out[i] = 0u;

    // ---- bits per block
    const unsigned* dct = t.dc[tc];
    const unsigned* act = t.ac[tc];
    int dcd = 0;
    if (active) {
        dcd = t.dcv[c][m] - (m > 0 ? t.dcv[c][m - 1] : 0);
        unsigned s = jpg_size(dcd);
        unsigned nbits = (dct[s] >> 16) + s;
        unsigned run = 0;
        for (int i = 1; i < 64; ++i) {
            const int v = coef[(unsigned)i * JPG_COEF_STRIDE + (unsigned)tid];
            if (v == 0) {
                ++run;
                continue;
            }
            s = jpg_size(v);
            nbits += (run >> 4) * (act[0xF0] >> 16) + (act[((run & 15u) << 4) | s] >> 16) + s;
            run = 0;
        }
        if (run) nbits += act[0] >> 16;
        t.bits[m * 3 + c] = nbits;
    }
    __syncthreads();
    unsigned excl, total;
    jpg_block_scan(t.bits[tid], t.scan, wave, lane, excl, total);
    t.bits[tid] = excl;                                 // (every thread reads and writes its own element)
    __syncthreads();

    // ---- the codes
    if (active) {
        const unsigned pos = t.bits[m * 3 + c];
        JpgBits w{out, pos >> 5, pos & 31u, 0ull};
        unsigned s = jpg_size(dcd);
        w.put(((dct[s] & 0xffffu) << s) | jpg_amp(dcd, s), (dct[s] >> 16) + s);
        unsigned run = 0;
        for (int i = 1; i < 64; ++i) {
            const int v = coef[(unsigned)i * JPG_COEF_STRIDE + (unsigned)tid];
            if (v == 0) {
                ++run;
                continue;
            }
            for (; run >= 16u; run -= 16u) w.put(act[0xF0] & 0xffffu, act[0xF0] >> 16);
            s = jpg_size(v);
            const unsigned cl = act[(run << 4) | s];
            w.put(((cl & 0xffffu) << s) | jpg_amp(v, s), (cl >> 16) + s);
            run = 0;
        }
        if (run) w.put(act[0] & 0xffffu, act[0] >> 16);
        if (m == nm - 1 && c == 2) {                    // the segment's last block: 1-bits to the byte boundary
            const unsigned padn = (8u - (total & 7u)) & 7u;
            if (padn) w.put((1u << padn) - 1u, padn);
        }
        w.flush();
    }
    __syncthreads();

    // ---- stuffing: thread tid owns the words [tid run, (tid + 1) run) of the n bytes
    const unsigned n = (total + 7u) >> 3, nw = (n + 3u) >> 2;
    const unsigned run = (nw + JPG_NT - 1u) / JPG_NT;
    const unsigned w0 = min(nw, (unsigned)tid * run), w1 = min(nw, w0 + run);
    unsigned ff = 0;
    for (unsigned k = w0; k < w1; ++k) {
        const unsigned v = out[k];
#pragma unroll
        for (unsigned h = 0; h < 4u; ++h) ff += (4u * k + h < n) && ((v >> (24u - 8u * h)) & 255u) == 255u;
    }
    unsigned ffx, fft;
    jpg_block_scan(ff, t.ffs, wave, lane, ffx, fft);
    unsigned char* dst = slots + (size_t)sid * g.slot + 4u * w0 + ffx;
    for (unsigned k = w0; k < w1; ++k) {
        const unsigned v = out[k];
#pragma unroll
        for (unsigned h = 0; h < 4u; ++h) {
            const unsigned byte = (v >> (24u - 8u * h)) & 255u;
            if (4u * k + h < n) {
                *dst++ = (unsigned char)byte;
                if (byte == 255u) *dst++ = 0;
            }
        }
    }
    if (tid == 0) sizes[sid] = n + fft;
}

// ---- 4:2:0 (tests/jpeg420_emu.py) ---------------------------------------------------------------------------------------------------------------
// Launch 1 of lwg_jpeg420_scan_u8, one 384-thread workgroup per segment of g.ri <= 64 MCUs of 16 x 16 pixels: wave k = block k of the MCU (Y00 Y01
// Y10 Y11 Cb Cr), lane m = MCU m of the segment.  The MCUs' 16 x 48 pixel bytes -> LDS as above; a luminance wave converts its 8 x 8 pixels, a
// chrominance wave all 16 x 16 and averages the clamped values of every 2 x 2 square, (a + b + c + d + 2) >> 2; from there on - DCT, quantiser,
// bits per block, scan in MCU-major block order, bit writer, padding, stuffing - the steps of the 4:4:4 kernel over 384 blocks.  The Y predictor
// runs through the four Y blocks of an MCU and into the next MCU.  LDS: tables | coefficients int16 [64][6 ri] | pixels, then the bit buffer.
struct Jpg420Tables {
    unsigned dc[2][16];
    unsigned ac[2][256];
    int q[128];
    int dcv[6][JPG420_MAX_MCUS];
    unsigned bits[JPG420_NT];    // bits of block 6 m + k, then its bit offset in the segment
    unsigned scan[8];
    unsigned ffs[8];
};
static_assert(sizeof(Jpg420Tables) % 16 == 0, "the LDS carve-up keeps 16-byte offsets");

// byte j of a row of pixel bytes held as words
#define JPG_BYTE(w, j) ((int)(((w)[(j) >> 2] >> (8 * ((j) & 3))) & 255u))

__global__ void __launch_bounds__(JPG420_NT) lwg_jpeg420_segment_kernel(const unsigned char* __restrict__ u8, JpgGeom g, JpgQuant qt, int words_ok,
                                                                        unsigned* __restrict__ sizes, unsigned char* __restrict__ slots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jpg_lds[];
    Jpg420Tables& t = *reinterpret_cast<Jpg420Tables*>(jpg_lds);
    short* coef = reinterpret_cast<short*>(jpg_lds + sizeof(Jpg420Tables));                      // [64][6 ri]
    unsigned char* pix = jpg_lds + sizeof(Jpg420Tables) + jpg420_coef_bytes(g.ri);               // [nm][JPG420_PIX_STRIDE]
    unsigned* out = reinterpret_cast<unsigned*>(pix);                                            // [jpg420_out_words(ri)], once the pixels are dead
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int sid = blockIdx.x, b = sid / g.nseg, seg = sid - b * g.nseg;
    const int g0 = seg * g.ri, nm = min(g.ri, g.nmcu - g0);
    const unsigned char* img = u8 + (size_t)b * g.H * g.W * 3u;
    const size_t rowb = (size_t)g.W * 3u;

    for (int i = tid; i < 2 * 16 + 2 * 256; i += JPG420_NT) (&t.dc[0][0])[i] = (&jpg_codes.dc[0][0])[i];
    if (tid < 128) t.q[tid] = qt.q[tid];
    t.bits[tid] = 0u;

    // ---- pixels: word d of row r of MCU m, in the order (r, m, d): the MCUs of an MCU row are neighbours in memory
    const int per_row = nm * 12;
    for (int i = tid; i < 16 * per_row; i += JPG420_NT) {
        const int r = i / per_row, rem = i - r * per_row, m = rem / 12, d = rem - m * 12;
        const int gm = g0 + m, my = gm / g.mcux, mx = gm - my * g.mcux;
        const int y = min(my * 16 + r, g.H - 1), x0 = mx * 16;
        const unsigned char* row = img + (size_t)y * rowb;
        unsigned v;
        if (words_ok && x0 + 16 <= g.W) {
            v = *reinterpret_cast<const unsigned*>(row + (size_t)x0 * 3u + 4u * (unsigned)d);
        } else {
            v = 0u;
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int j = 4 * d + h, px = min(x0 + j / 3, g.W - 1);
                v |= (unsigned)row[(size_t)px * 3u + (unsigned)(j % 3)] << (8 * h);
            }
        }
        *reinterpret_cast<unsigned*>(pix + (unsigned)m * JPG420_PIX_STRIDE + (unsigned)r * 48u + 4u * (unsigned)d) = v;
    }
    __syncthreads();

    // ---- wave k, lane m: block (m, k)
    const int k = wave, m = lane;
    const bool active = m < nm;
    const int c = k < 4 ? 0 : k - 3, tc = c ? 1 : 0;
    const unsigned cs = 6u * (unsigned)g.ri, ci = (unsigned)(k * g.ri + m);                       // the coefficients' stride and this block's column
    if (active) {
        const int kr = c == 0 ? 19595 : c == 1 ? -11059 : 32768;
        const int kg = c == 0 ? 38470 : c == 1 ? -21709 : -27439;
        const int kb = c == 0 ? 7471 : c == 1 ? 32768 : -5329;
        const int add = c == 0 ? 32768 : (128 << 16) + 32767;
        const unsigned* p = reinterpret_cast<const unsigned*>(pix + (unsigned)m * JPG420_PIX_STRIDE);
        int X[8][8];
        if (c == 0) {                                   // rows 8 (k >> 1) .., bytes 24 (k & 1) .. of the MCU
            p += (k >> 1) * 8 * 12 + (k & 1) * 6;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                unsigned w[6];
#pragma unroll
                for (int d = 0; d < 6; ++d) w[d] = p[r * 12 + d];
#pragma unroll
                for (int x = 0; x < 8; ++x) {
                    const int v = (kr * JPG_BYTE(w, 3 * x) + kg * JPG_BYTE(w, 3 * x + 1) + kb * JPG_BYTE(w, 3 * x + 2) + add) >> 16;
                    X[r][x] = min(max(v, 0), 255) - 128;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                int sum[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) sum[x] = 2;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    unsigned w[12];
#pragma unroll
                    for (int d = 0; d < 12; ++d) w[d] = p[(2 * r + h) * 12 + d];
#pragma unroll
                    for (int x = 0; x < 16; ++x) {
                        const int v = (kr * JPG_BYTE(w, 3 * x) + kg * JPG_BYTE(w, 3 * x + 1) + kb * JPG_BYTE(w, 3 * x + 2) + add) >> 16;
                        sum[x >> 1] += min(max(v, 0), 255);
                    }
                }
#pragma unroll
                for (int x = 0; x < 8; ++x) X[r][x] = (sum[x] >> 2) - 128;
            }
        }
        // columns: T = (M X + 1024) >> 11 (|X| <= 128, |M| <= 4017, |T| <= 1449: every product is a 24-bit one)
        int T[8][8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                int s = 1024;
#pragma unroll
                for (int n = 0; n < 8; ++n) s += __mul24(JPG_DCT[u][n], X[n][x]);
                T[u][x] = s >> 11;
            }
        }
        // rows: F = T M^T, the quantiser, zigzag
        const int* q = t.q + 64 * tc;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
#pragma unroll
            for (int l = 0; l < 8; ++l) {
                int f = 0;
#pragma unroll
                for (int x = 0; x < 8; ++x) f += __mul24(T[u][x], JPG_DCT[l][x]);
                const unsigned Q = (unsigned)q[u * 8 + l];
                const unsigned a = (unsigned)(f < 0 ? -f : f);
                int v = (int)((a + (Q << 14)) / (Q << 15));
                if (u + l) v = min(v, 1023);
                v = f < 0 ? -v : v;
                coef[(unsigned)JPG_UNZIG.pos[u * 8 + l] * cs + ci] = (short)v;
                if (u + l == 0) t.dcv[k][m] = v;
            }
        }
    }
    __syncthreads();                                    // the pixels are dead: their bytes become the bit buffer
    const unsigned out_words = jpg420_out_words(g.ri);
    for (unsigned i = tid; i < out_words; i += JPG420_NT) out[i] = 0u;

    // ---- bits per block
    const unsigned* dct = t.dc[tc];
    const unsigned* act = t.ac[tc];
    int dcd = 0;
    if (active) {
        // the block in front of this one in its component: Y k - 1 of the MCU, Y11 of the MCU before, or the chroma block of the MCU before
        int prev = 0;
        if (c == 0 && k > 0) prev = t.dcv[k - 1][m];
        else if (m > 0) prev = t.dcv[c == 0 ? 3 : k][m - 1];
        dcd = t.dcv[k][m] - prev;
        unsigned s = jpg_size(dcd);
        unsigned nbits = (dct[s] >> 16) + s;
        unsigned run = 0;
        for (int i = 1; i < 64; ++i) {
            const int v = coef[(unsigned)i * cs + ci];
            if (v == 0) {
                ++run;
                continue;
            }
            s = jpg_size(v);
            nbits += (run >> 4) * (act[0xF0] >> 16) + (act[((run & 15u) << 4) | s] >> 16) + s;
            run = 0;
        }
        if (run) nbits += act[0] >> 16;
        t.bits[m * 6 + k] = nbits;
    }
    __syncthreads();
    unsigned excl, total;
    jpg_block_scan<JPG420_NT / 64>(t.bits[tid], t.scan, wave, lane, excl, total);
    t.bits[tid] = excl;                                 // (every thread reads and writes its own element)
    __syncthreads();

    // ---- the codes
    if (active) {
        const unsigned pos = t.bits[m * 6 + k];
        JpgBits w{out, pos >> 5, pos & 31u, 0ull};
        unsigned s = jpg_size(dcd);
        w.put(((dct[s] & 0xffffu) << s) | jpg_amp(dcd, s), (dct[s] >> 16) + s);
        unsigned run = 0;
        for (int i = 1; i < 64; ++i) {
            const int v = coef[(unsigned)i * cs + ci];
            if (v == 0) {
                ++run;
                continue;
            }
            for (; run >= 16u; run -= 16u) w.put(act[0xF0] & 0xffffu, act[0xF0] >> 16);
            s = jpg_size(v);
            const unsigned cl = act[(run << 4) | s];
            w.put(((cl & 0xffffu) << s) | jpg_amp(v, s), (cl >> 16) + s);
            run = 0;
        }
        if (run) w.put(act[0] & 0xffffu, act[0] >> 16);
        if (m == nm - 1 && k == 5) {                    // the segment's last block: 1-bits to the byte boundary
            const unsigned padn = (8u - (total & 7u)) & 7u;
            if (padn) w.put((1u << padn) - 1u, padn);
        }
        w.flush();
    }
    __syncthreads();

    // ---- stuffing: thread tid owns the words [tid run, (tid + 1) run) of the n bytes
    const unsigned n = (total + 7u) >> 3, nw = (n + 3u) >> 2;
    const unsigned run = (nw + JPG420_NT - 1u) / JPG420_NT;
    const unsigned w0 = min(nw, (unsigned)tid * run), w1 = min(nw, w0 + run);
    unsigned ff = 0;
    for (unsigned i = w0; i < w1; ++i) {
        const unsigned v = out[i];
#pragma unroll
        for (unsigned h = 0; h < 4u; ++h) ff += (4u * i + h < n) && ((v >> (24u - 8u * h)) & 255u) == 255u;
    }
    unsigned ffx, fft;
    jpg_block_scan<JPG420_NT / 64>(ff, t.ffs, wave, lane, ffx, fft);
    unsigned char* dst = slots + (size_t)sid * g.slot + 4u * w0 + ffx;
    for (unsigned i = w0; i < w1; ++i) {
        const unsigned v = out[i];
#pragma unroll
        for (unsigned h = 0; h < 4u; ++h) {
            const unsigned byte = (v >> (24u - 8u * h)) & 255u;
            if (4u * i + h < n) {
                *dst++ = (unsigned char)byte;
                if (byte == 255u) *dst++ = 0;
            }
        }
    }
    if (tid == 0) sizes[sid] = n + fft;
}
#undef JPG_BYTE

// Launch 2 (both formats): segment (b, seg) of the workspace -> scans[b] behind the segments and markers before it; the marker behind it, or nbytes.
__global__ void __launch_bounds__(JPG_NT) lwg_jpeg_pack_kernel(JpgGeom g, const unsigned* __restrict__ sizes, const unsigned char* __restrict__ slots,
                                                               unsigned char* __restrict__ scans, int* __restrict__ nbytes) {
    __shared__ unsigned part[JPG_NT / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int sid = blockIdx.x, b = sid / g.nseg, seg = sid - b * g.nseg;
    const unsigned* fs = sizes + (size_t)b * g.nseg;
    unsigned before = 0;
    for (int k = tid; k < seg; k += JPG_NT) before += fs[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    if (lane == 0) part[wave] = before;
    __syncthreads();
    const size_t off = 2u * (size_t)seg + part[0] + part[1] + part[2] + part[3];
    const unsigned size = fs[seg];
    unsigned char* dst = scans + (size_t)b * g.cap + off;
    const unsigned char* src = slots + (size_t)sid * g.slot;
    const unsigned* src32 = reinterpret_cast<const unsigned*>(src);
    // destination words whole, the bytes in front of the first and behind the last one by one; a source word pair is funnelled into each
    const unsigned head = min(size, (unsigned)((4u - ((uintptr_t)dst & 3u)) & 3u));
    const unsigned nwords = (size - head) / 4u, tail0 = head + 4u * nwords;
    if ((unsigned)tid < head) dst[tid] = src[tid];
    if ((unsigned)tid < size - tail0) dst[tail0 + tid] = src[tail0 + tid];
    unsigned* dst32 = reinterpret_cast<unsigned*>(dst + head);
    const unsigned sh = 8u * head;
    for (unsigned k = tid; k < nwords; k += JPG_NT) {
        const unsigned lo = src32[k];
        unsigned v = lo;
        if (sh) v = (lo >> sh) | (src32[k + 1u] << (32u - sh));             // (within the slot: it ends >= 16 bytes behind the segment)
        dst32[k] = v;
    }
    if (tid == 0) {
        if (seg < g.nseg - 1) dst[size] = 0xff, dst[size + 1u] = (unsigned char)(0xd0 + (seg & 7));
        else nbytes[b] = (int)(off + size);
    }
}

}  // namespace

extern "C" int lwg_jpeg_max_mcus_per_segment(void) { return JPG_MAX_MCUS; }

extern "C" size_t lwg_jpeg_scan_capacity(int H, int W, int mcus_per_segment) {
    JpgGeom g;
    return jpg_geom(1, H, W, mcus_per_segment, g) ? g.cap : 0;
}

extern "C" size_t lwg_jpeg_scan_ws_bytes(int B, int H, int W, int mcus_per_segment) {
    JpgGeom g;
    if (!jpg_geom(B, H, W, mcus_per_segment, g)) return 0;
    return (size_t)g.meta + (size_t)B * g.nseg * g.slot;
}

extern "C" int lwg_jpeg_scan_u8(const uint8_t* u8, int B, int H, int W, const uint8_t* qtab, int mcus_per_segment, void* ws, uint8_t* scans, int32_t* nbytes,
                                lwg_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    JpgGeom g;
    if (!u8 || !qtab || !ws || !scans || !nbytes || ((uintptr_t)ws & 15u) || !jpg_geom(B, H, W, mcus_per_segment, g)) return (int)hipErrorInvalidValue;
    JpgQuant qt;
    for (int i = 0; i < 128; ++i) {
        if (qtab[i] == 0) return (int)hipErrorInvalidValue;
        qt.q[i] = qtab[i];
    }
    const size_t nslots = (size_t)B * g.nseg;
    unsigned* sizes = reinterpret_cast<unsigned*>(ws);
    unsigned char* slots = reinterpret_cast<unsigned char*>(ws) + g.meta;
    const size_t pixb = ((size_t)g.ri * JPG_PIX_STRIDE + 15u) & ~(size_t)15u, outb = (4u * (size_t)jpg_out_words(g.ri) + 15u) & ~(size_t)15u;
    const size_t lds = sizeof(JpgTables) + JPG_COEF_BYTES + (pixb > outb ? pixb : outb);
    if (lds > 65536) {
        static unsigned long long lds_ok = 0;
        const hipError_t e = lwg_allow_dynamic_lds(reinterpret_cast<const void*>(lwg_jpeg_segment_kernel), 160 * 1024, lds_ok);
        if (e != hipSuccess) return (int)e;
    }
    // whole words of pixels can be loaded where every row of every frame starts on a word
    const int words_ok = ((uintptr_t)u8 & 3u) == 0 && (W & 3) == 0;
    hipLaunchKernelGGL(lwg_jpeg_segment_kernel, dim3((unsigned)nslots), dim3(JPG_NT), lds, stream, (const unsigned char*)u8, g, qt, words_ok, sizes, slots);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lwg_jpeg_pack_kernel, dim3((unsigned)nslots), dim3(JPG_NT), 0, stream, g, (const unsigned*)sizes, (const unsigned char*)slots, scans, nbytes);
    return (int)hipGetLastError();
}

// ---- 4:2:0: the same two launches; launch 2 is lwg_jpeg_pack_kernel itself on the six-block geometry
extern "C" int lwg_jpeg420_max_mcus_per_segment(void) { return JPG420_MAX_MCUS; }

extern "C" size_t lwg_jpeg420_scan_capacity(int H, int W, int mcus_per_segment) {
    JpgGeom g;
    return jpg420_geom(1, H, W, mcus_per_segment, g) ? g.cap : 0;
}

extern "C" size_t lwg_jpeg420_scan_ws_bytes(int B, int H, int W, int mcus_per_segment) {
    JpgGeom g;
    if (!jpg420_geom(B, H, W, mcus_per_segment, g)) return 0;
    return (size_t)g.meta + (size_t)B * g.nseg * g.slot;
}

extern "C" int lwg_jpeg420_scan_u8(const uint8_t* u8, int B, int H, int W, const uint8_t* qtab, int mcus_per_segment, void* ws, uint8_t* scans, int32_t* nbytes,
                                   lwg_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    JpgGeom g;
    if (!u8 || !qtab || !ws || !scans || !nbytes || ((uintptr_t)ws & 15u) || !jpg420_geom(B, H, W, mcus_per_segment, g)) return (int)hipErrorInvalidValue;
    JpgQuant qt;
    for (int i = 0; i < 128; ++i) {
        if (qtab[i] == 0) return (int)hipErrorInvalidValue;
        qt.q[i] = qtab[i];
    }
    const size_t nslots = (size_t)B * g.nseg;
    unsigned* sizes = reinterpret_cast<unsigned*>(ws);
    unsigned char* slots = reinterpret_cast<unsigned char*>(ws) + g.meta;
    const size_t pixb = ((size_t)g.ri * JPG420_PIX_STRIDE + 15u) & ~(size_t)15u, outb = (4u * (size_t)jpg420_out_words(g.ri) + 15u) & ~(size_t)15u;
    const size_t lds = sizeof(Jpg420Tables) + jpg420_coef_bytes(g.ri) + (pixb > outb ? pixb : outb);      // 134 864 bytes at 64 MCUs, 70 352 at 32
    if (lds > 65536) {
        static unsigned long long lds_ok = 0;
        const hipError_t e = lwg_allow_dynamic_lds(reinterpret_cast<const void*>(lwg_jpeg420_segment_kernel), 160 * 1024, lds_ok);
        if (e != hipSuccess) return (int)e;
    }
    // whole words of pixels can be loaded where every row of every frame starts on a word
    const int words_ok = ((uintptr_t)u8 & 3u) == 0 && (W & 3) == 0;
    hipLaunchKernelGGL(lwg_jpeg420_segment_kernel, dim3((unsigned)nslots), dim3(JPG420_NT), lds, stream, (const unsigned char*)u8, g, qt, words_ok, sizes, slots);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lwg_jpeg_pack_kernel, dim3((unsigned)nslots), dim3(JPG_NT), 0, stream, g, (const unsigned*)sizes, (const unsigned char*)slots, scans, nbytes);
    return (int)hipGetLastError();
}
