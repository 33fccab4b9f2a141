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
// Per-frame Huffman tables ('lwg_jpeg_scan_opt_u8', 'lwg_jpeg420_scan_opt_u8', tests/jpeghuff_emu.py): both launch-1 kernels are templates on what they
// do behind the quantiser - code with the fixed tables, count symbols, or code with the frame's own tables - and 'lwg_jpeg_huff_kernel' between the
// counting and the coding launch builds those tables, one wave per frame and table.
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

// What a segment kernel does behind the quantiser.  JPG_FIXED: codes with the Annex K tables (lwg_jpeg_scan_u8, lwg_jpeg420_scan_u8).  JPG_GIVEN: codes
// with the frame's own 544 words at codes + b JPG_HIST_WORDS, on the 212-byte block bound.  JPG_COUNT: codes nothing - the tables' LDS words count the
// segment's symbols and go to hist + sid JPG_HIST_WORDS (plain stores: a partial histogram per segment, summed by the table kernel).
enum { JPG_FIXED = 0, JPG_GIVEN = 1, JPG_COUNT = 2 };
constexpr unsigned jpg_block_bytes(int mode) { return mode == JPG_GIVEN ? JPG_OPT_BLOCK_BYTES : JPG_BLOCK_BYTES; }

template <int MODE>
__device__ __forceinline__ unsigned jpg_table_word(const unsigned* __restrict__ codes, int b, int i) {
    if constexpr (MODE == JPG_FIXED) return (&jpg_codes.dc[0][0])[i];
    else if constexpr (MODE == JPG_GIVEN) return codes[(size_t)b * JPG_HIST_WORDS + i];
    else return 0u;
}

// the symbols of one block, in the order the bit-count loop visits them: += 1 in the LDS counters of its two tables
__device__ __forceinline__ void jpg_count_block(unsigned* dct, unsigned* act, int dcd, const short* coef, unsigned stride) {
    atomicAdd(&dct[jpg_size(dcd)], 1u);
    unsigned run = 0;
    for (int i = 1; i < 64; ++i) {
        const int v = coef[(unsigned)i * stride];
        if (v == 0) {
            ++run;
            continue;
        }
        if (run >> 4) atomicAdd(&act[0xF0], run >> 4);
        atomicAdd(&act[((run & 15u) << 4) | jpg_size(v)], 1u);
        run = 0;
    }
    if (run) atomicAdd(&act[0], 1u);
}

template <int MODE>
__global__ void __launch_bounds__(JPG_NT) lwg_jpeg_segment_kernel(const unsigned char* __restrict__ u8, JpgGeom g, JpgQuant qt, int words_ok,
                                                                  const unsigned* __restrict__ codes, unsigned* __restrict__ hist,
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

    for (int i = tid; i < JPG_HIST_WORDS; i += JPG_NT) (&t.dc[0][0])[i] = jpg_table_word<MODE>(codes, b, i);
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
    if constexpr (MODE == JPG_COUNT) {
        if (active) jpg_count_block(t.dc[tc], t.ac[tc], t.dcv[c][m] - (m > 0 ? t.dcv[c][m - 1] : 0), coef + tid, JPG_COEF_STRIDE);
        __syncthreads();
        for (int i = tid; i < JPG_HIST_WORDS; i += JPG_NT) hist[(size_t)sid * JPG_HIST_WORDS + i] = (&t.dc[0][0])[i];
        return;
    }
    const unsigned out_words = jpg_out_words_of(g.ri, 3u, jpg_block_bytes(MODE));
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

template <int MODE>
__global__ void __launch_bounds__(JPG420_NT) lwg_jpeg420_segment_kernel(const unsigned char* __restrict__ u8, JpgGeom g, JpgQuant qt, int words_ok,
                                                                        const unsigned* __restrict__ codes, unsigned* __restrict__ hist,
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

    for (int i = tid; i < JPG_HIST_WORDS; i += JPG420_NT) (&t.dc[0][0])[i] = jpg_table_word<MODE>(codes, b, i);
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
    if constexpr (MODE == JPG_COUNT) {
        if (active) {
            int prev = 0;
            if (c == 0 && k > 0) prev = t.dcv[k - 1][m];
            else if (m > 0) prev = t.dcv[c == 0 ? 3 : k][m - 1];
            jpg_count_block(t.dc[tc], t.ac[tc], t.dcv[k][m] - prev, coef + ci, cs);
        }
        __syncthreads();
        for (int i = tid; i < JPG_HIST_WORDS; i += JPG420_NT) hist[(size_t)sid * JPG_HIST_WORDS + i] = (&t.dc[0][0])[i];
        return;
    }
    const unsigned out_words = jpg_out_words_of(g.ri, 6u, jpg_block_bytes(MODE));
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


// ---- per-frame Huffman tables (tests/jpeghuff_emu.py) -------------------------------------------------------------------------------------------
// lwg_jpeg_hist_u8's second launch, one workgroup per frame: the segments' partial histograms (JpgCodes layout) -> hist (B, 4, 256) in DHT order - DC
// luminance, AC luminance, DC chrominance, AC chrominance; the DC rows are 0 from symbol 16 on.
__global__ void __launch_bounds__(JPG_NT) lwg_jpeg_hist_sum_kernel(const unsigned* __restrict__ parts, int nparts, unsigned* __restrict__ hist) {
    const int b = blockIdx.x;
    const unsigned* src = parts + (size_t)b * nparts * JPG_HIST_WORDS;
    for (int w = threadIdx.x; w < 4 * 256; w += JPG_NT) {
        const int k = w >> 8, sym = w & 255, tc = k >> 1;
        unsigned v = 0;
        if ((k & 1) || sym < 16) {
            const int off = (k & 1) ? 32 + 256 * tc + sym : 16 * tc + sym;
            for (int p = 0; p < nparts; ++p) v += src[(size_t)p * JPG_HIST_WORDS + off];
        }
        hist[(size_t)b * 1024 + w] = v;
    }
}

__device__ __forceinline__ unsigned long long jpg_shfl_xor64(unsigned long long v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// Table construction, ONE wave per (frame, table), table k in DHT order: the rule of tests/jpeghuff_emu.py 'table' (Annex K.2 as libjpeg 6b codes it).
// Slot i of the 257 (256: the reserved symbol, count 1) lives in lane i % 64, register i / 64.  A slot that heads a set holds the key
// count << 9 | (256 - i): the least key is the least count and, among equal counts, the largest index (counts sum below 2^41).  A merge is one wave
// reduction for the TWO least keys; every lane then adds a bit to its slots of either set and renames them to c1.  At most 256 merges; a frame's table
// has a few dozen symbols.  Then lengths are counted in LDS (length <= 256), lane 0 limits them to 16 bits and takes the reserved code away, and
// the used symbols get their rank under (length before limiting, value) by counting smaller keys.
// hist: wide = 1: (B, 4, 256) counts of the caller; wide = 0: (B, nparts, JPG_HIST_WORDS) partial histograms of the segment kernels.
// dht (B, 4, JPG_DHT_BYTES): counts per length, symbols, unused slots 0.  codes (B, JPG_HIST_WORDS): code | length << 16 by symbol, 0: no code; a DC
// table holds its symbols below 16 there.
__global__ void __launch_bounds__(64) lwg_jpeg_huff_kernel(const unsigned* __restrict__ hist, int nparts, int wide, unsigned char* __restrict__ dht,
                                                           unsigned* __restrict__ codes) {
    __shared__ unsigned nlen[260];                   // codes per length 0 .. 257
    __shared__ unsigned keys[256];                   // the used symbols in value order: length before limiting << 8 | symbol
    __shared__ unsigned first[17], before[17];       // per length 1 .. 16: its first code, the symbols in front of it
    __shared__ unsigned cw[256];
    __shared__ __attribute__((aligned(4))) unsigned char outb[JPG_DHT_BYTES];
    constexpr unsigned long long NOKEY = ~0ull;
    const int lane = threadIdx.x, b = blockIdx.x >> 2, k = blockIdx.x & 3, tc = k >> 1, isac = k & 1;
    const int coff = isac ? 32 + 256 * tc : 16 * tc;             // the table's place in the JpgCodes layout
    const int nsym = wide || isac ? 256 : 16;
    const unsigned* src = wide ? hist + ((size_t)b * 4 + k) * 256 : hist + (size_t)b * nparts * JPG_HIST_WORDS + coff;
    const size_t pstride = wide ? 0 : JPG_HIST_WORDS;
    const int np = wide ? 1 : nparts;

    unsigned long long key[5];
    int set[5];
    unsigned depth[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int i = lane + 64 * j;
        unsigned long long cnt = 0;
        if (i < nsym) {
            for (int p = 0; p < np; ++p) cnt += src[(size_t)p * pstride + i];
        } else if (i == 256) {
            cnt = 1;
        }
        key[j] = cnt ? (cnt << 9) | (unsigned)(256 - i) : NOKEY;
        set[j] = i <= 256 ? i : -1;
        depth[j] = 0;
    }
    for (int it = 0; it < 256; ++it) {
        unsigned long long m1 = NOKEY, m2 = NOKEY;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const unsigned long long v = key[j];
            if (v < m1) m2 = m1, m1 = v;
            else if (v < m2) m2 = v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long o1 = jpg_shfl_xor64(m1, o), o2 = jpg_shfl_xor64(m2, o);
            const unsigned long long lo = m1 < o1 ? m1 : o1, hi = m1 < o1 ? o1 : m1, r = m2 < o2 ? m2 : o2;
            m1 = lo, m2 = hi < r ? hi : r;
        }
        if (m2 == NOKEY) break;                                  // (the same in every lane)
        const int c1 = 256 - (int)(m1 & 511u), c2 = 256 - (int)(m2 & 511u);
        const unsigned long long merged = (((m1 >> 9) + (m2 >> 9)) << 9) | (m1 & 511u);
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int i = lane + 64 * j;
            if (set[j] == c1 || set[j] == c2) ++depth[j], set[j] = c1;
            if (i == c1) key[j] = merged;
            if (i == c2) key[j] = NOKEY;
        }
    }

    for (int i = lane; i < 260; i += 64) nlen[i] = 0u;
    for (int i = lane; i < 256; i += 64) cw[i] = 0u;
    for (int i = lane; i < JPG_DHT_BYTES / 4; i += 64) reinterpret_cast<unsigned*>(outb)[i] = 0u;
    __syncthreads();
    unsigned n = 0, deepest = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const bool real = j < 4 && depth[j] > 0;
        if (depth[j]) atomicAdd(&nlen[depth[j]], 1u);            // depth <= 256; the reserved symbol counts
        deepest = max(deepest, depth[j]);
        const unsigned long long mask = __ballot(real);
        if (real) keys[n + __popcll(mask & ((1ull << lane) - 1ull))] = (depth[j] << 8) | (unsigned)(lane + 64 * j);
        n += (unsigned)__popcll(mask);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) deepest = max(deepest, (unsigned)__shfl_xor(deepest, o, 64));
    __syncthreads();
    if (lane == 0 && n) {
        for (int i = (int)deepest; i > 16; --i) {
            while ((int)nlen[i] > 0) {                           // (even at the deepest length of a full tree: it reaches 0)
                int j = i - 2;
                while (j > 0 && nlen[j] == 0) --j;
                nlen[i] -= 2, nlen[i - 1] += 1, nlen[j + 1] += 2, nlen[j] -= 1;
            }
        }
        for (int i = min((int)deepest, 16); i > 0; --i) {
            if (nlen[i]) {
                --nlen[i];
                break;
            }
        }
    }
    __syncthreads();
    if (lane >= 1 && lane <= 16) {
        unsigned code = 0, c = 0;
        for (int l = 1; l < lane; ++l) code += nlen[l] << (lane - l), c += nlen[l];
        first[lane] = code, before[lane] = c;
        outb[lane - 1] = (unsigned char)(n ? nlen[lane] : 0u);
    }
    __syncthreads();
    for (unsigned e = lane; e < n; e += 64) {
        const unsigned mine = keys[e];
        unsigned rank = 0;
        for (unsigned x = 0; x < n; ++x) rank += keys[x] < mine;
        int l = 1;
        while (l < 16 && before[l] + nlen[l] <= rank) ++l;
        outb[16 + rank] = (unsigned char)(mine & 255u);
        cw[mine & 255u] = (first[l] + rank - before[l]) | ((unsigned)l << 16);
    }
    __syncthreads();
    unsigned* d32 = reinterpret_cast<unsigned*>(dht + ((size_t)b * 4 + k) * JPG_DHT_BYTES);
    for (int i = lane; i < JPG_DHT_BYTES / 4; i += 64) d32[i] = reinterpret_cast<const unsigned*>(outb)[i];
    for (int i = lane; i < (isac ? 256 : 16); i += 64) codes[(size_t)b * JPG_HIST_WORDS + coff + i] = cw[i];
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------------
bool jpg_quant(const uint8_t* qtab, JpgQuant& qt) {
    for (int i = 0; i < 128; ++i) {
        if (qtab[i] == 0) return false;
        qt.q[i] = qtab[i];
    }
    return true;
}

// launch 1 of a format in one of its modes, one workgroup per segment
template <bool F420, int MODE>
hipError_t jpg_launch_segments(const uint8_t* u8, const JpgGeom& g, const JpgQuant& qt, const unsigned* codes, unsigned* hist, unsigned* sizes,
                               unsigned char* slots, hipStream_t stream) {
    const size_t nslots = (size_t)g.B * g.nseg;
    const size_t pixb = ((size_t)g.ri * (F420 ? JPG420_PIX_STRIDE : JPG_PIX_STRIDE) + 15u) & ~(size_t)15u;
    const size_t outb = MODE == JPG_COUNT ? 0 : (4u * (size_t)jpg_out_words_of(g.ri, F420 ? 6u : 3u, jpg_block_bytes(MODE)) + 15u) & ~(size_t)15u;
    // 4:2:0 at 64 MCUs: 134 864 bytes with the fixed tables, 136 400 with given ones; 70 352 / 71 120 at 32
    const size_t lds = (F420 ? sizeof(Jpg420Tables) + jpg420_coef_bytes(g.ri) : sizeof(JpgTables) + JPG_COEF_BYTES) + (pixb > outb ? pixb : outb);
    // whole words of pixels can be loaded where every row of every frame starts on a word
    const int words_ok = ((uintptr_t)u8 & 3u) == 0 && (g.W & 3) == 0;
    if constexpr (F420) {
        if (lds > 65536) {
            static unsigned long long lds_ok = 0;
            const hipError_t e = lwg_allow_dynamic_lds(reinterpret_cast<const void*>(lwg_jpeg420_segment_kernel<MODE>), 160 * 1024, lds_ok);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(lwg_jpeg420_segment_kernel<MODE>, dim3((unsigned)nslots), dim3(JPG420_NT), lds, stream, (const unsigned char*)u8, g, qt, words_ok,
                           codes, hist, sizes, slots);
    } else {
        if (lds > 65536) {
            static unsigned long long lds_ok = 0;
            const hipError_t e = lwg_allow_dynamic_lds(reinterpret_cast<const void*>(lwg_jpeg_segment_kernel<MODE>), 160 * 1024, lds_ok);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(lwg_jpeg_segment_kernel<MODE>, dim3((unsigned)nslots), dim3(JPG_NT), lds, stream, (const unsigned char*)u8, g, qt, words_ok, codes,
                           hist, sizes, slots);
    }
    return hipGetLastError();
}

template <bool F420>
bool jpg_geom_for(bool opt, int B, int H, int W, int ri, JpgGeom& g) {
    if (F420) return opt ? jpg420_geom_opt(B, H, W, ri, g) : jpg420_geom(B, H, W, ri, g);
    return opt ? jpg_geom_opt(B, H, W, ri, g) : jpg_geom(B, H, W, ri, g);
}

// the fixed-table scan: two launches
template <bool F420>
int jpg_scan_fixed(const uint8_t* u8, int B, int H, int W, const uint8_t* qtab, int ri, void* ws, uint8_t* scans, int32_t* nbytes, hipStream_t stream) {
    JpgGeom g;
    JpgQuant qt;
    if (!u8 || !qtab || !ws || !scans || !nbytes || ((uintptr_t)ws & 15u) || !jpg_geom_for<F420>(false, B, H, W, ri, g) || !jpg_quant(qtab, qt))
        return (int)hipErrorInvalidValue;
    unsigned* sizes = reinterpret_cast<unsigned*>(ws);
    unsigned char* slots = reinterpret_cast<unsigned char*>(ws) + g.meta;
    const hipError_t e = jpg_launch_segments<F420, JPG_FIXED>(u8, g, qt, nullptr, nullptr, sizes, slots, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lwg_jpeg_pack_kernel, dim3((unsigned)((size_t)B * g.nseg)), dim3(JPG_NT), 0, stream, g, (const unsigned*)sizes,
                       (const unsigned char*)slots, scans, nbytes);
    return (int)hipGetLastError();
}

// the workspace of the per-frame form: sizes | slots | the segments' partial histograms | the frames' code words
struct JpgOptWs {
    size_t slots, parts, codes, bytes;
};
JpgOptWs jpg_opt_ws(const JpgGeom& g) {
    JpgOptWs w;
    w.slots = g.meta;
    w.parts = w.slots + (size_t)g.B * g.nseg * g.slot;
    w.codes = w.parts + (size_t)g.B * g.nseg * JPG_HIST_WORDS * 4u;
    w.bytes = w.codes + (size_t)g.B * JPG_HIST_WORDS * 4u;
    return w;
}

template <bool F420>
size_t jpg_opt_ws_bytes(int B, int H, int W, int ri) {
    JpgGeom g;
    return jpg_geom_for<F420>(true, B, H, W, ri, g) ? jpg_opt_ws(g).bytes : 0;
}

template <bool F420>
int jpg_hist(const uint8_t* u8, int B, int H, int W, const uint8_t* qtab, int ri, void* ws, uint32_t* hist, hipStream_t stream) {
    JpgGeom g;
    JpgQuant qt;
    if (!u8 || !qtab || !ws || !hist || ((uintptr_t)ws & 15u) || ((uintptr_t)hist & 3u) || !jpg_geom_for<F420>(true, B, H, W, ri, g) || !jpg_quant(qtab, qt))
        return (int)hipErrorInvalidValue;
    unsigned* parts = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(ws) + jpg_opt_ws(g).parts);
    const hipError_t e = jpg_launch_segments<F420, JPG_COUNT>(u8, g, qt, nullptr, parts, nullptr, nullptr, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lwg_jpeg_hist_sum_kernel, dim3((unsigned)B), dim3(JPG_NT), 0, stream, (const unsigned*)parts, g.nseg, (unsigned*)hist);
    return (int)hipGetLastError();
}

// statistics, tables, coding, pack: four launches
template <bool F420>
int jpg_scan_opt(const uint8_t* u8, int B, int H, int W, const uint8_t* qtab, int ri, void* ws, uint8_t* scans, int32_t* nbytes, uint8_t* tables,
                 hipStream_t stream) {
    JpgGeom g;
    JpgQuant qt;
    if (!u8 || !qtab || !ws || !scans || !nbytes || !tables || ((uintptr_t)ws & 15u) || ((uintptr_t)tables & 3u) || B > 0x1fffffff ||
        !jpg_geom_for<F420>(true, B, H, W, ri, g) || !jpg_quant(qtab, qt))
        return (int)hipErrorInvalidValue;
    const JpgOptWs w = jpg_opt_ws(g);
    unsigned char* base = reinterpret_cast<unsigned char*>(ws);
    unsigned* sizes = reinterpret_cast<unsigned*>(base);
    unsigned char* slots = base + w.slots;
    unsigned* parts = reinterpret_cast<unsigned*>(base + w.parts);
    unsigned* codes = reinterpret_cast<unsigned*>(base + w.codes);
    hipError_t e = jpg_launch_segments<F420, JPG_COUNT>(u8, g, qt, nullptr, parts, nullptr, nullptr, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lwg_jpeg_huff_kernel, dim3(4u * (unsigned)B), dim3(64), 0, stream, (const unsigned*)parts, g.nseg, 0, (unsigned char*)tables, codes);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    e = jpg_launch_segments<F420, JPG_GIVEN>(u8, g, qt, codes, nullptr, sizes, slots, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lwg_jpeg_pack_kernel, dim3((unsigned)((size_t)B * g.nseg)), dim3(JPG_NT), 0, stream, g, (const unsigned*)sizes,
                       (const unsigned char*)slots, scans, nbytes);
    return (int)hipGetLastError();
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
                                lwg_stream_t stream) {
    return jpg_scan_fixed<false>(u8, B, H, W, qtab, mcus_per_segment, ws, scans, nbytes, reinterpret_cast<hipStream_t>(stream));
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
                                   lwg_stream_t stream) {
    return jpg_scan_fixed<true>(u8, B, H, W, qtab, mcus_per_segment, ws, scans, nbytes, reinterpret_cast<hipStream_t>(stream));
}

// ---- per-frame Huffman tables: both formats on the 212-byte block bound
extern "C" size_t lwg_jpeg_scan_opt_capacity(int H, int W, int mcus_per_segment) {
    JpgGeom g;
    return jpg_geom_opt(1, H, W, mcus_per_segment, g) ? g.cap : 0;
}
extern "C" size_t lwg_jpeg420_scan_opt_capacity(int H, int W, int mcus_per_segment) {
    JpgGeom g;
    return jpg420_geom_opt(1, H, W, mcus_per_segment, g) ? g.cap : 0;
}
extern "C" size_t lwg_jpeg_scan_opt_ws_bytes(int B, int H, int W, int mcus_per_segment) { return jpg_opt_ws_bytes<false>(B, H, W, mcus_per_segment); }
extern "C" size_t lwg_jpeg420_scan_opt_ws_bytes(int B, int H, int W, int mcus_per_segment) { return jpg_opt_ws_bytes<true>(B, H, W, mcus_per_segment); }

extern "C" int lwg_jpeg_hist_u8(const uint8_t* u8, int B, int H, int W, const uint8_t* qtab, int mcus_per_segment, void* ws, uint32_t* hist,
                                lwg_stream_t stream) {
    return jpg_hist<false>(u8, B, H, W, qtab, mcus_per_segment, ws, hist, reinterpret_cast<hipStream_t>(stream));
}
extern "C" int lwg_jpeg420_hist_u8(const uint8_t* u8, int B, int H, int W, const uint8_t* qtab, int mcus_per_segment, void* ws, uint32_t* hist,
                                   lwg_stream_t stream) {
    return jpg_hist<true>(u8, B, H, W, qtab, mcus_per_segment, ws, hist, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int lwg_jpeg_huff_tables(const uint32_t* hist, int B, uint8_t* tables, uint32_t* codes, lwg_stream_t stream) {
    if (!hist || !tables || !codes || B <= 0 || B > 0x1fffffff || ((uintptr_t)hist & 3u) || ((uintptr_t)tables & 3u) || ((uintptr_t)codes & 3u))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lwg_jpeg_huff_kernel, dim3(4u * (unsigned)B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), (const unsigned*)hist, 1, 1,
                       (unsigned char*)tables, (unsigned*)codes);
    return (int)hipGetLastError();
}

extern "C" int lwg_jpeg_scan_opt_u8(const uint8_t* u8, int B, int H, int W, const uint8_t* qtab, int mcus_per_segment, void* ws, uint8_t* scans,
                                    int32_t* nbytes, uint8_t* tables, lwg_stream_t stream) {
    return jpg_scan_opt<false>(u8, B, H, W, qtab, mcus_per_segment, ws, scans, nbytes, tables, reinterpret_cast<hipStream_t>(stream));
}
extern "C" int lwg_jpeg420_scan_opt_u8(const uint8_t* u8, int B, int H, int W, const uint8_t* qtab, int mcus_per_segment, void* ws, uint8_t* scans,
                                       int32_t* nbytes, uint8_t* tables, lwg_stream_t stream) {
    return jpg_scan_opt<true>(u8, B, H, W, qtab, mcus_per_segment, ws, scans, nbytes, tables, reinterpret_cast<hipStream_t>(stream));
}
