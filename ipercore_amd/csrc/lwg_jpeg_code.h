// The integer rules of the device JPEG encoder (jpeg_scan.hip) that need no device builtin: the launch geometry with its argument checks, the
// DCT matrix, the zigzag order, and the four FIXED Annex K Huffman tables as (code | length << 16) words, built at compile time from the
// counts-per-length / symbol lists a DHT segment carries.  tests/jpegdev_emu.py is the definition of the scan and states every constant.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int JPG_NT = 256;                    // threads per workgroup (both launches)
constexpr int JPG_MAX_MCUS = 64;               // MCUs of a segment: one lane of a wave each, one wave per component
constexpr unsigned JPG_BLOCK_BYTES = 208u;     // (11 + 11 + 63 (16 + 10) + 7) / 8: every coefficient with the longest code and amplitude
constexpr unsigned JPG_MCU_BYTES = 3u * JPG_BLOCK_BYTES;
constexpr unsigned JPG_PIX_STRIDE = 196u;      // LDS bytes of an MCU's 8 x 24 pixel bytes: 49 words, an odd word stride across the lanes
constexpr unsigned JPG_COEF_STRIDE = 3u * JPG_MAX_MCUS;

struct JpgGeom {
    int B, H, W, ri;          // ri: MCUs per segment
    int mcux, nmcu, nseg;     // MCU columns, MCUs and segments of a frame
    unsigned slot;            // bytes of a segment's workspace slot: a 16-byte multiple, >= 2 ri 624 + 16
    unsigned meta;            // bytes of the sizes in front of the slots (B nseg uint32, rounded up to 16)
    size_t cap;               // bytes of a frame's scan buffer
};

// false: arguments the encoder does not take.  side: pixels along an MCU's side; mcu_bytes: the bound of an MCU's coded bytes
static inline bool jpg_geom_of(int B, int H, int W, int ri, int side, int most, unsigned mcu_bytes, JpgGeom& g) {
    if (B <= 0 || H <= 0 || W <= 0 || ri <= 0 || ri > most || ri > 65535) return false;
    if (H > 65535 || W > 65535) return false;                                         // SOF0 carries 16-bit sizes
    const long long mcux = ((long long)W + side - 1) / side, mcuy = ((long long)H + side - 1) / side;
    const long long nmcu = mcux * mcuy, nseg = (nmcu + ri - 1) / ri;
    const long long cap = nmcu * 2ll * mcu_bytes + 2ll * (nseg - 1);
    if (cap > 0x7fffffffll || nseg * B > 0x7fffffffll) return false;                  // nbytes is an int32; the grid is B nseg workgroups
    g.B = B, g.H = H, g.W = W, g.ri = ri;
    g.mcux = (int)mcux, g.nmcu = (int)nmcu, g.nseg = (int)nseg;
    g.slot = ((2u * (unsigned)ri * mcu_bytes + 15u) & ~15u) + 16u;
    g.meta = (unsigned)(((size_t)B * (size_t)nseg * 4u + 15u) & ~(size_t)15u);
    g.cap = (size_t)cap;
    return true;
}
static inline bool jpg_geom(int B, int H, int W, int ri, JpgGeom& g) { return jpg_geom_of(B, H, W, ri, 8, JPG_MAX_MCUS, JPG_MCU_BYTES, g); }
// words of launch 1's bit buffer: the unstuffed bytes of a full segment, one word of slack
constexpr unsigned jpg_out_words(int ri) { return (unsigned)ri * (JPG_MCU_BYTES / 4u) + 2u; }

// ---- 4:2:0 (lwg_jpeg420_scan_u8; tests/jpeg420_emu.py): an MCU is 16 x 16 pixels and six blocks - Y00 Y01 Y10 Y11 Cb Cr.  Launch 1 runs one wave
// per block of the MCU, one lane per MCU of the segment; launch 2 is the 4:4:4 one, on a JpgGeom whose slot and cap follow the six-block MCU.
constexpr int JPG420_NT = 384;                 // threads per workgroup of launch 1: six waves
constexpr int JPG420_MAX_MCUS = 64;            // MCUs of a segment: one lane each
constexpr unsigned JPG420_MCU_BYTES = 6u * JPG_BLOCK_BYTES;
constexpr unsigned JPG420_PIX_STRIDE = 772u;   // LDS bytes of an MCU's 16 x 48 pixel bytes: 193 words, an odd word stride across the lanes

static inline bool jpg420_geom(int B, int H, int W, int ri, JpgGeom& g) { return jpg_geom_of(B, H, W, ri, 16, JPG420_MAX_MCUS, JPG420_MCU_BYTES, g); }
constexpr unsigned jpg420_out_words(int ri) { return (unsigned)ri * (JPG420_MCU_BYTES / 4u) + 2u; }
// bytes of launch 1's coefficients: int16 [64 positions][6 ri]: the thread of block k, MCU m at k ri + m
constexpr unsigned jpg420_coef_bytes(int ri) { return 64u * 6u * (unsigned)ri * 2u; }

// ---- per-frame Huffman tables (lwg_jpeg_scan_opt_u8, lwg_jpeg420_scan_opt_u8; tests/jpeghuff_emu.py): a DC code may have 16 bits, so a block is at
// most (16 + 11 + 63 (16 + 10) + 7) / 8 = 209 bytes; slots, capacity and bit buffers follow the next multiple of 4 (their word counts are bytes / 4).
constexpr unsigned JPG_OPT_BLOCK_BYTES = 212u;
constexpr int JPG_HIST_WORDS = 2 * 16 + 2 * 256;   // a histogram, and a frame's code words, in the JpgCodes layout below
constexpr int JPG_DHT_BYTES = 16 + 256;            // a table for the host: codes per length 1 .. 16, then the symbols in code order (unused slots 0)
static_assert(JPG_OPT_BLOCK_BYTES % 4u == 0 && JPG_OPT_BLOCK_BYTES >= 209u, "the block bound is whole words");

static inline bool jpg_geom_opt(int B, int H, int W, int ri, JpgGeom& g) { return jpg_geom_of(B, H, W, ri, 8, JPG_MAX_MCUS, 3u * JPG_OPT_BLOCK_BYTES, g); }
static inline bool jpg420_geom_opt(int B, int H, int W, int ri, JpgGeom& g) {
    return jpg_geom_of(B, H, W, ri, 16, JPG420_MAX_MCUS, 6u * JPG_OPT_BLOCK_BYTES, g);
}
// words of launch 1's bit buffer for nb blocks per MCU of bb bytes each
constexpr unsigned jpg_out_words_of(int ri, unsigned nb, unsigned bb) { return (unsigned)ri * (nb * bb / 4u) + 2u; }
static_assert(jpg_out_words_of(7, 3u, JPG_BLOCK_BYTES) == jpg_out_words(7) && jpg_out_words_of(7, 6u, JPG_BLOCK_BYTES) == jpg420_out_words(7), "one rule");

// M[k][n] = rint(8192 a_k cos((2n + 1) k pi / 16)), a_0 = sqrt(1/8), a_k = sqrt(2/8)
constexpr int JPG_DCT[8][8] = {
    {2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},     {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
    {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
    {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
    {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

// zigzag position -> natural index (vertical frequency x 8 + horizontal frequency)
constexpr unsigned char JPG_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.3 - K.6: codes per length 1 .. 16, then the symbols in code order
constexpr unsigned char JPG_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr unsigned char JPG_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr unsigned char JPG_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// code | length << 16 per symbol: DC by size 0 .. 11 (16 entries), AC by run << 4 | size; table 0 luminance, 1 chrominance
struct JpgCodes {
    unsigned dc[2][16];
    unsigned ac[2][256];
};

constexpr JpgCodes jpg_make_codes() {
    JpgCodes t{};
    for (int tc = 0; tc < 2; ++tc) {
        unsigned code = 0;
        int k = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < JPG_DC_BITS[tc][l - 1]; ++i) t.dc[tc][k++] = code++ | ((unsigned)l << 16);     // the DC symbols are 0 .. 11 in order
            code <<= 1;
        }
        code = 0, k = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < JPG_AC_BITS[tc][l - 1]; ++i) t.ac[tc][JPG_AC_VALS[tc][k++]] = code++ | ((unsigned)l << 16);
            code <<= 1;
        }
    }
    return t;
}
