// The integer rules of the device PNG encoder (png_deflate.hip) that a host program can run as they are: the launch geometry and its argument
// checks, the Paeth predictor, the two sort orders of the symbols, the Huffman merge with miniz's length limit, the length a rank receives,
// the bytes of a stored block, the sizes, and the Adler-32 combination of per-segment partial sums.  The kernels call these functions;
// tests/test_png_device_cpu.py compiles the same text for the host and holds it to tests/pngdev_emu.py, the definition of the stream.
// No device builtins.
#pragma once
#ifdef __HIPCC__
#include "lwg_common.h"
#define PNG_FN __host__ __device__ __forceinline__
#else
#include <stddef.h>
#include <stdint.h>
#define PNG_FN static inline
#endif

constexpr int PNG_NT = 256;                    // threads per workgroup (both launches)
constexpr unsigned PNG_MAX_SEG = 65535u;       // raw bytes of a segment: LEN of a stored block
constexpr unsigned PNG_HEADER_BITS = 1106u;    // 17 + 19 x 3 + 258 x 4
constexpr unsigned PNG_ADLER = 65521u;
constexpr int PNG_MAXLEN = 15;
constexpr int PNG_NSYM = 257;                  // literals + end of block

struct PngGeom {
    int B, H, W, rows, nseg;  // rows: min(rows_per_segment, H)
    unsigned rowlen;          // 1 + 3W
    unsigned nfull;           // raw bytes of a full segment
    unsigned slot;            // bytes of a segment's workspace slot: a 16-byte multiple, >= nfull + 5 + 16
    size_t cap;               // bytes of a frame's stream buffer
};

// ws: [B nseg] of these, then [B nseg] slots
struct PngMeta { unsigned size, s1, s2, n; };

// false: arguments the encoder does not take
static inline bool png_geom(int B, int H, int W, int rows, PngGeom& g) {
    if (B <= 0 || H <= 0 || W <= 0 || rows <= 0) return false;
    const long long rowlen = 1ll + 3ll * W;
    const long long rr = rows < H ? rows : H;
    if (rowlen * rr > (long long)PNG_MAX_SEG) return false;              // a stored block's LEN
    const long long nseg = ((long long)H + rr - 1) / rr;
    const long long cap = rowlen * H + 5 * nseg + 11;
    if (cap > 0x7fffffffll || nseg * B > 0x7fffffffll) return false;     // nbytes is an int32; the grid is B nseg workgroups
    g.B = B, g.H = H, g.W = W, g.rows = (int)rr, g.nseg = (int)nseg;
    g.rowlen = (unsigned)rowlen;
    g.nfull = (unsigned)(rowlen * rr);
    g.slot = ((g.nfull + 5u + 15u) & ~15u) + 16u;
    g.cap = (size_t)cap;
    return true;
}
// LDS of launch 1: raw bytes | tables | output words
PNG_FN unsigned png_lds_raw(const PngGeom& g) { return (g.nfull + 15u) & ~15u; }
PNG_FN unsigned png_out_words(const PngGeom& g) { return (g.nfull + 5u) / 4u + 3u; }

PNG_FN unsigned png_paeth(unsigned a, unsigned b, unsigned c) {
    const int p = (int)a + (int)b - (int)c;
    const int da = p - (int)a, db = p - (int)b, dc = p - (int)c;
    const int pa = da < 0 ? -da : da, pb = db < 0 ? -db : db, pc = dc < 0 ? -dc : dc;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// raw byte i of the segment that starts at image row r0: the filter byte, or the Paeth residual against the IMAGE's neighbours
PNG_FN unsigned png_raw_byte(const unsigned char* img, unsigned rowlen, int r0, unsigned i) {
    const unsigned r = i / rowlen, j = i - r * rowlen;
    if (j == 0u) return 4u;
    const unsigned stride = rowlen - 1u, jj = j - 1u;
    const int y = r0 + (int)r;
    const unsigned char* row = img + (size_t)y * stride;
    const unsigned a = jj >= 3u ? row[jj - 3u] : 0u;
    const unsigned up = y > 0 ? (row - stride)[jj] : 0u;
    const unsigned ul = (y > 0 && jj >= 3u) ? (row - stride)[jj - 3u] : 0u;
    return ((unsigned)row[jj] - png_paeth(a, up, ul)) & 255u;
}

// does the used symbol (cq, q) stand before (c, s): ascending by (count, symbol) - the leaves of the merge; and by (count descending,
// symbol ascending) - the order in which lengths are handed out.  Unused symbols (count 0) stand nowhere.
PNG_FN bool png_before_asc(unsigned cq, int q, unsigned c, int s) { return cq != 0u && (cq < c || (cq == c && q < s)); }
PNG_FN bool png_before_desc(unsigned cq, int q, unsigned c, int s) { return cq != 0u && (cq > c || (cq == c && q < s)); }

// Huffman by two queues over the m >= 2 leaf weights weight[0 .. m) (ascending), then miniz's limit to 15 bits.  weight / parent / depth
// hold 2m - 1 nodes.  -> cum[l] = codes of length <= l, nxt[l] = first canonical code of length l (l = 0 .. 15).
template <typename W, typename P>
PNG_FN void png_code_build(W* weight, P* parent, P* depth, unsigned m, unsigned* cum, unsigned* nxt) {
    unsigned li = 0, ii = m, nn = m;
    for (unsigned k = 0; k + 1 < m; ++k) {
        unsigned pick[2];
        for (int h = 0; h < 2; ++h) {
            if (li < m && (ii >= nn || weight[li] <= weight[ii])) pick[h] = li++;      // on equal weight the leaf first
            else pick[h] = ii++;
        }
        weight[nn] = weight[pick[0]] + weight[pick[1]];
        parent[pick[0]] = (P)nn;
        parent[pick[1]] = (P)nn;
        ++nn;
    }
    unsigned num[PNG_MAXLEN + 1];
    for (int l = 0; l <= PNG_MAXLEN; ++l) num[l] = 0u;
    depth[2 * m - 2] = 0;
    for (int node = (int)(2 * m) - 3; node >= 0; --node) {
        const unsigned d = (unsigned)depth[parent[node]] + 1u;
        depth[node] = (P)d;
        if ((unsigned)node < m) num[d < (unsigned)PNG_MAXLEN ? d : (unsigned)PNG_MAXLEN] += 1u;
    }
    unsigned total = 0;
    for (int l = 1; l <= PNG_MAXLEN; ++l) total += num[l] << (PNG_MAXLEN - l);
    while (total > (1u << PNG_MAXLEN)) {
        num[PNG_MAXLEN] -= 1u;
        for (int i = PNG_MAXLEN - 1; i >= 1; --i)
            if (num[i]) {
                num[i] -= 1u;
                num[i + 1] += 2u;
                break;
            }
        total -= 1u;
    }
    unsigned c = 0, code = 0;
    cum[0] = 0u;
    nxt[0] = 0u;
    for (int l = 1; l <= PNG_MAXLEN; ++l) {
        code = (code + (l > 1 ? num[l - 1] : 0u)) << 1;
        nxt[l] = code;
        c += num[l];
        cum[l] = c;
    }
}

// the length of the symbol at position k of the (count descending, symbol ascending) order
PNG_FN unsigned png_len_of_rank(const unsigned* cum, unsigned k) {
    unsigned l = 1;
    while (l < (unsigned)PNG_MAXLEN && cum[l] <= k) ++l;
    return l;
}

// a code as it is ORed into the LSB-first bit stream: most significant bit first
PNG_FN unsigned png_rev(unsigned code, unsigned len) {
    unsigned r = 0;
    for (unsigned k = 0; k < len; ++k) r |= ((code >> k) & 1u) << (len - 1u - k);
    return r;
}

// bytes of the dynamic form (the empty stored block behind it included) for payload = sum hist[s] len[s] bits; the segment is stored
// if and only if that exceeds n + 5
PNG_FN unsigned png_dyn_bytes(unsigned payload) { return (PNG_HEADER_BITS + payload + 3u + 7u) / 8u + 4u; }

// byte k of a stored segment of n raw bytes (k < n + 5; zeros behind it)
PNG_FN unsigned png_stored_byte(const unsigned char* raw, unsigned n, unsigned k) {
    if (k >= 5u) return k - 5u < n ? raw[k - 5u] : 0u;
    return k == 0u ? 0u : k == 1u ? (n & 255u) : k == 2u ? (n >> 8) : k == 3u ? (~n & 255u) : ((~n >> 8) & 255u);
}

// Adler-32 (A, Bs) after a segment of n bytes with s1 = sum v mod 65521, s2 = sum (n - i) v mod 65521 (i = 0 .. n - 1)
PNG_FN void png_adler_step(unsigned& A, unsigned& Bs, unsigned n, unsigned s1, unsigned s2) {
    Bs = (unsigned)((Bs + (unsigned long long)(n % PNG_ADLER) * A + s2) % PNG_ADLER);
    A = (A + s1) % PNG_ADLER;
}
