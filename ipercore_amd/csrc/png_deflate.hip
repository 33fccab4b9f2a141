// Output stage: the zlib stream of a PNG's IDAT chunk, written on the device (include/lwg_hip.h 'lwg_png_deflate_u8' gives the format;
// tests/pngdev_emu.py is its definition, which these kernels equal byte for byte).  Integers only - no fp32 arithmetic, so the pixels a
// decoder gets back are lwg_frames_to_u8's.
//
// Launch 1, one 256-thread workgroup per segment (rows_per_segment scanlines of one frame, n = rows (1 + 3W) <= 65 535 raw bytes):
//   Paeth residuals -> LDS (n bytes) + per-wave histograms + the segment's Adler partial sums; the literal code (rank sorts on all threads,
//   the two-queue Huffman merge and the length limit on thread 0: <= 256 merges); sum hist x len decides dynamic / stored before a bit is
//   written; every thread encodes a fixed run of ceil(n / 256) bytes at the bit offset a block scan gives it, ORing words into zeroed LDS
//   (<= n + 5 bytes); the words go out coalesced to the segment's slot of the workspace.
// Launch 2, one workgroup per segment: prefix sum of the frame's segment sizes, the slot's bytes packed behind the zlib header, and - the
//   last segment's workgroup - the final block, the Adler-32 combined from the partial sums, nbytes[b].
// Every loop bound is an argument the host validated.
#include "lwg_common.h"
#include "lwg_png_code.h"
#include "../../include/lwg_hip.h"

namespace {

// tables of launch 1 behind the two byte arrays of the dynamic LDS block
struct PngTables {
    unsigned whist[4][256];
    unsigned hist[260];
    unsigned codelen[260];       // bit-reversed code | length << 16
    unsigned weight[516];        // nodes: the m leaves ascending by (count, symbol), then the internal nodes in creation order
    unsigned short parent[516];
    unsigned short depth[516];
    unsigned short rank2[260];   // position of a symbol in the (count descending, symbol ascending) order
    unsigned char lens[260];
    unsigned cum[16];            // cum[l] = codes of length <= l
    unsigned nxt[16];            // first canonical code of length l
    unsigned scan[4];
    unsigned payload;            // sum hist[s] len[s] (end of block included)
    unsigned m;                  // used symbols
    unsigned long long red[2][4];
};

// value (nbits <= 16, LSB first) ORed into the word array at bit position pos
__device__ __forceinline__ void png_put(unsigned* out, unsigned pos, unsigned value, unsigned nbits) {
    if (nbits == 0) return;
    const unsigned long long v = (unsigned long long)value << (pos & 31u);
    atomicOr(&out[pos >> 5], (unsigned)v);
    if ((unsigned)(v >> 32)) atomicOr(&out[(pos >> 5) + 1], (unsigned)(v >> 32));
}

__global__ void __launch_bounds__(PNG_NT) lwg_png_segment_kernel(const unsigned char* __restrict__ u8, PngGeom g, unsigned lds_raw, PngMeta* __restrict__ meta,
                                                                 unsigned char* __restrict__ slots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char png_lds[];
    unsigned char* raw = png_lds;                                                   // [lds_raw]
    PngTables& t = *reinterpret_cast<PngTables*>(png_lds + lds_raw);
    unsigned* out = reinterpret_cast<unsigned*>(png_lds + lds_raw + sizeof(PngTables));       // [(nfull + 5) / 4 + 3] words
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int sid = blockIdx.x, b = sid / g.nseg, seg = sid - b * g.nseg;
    const int r0 = seg * g.rows, nr = min(g.rows, g.H - r0);
    const unsigned n = (unsigned)nr * g.rowlen;
    const unsigned out_words = png_out_words(g);
    const unsigned char* img = u8 + (size_t)b * g.H * (g.rowlen - 1u);

    for (unsigned i = tid; i < out_words; i += PNG_NT) out[i] = 0u;
    for (int i = tid; i < 4 * 256; i += PNG_NT) (&t.whist[0][0])[i] = 0u;
    if (tid == 0) t.payload = 0u;
    __syncthreads();

    // ---- residuals, histograms, Adler partial sums: s1 = sum v, s2 = sum (n - i) v over the segment's bytes
    unsigned long long s1 = 0, s2 = 0;
    for (unsigned i = tid; i < n; i += PNG_NT) {
        const unsigned v = png_raw_byte(img, g.rowlen, r0, i);
        raw[i] = (unsigned char)v;
        atomicAdd(&t.whist[wave][v], 1u);
        s1 += v;
        s2 += (unsigned long long)(n - i) * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    if (lane == 0) t.red[0][wave] = s1, t.red[1][wave] = s2;
    __syncthreads();
    for (int s = tid; s < 257; s += PNG_NT) t.hist[s] = s < 256 ? t.whist[0][s] + t.whist[1][s] + t.whist[2][s] + t.whist[3][s] : 1u;
    __syncthreads();

    // ---- the two orders: leaves ascending by (count, symbol) for the merge, (count descending, symbol ascending) for handing out lengths
    for (int s = tid; s < 257; s += PNG_NT) {
        const unsigned c = t.hist[s];
        unsigned r1 = 0, r2 = 0, used = 0;
        for (int q = 0; q < 257; ++q) {
            const unsigned cq = t.hist[q];
            used += cq != 0u;
            r1 += png_before_asc(cq, q, c, s);
            r2 += png_before_desc(cq, q, c, s);
        }
        if (c) {
            t.weight[r1] = c;
            t.rank2[s] = (unsigned short)r2;
        }
        if (s == 0) t.m = used;
    }
    __syncthreads();

    // ---- Huffman by two queues + miniz's length limit (serial: m - 1 <= 256 merges)
    if (tid == 0) png_code_build(t.weight, t.parent, t.depth, t.m, t.cum, t.nxt);
    __syncthreads();

    for (int s = tid; s < 257; s += PNG_NT) {
        t.lens[s] = (unsigned char)(t.hist[s] ? png_len_of_rank(t.cum, t.rank2[s]) : 0u);
    }
    __syncthreads();
    for (int s = tid; s < 257; s += PNG_NT) {
        const unsigned l = t.lens[s];
        unsigned cl = 0;
        if (l) {
            unsigned idx = 0;
            for (int q = 0; q < s; ++q) idx += t.lens[q] == l;
            cl = png_rev(t.nxt[l] + idx, l) | (l << 16);
            atomicAdd(&t.payload, t.hist[s] * l);
        }
        t.codelen[s] = cl;
    }
    __syncthreads();

    const unsigned payload = t.payload;
    const unsigned dyn = png_dyn_bytes(payload);
    const bool stored = dyn > n + 5u;
    const unsigned size = stored ? n + 5u : dyn;
    unsigned* dst = reinterpret_cast<unsigned*>(slots + (size_t)sid * g.slot);

    if (stored) {
        for (unsigned w = tid; w < (size + 3u) / 4u; w += PNG_NT) {
            unsigned word = 0;
#pragma unroll
            for (unsigned h = 0; h < 4u; ++h) word |= png_stored_byte(raw, n, 4u * w + h) << (8u * h);
            dst[w] = word;
        }
    } else {
        // block header: BFINAL 0, BTYPE 2, HLIT 0, HDIST 0, HCLEN 15; the 19 code-length code lengths (order 16 17 18 0 8 ...): 0 0 0 then 4 x 16
        if (tid == 0) {
            png_put(out, 0u, 2u << 1, 3u);
            png_put(out, 13u, 15u, 4u);
            for (unsigned k = 3; k < 19u; ++k) png_put(out, 17u + 3u * k, 4u, 3u);
            png_put(out, 74u + 4u * 257u, 0u, 4u);                                          // the one distance code: length 0
            const unsigned cl = t.codelen[256];
            png_put(out, PNG_HEADER_BITS + payload - (cl >> 16), cl & 0xffffu, cl >> 16);   // end of block
            png_put(out, 8u * (dyn - 2u), 0xffffu, 16u);                                    // 000 + padding, then 00 00 FF FF
        }
        for (int s = tid; s < 257; s += PNG_NT) png_put(out, 74u + 4u * (unsigned)s, png_rev(t.lens[s], 4u), 4u);
        // literals: thread tid owns the bytes [tid run, (tid + 1) run)
        const unsigned run = (n + PNG_NT - 1u) / PNG_NT;
        const unsigned i0 = min(n, (unsigned)tid * run), i1 = min(n, i0 + run);
        unsigned bits = 0;
        for (unsigned i = i0; i < i1; ++i) bits += t.lens[raw[i]];
        unsigned inc = bits;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(inc, o, 64);
            if (lane >= o) inc += v;
        }
        if (lane == 63) t.scan[wave] = inc;
        __syncthreads();
        unsigned pos = PNG_HEADER_BITS + inc - bits;
        for (int w = 0; w < wave; ++w) pos += t.scan[w];
        unsigned wi = pos >> 5, nb = pos & 31u;
        unsigned long long acc = 0;
        for (unsigned i = i0; i < i1; ++i) {
            const unsigned cl = t.codelen[raw[i]];
            acc |= (unsigned long long)(cl & 0xffffu) << nb;
            nb += cl >> 16;
            if (nb >= 32u) {
                atomicOr(&out[wi], (unsigned)acc);
                ++wi;
                acc >>= 32;
                nb -= 32u;
            }
        }
        if (nb && (unsigned)acc) atomicOr(&out[wi], (unsigned)acc);
        __syncthreads();
        for (unsigned w = tid; w < (size + 3u) / 4u; w += PNG_NT) dst[w] = out[w];
    }
    if (tid == 0) {
        const unsigned long long a1 = t.red[0][0] + t.red[0][1] + t.red[0][2] + t.red[0][3];
        const unsigned long long a2 = t.red[1][0] + t.red[1][1] + t.red[1][2] + t.red[1][3];
        PngMeta mt;
        mt.size = size;
        mt.s1 = (unsigned)(a1 % PNG_ADLER);
        mt.s2 = (unsigned)(a2 % PNG_ADLER);
        mt.n = n;
        meta[sid] = mt;
    }
}

// Launch 2: segment (b, seg) of the workspace -> streams[b] at 2 + the sizes before it; header, final block, Adler-32, nbytes.
__global__ void __launch_bounds__(PNG_NT) lwg_png_pack_kernel(PngGeom g, const PngMeta* __restrict__ meta, const unsigned char* __restrict__ slots,
                                                              unsigned char* __restrict__ streams, int* __restrict__ nbytes) {
    __shared__ unsigned part[PNG_NT / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int sid = blockIdx.x, b = sid / g.nseg, seg = sid - b * g.nseg;
    const PngMeta* fm = meta + (size_t)b * g.nseg;
    unsigned before = 0;
    for (int k = tid; k < seg; k += PNG_NT) before += fm[k].size;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    if (lane == 0) part[wave] = before;
    __syncthreads();
    const size_t off = 2u + (size_t)part[0] + part[1] + part[2] + part[3];
    const unsigned size = fm[seg].size;
    unsigned char* frame = streams + (size_t)b * g.cap;
    unsigned char* dst = frame + off;
    const unsigned char* src = slots + (size_t)sid * g.slot;
    const unsigned* src32 = reinterpret_cast<const unsigned*>(src);
    // destination words whole, the bytes in front of the first and behind the last one by one; a source word pair is funnelled into each
    const unsigned head = min(size, (unsigned)((4u - ((uintptr_t)dst & 3u)) & 3u));
    const unsigned nwords = (size - head) / 4u, tail0 = head + 4u * nwords;
    if ((unsigned)tid < head) dst[tid] = src[tid];
    if ((unsigned)tid < size - tail0) dst[tail0 + tid] = src[tail0 + tid];
    unsigned* dst32 = reinterpret_cast<unsigned*>(dst + head);
    const unsigned sh = 8u * (head & 3u), q0 = head >> 2;
    for (unsigned k = tid; k < nwords; k += PNG_NT) {
        const unsigned lo = src32[q0 + k];
        unsigned v = lo;
        if (sh) v = (lo >> sh) | (src32[q0 + k + 1u] << (32u - sh));        // (within the slot: it ends >= 16 bytes behind the segment)
        dst32[k] = v;
    }
    if (tid == 0 && seg == 0) frame[0] = 0x78, frame[1] = 0x01;
    if (tid == 0 && seg == g.nseg - 1) {
        unsigned A = 1u, Bs = 0u;
        for (int k = 0; k < g.nseg; ++k) {
            const PngMeta mt = fm[k];
            png_adler_step(A, Bs, mt.n, mt.s1, mt.s2);
        }
        unsigned char* e = dst + size;
        e[0] = 0x01, e[1] = 0x00, e[2] = 0x00, e[3] = 0xff, e[4] = 0xff;
        e[5] = (unsigned char)(Bs >> 8), e[6] = (unsigned char)Bs, e[7] = (unsigned char)(A >> 8), e[8] = (unsigned char)A;
        nbytes[b] = (int)(off + size + 9u);
    }
}

}  // namespace

extern "C" size_t lwg_png_stream_capacity(int H, int W, int rows_per_segment) {
    PngGeom g;
    return png_geom(1, H, W, rows_per_segment, g) ? g.cap : 0;
}

extern "C" size_t lwg_png_deflate_ws_bytes(int B, int H, int W, int rows_per_segment) {
    PngGeom g;
    if (!png_geom(B, H, W, rows_per_segment, g)) return 0;
    return (size_t)B * g.nseg * (sizeof(PngMeta) + g.slot);
}

extern "C" int lwg_png_deflate_u8(const uint8_t* u8, int B, int H, int W, int rows_per_segment, void* ws, uint8_t* streams, int32_t* nbytes,
                                  lwg_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    PngGeom g;
    if (!u8 || !ws || !streams || !nbytes || ((uintptr_t)ws & 15u) || !png_geom(B, H, W, rows_per_segment, g)) return (int)hipErrorInvalidValue;
    const size_t nslots = (size_t)B * g.nseg;
    PngMeta* meta = reinterpret_cast<PngMeta*>(ws);
    unsigned char* slots = reinterpret_cast<unsigned char*>(ws) + nslots * sizeof(PngMeta);
    const unsigned lds_raw = png_lds_raw(g);
    const size_t lds = (size_t)lds_raw + sizeof(PngTables) + 4u * (size_t)png_out_words(g);
    if (lds > 65536) {
        static unsigned long long lds_ok = 0;
        const hipError_t e = lwg_allow_dynamic_lds(reinterpret_cast<const void*>(lwg_png_segment_kernel), 160 * 1024, lds_ok);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(lwg_png_segment_kernel, dim3((unsigned)nslots), dim3(PNG_NT), lds, stream, (const unsigned char*)u8, g, lds_raw, meta, slots);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lwg_png_pack_kernel, dim3((unsigned)nslots), dim3(PNG_NT), 0, stream, g, (const PngMeta*)meta, (const unsigned char*)slots, streams,
                       nbytes);
    return (int)hipGetLastError();
}
