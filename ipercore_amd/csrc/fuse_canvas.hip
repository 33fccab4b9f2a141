// Output stage: the comparison canvas [source panel | pad | reference | pad | out0 | pad | out1 ...] of fuse_src_ref_multi_outputs
// (tools/utils/multimedia/video.py:451-505), composed on the device straight from the fp32 frames (include/lwg_hip.h 'lwg_fuse_canvas_u8';
// tests/fusecanvas_emu.py is the definition, which these kernels equal byte for byte).  Every layout decision is lwg_fuse_geom.h's.
//
// lwg_fuse_sources_kernel, once per source set: one thread per panel pixel; plain code.
// lwg_fuse_canvas_kernel, per frame batch, HBM-bound: the canvas of a batch is ONE run of B S 3Wc bytes, and 3Wc, 3pad are in general no
//   multiples of 4 - a 32-bit word of it can hold bytes of two regions or of two rows.  A 256-thread workgroup takes R consecutive rows
//   (of any frames) and builds their bytes in LDS at the canvas's own alignment: the fp32 planes come in as 16-byte loads along a row (four
//   pixels of three channels -> 12 bytes), the reference and the panel as aligned 32-bit words of their rows, the pads as constants.  Then
//   the workgroup stores the words that START in its rows, each an aligned 32-bit store, coalesced; the up to 3 bytes such a word takes from
//   the row behind are composed by the same workgroup one byte at a time (lwg_fuse_locate).  Only the batch's last word, when B S 3Wc % 4 != 0,
//   goes out bytewise; nothing outside the canvas is touched, and nothing is read outside the inputs.
// Every loop bound is an argument the host validated.
#include "lwg_common.h"
#include "lwg_fuse_geom.h"
#include "../../include/lwg_hip.h"

namespace {

struct FuseOuts { const float* p[LWG_FUSE_MAX_OUTS]; };

// lwg_frames_to_u8's value (head.hip): uint8((x + 1) / 2.0 * 255), every operation rounded in fp32, the conversion truncates
__device__ __forceinline__ unsigned fuse_out_u8(float x) {
    const float y = __fmul_rn(__fmul_rn(__fadd_rn(x, 1.f), 0.5f), 255.f);
    return (unsigned)(unsigned char)(int)y;
}

// a source pixel as the 8-bit file value it came from (load_images: v / 255 * 2 - 1): rint, ties to even, clamped, NaN -> 0
__device__ __forceinline__ int fuse_src_u8(float x) {
    const float t = rintf(__fmul_rn(__fadd_rn(x, 1.f), 127.5f));
    return (int)fminf(fmaxf(t, 0.f), 255.f);
}

__global__ __launch_bounds__(256) void lwg_fuse_sources_kernel(const float* __restrict__ src, int ns, int S, int Wp, unsigned char* __restrict__ panel) {
    LwgFuseCell cells[LWG_FUSE_MAX_CELLS] = {};
    int ncells;
    lwg_fuse_panel_cells(ns, S, cells, ncells);
    const int total = S * Wp;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int y = i / Wp, x = i - y * Wp;
        int v[3] = {0, 0, 0};
#pragma unroll
        for (int c = 0; c < LWG_FUSE_MAX_CELLS; ++c) {          // (unrolled: the cells stay in registers)
            const LwgFuseCell cell = cells[c];
            if (c >= ncells || y < cell.top || y >= cell.top + cell.size || x < cell.left || x >= cell.left + cell.size || cell.src < 0) continue;
            int sy, sx;
            const int f = S / cell.size, y0 = lwg_fuse_tap0(y - cell.top, f, sy), x0 = lwg_fuse_tap0(x - cell.left, f, sx);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float* p = src + ((size_t)cell.src * 3 + ch) * S * S + (size_t)y0 * S + x0;
                v[ch] = (fuse_src_u8(p[0]) + fuse_src_u8(p[sx]) + fuse_src_u8(p[(size_t)sy * S]) + fuse_src_u8(p[(size_t)sy * S + sx]) + 2) >> 2;
            }
        }
        unsigned char* o = panel + (size_t)i * 3;
        o[0] = (unsigned char)v[0];
        o[1] = (unsigned char)v[1];
        o[2] = (unsigned char)v[2];
    }
}

// the aligned word w of a byte array of `total` bytes (4-byte aligned base); the bytes of a last, partial word one at a time
__device__ __forceinline__ unsigned fuse_load_word(const unsigned char* __restrict__ base, size_t w, size_t total) {
    if (4 * w + 4 <= total) return reinterpret_cast<const unsigned*>(base)[w];
    unsigned v = 0;
    for (int t = 0; t < 4; ++t)
        if (4 * w + t < total) v |= (unsigned)base[4 * w + t] << (8 * t);
    return v;
}

// item idx of the copy of base[sa, sa + n) to dst[0, n): the idx-th aligned word that overlaps the run, its bytes inside the run
__device__ __forceinline__ void fuse_copy_item(const unsigned char* __restrict__ base, size_t sa, int n, size_t total, unsigned char* dst, int idx) {
    const size_t w = (sa >> 2) + idx;
    if (4 * w >= sa + n) return;
    const unsigned v = fuse_load_word(base, w, total);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const size_t o = 4 * w + t;
        if (o >= sa && o < sa + n) dst[o - sa] = (unsigned char)(v >> (8 * t));
    }
}

// one canvas byte by the definition: row gr of the batch (frame gr / S), byte xb of that row
__device__ unsigned fuse_byte(const unsigned char* __restrict__ panel, const unsigned char* __restrict__ ref, const FuseOuts& outs, const LwgFuseGeom& g,
                              int pad_val, size_t gr, int xb) {
    int region, off;
    lwg_fuse_locate(g, xb, region, off);
    const size_t b = gr / g.S;
    const int y = (int)(gr - b * g.S);
    if (region == LWG_FUSE_PANEL) return panel[(size_t)y * 3 * g.Wp + off];
    if (region == LWG_FUSE_PAD) return (unsigned)pad_val;
    if (region == LWG_FUSE_REF) return ref[gr * 3 * g.S + off];
    const int px = off / 3, ch = off - 3 * px;
    const float* p = outs.p[0];
    for (int k = 1; k < LWG_FUSE_MAX_OUTS; ++k)          // (no dynamic index into the by-value pointer array: it would go to scratch)
        if (region - LWG_FUSE_OUT0 == k) p = outs.p[k];
    return fuse_out_u8(p[((size_t)b * 3 + ch) * g.S * g.S + (size_t)y * g.S + px]);
}

// VEC: S % 4 == 0 and every out base 16-byte aligned - four pixels per item, 16-byte loads; otherwise one pixel per item
template <bool VEC>
__global__ __launch_bounds__(256) void lwg_fuse_canvas_kernel(const unsigned char* __restrict__ panel, const unsigned char* __restrict__ ref, FuseOuts outs,
                                                              LwgFuseGeom g, int B, int R, int pad_val, unsigned char* __restrict__ canvas) {
    extern __shared__ unsigned fuse_lds_w[];
    unsigned char* lds = reinterpret_cast<unsigned char*>(fuse_lds_w);
    const int tid = threadIdx.x;
    const size_t rows = (size_t)B * g.S;
    const size_t r0 = (size_t)blockIdx.x * R;
    const int nr = rows - r0 < (size_t)R ? (int)(rows - r0) : R;
    const size_t b0 = r0 * g.row3, b1 = b0 + (size_t)nr * g.row3, N = rows * g.row3;
    // LDS byte i is canvas byte 4 (b0 >> 2) + i: the rows start `lead` bytes in
    const int lead = (int)(b0 & 3);
    unsigned char* rows_lds = lds + lead;

    // ---- the panel: aligned words of its row
    {
        const int n = 3 * g.Wp, per_row = (n + 3) / 4 + 1;
        const size_t total = (size_t)g.S * n;
        for (int it = tid; it < nr * per_row; it += 256) {
            const int lr = it / per_row, idx = it - lr * per_row;
            const int y = (int)((r0 + lr) % g.S);
            fuse_copy_item(panel, (size_t)y * n, n, total, rows_lds + (size_t)lr * g.row3, idx);
        }
    }
    // ---- the reference frame's row (row gr of the (B,S,S,3) tensor)
    if (g.has_ref) {
        const int n = 3 * g.S, per_row = (n + 3) / 4 + 1;
        const size_t total = rows * n;
        for (int it = tid; it < nr * per_row; it += 256) {
            const int lr = it / per_row, idx = it - lr * per_row;
            fuse_copy_item(ref, (r0 + lr) * n, n, total, rows_lds + (size_t)lr * g.row3 + lwg_fuse_slot_image3(g, 0), idx);
        }
    }
    // ---- the pads
    {
        const int n = 3 * g.pad, per_row = (g.has_ref + g.n_out) * n;
        for (int it = tid; it < nr * per_row; it += 256) {
            const int lr = it / per_row, idx = it - lr * per_row, j = idx / n;
            rows_lds[(size_t)lr * g.row3 + 3 * g.Wp + j * g.slot3 + (idx - j * n)] = (unsigned char)pad_val;
        }
    }
    // ---- the outs
    const size_t P = (size_t)g.S * g.S;
    if (VEC) {
        const int S4 = g.S >> 2, per_row = g.n_out * S4;
        for (int it = tid; it < nr * per_row; it += 256) {
            const int lr = it / per_row, idx = it - lr * per_row, k = idx / S4, gi = idx - k * S4;
            const size_t gr = r0 + lr, b = gr / g.S;
            const int y = (int)(gr - b * g.S);
            const float* p = outs.p[0];
            for (int kk = 1; kk < LWG_FUSE_MAX_OUTS; ++kk)
                if (k == kk) p = outs.p[kk];
            p += b * 3 * P + (size_t)y * g.S + 4 * gi;
            const floatx4 c0 = *reinterpret_cast<const floatx4*>(p), c1 = *reinterpret_cast<const floatx4*>(p + P), c2 = *reinterpret_cast<const floatx4*>(p + 2 * P);
            unsigned v[12];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                v[3 * t] = fuse_out_u8(c0[t]);
                v[3 * t + 1] = fuse_out_u8(c1[t]);
                v[3 * t + 2] = fuse_out_u8(c2[t]);
            }
            const int d = lead + lr * g.row3 + lwg_fuse_slot_image3(g, g.has_ref + k) + 12 * gi;          // (a workgroup's LDS is below 64 KB)
            if ((d & 3) == 0) {
#pragma unroll
                for (int t = 0; t < 3; ++t)
                    fuse_lds_w[(d >> 2) + t] = v[4 * t] | v[4 * t + 1] << 8 | v[4 * t + 2] << 16 | v[4 * t + 3] << 24;
            } else {
#pragma unroll
                for (int t = 0; t < 12; ++t) lds[d + t] = (unsigned char)v[t];
            }
        }
    } else {
        const int per_row = g.n_out * g.S;
        for (int it = tid; it < nr * per_row; it += 256) {
            const int lr = it / per_row, idx = it - lr * per_row, k = idx / g.S, x = idx - k * g.S;
            const size_t gr = r0 + lr, b = gr / g.S;
            const int y = (int)(gr - b * g.S);
            const float* p = outs.p[0];
            for (int kk = 1; kk < LWG_FUSE_MAX_OUTS; ++kk)
                if (k == kk) p = outs.p[kk];
            p += b * 3 * P + (size_t)y * g.S + x;
            unsigned char* d = rows_lds + (size_t)lr * g.row3 + lwg_fuse_slot_image3(g, g.has_ref + k) + 3 * x;
            d[0] = (unsigned char)fuse_out_u8(p[0]);
            d[1] = (unsigned char)fuse_out_u8(p[P]);
            d[2] = (unsigned char)fuse_out_u8(p[2 * P]);
        }
    }
    // ---- the bytes of the row behind that complete this workgroup's last word
    {
        const int nhead = (int)((4 - (b1 & 3)) & 3);
        if (tid < nhead && b1 + tid < N) {
            const size_t o = b1 + tid, gr = o / g.row3;
            rows_lds[(size_t)nr * g.row3 + tid] = (unsigned char)fuse_byte(panel, ref, outs, g, pad_val, gr, (int)(o - gr * g.row3));
        }
    }
    __syncthreads();
    // ---- the words that start in [b0, b1): aligned 32-bit stores; the batch's last, partial word bytewise
    const size_t w0 = (b0 + 3) >> 2, w1 = (b1 + 3) >> 2, wl = b0 >> 2;
    for (size_t w = w0 + tid; w < w1; w += 256) {
        const unsigned v = fuse_lds_w[w - wl];
        if (4 * w + 4 <= N) {
            reinterpret_cast<unsigned*>(canvas)[w] = v;
        } else {
            for (int t = 0; t < 4; ++t)
                if (4 * w + t < N) canvas[4 * w + t] = (unsigned char)(v >> (8 * t));
        }
    }
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// rows per workgroup and the LDS bytes they take (3 bytes of lead, 3 of the row behind, rounded up to a word); 0: a row does not fit
int fuse_rows_per_block(int row3, size_t& lds_bytes) {
    int R = 12288 / row3;
    R = R < 1 ? 1 : (R > 16 ? 16 : R);
    lds_bytes = ((size_t)R * row3 + 8 + 3) & ~(size_t)3;
    return lds_bytes <= 65536 ? R : 0;
}

}  // namespace

extern "C" int lwg_fuse_panel_width(int ns, int S) {
    LwgFuseCell cells[LWG_FUSE_MAX_CELLS];
    int ncells;
    const int Wp = lwg_fuse_panel_cells(ns, S, cells, ncells);
    LwgFuseGeom g;
    return Wp > 0 && lwg_fuse_geom_of(S, Wp, 0, 0, 1, g) ? Wp : 0;
}

extern "C" int lwg_fuse_canvas_width(int ns, int S, int pad, int has_ref, int n_out) {
    const int Wp = lwg_fuse_panel_width(ns, S);
    LwgFuseGeom g;
    size_t lds_bytes;
    if (Wp <= 0 || !lwg_fuse_geom_of(S, Wp, pad, has_ref, n_out, g) || !fuse_rows_per_block(g.row3, lds_bytes)) return 0;
    return g.Wc;
}

extern "C" int lwg_fuse_sources_u8(const float* src, int ns, int S, uint8_t* panel, lwg_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int Wp = lwg_fuse_panel_width(ns, S);
    if (!src || !panel || Wp <= 0 || !aligned_to(src, 4) || !aligned_to(panel, 4)) return (int)hipErrorInvalidValue;
    const int total = S * Wp;
    const int blocks = (total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192;
    hipLaunchKernelGGL(lwg_fuse_sources_kernel, dim3(blocks), dim3(256), 0, stream, src, ns, S, Wp, panel);
    return (int)hipGetLastError();
}

extern "C" int lwg_fuse_canvas_u8(const uint8_t* panel, int Wp, const uint8_t* ref, const float* const* outs, int n_out, int B, int S, int pad,
                                  int pad_val, uint8_t* canvas, lwg_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    LwgFuseGeom g;
    size_t lds_bytes;
    if (!panel || !outs || !canvas || B <= 0 || pad_val < 0 || pad_val > 255 || !lwg_fuse_geom_of(S, Wp, pad, ref != nullptr, n_out, g)) return (int)hipErrorInvalidValue;
    if (!aligned_to(panel, 4) || !aligned_to(ref, 4) || !aligned_to(canvas, 4)) return (int)hipErrorInvalidValue;
    const int R = fuse_rows_per_block(g.row3, lds_bytes);
    if (!R) return (int)hipErrorInvalidValue;
    FuseOuts o = {};
    bool vec = (S & 3) == 0;
    for (int k = 0; k < n_out; ++k) {
        if (!outs[k] || !aligned_to(outs[k], 4)) return (int)hipErrorInvalidValue;
        o.p[k] = outs[k];
        vec = vec && aligned_to(outs[k], 16);
    }
    const size_t rows = (size_t)B * S, blocks = (rows + R - 1) / R;
    if (blocks >= (1ull << 31)) return (int)hipErrorInvalidValue;
    if (vec) hipLaunchKernelGGL(lwg_fuse_canvas_kernel<true>, dim3((unsigned)blocks), dim3(256), lds_bytes, stream, panel, ref, o, g, B, R, pad_val, canvas);
    else hipLaunchKernelGGL(lwg_fuse_canvas_kernel<false>, dim3((unsigned)blocks), dim3(256), lds_bytes, stream, panel, ref, o, g, B, R, pad_val, canvas);
    return (int)hipGetLastError();
}
