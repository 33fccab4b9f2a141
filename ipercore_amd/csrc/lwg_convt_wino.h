// What the two fused Winograd forms of nn.ConvTranspose2d(4, 2, 1) share - convt_winograd.hip (F(2x2, 2x2)) and convt_winograd24.hip (F(2x4, 2x2)):
// the block footprint (16 x 16 input pixels -> 32 x 32 output pixels x 32 output channels, 512 threads), the persistent-workgroup walk and its
// XCD-aware block order, the 18 x 18 x 8 halo staging, the store phase and the host entry point's contract and launch.  Each kernel keeps its K
// loop, its V-plane layout, its output transform and its exchange-buffer slot map.
//   Part 1 is plain integer arithmetic that a host compiler can include: tests/test_conv_offsets_cpu.py compiles these very functions with
// signed-overflow traps and drives them over the corner shapes of the contract.  Part 2 (hipcc only) is the device code around them.
#pragma once
#include <stddef.h>
#include "lwg_conv_args.h"

#ifdef __HIPCC__
#define CTW_FN __host__ __device__ __forceinline__
#else
#define CTW_FN static inline
#endif
#define WG_THREADS 512
#define CTW_EDGE 16                          // input pixels per block edge (F(2x2, 2x2): 8 x 8 patches, F(2x4, 2x2): 8 x 4 patches)
#define NBT 32                               // output channels per block
#define KS 8                                 // input channels per stage
#define HALO 18
#define PLANE (HALO * HALO)
#define RAW_FLOATS (KS * PLANE)              // [c][py][px]
#define OROW 36                              // floats per pixel row of the epilogue's exchange buffer [32 x 32 output pixels][32 channels + 4]
#define OUT_FLOATS (32 * 32 * OROW)
#define DUMP_OFF (2 * RAW_FLOATS + 2 * VS_FLOATS)    // behind the K loop's buffers (VS_FLOATS: the kernel's V planes): where the threads without a halo element store their zeros (dead LDS)
#define LOOP_FLOATS (DUMP_OFF + WG_THREADS + 3 * PLANE + RAW_FLOATS)
#define BIAS_OFF (LOOP_FLOATS > OUT_FLOATS ? LOOP_FLOATS : OUT_FLOATS)    // the block's 32 bias values, behind both uses of the LDS
#define WINO_OOB 0xC0000000u                 // >= any image's byte size (host: H * W * C * 4 < 3 GiB): the buffer load returns 0, the store is dropped

// ---- part 1: integer arithmetic, host-compilable ----
// ---- the block grid of a launch: bx x by blocks per image, tiles = blocks of all images, total = tiles x column blocks
struct CtwGrid { int bx, by, tiles, total; };

CTW_FN CtwGrid ctw_grid(int B, int H, int W, int N) {
    const int bx = (W + CTW_EDGE - 1) / CTW_EDGE, by = (H + CTW_EDGE - 1) / CTW_EDGE, tiles = bx * by * B;
    return CtwGrid{bx, by, tiles, tiles * (N / NBT)};
}
CTW_FN long ctw_total_blocks(int B, int H, int W, int N) {      // (the host's count: 64 bits, before the grid is cut to the CUs)
    return (long)((W + CTW_EDGE - 1) / CTW_EDGE) * ((H + CTW_EDGE - 1) / CTW_EDGE) * B * (N / NBT);
}

// ---- the block order.  Persistent workgroups (round 6, as conv_winograd.hip): min(blocks, CUs) workgroups walk the block ids wg + k nwg
// (id = column block * tiles + tile); the next block's first halo stages and weights are requested inside this block's epilogue.  Bitwise the
// one-block-per-workgroup results.
//   XCD-aware order (as conv_winograd4.hip; persistent grids of a multiple of 8 workgroups, N / 32 = 2, 4 or 8 column blocks): workgroup w runs on
// XCD w % 8 and keeps ONE column block, (w % 8) % ncb, for the whole launch (an XCD's L2 holds that column block's panel only), while the ncb
// workgroups (w % 8) / ncb, w / 8 of adjacent XCDs walk the same tile sequence in step: a tile's halo comes from HBM once instead of ncb times
struct CtwOrder {
    int nwg, wg;          // workgroups of the launch, this one
    int ncb, tiles, total;
    bool xcd;             // the XCD-aware order applies
    int xg;               // workgroups per column block = tiles per round
    int xr;               // this workgroup's place among them
};

CTW_FN bool ctw_xcd_applies(unsigned nwg, int ncb, int tiles, int total) {
    return (nwg & 7u) == 0 && (ncb == 2 || ncb == 4 || ncb == 8) && (int)nwg < total && tiles >= (int)nwg / ncb;
}
CTW_FN CtwOrder ctw_order(bool xcd_enabled, unsigned nwg, unsigned wg, int N, const CtwGrid& g) {
    const int ncb = N / NBT;
    return CtwOrder{(int)nwg, (int)wg, ncb, g.tiles, g.total, xcd_enabled && ctw_xcd_applies(nwg, ncb, g.tiles, g.total),
                    (int)nwg / ncb, (int)(((wg & 7u) / (unsigned)ncb) * (nwg >> 3) + (wg >> 3))};
}
CTW_FN bool ctw_has_block(const CtwOrder& o, int id) {         // (id = wg + k nwg)
    const int tiles = o.tiles, total = o.total;                // (read up front: one load through a selected field address keeps the whole state in scratch)
    return o.xcd ? (id / o.nwg) * o.xg + o.xr < tiles : id < total;
}
CTW_FN int ctw_col_block(const CtwOrder& o, int id) {
    return o.xcd ? (int)((unsigned)o.wg & 7u) & (o.ncb - 1) : id / o.tiles;
}
CTW_FN int ctw_tile(const CtwOrder& o, int id, int cb) {
    return o.xcd ? (id / o.nwg) * o.xg + o.xr : id - cb * o.tiles;
}
CTW_FN int ctw_image(const CtwGrid& g, int t) { return t / (g.bx * g.by); }

// the block's input corner (x0, y0) and first output column n0 from its tile inside image b (t - b bx by) and its column block
CTW_FN void ctw_corner(const CtwGrid& g, int t_in_image, int cb, int& x0, int& y0, int& n0) {
    x0 = (t_in_image % g.bx) * CTW_EDGE;
    y0 = (t_in_image / g.bx) * CTW_EDGE;
    n0 = cb * NBT;
}

// ---- the halo: element i (< 2 PLANE: pixel i / 2 of the 18 x 18 halo, channel quad i % 2 of the stage's eight; a thread holds i = tid and
// tid + 512) -> byte offset of the pixel inside the image (out of range: padding / none), the stage's channels through the scalar offset
CTW_FN unsigned ctw_halo_voff(int i, int x0, int y0, int H, int W, int Cin) {
    const int pix = i >> 1, half = i & 1, hy = pix / HALO, hx = pix - hy * HALO;
    const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
    const bool in = i < PLANE * 2 && gy >= 0 && gy < H && gx >= 0 && gx < W;
    return in ? (unsigned)((gy * W + gx) * Cin + 4 * half) * 4u : WINO_OOB;
}
CTW_FN unsigned ctw_halo_soff(int st) { return (unsigned)(st * KS) * 4u; }
// ... and its LDS slot inside raw[u] ([c][py][px]; the threads without an element store their zeros at dump, dead LDS)
CTW_FN int ctw_halo_slot(int i, int dump) { return i < PLANE * 2 ? 4 * (i & 1) * PLANE + (i >> 1) : dump; }

// ---- the store phase.  The block's 32 x 32 x 32 outputs leave as BUFFER stores (round 6): an image is one buffer, a thread's offset inside it is
// computed once, the sixteen passes differ by one 32-bit add - no per-pass 64-bit address arithmetic, no per-pass bounds branch (profiles/r06_m_*:
// the store phase was 4.2-5.4 k cycles of instruction issue per block).  Pixels right of the image: an out-of-range thread offset (the store is
// dropped); rows below it: beyond the buffer's end in the NHWC layout (rows are its slowest dimension; host: 32 rows of slack), the marker for
// the pass in the plane layout.
struct CtwStore {
    int lx, lyh, cq;      // this thread's pixel column, row parity and channel quad inside the block (pass p stores row lyh + 2 p)
    unsigned yv, rowpair; // byte offset of pass 0, or the marker; bytes between the rows of two passes
};
// channel-quad planes (B, YC/4, YH, YW, 4): 32 lanes = one output row of the block in one plane, 512 contiguous bytes;
// NHWC: 8 lanes = the block's 32 channels of one pixel, 128 contiguous bytes
CTW_FN CtwStore ctw_store_thread(bool q4, int tide, int ex0, int ey0, int ycoff, int en0, int YH, int YW, int YC) {
    const int oy0 = 2 * ey0, ox0 = 2 * ex0;
    const size_t plane = (size_t)YH * YW;
    CtwStore s;
    s.lyh = tide >> 8;
    if (q4) {
        s.lx = tide & 31;
        s.cq = (tide >> 5) & 7;
        s.yv = ox0 + s.lx < YW ? (unsigned)((((ycoff + en0) >> 2) + s.cq) * (int)plane + (oy0 + s.lyh) * YW + ox0 + s.lx) * 16u : WINO_OOB;
        s.rowpair = (unsigned)YW * 32u;                        // (two rows of 16-byte pixels)
    } else {
        s.cq = tide & 7;
        s.lx = (tide >> 3) & 31;
        const bool in_x = ox0 + s.lx < YW;
        s.yv = in_x ? (unsigned)(((oy0 + s.lyh) * YW + ox0 + s.lx) * YC + ycoff + en0 + 4 * s.cq) * 4u : WINO_OOB;
        // right of the image every pass keeps the marker: added to it, the pass offsets wrapped past 2^32 into the image once 15 rowpair
        // reached 1 GiB (tests/test_conv_offsets_cpu.py); rows below the image lie beyond the buffer's end
        s.rowpair = in_x ? (unsigned)YW * (unsigned)YC * 8u : 0u;
    }
    return s;
}

// the VECTOR offset of pass p (the scalar offset of a store stays the constant 0: see ctw_store_block)
CTW_FN unsigned ctw_store_voff(bool q4, const CtwStore& s, int pass, int ey0, int YH) {
    if (q4) return 2 * ey0 + 2 * pass < YH ? s.yv + (unsigned)pass * s.rowpair : WINO_OOB;
    return s.yv + (unsigned)pass * s.rowpair;
}

// ---- the host contract: the parity-(0, 0) launch description of lwg_conv_transpose4_nhwc_f32 (ntaps = 4, stride = 1, omul = 2, OH = H, OW = W,
// YH = 2 H, YW = 2 W, LWG_EPI_NONE, one input) with Cin % 16 == 0, N % 32 == 0, ydt LWG_DT_F32 or LWG_DT_F32_Q4, ycoff / YC channel slices, any
// activation of the forward path; args->w = the kernel's own panel of pair_bytes per (input channel, output channel), smaller than panel_limit
CTW_FN bool ctw_contract_ok(const LwgConvArgs& a, unsigned long long pair_bytes, unsigned long long panel_limit) {
    if (!a.x0 || !a.w || !a.y || a.M <= 0 || a.ntaps != 4 || a.stride != 1 || a.omul != 2 || a.C0 <= 0 || (a.C0 % (2 * KS)) != 0 || a.C1 != 0 ||
        a.N <= 0 || (a.N % NBT) != 0 || a.OH != a.H || a.OW != a.W || a.YH != 2 * a.H || a.YW != 2 * a.W || a.xdt != LWG_DT_F32 ||
        (a.ydt != LWG_DT_F32 && a.ydt != LWG_DT_F32_Q4) || a.M != a.B * a.H * a.W || a.epi != LWG_EPI_NONE || a.act == LWG_ACTIVATION_RELU_MASK ||
        a.ycoff < 0 || (a.ycoff % 4) != 0 || (a.YC % 4) != 0 || a.ycoff + a.N > a.YC)
        return false;
    if ((unsigned long long)a.H * a.W * a.C0 * 4ull >= (unsigned long long)WINO_OOB || pair_bytes * a.C0 * a.N >= panel_limit) return false;
    // (an output image is one buffer of the store path: byte offsets + the sixteen row-pair offsets of a block stay below the out-of-range marker)
    if ((unsigned long long)a.YH * a.YW * a.YC * 4ull + 32ull * a.YW * a.YC * 4ull >= (unsigned long long)WINO_OOB) return false;
    return true;
}

// ---- part 2: device code and the launch ----
#ifdef __HIPCC__
#include "lwg_common.h"

template <int V> struct IntT { static constexpr int value = V; };

__device__ __forceinline__ floatx4 ctw_buf_load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}

// The workgroup's walk over its blocks and the per-block state (workgroup-uniform): image b, block corner (x0, y0), first output column n0, this
// image as a buffer; this thread's two halo elements.  XCD: the lab switch of the block order (0 = column-block-major).
template <bool XCD>
struct CtwBlock {
    CtwGrid g;
    CtwOrder o;
    int b, x0, y0, n0;
    __amdgpu_buffer_rsrc_t rx0;
    unsigned voff0[2];
    int wst[2];           // the halo elements' LDS slot

    __device__ __forceinline__ CtwBlock(const LwgConvArgs& a, int tid, int dump_off) {
        g = ctw_grid(a.B, a.H, a.W, a.N);
        o = ctw_order(XCD, gridDim.x, blockIdx.x, a.N, g);
#pragma unroll
        for (int q = 0; q < 2; ++q) wst[q] = ctw_halo_slot(tid + WG_THREADS * q, dump_off + tid);
    }
    __device__ __forceinline__ bool has_block(int id) const { return ctw_has_block(o, id); }
    __device__ __forceinline__ void setup(const LwgConvArgs& a, int tid, int id) {
        int cb = ctw_col_block(o, id);                       // (the XCD order's column block is scalar arithmetic on the workgroup id already)
        if (!o.xcd) cb = __builtin_amdgcn_readfirstlane(cb);
        const int t = __builtin_amdgcn_readfirstlane(ctw_tile(o, id, cb));
        b = __builtin_amdgcn_readfirstlane(ctw_image(g, t));
        ctw_corner(g, t - b * g.bx * g.by, cb, x0, y0, n0);
        rx0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x0 + (size_t)b * a.H * a.W * a.C0), 0,
                                                (int)((unsigned)(a.H * a.W) * (unsigned)a.C0 * 4u), 0x00020000);
#pragma unroll
        for (int q = 0; q < 2; ++q) voff0[q] = ctw_halo_voff(tid + WG_THREADS * q, x0, y0, a.H, a.W, a.C0);
    }
    // halo element q of stage st: global -> registers -> raw[buf]
    __device__ __forceinline__ floatx4 rld1(int st, int q) const { return ctw_buf_load(rx0, voff0[q], ctw_halo_soff(st)); }
    __device__ __forceinline__ void rst1(float* raw0, int buf, int q, floatx4 v) const {
        float* dst = raw0 + buf * RAW_FLOATS + wst[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k * PLANE] = v[k];
    }
};

// The store phase of block (eb, ex0, ey0, en0): the exchange buffer smem (rows of 32 pixel slots x OROW floats, pixel (ly, lx) of the block in slot
// slot(ly, lx) of row ly) -> global memory, 16 passes of one 16-byte buffer store per thread.  NT: the cache policy of the stores (0 = default).
//   The pass offset goes into the VECTOR offset, the scalar offset stays the constant 0: with a register in the scalar-offset field the compiler
// plans no wait state between a 16-byte store and a VALU write of its data registers - and the next pass's address add landed in the first data
// register right behind the store: intermittently corrupted first channels, found by tools/determinism_stress.py; r06_ar, DESIGN.md 3.12c (i)
template <int NT, class Slot>
__device__ __forceinline__ void ctw_store_block(const LwgConvArgs& a, const float* smem, int tide, int eb, int ex0, int ey0, int en0, Slot slot) {
    typedef unsigned int ctw_u4 __attribute__((ext_vector_type(4)));
    const size_t plane = (size_t)a.YH * a.YW;
    auto passes = [&](auto Q4) {
        constexpr bool q4 = decltype(Q4)::value != 0;
        const __amdgpu_buffer_rsrc_t ry =
            q4 ? __builtin_amdgcn_make_buffer_rsrc(a.y + (size_t)eb * (size_t)(a.YC >> 2) * plane * 4, 0, (int)((unsigned)(a.YC >> 2) * (unsigned)plane * 16u), 0x00020000)
               : __builtin_amdgcn_make_buffer_rsrc(a.y + (size_t)eb * plane * a.YC, 0, (int)((unsigned)plane * (unsigned)a.YC * 4u), 0x00020000);
        const CtwStore s = ctw_store_thread(q4, tide, ex0, ey0, a.ycoff, en0, a.YH, a.YW, a.YC);
#pragma unroll
        for (int pass = 0; pass < 16; ++pass) {
            const int ly = s.lyh + 2 * pass;
            const ctw_u4 v = *reinterpret_cast<const ctw_u4*>(smem + (ly * 32 + slot(ly, s.lx)) * OROW + 4 * s.cq);
            __builtin_amdgcn_raw_buffer_store_b128(v, ry, (int)ctw_store_voff(q4, s, pass, ey0, a.YH), 0, NT);
        }
    };
    if (a.ydt == LWG_DT_F32_Q4) passes(IntT<1>()); else passes(IntT<0>());
}

// The common tail of the two entry points: the contract, the dynamic-LDS opt-in (done: the entry point's own once-per-device flags), persistent
// workgroups - one per CU (LDS) at most - and the launch.
template <class Kernel>
static inline int ctw_launch(Kernel kernel, const LwgConvArgs* pa, lwg_stream_t stream_, unsigned long long pair_bytes, unsigned long long panel_limit,
                             size_t lds, unsigned long long& done) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!pa || !ctw_contract_ok(*pa, pair_bytes, panel_limit)) return (int)hipErrorInvalidValue;
    const LwgConvArgs& a = *pa;
    if (hipError_t e = lwg_allow_dynamic_lds(reinterpret_cast<const void*>(kernel), lds, done); e != hipSuccess) return (int)e;
    const long total = ctw_total_blocks(a.B, a.H, a.W, a.N);
    const int cus = lwg_device_cus();
    hipLaunchKernelGGL(kernel, dim3((unsigned)(LWG_WINO_PERSIST && total > cus ? cus : total)), dim3(WG_THREADS), lds, stream, a);
    return (int)hipGetLastError();
}
#endif  // __HIPCC__
