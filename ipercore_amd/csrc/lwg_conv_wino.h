// What the three fused Winograd forms of the 3 x 3 / stride 1 / pad 1 convolution share - conv_winograd.hip (fp32 F(2x2, 3x3)), conv_winograd4.hip
// (fp32 F(4x4, 3x3)) and conv_winograd_bf16.hip (bf16 F(2x2, 3x3)): the block grid, the persistent-workgroup walk and its block orders, the halo
// offsets with their out-of-range marker, the per-image buffer descriptors, the one / two-input halo loads, F(4x4)'s output offsets, the host
// contracts, the panel entry points' tap check and the launch.  Each kernel keeps its tile and LDS constants, its K loop and slot plan, its
// transforms, fragment loads, LDS slot map, exchange buffer, output transform and lab switches.  The bf16 kernel takes the grid,
// the halo offsets, the image descriptor and the contract only: its body holds the halo as pixel indices (three registers, not six offsets).
//   Part 1 is plain integer arithmetic that a host compiler can include: tests/test_conv_offsets_cpu.py compiles these very functions with
// signed-overflow traps and drives them over the corner shapes of the contracts.  Part 2 (hipcc only) is the device code around them.
// Not merged with lwg_convt_wino.h: the block orders' rules differ (F(4x4) takes the XCD-aware order at two column blocks only for Cin >= 192, and
// has a chunked order besides), and so does the rest of the device code.
#pragma once
#include <stddef.h>
#include "lwg_conv_args.h"

#ifdef __HIPCC__
#define CW_FN static __host__ __device__ __forceinline__
#else
#define CW_FN static inline
#endif
#ifdef __HIP_DEVICE_COMPILE__
#define CW_UNIFORM(v) __builtin_amdgcn_readfirstlane(v)   // a workgroup-uniform value, into a scalar register (host: the value)
#else
#define CW_UNIFORM(v) (v)
#endif
#define CW_OOB 0xC0000000u                   // >= any image's byte size (host: H * W * C * bytes < 3 GiB): the buffer load returns 0, the store is dropped
#define CW_KS 8                              // input channels per stage of the fp32 kernels
#define CW_NB 64                             // output channels per block (fp32 small forms: 32)
// ---- part 1: integer arithmetic, host-compilable ----
// The block grid of a launch: blocks of ex x ey output pixels (16 x 16: F(2x2) and bf16, 32 x 16: F(4x4)) x nbv output channels; bx x by
// blocks per image, tiles = blocks of all images, total = tiles x column blocks
struct CwGrid { int bx, by, tiles, total; };
CW_FN CwGrid cw_grid(int B, int H, int W, int N, int ex, int ey, int nbv) {
    const int bx = (W + ex - 1) / ex, by = (H + ey - 1) / ey, tiles = bx * by * B;
    return CwGrid{bx, by, tiles, tiles * (N / nbv)};
}
CW_FN long long cw_total_blocks(int B, int H, int W, int N, int ex, int ey, int nbv) {      // (the host's count: 64 bits, before the grid is cut to the CUs)
    return (long long)((W + ex - 1) / ex) * ((H + ey - 1) / ey) * B * (N / nbv);
}

// ---- the block order: nwg persistent workgroups, workgroup wg walks the block ids wg + k nwg.
//   CW_COLMAJOR (F(2x2); bf16 behind its lwg_xcd_remap; F(4x4) otherwise): id = column block * tiles + tile.
//   CW_CHUNK (F(4x4), layers whose WHOLE fragment panel stays in an XCD's 4 MB L2 - in the generator N = 128): the grid's G persistent workgroups walk
// a chunk of G tiles through ALL column blocks before the next chunk (workgroup w: tile ch G + w in N / 64 consecutive blocks) - a tile's halo is
// re-read one round after its first read instead of a whole pass over the batch apart.  Measured inside the 300-frame step (profiles/r06_ag_*):
// 2-3.4 % faster per launch for N = 128, 2-5 % SLOWER for N >= 256 (every round then pulls another column block's panel through L2): those keep
// the column-block-major order.
//   CW_XCD (F(4x4), 8-wave form, persistent grids of a multiple of 8 workgroups, N / 64 = 2, 4 or 8 column blocks): workgroup w runs on XCD w % 8
// (round-robin dispatch) and keeps ONE column block, (w % 8) % ncb, for the whole launch - an XCD's 4 MB L2 holds that column block's panel only and
// never turns it over -, while the ncb workgroups (w % 8) / ncb, w / 8 of adjacent XCDs walk the SAME tile sequence in step: a tile's halo is fetched
// by ncb XCDs at about the same time - once from HBM, the rest out of the memory-side cache - instead of ncb times a whole pass over the batch apart.
// Measured inside the 300-frame step (profiles/r06_am_*): 2-7 % per launch for N >= 256 and for N = 128 with Cin >= 192; the N = 128 layers with
// Cin <= 128 keep the chunked order (1-4 % faster there).
enum { CW_COLMAJOR = 0, CW_CHUNK = 1, CW_XCD = 2 };
struct CwOrder { int kind, nwg, wg, ncb, tiles, total, xg, xr; };    // xg, xr (CW_XCD): workgroups per column block = tiles per round, this one's place among them

// F(4x4)'s rule.  xcd_sw / chunk_sw: the lab switches LWG_W4_XCD (0 off, 1 the rule, 2 two column blocks at any Cin) / LWG_W4_CHUNK (0 never, 1 where
// the 144-byte-per-pair panel is at most 5 MiB, 2 always); sm: the 4-wave form (never XCD-aware)
CW_FN int cw4_order_kind(int xcd_sw, int chunk_sw, bool sm, unsigned nwg, int ncb, int Cin, int N, int tiles, int total) {
    const bool xcd = xcd_sw && !sm && (nwg & 7u) == 0 && (ncb == 4 || ncb == 8 || (ncb == 2 && (Cin >= 192 || xcd_sw == 2))) && (int)nwg < total && tiles >= (int)nwg / ncb;
    return xcd ? CW_XCD : chunk_sw == 2 || (chunk_sw == 1 && 144u * (unsigned)Cin * (unsigned)N <= (5u << 20)) ? CW_CHUNK : CW_COLMAJOR;
}
CW_FN CwOrder cw_order(int kind, unsigned nwg, unsigned wg, int ncb, const CwGrid& g) {
    return CwOrder{kind, (int)nwg, (int)wg, ncb, g.tiles, g.total, (int)nwg / ncb, (int)(((wg & 7u) / (unsigned)ncb) * (nwg >> 3) + (wg >> 3))};
}
CW_FN bool cw_has_block(const CwOrder& o, int id) {            // (id = wg + k nwg)
    return o.kind == CW_XCD ? (id / o.nwg) * o.xg + o.xr < o.tiles : id < o.total;
}
// block id -> column block and tile (the XCD order's column block is scalar arithmetic on the workgroup id already)
CW_FN void cw_block(const CwOrder& o, int id, int& cb, int& t) {
    if (o.kind == CW_XCD) {
        cb = (int)((unsigned)o.wg & 7u) & (o.ncb - 1);
        t = CW_UNIFORM((id / o.nwg) * o.xg + o.xr);
    } else if (o.kind == CW_CHUNK) {
        const int G = o.nwg, per = G * o.ncb;
        const int ch = CW_UNIFORM(id / per);
        const int r = id - ch * per, base = ch * G;
        const int nt = o.tiles - base < G ? o.tiles - base : G;
        cb = CW_UNIFORM(r / nt);
        t = CW_UNIFORM(base + r - cb * nt);
    } else {
        cb = CW_UNIFORM(id / o.tiles);
        t = CW_UNIFORM(id - cb * o.tiles);
    }
}
CW_FN int cw_image(const CwGrid& g, int t) { return t / (g.bx * g.by); }
// the block's corner (x0, y0) from its tile inside image b (t - b bx by); its first output column from its column block
CW_FN void cw_corner(const CwGrid& g, int t_in_image, int ex, int ey, int& x0, int& y0) { x0 = (t_in_image % g.bx) * ex, y0 = (t_in_image / g.bx) * ey; }
CW_FN int cw_n0(int cb, int nbv) { return cb * nbv; }
// (F(4x4), 4-wave form with the SPADE epilogue: the block's 32 accumulator rows are gamma | beta of the SAME 16 channels - columns n0 .. + 15 and
// n0 + 32 .. + 47 of the stacked panel - so the modulation still finds both in one block)
CW_FN int cw4_n0_spade_small(int cb) { return (cb >> 1) * 64 + (cb & 1) * 16; }
// ---- the halo: element i of a stage (nel of them: pixel i >> lgp of the hw pixels wide halo, 16-byte piece i % 2^lgp of the stage's channels; a
// thread holds i = tid + k threads) -> the pixel inside the image (linear index, or -1: padding / no element) -> its byte offset inside an input
// of C channels of ebytes bytes, or the marker (the hardware returns zeros: no branches, no exec masks); the stage's channels through the scalar
// offset.  fp32: 2 quads per pixel (lgp 1), bf16: 4 octets (lgp 2)
CW_FN int cw_halo_pixel(int i, int hw, int nel, int lgp, int x0, int y0, int H, int W) {
    const int pix = i >> lgp, hy = pix / hw, hx = pix - hy * hw;
    const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
    return i < nel && gy >= 0 && gy < H && gx >= 0 && gx < W ? gy * W + gx : -1;
}
CW_FN unsigned cw_halo_pixel_voff(int lin, int i, int lgp, int C, int ebytes) {
    return lin >= 0 ? (unsigned)(lin * C + (16 / ebytes) * (i & ((1 << lgp) - 1))) * (unsigned)ebytes : CW_OOB;
}
CW_FN unsigned cw_halo_voff(int i, int hw, int nel, int lgp, int x0, int y0, int H, int W, int C, int ebytes) {
    return cw_halo_pixel_voff(cw_halo_pixel(i, hw, nel, lgp, x0, y0, H, W), i, lgp, C, ebytes);
}
// a stage's channels c .. lie in ONE input (C0 is a multiple of the stage): in the second one (two-input launches) at c - C0
CW_FN bool cw_stage_second(int c, int C0, bool two) { return two && c >= C0; }
CW_FN unsigned cw_stage_soff(int c, int C0, bool two, int ebytes) { return (unsigned)(cw_stage_second(c, C0, two) ? c - C0 : c) * (unsigned)ebytes; }
// ---- F(4x4)'s output pixels.  Image eb of the output (and of res / xn: the output's layout) is ONE buffer: a reader thread's pixel (ox, oy), first
// channel chan, is a 32-bit offset inside it (out of range: right of / below the image - the hardware drops the store and returns zeros for the
// load), the second channel group (+ 32 channels; 8-wave form, not the SPADE store) an increment of the VECTOR offset: the scalar offset of the
// stores and loads stays the constant 0 (test_no_wide_buffer_store_with_register_soffset; lwg_convt_wino.h: ctw_store_block)
CW_FN unsigned cw4_out_voff(int ox, int oy, int H, int W, int YC, int chan) {
    return ox < W && oy < H ? (unsigned)((oy * W + ox) * YC + chan) * 4u : CW_OOB;
}
CW_FN unsigned cw4_out_group(unsigned vo, int h, bool grouped) { return vo + (grouped ? 128u * (unsigned)h : 0u); }

// ---- list-driven launches of F(4x4) (lwg_conv2d_winograd4_list_f32, spade_skip.hip).  A tile (one 32 x 16 block position of one image,
// cw_grid's numbering) is HEAVY when the window of its block - the block grown by d pixels, clipped to the image - holds a pixel with an in-image tap of
// any source, else LIGHT.  The launch's entries: heavy entry e = (tile heavy[e / ncb], column block e % ncb) for e < nhe = heavy tiles x ncb, then light
// entry e - nhe the same way through the light list; persistent workgroup wg of nwg walks the ids wg + k nwg of [0, nhe + nle) - its heavy ones through the
// K loop first, then its light ones in the streaming loop (which starts at cw_list_first_light).
struct CwWindow { int x0, y0, x1, y1; };     // [x0, x1) x [y0, y1)
CW_FN CwWindow cw_block_window(int x0, int y0, int ex, int ey, int d, int H, int W) {
    return CwWindow{x0 - d > 0 ? x0 - d : 0, y0 - d > 0 ? y0 - d : 0, x0 + ex + d < W ? x0 + ex + d : W, y0 + ey + d < H ? y0 + ey + d : H};
}
CW_FN void cw_list_entry(int e, int ncb, int& slot, int& cb) { slot = e / ncb, cb = e - slot * ncb; }
CW_FN int cw_list_first_light(int wg, int nwg, int nhe) { return wg >= nhe ? wg : wg + (nhe - wg + nwg - 1) / nwg * nwg; }
// a light block's elements: pass it of thread tid (nth threads) -> pixel (px, py) of the 32 x 16 block and 16-byte channel quad q4 of its nq quads (a
// power of two: 16 - the block's 64 columns -, SPADE 8 - its 32 channels); nth % nq == 0: a thread keeps its quad through the passes
CW_FN void cw4_light_elem(int tid, int it, int nth, int nq, int& px, int& py, int& q4) {
    const int e = it * nth + tid, p = e / nq;
    q4 = e - p * nq, px = p & 31, py = p >> 5;
}

// ---- sub-tile lists of F(4x4) (lwg_conv2d_winograd4_fine_f32 / _q8_f32, spade_skip.hip).  A 32 x 16 block is NS sub-tiles of SX x SY
// output pixels (patch-aligned: SX / 4 x SY / 4 patches); sub-tile u = NS * block + s, s = sub-tile row * NSX + sub-tile column - so the sub-tiles of
// a launch whose sub-tiles are all heavy are exactly the plain blocks, in their order.  A sub-tile is heavy / light by the block rule applied to ITS
// window (cw_block_window of the sub-tile); sub-tiles wholly outside the image are in neither list.  The launch's heavy entries: entry e = (group
// e / ncb, column block e % ncb), the group's NS slots = heavy[NS * group ..] (slots past the count: empty); patch (pty, ptx) of the workgroup's
// 4 x 8 patches belongs to slot slot_of_patch - a group that is one whole block has the plain block's patch numbering.
//   Two geometries: Cw4F, 16 x 8 (four slots of 4 x 2 patches), and Cw4Q, 8 x 8 (eight slots of 2 x 2 patches: sub-tile u = 8 * block + 4 * (sub-tile
// row) + sub-tile column).  A 16 x 8 sub-tile is the 8 x 8 sub-tiles 4 r + 2 c, 4 r + 2 c + 1 of its block: its window is the union of theirs, its
// mark their OR.  What differs between the two beyond SX, SY - which wave stages which slot, the LDS placement, the 8 x 8 reader - follows the struct.
template <int SX_, int SY_>
struct Cw4Sub {
    static constexpr int SX = SX_, SY = SY_, NSX = 32 / SX, NS = NSX * (16 / SY);
    static constexpr int HW = SX + 2, HH = SY + 2;           // a sub-tile's halo: 18 x 10 | 10 x 10 pixels
    static constexpr int NEL = HW * HH * 2;                  // ... (pixel, channel quad) elements of a stage
    static constexpr int ROUNDS = (NEL + 63) / 64;           // ... in wave rounds of 64 (cw4_halo_elem: a wave stages ONE slot - one image descriptor)
    CW_FN int slot_of_patch(int pty, int ptx) { return (pty / (SY / 4)) * NSX + ptx / (SX / 4); }
    CW_FN void patch_in_slot(int pty, int ptx, int& ly, int& lx) { ly = pty % (SY / 4), lx = ptx % (SX / 4); }
    // sub-tile u -> its image and corner
    CW_FN void corner(const CwGrid& g, int u, int& b, int& x0, int& y0) {
        const int t = u / NS, s = u - t * NS;
        b = cw_image(g, t);
        cw_corner(g, t - b * g.bx * g.by, 32, 16, x0, y0);
        x0 += (s % NSX) * SX, y0 += (s / NSX) * SY;
    }
    CW_FN bool in_image(int x0, int y0, int H, int W) { return x0 < W && y0 < H; }
    CW_FN int in_image_total(int B, int H, int W) { return B * ((W + SX - 1) / SX) * ((H + SY - 1) / SY); }
    CW_FN int groups(int nh) { return (nh + NS - 1) / NS; }
    CW_FN int slot_index(int grp, int k, int nh) { return grp * NS + k < nh ? grp * NS + k : -1; }      // the heavy list's index, -1: empty
    // the classifier: which sub-tiles of the block at (x0, y0) hold the image pixel (x, y) in their window (bit s)
    CW_FN unsigned reached(int x, int y, int x0, int y0, int d) {
        unsigned m = 0;
        for (int s = 0; s < NS; ++s) {
            const int sx = x0 + (s % NSX) * SX, sy = y0 + (s / NSX) * SY;
            m |= (x >= sx - d && x < sx + SX + d && y >= sy - d && y < sy + SY + d ? 1u : 0u) << s;
        }
        return m;
    }
    // element j of a slot's halo (cw4_halo_elem) -> its halo pixel (hy, hx) and channel quad hq; its byte offset inside the image of the sub-tile
    // at (x0, y0), or the marker (present = false: an empty slot - nothing but markers)
    CW_FN void halo_place(int j, int& hy, int& hx, int& hq) {
        const int pix = j >> 1;
        hq = j & 1, hy = pix / HW, hx = pix - hy * HW;
    }
    CW_FN unsigned halo_voff(bool present, int j, int x0, int y0, int H, int W, int C) {
        int hy, hx, hq;
        halo_place(j, hy, hx, hq);
        const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
        return present && j < NEL && gy >= 0 && gy < H && gx >= 0 && gx < W ? (unsigned)((gy * W + gx) * C + 4 * hq) * 4u : CW_OOB;
    }
    // a light sub-tile's elements from cw4_light_elem's (px, py) of the first SX * SY pixels
    CW_FN void light_pixel(int& px, int& py) {
        const int p = py * 32 + px;
        py = p / SX, px = p - py * SX;
    }
};
using Cw4F = Cw4Sub<16, 8>;
using Cw4Q = Cw4Sub<8, 8>;
// halo element i = tid + 512 k of a stage (wave (i / 64) % 8, its round k) -> its slot - the wave's - and its element j inside the slot's halo
// (j >= NEL: none).  16 x 8: waves 2 s, 2 s + 1 share slot s, three of its six rounds each.  8 x 8: wave w stages slot w in four rounds (no element:
// the last 56 lanes of round 3)
CW_FN void cw4_halo_elem(Cw4F, int i, int& slot, int& j) {
    const int wave = (i >> 6) & 7, k = i >> 9, per = Cw4F::ROUNDS / 3, wr = 3 * wave + k;
    slot = wave / per, j = (wr - slot * Cw4F::ROUNDS) * 64 + (i & 63);
}
CW_FN void cw4_halo_elem(Cw4Q, int i, int& slot, int& j) { slot = (i >> 6) & 7, j = (i >> 9) * 64 + (i & 63); }
// the 16 x 8 marks from the 8 x 8 ones of a block (bit s: sub-tile s)
CW_FN unsigned cw4_marks16_of8(unsigned m8) { return ((m8 | (m8 >> 1)) & 1u) | (((m8 >> 2) | (m8 >> 3)) & 1u) << 1 | (((m8 >> 4) | (m8 >> 5)) & 1u) << 2 | (((m8 >> 6) | (m8 >> 7)) & 1u) << 3; }
// 8 x 8: a slot's sub-plane inside a channel plane of the LDS halo buffer (floats): rows of RS floats, two slots side by side 16 floats apart, four slot
// rows of ten halo rows with 0 / 8 / 16 floats between them - so that the sixteen patches of either ds_read_b128 lane group of the input transform
// (lanes 0-3, 12-15, 20-27 | the rest of a half wave, lane = patch) start in sixteen distinct bank quads (tests/test_spade_skip_q8_cpu.py enumerates them;
// four slots side by side in rows of 48 - 60 floats have no such padding: a patch row is a multiple of four bank quads).  (The 16 x 8 form's placement
// shares the plain kernel's rows: conv_winograd4.hip, W4FLds.)
struct Cw4QLds {
    static constexpr int RS = 28;
    static constexpr int PLN = 4 * Cw4Q::HH * RS + 24 + 4;  // + 4: 4 PLN = 16 mod 32, the two channel quads of a pixel fall into different banks
    CW_FN int slot(int s) { const int r = s >> 1; return r * (Cw4Q::HH * RS) + 4 * r * (r - 1) + (s & 1) * 16; }
    CW_FN int patch(int pty, int ptx) {                      // the first float of patch (pty, ptx)'s 6 x 6 input window inside a channel plane
        int ly, lx;
        Cw4Q::patch_in_slot(pty, ptx, ly, lx);
        return slot(Cw4Q::slot_of_patch(pty, ptx)) + 4 * ly * RS + 4 * lx;
    }
};
// 8 x 8: the epilogue's reader: wave wid, lane -> its output column rb inside a patch and its patch inside the pass (0..15: patch row p / 8 of the pass,
// patch column p % 8).  A wave's patches of a pass are the 2 x 2 of ONE slot, 4 pass + wid / 2 - image, corner, mean / rstd and the buffer descriptors stay
// wave-uniform -, its half waves own the output columns 2 (wid % 2) and + 1 (the 16 x 8 form: one column per wave, a slot's 4 x 2 patches per wave pair).
// gsel / gidx: the lane's ds_read_b128 lane group and its place in it, as in the plain reader - a group reads the eight channel quads of patches a, a + 8
CW_FN void cw4_reader8(int wid, int lane, int& rb, int& p16) {
    const unsigned l5 = (unsigned)lane & 31u, gsel = (0x0FF0F00Fu >> l5) & 1u;
    const int gidx = __builtin_popcount((gsel ? 0x0FF0F00Fu : 0xF00F0FF0u) & ((1u << l5) - 1u));
    rb = 2 * (wid & 1) + (lane >> 5);
    p16 = 2 * (wid >> 1) + (gsel ? 0 : 1) + 8 * (gidx >> 3);
}

// ---- split-K launches of F(4x4) (lwg_conv2d_winograd4_f32_ws): the training step's one-sample launches.  The 4-wave form's blocks
// (32 x 16 pixels x 32 channels) x `slices` workgroups, slice z owns the K stages [z sps, min((z + 1) sps, nst)) of its block - sps even, so every
// slice is an even number of stages - and writes its raw partial outputs to the dense (M, N) slab z of the workspace; the finishing kernel of the
// direct engine adds the slabs in slice order.  The plan (slices = 0: run the launch whole): a launch whose blocks32 4-wave blocks cover half the
// compute units or less, in min(8, cus / blocks32) slices of at least CW4_SPLIT_MIN_STAGES stages each (a slice pays the block's prologue and the
// 28-plane epilogue again); finishable = an epilogue the finishing kernel finishes (plain, or the ReLU-mask data gradient); slab_ok = a slab image is
// one buffer of the store path (cw4_slab_image_ok)
#define CW4_SPLIT_MIN_STAGES 8
#define CW4_SPLIT_MAX_SLICES 8
struct Cw4Split { int slices, sps; };
CW_FN Cw4Split cw4_split_plan(long long blocks32, int nst, int cus, bool finishable, bool slab_ok) {
    if (!finishable || !slab_ok || blocks32 < 1 || 2 * blocks32 > (long long)cus) return Cw4Split{0, 0};
    int want = (int)((long long)cus / blocks32);
    if (want > CW4_SPLIT_MAX_SLICES) want = CW4_SPLIT_MAX_SLICES;
    int sps = (nst + want - 1) / want;
    if (sps < CW4_SPLIT_MIN_STAGES) sps = CW4_SPLIT_MIN_STAGES;
    sps += sps & 1;
    const int slices = (nst + sps - 1) / sps;
    return slices < 2 ? Cw4Split{0, 0} : Cw4Split{slices, sps};
}
CW_FN int cw4_slice_begin(int slice, int sps) { return slice * sps; }
CW_FN int cw4_slice_end(int slice, int sps, int nst) { return (slice + 1) * sps < nst ? (slice + 1) * sps : nst; }
// slab `slice` of the workspace, in floats from its start (into the BASE POINTER of the slab's image buffers - never a scalar offset of the stores)
CW_FN size_t cw4_slab_offset(int slice, int M, int N) { return (size_t)slice * (size_t)M * (size_t)N; }
CW_FN bool cw4_slab_image_ok(int H, int W, int N) { return (unsigned long long)H * W * N * 4ull + 256ull < (unsigned long long)CW_OOB; }

// ---- the host contracts.  fp32 (lwg_conv2d_winograd_f32 / _f32_ws, lwg_conv2d_winograd4_f32): the launch description of the 3 x 3 / stride 1 /
// pad 1 convolution as lwg_conv2d_nhwc_f32 takes it (nine taps, omul = 1, OH = H, OW = W, one or two inputs with C0 % 8 == 0, C1 % 8 == 0 and
// (C0 + C1) % 16 == 0, N % 64 == 0, YC % 4 == 0; LWG_EPI_NONE, LWG_EPI_RESIDUAL (ycoff % 4 == 0) or LWG_EPI_SPADE (N = 2 YC, columns gamma | beta
// interleaved in blocks of 32, ycoff = 0); any activation of lwg_act, the ReLU mask with LWG_EPI_RESIDUAL; every image of an input < 3 GiB) EXCEPT
// args->w = the kernel's fragment panel of pair_bytes per (input channel, output column): F(2x2) 64 - Upk[16][Cin/8][2][N][4], element (p, s, kh,
// n, kk) = (G w G^T)[xi = p / 4][nu = p % 4] of input channel 8 s + 2 kk + kh (concatenated order) and output column n -, F(4x4) 144 (see
// lwg_winograd4_panel_f32).  out_slack: bytes beyond an output image that its offsets may reach where the image is one buffer of the store path
// (F(4x4): 256), CW_NO_OUT_BUFFER where the stores go through 64-bit pointers (F(2x2): no limit on the output image)
#define CW_NO_OUT_BUFFER (-1ll)
CW_FN bool cw_contract_ok(const LwgConvArgs& a, unsigned long long pair_bytes, long long out_slack) {
    if (!a.x0 || !a.w || !a.y || a.M <= 0 || a.ntaps != 9 || a.stride != 1 || a.omul != 1 || a.C0 <= 0 || (a.C0 % CW_KS) != 0 || a.C1 < 0 ||
        (a.C1 % CW_KS) != 0 || ((a.C0 + a.C1) % (2 * CW_KS)) != 0 || (a.C1 > 0 && !a.x1) || a.N <= 0 || (a.N % CW_NB) != 0 || a.OH != a.H ||
        a.OW != a.W || a.YH != a.H || a.YW != a.W || a.xdt != LWG_DT_F32 || a.ydt != LWG_DT_F32 || (long long)a.M != (long long)a.B * a.H * a.W ||
        a.ycoff < 0 || (a.ycoff % 4) != 0 || (a.YC % 4) != 0 || (a.act == LWG_ACTIVATION_RELU_MASK && a.epi != LWG_EPI_RESIDUAL))
        return false;
    if (a.epi == LWG_EPI_SPADE) {
        if (!a.xn || !a.mean || !a.rstd || !a.bias || a.YC * 2 != a.N || a.ycoff != 0) return false;
    } else {
        if (a.ycoff + a.N > a.YC) return false;
        if (a.epi != LWG_EPI_NONE && (a.epi != LWG_EPI_RESIDUAL || !a.res)) return false;
    }
    const unsigned long long cmax = (unsigned long long)(a.C0 > a.C1 ? a.C0 : a.C1);
    if ((unsigned long long)a.H * a.W * cmax * 4ull >= (unsigned long long)CW_OOB || pair_bytes * (a.C0 + a.C1) * a.N >= 0xffffffffull) return false;
    if (out_slack >= 0 && (unsigned long long)a.H * a.W * a.YC * 4ull + (unsigned long long)out_slack >= (unsigned long long)CW_OOB) return false;
    return true;
}
// the list-driven F(4x4) launch besides: its calibration frame (one image of YC - SPADE: N - channels) is one buffer of the same kind
CW_FN bool cw_contract_calib_ok(const LwgConvArgs& a) {
    return (unsigned long long)a.H * a.W * (unsigned long long)(a.epi == LWG_EPI_SPADE ? a.N : a.YC) * 4ull + 256ull < (unsigned long long)CW_OOB;
}
// bf16 (lwg_conv2d_winograd_bf16; include/lwg_hip.h): bf16 in and out, the taps ascending in (dy, dx) (the order the panel was built in), Cin and N
// multiples of 64 (a second input: C0 too), 8-channel slices, activation none / ReLU / tanh / sigmoid - no ReLU mask.  32-bit offsets: one IMAGE
// of either input (per-image buffer descriptors, so any batch) and the 32-byte-per-pair panel; nothing wraps - larger is refused
CW_FN bool cwb_contract_ok(const LwgConvArgs& a) {
    if (!a.x0 || !a.w || !a.y || a.B <= 0 || a.H <= 0 || a.W <= 0 || a.C0 <= 0 || a.C1 < 0 || a.N <= 0 || a.xdt != LWG_DT_BF16 || a.ydt != LWG_DT_BF16 ||
        a.ntaps != 9 || a.stride != 1 || a.omul != 1 || a.ooy != 0 || a.oox != 0 || a.OH != a.H || a.OW != a.W || a.YH != a.H || a.YW != a.W ||
        (long long)a.M != (long long)a.B * a.H * a.W)
        return false;
    for (int t = 0; t < 9; ++t)
        if (a.dy[t] != t / 3 - 1 || a.dx[t] != t % 3 - 1) return false;
    const int Cin = a.C0 + a.C1;
    if (a.N % 64 != 0 || Cin % 64 != 0 || (a.YC & 7) != 0 || (a.ycoff & 7) != 0 || a.ycoff < 0 || (a.C1 != 0 && (a.C0 % 64 != 0 || !a.x1))) return false;
    if (a.act != LWG_ACTIVATION_NONE && a.act != LWG_ACTIVATION_RELU && a.act != LWG_ACTIVATION_TANH && a.act != LWG_ACTIVATION_SIGMOID) return false;
    if ((unsigned long long)a.H * a.W * (unsigned long long)(a.C0 > a.C1 ? a.C0 : a.C1) * 2ull >= (unsigned long long)CW_OOB ||
        32ull * (unsigned long long)Cin * (unsigned long long)a.N >= (unsigned long long)CW_OOB || cw_total_blocks(a.B, a.H, a.W, a.N, 16, 16, 64) >= 0x7fffffffll)
        return false;
    if (a.epi == LWG_EPI_SPADE) return a.xn && a.mean && a.rstd && a.bias && a.YC * 2 == a.N && a.ycoff == 0;
    return a.ycoff + a.N <= a.YC && (a.epi == LWG_EPI_NONE || (a.epi == LWG_EPI_RESIDUAL && a.res));
}

// the fp32 panel entry points' arguments (lwg_winograd_panel_f32, lwg_winograd4_panel_f32): tap9[3 r + s] = the tap index of kernel position
// (dy, dx) = (r - 1, s - 1) in the GEMM panel
struct LwgWinoTaps { int t[9]; };
CW_FN bool cw_panel_args_ok(const float* wpanel, const float* upk, int Cin, int N, const int* tap9, LwgWinoTaps& taps) {
    if (!wpanel || !upk || !tap9 || Cin <= 0 || (Cin % 32) != 0 || N <= 0) return false;
    for (int i = 0; i < 9; ++i) {
        if (tap9[i] < 0 || tap9[i] > 8) return false;
        taps.t[i] = tap9[i];
    }
    return true;
}

// ---- part 2: device code and the launch ----
#ifdef __HIPCC__
#include "lwg_conv_direct.h"

// POLICY: the cache policy of the load (0 = default; F(4x4)'s halo loads pass W4_NT_LD)
template <int POLICY = 0>
__device__ __forceinline__ floatx4 cw_buf_load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, POLICY));
}
// image b of an input (B, H, W, C) of ebytes-byte elements as a buffer
__device__ __forceinline__ __amdgpu_buffer_rsrc_t cw_image_rsrc(const void* x, int b, int H, int W, int C, unsigned ebytes) {
    const unsigned img = (unsigned)(H * W);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(x)) + (size_t)b * img * C * ebytes, 0, (int)(img * (unsigned)C * ebytes), 0x00020000);
}

// The per-block state of the fp32 kernels (workgroup-uniform): image b, block corner (x0, y0), first output column n0, this image of each input
// as a buffer; this thread's NQ halo elements (pixel, channel quad): byte offsets inside either input.
// TWO (round 6): the launch has a second input (skip concatenation).  One-input launches - four fifths of the engine's time - carry no per-load choice
// of the source tensor at all: as a uniform branch pair around every halo load it cost 1.9 % of the K loop and 700 cycles of every block's set-up
// (profiles/r06_k_*); the two-input form selects the descriptor / offset (scalar selects + one v_cndmask per load) instead of branching.
template <int NQ, bool TWO>
struct CwBlock {
    int b, x0, y0, n0;
    __amdgpu_buffer_rsrc_t rx0, rx1;
    unsigned voff0[NQ], voff1[NQ];

    // tile t of the grid (ex x ey pixels per block), first output column n
    __device__ __forceinline__ void locate(const LwgConvArgs& a, const CwGrid& g, int t, int ex, int ey, int n) {
        b = __builtin_amdgcn_readfirstlane(cw_image(g, t));
        cw_corner(g, t - b * g.bx * g.by, ex, ey, x0, y0);
        n0 = n;
        rx0 = cw_image_rsrc(a.x0, b, a.H, a.W, a.C0, 4u);
        if constexpr (TWO) rx1 = cw_image_rsrc(a.x1, b, a.H, a.W, a.C1, 4u);
    }
    // the elements tid + nth k of the hw pixels wide halo (nel elements); padding pixels / threads without an element: an out-of-range offset (zeros)
    __device__ __forceinline__ void halo(const LwgConvArgs& a, int tid, int nth, int hw, int nel) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            voff0[k] = cw_halo_voff(tid + nth * k, hw, nel, 1, x0, y0, a.H, a.W, a.C0, 4);
            if constexpr (TWO) voff1[k] = cw_halo_voff(tid + nth * k, hw, nel, 1, x0, y0, a.H, a.W, a.C1, 4);
        }
    }
    // halo element k of the stage whose first channel (concatenated order) is c
    template <int POLICY = 0>
    __device__ __forceinline__ floatx4 rld1(const LwgConvArgs& a, int c, int k) const {
        if constexpr (!TWO) {
            return cw_buf_load<POLICY>(rx0, voff0[k], cw_stage_soff(c, a.C0, false, 4));
        } else {
            const bool second = cw_stage_second(c, a.C0, true);
            const __amdgpu_buffer_rsrc_t r = second ? rx1 : rx0;
            const unsigned v = second ? voff1[k] : voff0[k];
            return cw_buf_load<POLICY>(r, v, cw_stage_soff(c, a.C0, true, 4));
        }
    }
};
// a halo element's four channels -> its slot of the channel-major planes raw[buf] (plane floats apart)
__device__ __forceinline__ void cw_rst1(float* dst, int plane, floatx4 v) {
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k * plane] = v[k];
}

// The dynamic-LDS opt-in of one kernel instantiation (once per device) and its launch: lwg_launch_lds (lwg_conv_direct.h)
template <void (*KERNEL)(const LwgConvArgs)>
static inline int cw_launch(dim3 grid, unsigned threads, size_t lds, hipStream_t stream, const LwgConvArgs& a) {
    return (int)lwg_launch_lds<KERNEL>(grid, dim3(threads), lds, stream, a);
}
// ... of a list-driven kernel (LwgConvArgs and the lists)
template <void (*KERNEL)(const LwgConvArgs, const LwgConvLists)>
static inline int cw_launch_lists(dim3 grid, unsigned threads, size_t lds, hipStream_t stream, const LwgConvArgs& a, const LwgConvLists& l) {
    return (int)lwg_launch_lds<KERNEL>(grid, dim3(threads), lds, stream, a, l);
}
// persistent workgroups: one per CU (LDS) at most, each walking block ids blockIdx.x + k gridDim.x (LWG_WINO_PERSIST = 0: one block per workgroup)
static inline dim3 cw_persistent_grid(long long total, int cus) { return dim3((unsigned)(LWG_WINO_PERSIST && total > cus ? cus : total)); }
#endif  // __HIPCC__
