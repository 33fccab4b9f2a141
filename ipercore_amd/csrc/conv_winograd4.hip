// Fused F(4x4, 3x3) Winograd form of the 3x3 / stride 1 / pad 1 fp32 convolution on v_mfma_f32_32x32x2_f32 (round 6; the sibling of conv_winograd.hip's
// F(2x2, 3x3) kernel for the layers whose K loop is long enough to pay for the larger transforms - DESIGN.md 3.12d; attlwb_spade_resunet.py:14-25,62-93,316-357).
//   y = act(bias + sum x * w [+ res]) computed as U = G w G^T (6 x 6 per channel pair; the fragment panel built by lwg_winograd4_panel_f32 below), V = B^T d B per
//   6 x 6 input patch d (patches overlap by two pixels), M_{xi,nu} = V_{xi,nu} U_{xi,nu} - thirty-six GEMMs over Cin -, Y = A^T M A (4 x 4 outputs per patch):
//   36 multiplies per 16 outputs = 2.25 per output instead of 9 (F(2x2, 3x3): 4).  Points 0, +-1, +-2, inf (Lavin & Gray):
//     B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//     G   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
//     A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
// Workgroup: 512 threads = 8 waves; block = 8 x 4 patches (32 x 16 output pixels) x 64 output channels.  Wave w = (q = w % 4, channel tile ct = w / 4) owns NINE
// products for the block's 32 patches x 32 channels (9 accumulator tiles of 32 x 32 = 144 VGPRs, rows = output channels - the transposed kernel's shape):
// the whole row xi = q of the transformed patch (nu = 0..5) and three products of row 4 + q / 2 (nu = 3 (q % 2) .. + 2).  The nu half of A^T M A is then
// register-local for rows 0..3 and half-local for rows 4, 5: 28 planes of (patch, channel) values cross LDS in the epilogue.
// A K stage is 8 input channels = four k-pairs; per k-pair a lane loads its nine weights as two 16-byte and one 4-byte buffer loads from the panel
// Upk[4][Cin/8][4][2][9 N] (every instruction reads contiguous memory; two k-pairs ahead, four register sets) and reads nine V fragments (4 bytes each) from LDS, each one right behind the MFMA that
// used its register for the previous k-pair.  The raw 34 x 18 x 8 halo goes global -> registers -> raw[s % 2] (channel-major planes, rows of 40 floats);
// the 256 (patch, channel) transforms of the next stage are shared by the 512 threads: waves 0-3 form rows 0..2 of B^T d B, waves 4-7 rows 3..5 (72 vector
// instructions per thread and stage), one barrier per stage in front of k-pair 3.
// Persistent workgroups in an XCD-aware block order (one column block per XCD for the whole launch; see the kernel), a 4-wave form for small launches.
// Rounding: relative L2 error against fp64 ~14-20x the direct fp32 convolution's (3e-6; tools/winograd_study.py --f43): fp32-grade, NOT the direct kernel's
// and not the F(2x2, 3x3) kernel's bits.  A frame's result does not depend on the batch it is launched in (per-image work in a fixed order).
#include <hip/hip_runtime.h>
#include <type_traits>
#include "lwg_common.h"
#include "lwg_conv_wino.h"

#define W4_THREADS 512
#define W4_PBX 8             // patches per block row: 32 output pixels
#define W4_PBY 4             // patch rows per block: 16 output pixels
#define W4_NB 64             // output channels per block
#define W4_KS 8              // input channels per stage
#define W4_HW 34             // halo pixels per row
#define W4_HH 18             // halo rows
#ifndef W4_RS
#define W4_RS 40             // floats per halo row in LDS (16-byte aligned rows).  40: a patch row (four halo rows) is 160 = 32 mod 64 floats, so the 16 lanes of a
                             // ds_read_b128 lane group - patches (pty, ptx 0-3 | 4-7) of four patch rows - read sixteen distinct bank quads in the transform
                             // (36: 144 = 16 mod 64, two-way conflicts on every patch-row read; PMC r06_ah / r06_ak)
#endif
#define W4_PLANE (18 * W4_RS + 4)   // floats per channel plane: 18 rows + 4 (4 PLANE = 16 mod 32: the two channel quads of a pixel fall into different banks)
                             // (lab: consecutive lanes = consecutive pixels of one quad + planes of 704 floats, i.e. ds_write2st64_b32 halo stores: 6-12 % SLOWER -
                             //  a lane pair no longer reads 32 contiguous bytes; profiles/r06_y3_*)
#define W4_RAW (W4_KS * W4_PLANE)
#define W4_VS (36 * W4_KS * 32)                  // [product 6 xi + nu][k][patch]
#define W4_NEL (W4_HW * W4_HH * 2)               // (pixel, channel quad) elements of a stage's halo
#define W4_NQ 3                                  // ... per thread (the third round: threads < W4_NEL - 1024 only)
#define W4_DUMP_OFF (2 * W4_RAW + 2 * W4_VS)     // where the threads without a halo element store their zeros (dead LDS)
#define W4_DUMP (W4_THREADS + 3 * W4_PLANE)
#define W4_LOOP (W4_DUMP_OFF + W4_DUMP)
#define W4_MSR 68                                // floats per (plane, patch) row of the epilogue's exchange buffer: 64 channels + 4
#define W4_NPL 28                                // planes: rows 0..3 x 4 output columns, rows 4 / 5: 2 halves x 3 partial sums
#define W4_MS (W4_NPL * 16 * W4_MSR)             // one pass = 16 patches
#define W4_BIAS_OFF (W4_LOOP > W4_MS ? W4_LOOP : W4_MS)          // the block's 64 bias values, behind both uses of the LDS
// The halo planes' placement in LDS per sub-tile geometry (lwg_conv_wino.h: Cw4Sub; void: the plain block above).
// Cw4F (16 x 8): the SAME rows of W4_RS = 40 floats - the 18-pixel halo rows of two slots side by side, 20 floats apart, the lower two slots ten rows
// down: a channel plane is 20 rows + 4 (4 PLANE = 16 mod 32 as above).  The patches (pty, ptx 0-3 | 4-7) of a ds_read_b128 lane group start in rows
// 0, 4, 10, 14 = bank quads 0, 8, 4, 12 (+ ptx % 4): sixteen distinct ones.
// Cw4Q (8 x 8): eight 10 x 10 sub-planes per channel plane in rows of Cw4QLds::RS floats (Cw4QLds has the layout and its bank-quad rule), FOUR halo
// pieces per thread and stage (a slot's 200 elements = four rounds of its wave)
template <typename G> struct W4Lds { static constexpr int RS = W4_RS, PLN = W4_PLANE; };
template <> struct W4Lds<Cw4F> {
    static constexpr int RS = W4_RS, PLN = Cw4F::NS / Cw4F::NSX * Cw4F::HH * W4_RS + 4;
    CW_FN int slot(int s) { return (s / Cw4F::NSX) * Cw4F::HH * W4_RS + (s % Cw4F::NSX) * (W4_RS / Cw4F::NSX); }
};
template <> struct W4Lds<Cw4Q> : Cw4QLds {};
// the block's 64 bias values, behind both uses of the LDS (the K loop's buffers as W4_LOOP counts them | the exchange buffer), in floats
template <typename G> constexpr int w4_loop = (2 * W4_KS + 3) * W4Lds<G>::PLN + 2 * W4_VS + W4_THREADS;
template <typename G> constexpr int w4_bias_off = w4_loop<G> > W4_MS ? w4_loop<G> : W4_MS;
static_assert(w4_bias_off<void> == W4_BIAS_OFF && W4_RS / Cw4F::NSX >= Cw4F::HW && (W4_RS / Cw4F::NSX) % 4 == 0 && W4Lds<Cw4F>::PLN >= W4_PLANE, "two sub-tile halo rows per LDS row");
static_assert(Cw4F::SX == 16 && Cw4F::SY == 8 && Cw4F::NS * Cw4F::ROUNDS * 64 == W4_NQ * W4_THREADS, "sub-tile halo: four slots x six wave rounds = the staged elements");
static_assert(Cw4Q::NS == 8 && Cw4Q::ROUNDS == 4 && Cw4QLds::RS % 4 == 0 && Cw4QLds::RS >= 16 + Cw4Q::HW && (w4_bias_off<Cw4Q> + 64) * 4 <= 160 * 1024, "8 x 8 sub-tile halo: one slot per wave, inside the LDS");
#ifndef LWG_W4_XCD
#define LWG_W4_XCD 1         // XCD-aware block order (see the kernel): 0 = off (lab)
#endif
#ifndef LWG_W4_CHUNK
#define LWG_W4_CHUNK 1       // block order: 1 = chunks of gridDim.x tiles through every column block where the panel fits L2, 2 = always, 0 = never (lab)
#endif
#ifndef LWG_W4_RDMAP
#define LWG_W4_RDMAP 1       // epilogue reader lanes mapped to the ds_read_b128 lane groups (lab: 0 = lane order)
#endif
#ifndef LWG_W4_SMALL
#define LWG_W4_SMALL 1       // the 4-wave form for small launches (lab: 0 = off)
#endif
#define W4SB() __builtin_amdgcn_sched_barrier(0)

// lab instrumentation (compiled out of the product): tools/wino4lab.py --ts on a -DLWG_W4_TS variant library; wave 0 stamps into args->res (LWG_EPI_NONE)
#ifdef LWG_W4_TS
#define W4TS(i) do { if (tid == 0 && lab_bi == 1) reinterpret_cast<unsigned long long*>(const_cast<float*>(a.res))[(size_t)blockIdx.x * 16 + (i)] = __builtin_readcyclecounter(); } while (0)
#define W4TSA(i) do { if (tid == 0) reinterpret_cast<unsigned long long*>(const_cast<float*>(a.res))[(size_t)blockIdx.x * 16 + (i)] = __builtin_readcyclecounter(); } while (0)
#else
#define W4TS(i) do { } while (0)
#define W4TSA(i) do { } while (0)
#endif

#ifndef W4_NT
#define W4_NT 0              // cache policy of the activation traffic (halo loads, output stores): 0 = default; 2 = non-temporal: measured 20 % SLOWER (profiles/r06_w_*)
#endif
#ifndef W4_NT_LD
#define W4_NT_LD W4_NT       // ... of the halo loads alone
#endif
#ifndef W4_NT_RES
#define W4_NT_RES 0          // ... of the epilogue's residual / xn loads (read once per launch)
#endif
#ifndef W4_NT_ST
#define W4_NT_ST 2           // ... of the output stores alone: NON-TEMPORAL - the block's 128 KB of outputs are not read again by this launch and otherwise push
                             // panel and halo lines out of the XCD's L2: +0.4-0.6 % in the step (A/B/A/B and five policies, profiles/r06_ay_*; the halo LOADS
                             // non-temporal were the 20 % loss of r06_w)
#endif

// the 1-D input transform B^T (.) of six values
__device__ __forceinline__ void w4_bt6(const float (&r)[6], float (&v)[6]) {
    const float a = __builtin_fmaf(-4.f, r[2], r[4]), b = __builtin_fmaf(-4.f, r[1], r[3]);
    const float c = r[4] - r[2], e = r[3] - r[1];
    v[0] = __builtin_fmaf(-5.f, r[2], __builtin_fmaf(4.f, r[0], r[4]));
    v[1] = a + b;
    v[2] = a - b;
    v[3] = __builtin_fmaf(2.f, e, c);
    v[4] = __builtin_fmaf(-2.f, e, c);
    v[5] = __builtin_fmaf(-5.f, r[3], __builtin_fmaf(4.f, r[1], r[5]));
}

// SM (small launches - a frame or two -, every epilogue): 256 threads = the four waves q = 0..3 of ONE 32-channel tile - block = the same 32 patches x
// 32 channels: twice the workgroups (one wave per SIMD: the 36 MFMAs of a wave and stage run unshared), every thread forms BOTH halves of its (patch, channel)
// transform and stages five halo pieces.  Every output element is accumulated over the stages and k-pairs in the same order and finished by the same
// expressions in both forms (the transform, the folds and the reader are explicit fma / add sequences): bitwise the same result - a frame does not depend on
// its batch (check_winograd4: frame n of a 40-frame launch = the frame alone, across the forms).
// The SPADE modulation and the activation of sixteen outputs: what the epilogue and the light-tile loop of the list-driven form both apply
__device__ __forceinline__ float w4_spade_mod(float x, float mu, float rs, float gam, float bet) { return (x - mu) * rs * (1.f + gam) + bet; }
// (the activation resolved once per sixteen values - lwg_common.h; around the whole output pass the four copies of the pass cost registers:
// 40-90 spilled, their reloads between the stores each waiting for every store before them)
template <int NR>
__device__ __forceinline__ void w4_act16(int act, floatx4 (&o)[NR]) {
    lwg_act_dispatch(act, [&](auto ACTC) {
        constexpr int EA = decltype(ACTC)::value;
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) o[i][c] = lwg_act_c<EA>(o[i][c], act);
    });
}

// LIST (lwg_conv2d_winograd4_list_f32; 8-wave form, LWG_EPI_NONE / LWG_EPI_SPADE, one input): the workgroup's blocks come from two tile lists in device
// memory (lwg_conv_wino.h: cw_list_entry) - the heavy entries through the K loop and epilogue below, untouched, then the light ones from the calibration
// frame in a streaming loop without LDS.  Heavy first: a static walk that mixed them would leave most workgroups waiting for the few
// that drew the heavy blocks of a clustered body.
// GEO (the lists' granularity; void: 32 x 16 blocks, or no lists.  SUB = not void, always a LIST form): the lists hold the sub-tiles of one geometry
// (lwg_conv_wino.h: Cw4Sub); a workgroup's "block" is a GROUP of NS heavy sub-tiles - any frames, any positions - in the NS slots of its 4 x 8 patches
// (slot_of_patch).  Only the halo staging (NS sub-planes per channel plane, a wave stages the halo of one slot = one image descriptor), the transform's
// base addresses and the epilogue's output bases (the reader's slot is wave-uniform per pass) differ; the K loop is the same code.
//   FINE = Cw4F (lwg_conv2d_winograd4_fine_f32): 16 x 8 sub-tiles, a group = four of them in four slots of 4 x 2 patches; waves 2 s, 2 s + 1 stage slot s.
//   Q8 = Cw4Q (lwg_conv2d_winograd4_q8_f32): 8 x 8 sub-tiles, a group = EIGHT in the eight slots of 2 x 2 patches; wave w stages slot w.  Besides what
// differs in FINE, the epilogue's reader lanes are mapped so that a wave's patches of a pass are ONE slot's (cw4_reader8: its half waves take two output
// columns instead of two patch columns) - the same loads, sums and stores per output element.
// SPLIT (lwg_conv2d_winograd4_f32_ws: the training step's one-sample launches; the 4-wave form, plain epilogue): ONE block per workgroup, blockIdx.z owns
// the K stages [z a.cshift, (z + 1) a.cshift) of it (lwg_conv_wino.h: cw4_slice_begin / _end; an even number of them) and writes its raw partial outputs -
// behind the output transform - to slab z of the workspace, a.y + z M N (the host passes YC = N, ycoff = 0, no bias, no activation): the slab goes into
// the BASE of the block's image buffer, the stores' offsets are the whole launch's.  The K loop is the same code on absolute stage indices; the panel's
// strides stay the layer's.  lwg_splitk_finish_kernel adds the slabs in slice order and finishes.
template <int EPI, bool TWO, bool SM, bool LIST, typename GEO = void, bool SPLIT = false>
__device__ __forceinline__ void w4_body(const LwgConvArgs& a, const LwgConvLists& sk) {
    constexpr bool SUB = !std::is_void<GEO>::value, FINE = std::is_same<GEO, Cw4F>::value, Q8 = std::is_same<GEO, Cw4Q>::value;
    using G = std::conditional_t<SUB, GEO, Cw4F>;            // the sub-tile geometry (named under SUB only)
    using L = W4Lds<GEO>;                                    // the halo planes' geometry in LDS
    static_assert(!SUB || (LIST && !SM && !TWO && !SPLIT && LWG_W4_RDMAP), "the sub-tile forms: a list-driven 8-wave launch");
    static_assert(!SPLIT || (SM && !LIST && EPI == LWG_EPI_NONE), "the split form: 4-wave blocks, plain epilogue");
    constexpr int RS = L::RS, PLANE = L::PLN;
    constexpr int RAW = W4_KS * PLANE;
    constexpr int DUMP_OFF = 2 * RAW + 2 * W4_VS;
    constexpr int BIAS_OFF = w4_bias_off<GEO>;
    constexpr bool SMS = SM && EPI == LWG_EPI_SPADE;          // (its 32 accumulator rows: gamma | beta of the SAME 16 channels, cw4_n0_spade_small)
    constexpr int NVP = SM && !SMS ? 2 : 1;                  // patches per reader thread and pass
    constexpr int NTH = SM ? 256 : W4_THREADS;               // threads per workgroup
    constexpr int NQ = SM ? 5 : W4_NQ + (Q8 ? G::ROUNDS - W4_NQ : 0); // halo pieces per thread and stage
    constexpr int NBV = SM ? 32 : W4_NB;                     // output channels per block
    constexpr int MSR = SM ? 36 : W4_MSR;                    // floats per (plane, patch) row of the exchange buffer
    constexpr int NHF = SM ? 2 : 1;                          // halves of the input transform per thread
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float* __restrict__ bias = a.bias;
    const int H = a.H, W = a.W, Cin = a.C0 + a.C1, N = a.N;
    float* __restrict__ y = SPLIT ? a.y + cw4_slab_offset((int)blockIdx.z, a.M, N) : a.y;
    float* const raw0 = smem;                                // [2][RAW], then [2][VS]
    float* const Ms = smem;                                  // the epilogue's exchange buffer (after the K loop)
    const int tid = threadIdx.x, lane = tid & 63;
    // persistent workgroups (as conv_winograd.hip): min(blocks, CUs) workgroups walk the block ids blockIdx.x + k gridDim.x in one of three block
    // orders - XCD-aware, chunked, column-block-major (lwg_conv_wino.h: cw4_order_kind)
    const CwGrid g = cw_grid(a.B, H, W, N, 4 * W4_PBX, 4 * W4_PBY, NBV);
    const CwOrder o = cw_order(cw4_order_kind(LWG_W4_XCD, LWG_W4_CHUNK, SM, gridDim.x, N / NBV, Cin, N, g.tiles, g.total), gridDim.x, blockIdx.x, N / NBV, g);
    int blk = blockIdx.x;
    // LIST: the heavy entries' number (the ids below it run the K loop); a workgroup may own none
    // (counts and tile ids are clamped to the launch's grid: lists that do not belong to this launch must not become addresses)
    // (SUB: the entries are sub-tiles, nhe counts their groups)
    const int nall = SUB ? G::in_image_total(a.B, H, W) : g.tiles;
    const int nht = LIST ? min(max(__builtin_amdgcn_readfirstlane(sk.counts[0]), 0), nall) : 0;
    const int nhe = (SUB ? G::groups(nht) : nht) * (N / NBV);
    // a launch whose tiles are ALL heavy (a frame batch without background) walks its blocks in the plain entry point's order - decided here, on the
    // device: the list order costs such a launch 0.3-3 % (profiles/spade_skip_ab_tool_list_order.txt)
    // (SUB: the entry point's second kernel runs the plain body for such a launch - this body always walks its lists)
    const bool lst = SUB ? true : LIST ? nht < nall : false;
    const bool run = lst ? blk < nhe : true;
    const int nst = Cin / W4_KS;                             // even (host: Cin % 16 == 0)
    const int sbeg = SPLIT ? cw4_slice_begin((int)blockIdx.z, a.cshift) : 0;       // this workgroup's stages [sbeg, send): the layer's, or its slice
    const int send = SPLIT ? cw4_slice_end((int)blockIdx.z, a.cshift, nst) : nst;
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, (int)(144u * (unsigned)Cin * (unsigned)N), 0x00020000);
    const int q = wid & 3, ct = SM ? 0 : wid >> 2;           // this wave's product set and 32-channel tile
    const int half = SM ? 0 : wid >> 2;                      // ... and its half of the input transform (rows 3 half .. 3 half + 2 of B^T d B; SM: both)
    floatx16 acc[9];                                         // products 0..5: (xi = q, nu); 6..8: (xi = 4 + q / 2, nu = 3 (q % 2) + 0..2)
    CwBlock<NQ, TWO> bk;                                     // the per-block state (lwg_conv_wino.h), this thread's NQ halo offsets in it
    unsigned uvoff, uvoffc;                                  // this lane's column of the fragment panel: the 16-byte parts, the ninth product
    int fs0 = 0, fs1 = 0;                                    // SUB: the sub-tiles of this wave's reader patches, passes 0 | 1 (-1: an empty slot)
    auto setup = [&](int id) {
        int cb, t;
        if constexpr (SUB) {
            int tids = tid;
            asm volatile("" : "+v"(tids));
            int slot;
            cw_list_entry(id, N / NBV, slot, cb);
            auto sub = [&](int k) {                          // the group's sub-tile in slot k (wave-uniform), -1: an empty slot
                const int ix = G::slot_index(slot, k, nht);
                return ix < 0 ? -1 : min(max(__builtin_amdgcn_readfirstlane(sk.heavy[ix]), 0), G::NS * g.tiles - 1);
            };
            bk.n0 = cw_n0(cb, NBV);
            // a wave stages the halo of ONE slot (cw4_halo_elem: slot wid / 2 | wid) - one image descriptor.  FINE reads the whole group once: the three
            // slots a wave needs are selected from registers
            int fsub[FINE ? G::NS : 1], u;
            if constexpr (FINE) {
#pragma unroll
                for (int k = 0; k < G::NS; ++k) fsub[k] = sub(k);
                const int hs = wid >> 1;
                u = hs == 0 ? fsub[0] : hs == 1 ? fsub[1] : hs == 2 ? fsub[2] : fsub[3];
            } else {
                u = sub(wid);
            }
            int b, x0, y0;
            G::corner(g, max(u, 0), b, x0, y0);
            bk.rx0 = cw_image_rsrc(a.x0, __builtin_amdgcn_readfirstlane(b), H, W, a.C0, 4u);
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                int s, j;
                cw4_halo_elem(G{}, tids + NTH * k, s, j);
                bk.voff0[k] = G::halo_voff(u >= 0, j, x0, y0, H, W, a.C0);
            }
            // the epilogue's slots of this wave, passes ph = 0 | 1.  FINE: the pass reads patch rows 2 ph, 2 ph + 1, this wave the columns 4 (wid / 4) .. + 3 -
            // slot 2 ph + wid / 4.  Q8 (cw4_reader8): slot 4 ph + wid / 2
            if constexpr (FINE) fs0 = (wid >> 2) ? fsub[1] : fsub[0], fs1 = (wid >> 2) ? fsub[G::NSX + 1] : fsub[G::NSX];
            else fs0 = sub(wid >> 1), fs1 = sub(G::NSX + (wid >> 1));
        } else if constexpr (LIST) {
            if (lst) {
                int slot;
                cw_list_entry(id, N / NBV, slot, cb);
                t = min(max(__builtin_amdgcn_readfirstlane(sk.heavy[slot]), 0), g.tiles - 1);
            } else {
                cw_block(o, id, cb, t);
            }
        } else {
            cw_block(o, id, cb, t);
        }
        if constexpr (!SUB) {
        bk.locate(a, g, t, 4 * W4_PBX, 4 * W4_PBY, SMS ? cw4_n0_spade_small(cb) : cw_n0(cb, NBV));
        int tids = tid;                                      // (through an empty asm: the halo geometry is recomputed per block - hoisted out of the block
        asm volatile("" : "+v"(tids));                       //  loop it would sit in registers through the K loop)
        bk.halo(a, tids, NTH, W4_HW, W4_NEL);
        }
        const int col = SMS ? bk.n0 + (((lane & 31) >> 4) << 5) + (lane & 15) : bk.n0 + ct * 32 + (lane & 31);      // this lane's accumulator row = panel column
        uvoff = (unsigned)(((lane >> 5) * 9 * N + 4 * col) * 4);
        uvoffc = (unsigned)(((lane >> 5) * 9 * N + 8 * N + col) * 4);
    };
    if (run) setup(blk);
    int wst[NQ];                                             // the halo elements' LDS slot
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const int i = tid + NTH * k;
        if constexpr (SUB) {
            int s, j, hy, hx, hq;
            cw4_halo_elem(G{}, i, s, j);
            G::halo_place(j, hy, hx, hq);
            wst[k] = j < G::NEL ? 4 * hq * PLANE + L::slot(s) + hy * RS + hx : DUMP_OFF + tid;
        } else {
        const int pix = i >> 1, hq = i & 1, hy = pix / W4_HW, hx = pix - hy * W4_HW;
        wst[k] = i < W4_NEL ? 4 * hq * PLANE + hy * RS + hx : DUMP_OFF + tid;
        }
    }
    floatx4 rreg[NQ];
    auto rld1 = [&](int st, int k) -> floatx4 {              // a stage's 8 channels lie in ONE input (C0 % 8 == 0)
#ifdef W4_LAB_HFIX            // lab: every halo load reads stage 0
        const int c = 0 * st;
#else
        const int c = st * W4_KS;
#endif
        return bk.template rld1<W4_NT_LD>(a, c, k);
    };
    auto rst1 = [&](int buf, int k, floatx4 v) { cw_rst1(raw0 + buf * RAW + wst[k], PLANE, v); };
    // weights: lane = (k-half lane / 32, channel lane % 32); element (q, stage, k-pair, k-half) = 9 N floats: [N][4] products 0-3, [N][4] products 4-7, [N] product 8 -
    // every load instruction reads contiguous memory (32 lanes x 16 bytes), nothing is padding
    floatx4 ufa[4], ufb[4];                                  // [register set = k-pair]: loaded TWO k-pairs ahead
    float ufc[4];
    const unsigned ukk = (unsigned)N * 72u;                  // bytes between two k-pairs: [2][9 N] floats
    const unsigned uq = (unsigned)q * (unsigned)nst * 4u * ukk;
    const unsigned ubo = (unsigned)N * 16u;                  // bytes from part A to part B
    auto uldpart = [&](int set, int st, int kk, int part) {  // part 0 | 1 | 2: products 0-3 | 4-7 | 8
#ifdef W4_LAB_UFIX
        const unsigned so = uq + 0u * (unsigned)(st + kk);
#else
        const unsigned so = uq + (unsigned)(st * 4 + kk) * ukk;
#endif
        if (part == 0) ufa[set] = cw_buf_load(ru, uvoff, so);
        else if (part == 1) ufb[set] = cw_buf_load(ru, uvoff, so + ubo);
        else ufc[set] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ru, (int)uvoffc, (int)so, 0));
    };
    auto uldset = [&](int set, int st, int kk) {
#ifdef W4_LAB_UFIX            // lab: every weight load reads k-pair 0 of stage 0 (cache-hot: the loads' issue / wait mechanics without the memory system behind them)
        const unsigned so = uq + 0u * (unsigned)(st + kk);
#else
        const unsigned so = uq + (unsigned)(st * 4 + kk) * ukk;
#endif
        ufa[set] = cw_buf_load(ru, uvoff, so);
        ufb[set] = cw_buf_load(ru, uvoff, so + ubo);
        ufc[set] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ru, (int)uvoffc, (int)so, 0));
    };
    // the input transform's thread: patch tid % 32, channel (tid / 32) % 8, rows 3 half .. 3 half + 2
    const int patch = tid & 31, tc = (tid >> 5) & 7;
    const int pty = patch >> 3, ptx = patch & 7;
    int pby = pty, pbx = ptx, pslot = 0;                     // SUB: the patch's 6 x 6 window inside its slot's sub-plane
    if constexpr (FINE) {
        G::patch_in_slot(pty, ptx, pby, pbx);
        pslot = L::slot(G::slot_of_patch(pty, ptx));
    }
    if constexpr (Q8) pby = 0, pbx = 0, pslot = L::patch(pty, ptx);
    unsigned dbs = (unsigned)(tc * PLANE + pslot + (4 * pby) * RS + 4 * pbx) >> 2;      // its 6 x 6 input patch inside raw[0] (float index; 16-byte aligned)
    asm volatile("" : "+v"(dbs));
    dbs <<= 2;
    // per half hf of the transform (this thread's one - index 0 - or, SM, both): the rows of X start at row hf; its 18 transformed values inside Vs[0]:
    // row X (xi = 0 | 5) and rows T+, T- (xi = 1, 2 | 3, 4); alpha, beta (wave-uniform: scalar operands)
    unsigned dbx[NHF], vbx[NHF], vbt[NHF];
    float alpha[NHF], beta[NHF], nbeta[NHF];
#pragma unroll
    for (int hi = 0; hi < NHF; ++hi) {
        const int hf = SM ? hi : half;
        dbx[hi] = (unsigned)(tc * PLANE + pslot + (4 * pby + hf) * RS + 4 * pbx) >> 2;
        asm volatile("" : "+v"(dbx[hi]));
        dbx[hi] <<= 2;
        vbx[hi] = (unsigned)(2 * RAW + (hf ? 30 : 0) * W4_KS * 32 + tc * 32 + patch);
        vbt[hi] = (unsigned)(2 * RAW + (hf ? 18 : 6) * W4_KS * 32 + tc * 32 + patch);
        asm volatile("" : "+v"(vbx[hi]));
        asm volatile("" : "+v"(vbt[hi]));
        alpha[hi] = hf ? -1.f : -4.f;
        beta[hi] = hf ? 2.f : 1.f;
        nbeta[hi] = -beta[hi];
    }
    unsigned fbs[2];                                         // this lane's fragments: products 0..5 | 6..8, inside Vs[0]
    fbs[0] = (unsigned)(2 * RAW + (6 * q) * W4_KS * 32 + lane);
    fbs[1] = (unsigned)(2 * RAW + (6 * (4 + (q >> 1)) + 3 * (q & 1)) * W4_KS * 32 + lane);
    asm volatile("" : "+v"(fbs[0]));
    asm volatile("" : "+v"(fbs[1]));
    float fb[9];                                             // the current k-pair's nine fragments (each refilled right behind its MFMA)
    auto frag1 = [&](int buf, int kk, int j) -> float {
        return smem[fbs[j < 6 ? 0 : 1] + buf * W4_VS + ((j < 6 ? j : j - 6) * W4_KS + 2 * kk) * 32];
    };
    auto rd6 = [&](unsigned base, int buf, int r, float (&d)[6]) {     // row r (from the base's row) of this thread's patch in raw[buf]
        const floatx4 v4 = *reinterpret_cast<const floatx4*>(smem + base + buf * RAW + r * RS);
        const float2 v2 = *reinterpret_cast<const float2*>(smem + base + buf * RAW + r * RS + 4);
        d[0] = v4[0]; d[1] = v4[1]; d[2] = v4[2]; d[3] = v4[3]; d[4] = v2.x; d[5] = v2.y;
    };
    auto vst6 = [&](unsigned base, int buf, int i, const float (&v)[6]) {   // six values of a row of V -> Vs[buf], row i behind the base's
        float* dst = smem + base + buf * W4_VS + (6 * i) * W4_KS * 32;
#pragma unroll
        for (int nu = 0; nu < 6; ++nu) dst[nu * W4_KS * 32] = v[nu];
    };
    // column pass of the transform, the SAME instructions in both halves (no branches, one copy of the K loop):
    //   X  = 4 dx0 - 5 dx1 + dx2 over the rows (half, half + 2, half + 4)           = t0 | t5
    //   P  = d4 + alpha d2, Q = d3 + alpha d1 (alpha = -4 | -1); T+ = P + beta Q, T- = P - beta Q (beta = 1 | 2)   = t1, t2 | t3, t4
    auto transform_full = [&](int buf) {                     // prologue only
#pragma unroll
        for (int hi = 0; hi < NHF; ++hi) {
            float X[6], P[6], Q[6], v[6];
            {
                float dR[3][6];
                rd6(dbx[hi], buf, 0, dR[0]); rd6(dbx[hi], buf, 2, dR[1]); rd6(dbx[hi], buf, 4, dR[2]);
#pragma unroll
                for (int j = 0; j < 6; ++j) X[j] = __builtin_fmaf(-5.f, dR[1][j], __builtin_fmaf(4.f, dR[0][j], dR[2][j]));
            }
            {
                float dR[2][6];
                rd6(dbs, buf, 2, dR[0]); rd6(dbs, buf, 4, dR[1]);
#pragma unroll
                for (int j = 0; j < 6; ++j) P[j] = __builtin_fmaf(alpha[hi], dR[0][j], dR[1][j]);
                rd6(dbs, buf, 1, dR[0]); rd6(dbs, buf, 3, dR[1]);
#pragma unroll
                for (int j = 0; j < 6; ++j) Q[j] = __builtin_fmaf(alpha[hi], dR[0][j], dR[1][j]);
            }
            w4_bt6(X, v); vst6(vbx[hi], buf, 0, v);
            float T[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) T[j] = __builtin_fmaf(beta[hi], Q[j], P[j]);
            w4_bt6(T, v); vst6(vbt[hi], buf, 0, v);
#pragma unroll
            for (int j = 0; j < 6; ++j) T[j] = __builtin_fmaf(nbeta[hi], Q[j], P[j]);
            w4_bt6(T, v); vst6(vbt[hi], buf, 1, v);
        }
    };
    auto iteration = [&](int s, auto SET, auto NXT) {
        constexpr int set = decltype(SET)::value;            // s % 2
        constexpr bool nxt = decltype(NXT)::value != 0;      // the last stage has no next one to prepare (peeled: no branches in the loop)
        const int s3 = s + 3 < send ? s + 3 : send - 1;      // past the end: a harmless re-load of the last stage (its halo store lands in a dead buffer)
        float X[6], P[6], Q[6], dR[3][6];
        auto mf = [&](int kk, int j, bool refill) {          // product j of k-pair kk; then its register takes the fragment of the next k-pair
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(j < 4 ? ufa[kk][j & 3] : j < 8 ? ufb[kk][j & 3] : ufc[kk], fb[j], acc[j], 0, 0, 0);
#ifndef W4_KO_FRAG
            // (two fragments per LDS instruction: products j - 1 and j lie 1 KB apart - ds_read2st64_b32 -, refilled behind the second one's MFMA)
            if (refill && (j & 1)) {
                fb[j - 1] = kk < 3 ? frag1(set, kk + 1, j - 1) : frag1(set ^ 1, 0, j - 1);
                fb[j] = kk < 3 ? frag1(set, kk + 1, j) : frag1(set ^ 1, 0, j);
            } else if (refill && j == 8) {
                fb[8] = kk < 3 ? frag1(set, kk + 1, 8) : frag1(set ^ 1, 0, 8);
            }
#endif
            W4SB();
        };
        auto ul = [&](int kk, int part) {                    // ONE load of them
#ifndef W4_KO_ULD
            if (kk < 2) uldpart(kk + 2, s, kk + 2, part);
            else if (nxt) uldpart(kk - 2, s + 1, kk - 2, part);
#endif
            W4SB();
        };
        auto halo = [&](int k) {                             // the halo of stage s + 2 -> raw[s % 2], the loads of stage s + 3
#ifdef W4_KO_HALO
            return;
#endif
            if (nxt) { rst1(set, k, rreg[k]); rreg[k] = rld1(s3, k); }
            W4SB();
        };
#ifdef W4_KO_TR
        constexpr bool trn = false;
#else
        constexpr bool trn = nxt;
#endif
        // the next stage's transform in fourteen steps per half: 0-2 the rows of X, 3-4 X, 5-6 rows 2 / 4, 7 X's row of V, 8 P, 9-10 rows 1 / 3, 11 Q, 12-13 the rows T+ / T-
        auto tr = [&](int hi, int step) {
            if (trn) {
                if (step < 3) rd6(dbx[hi], set ^ 1, 2 * step, dR[step]);
                else if (step < 5) {
#pragma unroll
                    for (int j = 3 * (step - 3); j < 3 * (step - 3) + 3; ++j) X[j] = __builtin_fmaf(-5.f, dR[1][j], __builtin_fmaf(4.f, dR[0][j], dR[2][j]));
                } else if (step < 7) rd6(dbs, set ^ 1, 2 * (step - 5) + 2, dR[step - 5]);
                else if (step == 7) {
                    float v[6];
                    w4_bt6(X, v);
                    vst6(vbx[hi], set ^ 1, 0, v);
                } else if (step == 8) {
#pragma unroll
                    for (int j = 0; j < 6; ++j) P[j] = __builtin_fmaf(alpha[hi], dR[0][j], dR[1][j]);
                } else if (step < 11) rd6(dbs, set ^ 1, 2 * (step - 9) + 1, dR[step - 9]);
                else if (step == 11) {
#pragma unroll
                    for (int j = 0; j < 6; ++j) Q[j] = __builtin_fmaf(alpha[hi], dR[0][j], dR[1][j]);
                } else {
                    float T[6], v[6];
#pragma unroll
                    for (int j = 0; j < 6; ++j) T[j] = __builtin_fmaf(step == 12 ? beta[hi] : nbeta[hi], Q[j], P[j]);
                    w4_bt6(T, v);
                    vst6(vbt[hi], set ^ 1, step - 12, v);
                }
            }
            W4SB();
        };
        // Slot plan: the stage's fifteen loads (twelve weight parts two k-pairs ahead, three halo pieces a stage ahead) ONE per MFMA slot - requested in
        // bursts (six weight loads at the top of a k-pair, by eight waves at once) the memory pipeline's queue fills and the wave stalls in front of its
        // next MFMA (profiles/r06_z_*: with every load cache-hot the K loop still lost 20 % to its fillers; the transform and the fragment reads cost 1 % each)
        if constexpr (!SM) {
            // k-pair 0: the halo of stage s + 2 -> raw[s % 2], the loads of stage s + 3; the rows of X of the next stage's patch
            mf(0, 0, true); ul(0, 0);
            mf(0, 1, true); halo(0);
            mf(0, 2, true); ul(0, 1); tr(0, 0);
            mf(0, 3, true); halo(1); tr(0, 1);
            mf(0, 4, true); ul(0, 2); tr(0, 2);
            mf(0, 5, true); halo(2);
            mf(0, 6, true); tr(0, 3);
            if constexpr (Q8) halo(3);                       // (the fourth piece: lanes 0-7 of every wave)
            mf(0, 7, true); tr(0, 4);
            mf(0, 8, true); tr(0, 5);
            // k-pair 1: the rest of the column pass, the row pass
            mf(1, 0, true); ul(1, 0); tr(0, 6);
            mf(1, 1, true); tr(0, 7);
            mf(1, 2, true); ul(1, 1); tr(0, 8); tr(0, 9);
            mf(1, 3, true); tr(0, 10);
            mf(1, 4, true); ul(1, 2);
            mf(1, 5, true); tr(0, 11);
            mf(1, 6, true); tr(0, 12);
            mf(1, 7, true);
            mf(1, 8, true); tr(0, 13);
            // k-pair 2
            mf(2, 0, true); ul(2, 0);
            mf(2, 1, true);
            mf(2, 2, true); ul(2, 1);
            mf(2, 3, true);
            mf(2, 4, true); ul(2, 2);
            mf(2, 5, true); mf(2, 6, true); mf(2, 7, true); mf(2, 8, true);
        } else {
            // the small form: five halo pieces and both halves of the transform per thread in front of the barrier
            mf(0, 0, true); ul(0, 0); halo(0);
            mf(0, 1, true); tr(0, 0);
            mf(0, 2, true); ul(0, 1); tr(0, 1);
            mf(0, 3, true); halo(1); tr(0, 2);
            mf(0, 4, true); ul(0, 2); tr(0, 3);
            mf(0, 5, true); halo(2); tr(0, 4);
            mf(0, 6, true); tr(0, 5);
            mf(0, 7, true); halo(3); tr(0, 6);
            mf(0, 8, true); tr(0, 7);
            mf(1, 0, true); ul(1, 0); tr(0, 8); tr(0, 9);
            mf(1, 1, true); halo(4); tr(0, 10);
            mf(1, 2, true); ul(1, 1); tr(0, 11);
            mf(1, 3, true); tr(0, 12);
            mf(1, 4, true); ul(1, 2); tr(0, 13);
            mf(1, 5, true); tr(1, 0);
            mf(1, 6, true); tr(1, 1);
            mf(1, 7, true); tr(1, 2);
            mf(1, 8, true); tr(1, 3);
            mf(2, 0, true); ul(2, 0); tr(1, 4);
            mf(2, 1, true); tr(1, 5);
            mf(2, 2, true); ul(2, 1); tr(1, 6);
            mf(2, 3, true); tr(1, 7);
            mf(2, 4, true); ul(2, 2); tr(1, 8); tr(1, 9);
            mf(2, 5, true); tr(1, 10);
            mf(2, 6, true); tr(1, 11);
            mf(2, 7, true); tr(1, 12);
            mf(2, 8, true); tr(1, 13);
        }
        // k-pair 3: behind the stage's barrier (the refills read the NEXT stage's fragments)
        __syncthreads();
        W4SB();
        mf(3, 0, nxt); ul(3, 0);
        mf(3, 1, nxt);
        mf(3, 2, nxt); ul(3, 1);
        mf(3, 3, nxt);
        mf(3, 4, nxt); ul(3, 2);
        mf(3, 5, nxt); mf(3, 6, nxt); mf(3, 7, nxt); mf(3, 8, nxt);
    };

    // prologue loads of a block: stages 0 and 1 (-> raw[0], raw[1]), stage 2's halo (kept in registers), the first two k-pairs' weights - requested here for
    // the workgroup's first block, for every later one from inside the previous block's epilogue (SPLIT: the slice's first stages - sbeg + 0, 1, 2)
    floatx4 r0[NQ], r1[NQ];
    float bq;                                                // the block's bias, one value per lane of wave 0: requested with the first loads, parked in LDS by the prologue
    auto issue_loads = [&]() {
        bq = bias ? bias[SMS ? bk.n0 + (((tid & 31) >> 4) << 5) + (tid & 15) : bk.n0 + (tid & (NBV - 1))] : 0.f;
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            r0[k] = rld1(sbeg, k);
            r1[k] = rld1(sbeg + 1, k);
        }
        uldset(0, sbeg, 0);
        uldset(1, sbeg, 1);
#pragma unroll
        for (int k = 0; k < NQ; ++k) rreg[k] = rld1(send - sbeg > 2 ? sbeg + 2 : sbeg + 1, k);
    };
    if (run) issue_loads();
#ifdef LWG_W4_TS
    int lab_bi = 0;
#endif
    W4TSA(11);
    if (run) for (;;) {
    W4TS(0);
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        rst1(0, k, r0[k]);
        rst1(1, k, r1[k]);
    }
    if (tid < NBV) smem[BIAS_OFF + tid] = bq;
    __syncthreads();
    transform_full(0);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 9; ++j) fb[j] = frag1(0, 0, j);
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    // the bias for free: A^T m = (1, 1, 1, 1) for m = (0, 1, 0, 0, 0, 0), so a constant c added to product (xi, nu) = (1, 1) of every patch adds c to all
    // sixteen outputs - the accumulator of that product starts at the bias of its channel (rows = channels) instead of zero
    if (q == 1) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const floatx4 b4 = *reinterpret_cast<const floatx4*>(smem + BIAS_OFF + ct * 32 + 8 * g + 4 * (lane >> 5));
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[1][4 * g + k] = b4[k];
        }
    }
    W4TS(1);
    {
        int s = sbeg;
        for (; s + 2 < send; s += 2) {
            iteration(s, IntC<0>(), IntC<1>());
            iteration(s + 1, IntC<1>(), IntC<1>());
        }
        iteration(s, IntC<0>(), IntC<1>());
        iteration(s + 1, IntC<1>(), IntC<0>());
    }
    W4TS(2);
    int eb = SUB ? 0 : bk.b, ex0 = SUB ? 0 : bk.x0, ey0 = SUB ? 0 : bk.y0;     // this block's coordinates (the state moves on to the next block below)
    const int en0 = bk.n0;
    const int es0 = fs0, es1 = fs1;
    // epilogue.  (1) M A in registers: row q -> F[b] (b = 0..3, into acc[0..3]); the half row -> three partial sums (into acc[6..8]):
    //   nu 0..2: a0 = m0 + m1 + m2, a1 = m1 - m2, a2 = m1 + m2;  nu 3..5: b0 = m3 + m4, b1 = m3 - m4, b2 = m5
    //   (F[0] = a0 + b0, F[1] = a1 + 2 b1, F[2] = a2 + 4 b0, F[3] = a1 + 8 b1 + b2: finished by the reader)
    // (2) two passes of 16 patches: the 28 planes cross LDS ([plane][patch][64 channels + 4]: 16-byte stores and loads, conflict-free both ways); a reader
    // thread owns one output column b of one patch x the channel quads n4.. and 32 + n4..: A^T (.) over xi, bias, (residual | SPADE modulation), activation,
    // 16-byte NHWC stores.  LWG_EPI_SPADE: the block's 64 columns are gamma | beta of the SAME 32 channels (as conv_winograd.hip).
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float m0 = acc[0][r], m1 = acc[1][r], m2 = acc[2][r], m3 = acc[3][r], m4 = acc[4][r], m5 = acc[5][r];
        const float s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
        acc[0][r] = (m0 + s12) + s34;
        acc[1][r] = __builtin_fmaf(2.f, d34, d12);
        acc[2][r] = __builtin_fmaf(4.f, s34, s12);
        acc[3][r] = __builtin_fmaf(8.f, d34, d12) + m5;
    }
    if (q & 1) {                                             // (ONE wave-uniform branch around the whole loop)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float h0 = acc[6][r], h1 = acc[7][r];
            acc[6][r] = h0 + h1;
            acc[7][r] = h0 - h1;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float h0 = acc[6][r], h1 = acc[7][r], h2 = acc[8][r];
            acc[6][r] = (h0 + h1) + h2;
            acc[7][r] = h1 - h2;
            acc[8][r] = h1 + h2;
        }
    }
    W4TS(4);
    int tide = tid;                                          // (through an empty asm per block: the epilogue's address arithmetic must not be hoisted out
    asm volatile("" : "+v"(tide));                           //  of the block loop - it would sit in registers through the K loop)
    const int lanee = tide & 63;
    int rb = wid & 3;                                        // reader: output column inside a patch (wave-uniform; Q8: per half wave)
    int p16q = 0;
    if constexpr (Q8) cw4_reader8(wid, lanee, rb, p16q);
    // ... patch inside the pass and channel quad (and 32 + n4).  8-wave form: a ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27} and
    // {4-11, 16-19, 28-31} of either half wave (MI355X_MICROARCH: LDS), and a 16-byte slot of the exchange buffer lies in bank quad (patch + quad) % 16
    // (rows of 68 floats): a group reads the eight quads of patches a and a + 8 - sixteen distinct bank quads (eight lanes per patch in lane order
    // cost 2-3 LDS cycles per group; PMC: 24 % of the kernel's LDS cycles were bank conflicts, profiles/r06_ah_pmc_lds_f32_512.md).
    // SM: patches lanee >> 3 and 8 + lanee >> 3, the block's only 32 channels; SM + SPADE: gamma | beta rows n4 and 16 + n4
    const unsigned l5 = (unsigned)lanee & 31u, gsel = (0x0FF0F00Fu >> l5) & 1u;                    // in the first group of its half wave?
    const int gidx = __builtin_popcount((gsel ? 0x0FF0F00Fu : 0xF00F0FF0u) & ((1u << l5) - 1u));   // its place in the group: 0..15
    const int p16 = Q8 ? p16q : LWG_W4_RDMAP && !SM ? (wid >> 2) * 4 + 2 * (lanee >> 5) + (gsel ? 0 : 1) + 8 * (gidx >> 3) : (wid >> 2) * 8 + (lanee >> 3);
    const int n4 = SMS ? (lanee & 3) * 4 : LWG_W4_RDMAP && !SM ? (gidx & 7) * 4 : (lanee & 7) * 4;
    const int cbase = SMS ? (en0 >> 6) * 32 + ((en0 >> 4) & 1) * 16 : en0 >> 1;       // SPADE: the block's first output channel
    floatx4 mu, rs;
    // image eb of the output (and of res / xn: the output's layout) as ONE buffer: a reader thread's four pixels are 32-bit offsets inside it (out of
    // range: right of / below the image - the hardware drops the store and returns zeros for the load), the second channel group an immediate
    typedef unsigned int w4_u4 __attribute__((ext_vector_type(4)));
    const unsigned img_bytes = (unsigned)(H * W) * (unsigned)a.YC * 4u;
    const float* const esrc = EPI == LWG_EPI_SPADE ? a.xn : EPI == LWG_EPI_RESIDUAL ? a.res : a.y;
    __amdgpu_buffer_rsrc_t ry, re;
    auto eframe = [&]() {                                    // image eb: once per block (SUB: per pass - the slot's image)
        if (EPI == LWG_EPI_SPADE) {
            mu = *reinterpret_cast<const floatx4*>(a.mean + (size_t)eb * a.YC + cbase + n4);
            rs = *reinterpret_cast<const floatx4*>(a.rstd + (size_t)eb * a.YC + cbase + n4);
        }
        ry = __builtin_amdgcn_make_buffer_rsrc(y + (size_t)eb * H * W * a.YC, 0, (int)img_bytes, 0x00020000);
        re = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(esrc) + (size_t)eb * H * W * a.YC, 0, (int)img_bytes, 0x00020000);
    };
    if constexpr (!SUB) eframe();
    const int chan = EPI == LWG_EPI_SPADE ? cbase + n4 : a.ycoff + en0 + n4;
    bool more = false;
    int nblk = blk;
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
        // (pass 0 needs no barrier in front of its writes: the last LDS reads of the K loop - the fragments of its last k-pair - were issued in front of
        // the last stage's barrier; pass 1 waits for the readers of pass 0)
        if (ph == 1) __syncthreads();
        if constexpr (SUB) {
            const int u = ph ? es1 : es0;
            int ub;
            G::corner(g, max(u, 0), ub, ex0, ey0);
            eb = __builtin_amdgcn_readfirstlane(ub);
            if (u < 0) ex0 = W, ey0 = H;                     // an empty slot: every store out of range
            eframe();
        }
        if (((lanee >> 4) & 1) == ph) {
            float* dst = Ms + (lanee & 15) * MSR + ct * 32 + 4 * (lanee >> 5);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int bb = 0; bb < 4; ++bb)
                    *reinterpret_cast<floatx4*>(dst + (4 * q + bb) * 16 * MSR + 8 * g) = floatx4{acc[bb][4 * g], acc[bb][4 * g + 1], acc[bb][4 * g + 2], acc[bb][4 * g + 3]};
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    *reinterpret_cast<floatx4*>(dst + (16 + 3 * q + i) * 16 * MSR + 8 * g) = floatx4{acc[6 + i][4 * g], acc[6 + i][4 * g + 1], acc[6 + i][4 * g + 2], acc[6 + i][4 * g + 3]};
            }
        }
        // this pass's pixels: patch p, output column rb, rows 0..3 (SM: two patches, one channel group)
        unsigned vo[NVP][4];
#pragma unroll
        for (int hp = 0; hp < NVP; ++hp) {
            const int p = ph * 16 + (SMS ? lanee >> 2 : SM ? 8 * hp + (lanee >> 3) : p16);
            const int ox = ex0 + 4 * (SUB ? (p & 7) % (G::SX / 4) : (p & 7)) + rb;
            const int oyb = ey0 + 4 * (SUB ? (p >> 3) % (G::SY / 4) : (p >> 3));
#pragma unroll
            for (int i = 0; i < 4; ++i)
                vo[hp][i] = cw4_out_voff(ox, oyb + i, H, W, a.YC, chan);
        }
        floatx4 ext[2][4];                                   // residual (both channel groups | SM: both patches) | xn (group 0)
        if (EPI != LWG_EPI_NONE) {
#pragma unroll
            for (int h = 0; h < (EPI == LWG_EPI_SPADE ? 1 : 2); ++h)
#pragma unroll
                for (int i = 0; i < 4; ++i) ext[h][i] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(re, (int)cw4_out_group(vo[NVP == 2 ? h : 0][i], h, !SM), 0, W4_NT_RES));
        }
        if (ph == 1) {
            // the next block of this workgroup: its first loads go out here - the accumulators are dead - and land under the second pass's output
            // (unconditional: the last block re-requests its own first stages, nobody waits for them; see conv_winograd.hip)
            W4TS(8);
            if constexpr (!SPLIT) {                          // (a split launch's workgroup has one block)
            nblk = blk + (int)gridDim.x;
            if constexpr (SUB) more = nblk < nhe;
            else if constexpr (LIST) more = lst ? nblk < nhe : cw_has_block(o, nblk);
            else more = cw_has_block(o, nblk);
            setup(more ? nblk : blk);
            W4TS(9);
            issue_loads();
            W4TS(10);
            }
        }
        __syncthreads();
        if (ph == 0) W4TS(5); else W4TS(7);
        floatx4 gam[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float* base = Ms + (SMS ? lanee >> 2 : SM ? 8 * h + (lanee >> 3) : p16) * MSR + (SMS ? h * 16 : SM ? 0 : h * 32) + n4;
            floatx4 F[6];
#pragma unroll
            for (int xi = 0; xi < 4; ++xi) F[xi] = *reinterpret_cast<const floatx4*>(base + (4 * xi + rb) * 16 * MSR);
            const int ia = rb == 0 ? 0 : rb == 2 ? 2 : 1, ib = (rb & 1) ? 4 : 3;
            const float cb = (float)(1 << rb);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const float* hb = base + (16 + 6 * r) * 16 * MSR;
                const floatx4 pa = *reinterpret_cast<const floatx4*>(hb + ia * 16 * MSR);
                const floatx4 pb = *reinterpret_cast<const floatx4*>(hb + ib * 16 * MSR);
                floatx4 f;
#pragma unroll
                for (int c = 0; c < 4; ++c) f[c] = __builtin_fmaf(cb, pb[c], pa[c]);
                if (rb == 3) f += *reinterpret_cast<const floatx4*>(hb + 5 * 16 * MSR);
                F[4 + r] = f;
            }
            floatx4 o[4];                                    // the four rows of this thread's output column (bias included: see the accumulators' start)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float s12 = F[1][c] + F[2][c], d12 = F[1][c] - F[2][c], s34 = F[3][c] + F[4][c], d34 = F[3][c] - F[4][c];
                o[0][c] = (F[0][c] + s12) + s34;
                o[1][c] = __builtin_fmaf(2.f, d34, d12);
                o[2][c] = __builtin_fmaf(4.f, s34, s12);
                o[3][c] = __builtin_fmaf(8.f, d34, d12) + F[5][c];
            }
            if (EPI == LWG_EPI_SPADE) {
                if (h == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) gam[i] = o[i];   // gamma
                    continue;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[i][c] = w4_spade_mod(ext[0][i][c], mu[c], rs[c], gam[i][c], o[i][c]);
            } else if (EPI == LWG_EPI_RESIDUAL) {
                if (a.act == LWG_ACT_RELU_MASK) {            // data gradient behind a ReLU: res = the forward input, the mask source
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int c = 0; c < 4; ++c) o[i][c] = ext[h][i][c] > 0.f ? o[i][c] : 0.f;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[i] += ext[h][i];
                }
            }
            w4_act16(a.act, o);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(w4_u4, o[i]), ry, (int)cw4_out_group(vo[NVP == 2 ? h : 0][i], h, EPI != LWG_EPI_SPADE && !SM), 0, W4_NT_ST);
        }
        if (ph == 0) W4TS(6);
    }
    W4TS(3);
#ifdef LWG_W4_TS
    ++lab_bi;
#endif
    if (!more) break;
    blk = nblk;
    __syncthreads();                                         // every reader is done with the exchange buffer: raw[0] / raw[1] (the same LDS) may be written
    }
    W4TSA(12);
#ifdef LWG_W4_TS
    if (tid == 0) reinterpret_cast<unsigned long long*>(const_cast<float*>(a.res))[(size_t)blockIdx.x * 16 + 13] = (unsigned long long)lab_bi;
#endif
    if constexpr (LIST) {
        // the light entries of this workgroup: its ids behind the heavy ones.  A block is 512 pixels x NQD 16-byte channel quads (LWG_EPI_NONE: the 64
        // columns; LWG_EPI_SPADE: the 32 channels whose gamma | beta the block's 64 columns are); a thread keeps one quad and walks the pixels in passes of
        // four loads / stores; consecutive lanes = the quads of a pixel (a pixel's 256 / 128 bytes contiguous).  Pixels right of / below the image: the
        // out-of-range offset (dropped stores, zero loads), as in the epilogue.
        typedef unsigned int w4_u4 __attribute__((ext_vector_type(4)));
        // SUB: a light entry is a sub-tile, its SX * SY pixels (G::light_pixel): NPASS passes in all, NI at a time
        constexpr int NQD = EPI == LWG_EPI_SPADE ? 8 : 16;
        constexpr int NPASS = (SUB ? G::SX * G::SY : 512) * NQD / W4_THREADS, NI = NPASS < 4 ? NPASS : 4;
        const int ncb = N / NBV;
        const int nend = nhe + min(max(__builtin_amdgcn_readfirstlane(sk.counts[1]), 0), nall - nht) * ncb;
        const unsigned img_bytes = (unsigned)(H * W) * (unsigned)a.YC * 4u;
        // the calibration frame (one image): the output's layout | SPADE: the N stacked gamma | beta columns
        const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(sk.cal), 0, (int)((unsigned)(H * W) * (unsigned)(EPI == LWG_EPI_SPADE ? N : a.YC) * 4u), 0x00020000);
#pragma unroll 1
        for (int id = cw_list_first_light((int)blockIdx.x, (int)gridDim.x, nhe); id < nend; id += (int)gridDim.x) {
            int slot, cb;
            cw_list_entry(id - nhe, ncb, slot, cb);
            const int t = min(max(__builtin_amdgcn_readfirstlane(sk.light[slot]), 0), (SUB ? G::NS : 1) * g.tiles - 1);
            const int en0 = cw_n0(cb, NBV);
            int eb, ex0, ey0;
            if constexpr (SUB) {
                G::corner(g, t, eb, ex0, ey0);
                eb = __builtin_amdgcn_readfirstlane(eb);
            } else {
                eb = __builtin_amdgcn_readfirstlane(cw_image(g, t));
                cw_corner(g, t - eb * g.bx * g.by, 4 * W4_PBX, 4 * W4_PBY, ex0, ey0);
            }
            const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(y + (size_t)eb * H * W * a.YC, 0, (int)img_bytes, 0x00020000);
            int px, py, q4;
            cw4_light_elem(tid, 0, W4_THREADS, NQD, px, py, q4);
            if constexpr (EPI == LWG_EPI_SPADE) {
                const __amdgpu_buffer_rsrc_t re = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.xn) + (size_t)eb * H * W * a.YC, 0, (int)img_bytes, 0x00020000);
                const int cbase = en0 >> 1;                  // the block's first output channel (its columns: gamma | beta of 32 channels)
                const floatx4 mu = *reinterpret_cast<const floatx4*>(a.mean + (size_t)eb * a.YC + cbase + 4 * q4);
                const floatx4 rs = *reinterpret_cast<const floatx4*>(a.rstd + (size_t)eb * a.YC + cbase + 4 * q4);
#pragma unroll 1
                for (int it = 0; it < NPASS; it += NI) {
                    unsigned vo[NI];
                    floatx4 o[NI], gam[NI], xv[NI];
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        cw4_light_elem(tid, it + i, W4_THREADS, NQD, px, py, q4);
                        if constexpr (SUB) G::light_pixel(px, py);
                        vo[i] = cw4_out_voff(ex0 + px, ey0 + py, H, W, a.YC, cbase + 4 * q4);
                        const unsigned vc = cw4_out_voff(ex0 + px, ey0 + py, H, W, N, en0 + 4 * q4);
                        gam[i] = cw_buf_load(rc, cw4_out_group(vc, 0, true), 0u);
                        o[i] = cw_buf_load(rc, cw4_out_group(vc, 1, true), 0u);       // beta: 32 columns on
                        xv[i] = cw_buf_load<W4_NT_RES>(re, vo[i], 0u);
                    }
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int c = 0; c < 4; ++c) o[i][c] = w4_spade_mod(xv[i][c], mu[c], rs[c], gam[i][c], o[i][c]);
                    w4_act16(a.act, o);
#pragma unroll
                    for (int i = 0; i < NI; ++i) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(w4_u4, o[i]), ry, (int)vo[i], 0, W4_NT_ST);
                }
            } else {
#pragma unroll 1
                for (int it = 0; it < NPASS; it += NI) {
                    unsigned vo[NI];
                    floatx4 o[NI];
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        cw4_light_elem(tid, it + i, W4_THREADS, NQD, px, py, q4);
                        if constexpr (SUB) G::light_pixel(px, py);
                        vo[i] = cw4_out_voff(ex0 + px, ey0 + py, H, W, a.YC, a.ycoff + en0 + 4 * q4);
                        o[i] = cw_buf_load(rc, vo[i], 0u);
                    }
#pragma unroll
                    for (int i = 0; i < NI; ++i) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(w4_u4, o[i]), ry, (int)vo[i], 0, W4_NT_ST);
                }
            }
        }
    }
}

template <int EPI, bool TWO, bool SM = false>
__global__ __launch_bounds__(SM ? 256 : W4_THREADS, 1) void lwg_conv_winograd4_kernel(const LwgConvArgs a) {
    w4_body<EPI, TWO, SM, false>(a, LwgConvLists{});
}
template <bool TWO>
__global__ __launch_bounds__(256, 1) void lwg_conv_winograd4_split_kernel(const LwgConvArgs a) {
    w4_body<LWG_EPI_NONE, TWO, true, false, void, true>(a, LwgConvLists{});
}
template <int EPI>
__global__ __launch_bounds__(W4_THREADS, 1) void lwg_conv_winograd4_list_kernel(const LwgConvArgs a, const LwgConvLists sk) {
    w4_body<EPI, false, false, true>(a, sk);
}
// The sub-tile forms (G = Cw4F | Cw4Q) ...
template <int EPI, typename G>
__global__ __launch_bounds__(W4_THREADS, 1) void lwg_conv_winograd4_sub_kernel(const LwgConvArgs a, const LwgConvLists sk) {
    if (__builtin_amdgcn_readfirstlane(sk.counts[0]) >= G::in_image_total(a.B, a.H, a.W)) return;      // nothing is light: the kernel below
    w4_body<EPI, false, false, true, G>(a, sk);
}
// ... and their companion, launched behind it: a launch in which nothing is light (a frame batch without background) runs the plain kernel's body - its
// block order, staging and epilogue - decided here, on the device; every other launch ends at once.  (Two kernels, not two bodies in one: the
// scalar-register spill lanes of both bodies together cost the SPADE form a vector register it does not have.)
template <int EPI, typename G>
__global__ __launch_bounds__(W4_THREADS, 1) void lwg_conv_winograd4_sub_plain_kernel(const LwgConvArgs a, const LwgConvLists sk) {
    if (__builtin_amdgcn_readfirstlane(sk.counts[0]) < G::in_image_total(a.B, a.H, a.W)) return;
    w4_body<EPI, false, false, false>(a, LwgConvLists{});
}

// The fragment panel from the fp32 GEMM panel of the same convolution (lwg_conv2d_nhwc_f32's w: [9 Cin / 4][N][4], k = ((c / 32) 9 + tap) 32 + c % 32):
// U = G w G^T (6 x 6) per (input channel, output column) in fp64, rounded once, written as Upk[4][Cin/8][4][2][9 N]: block (q, s, kk, kh) of input channel
// c = 8 s + 2 kk + kh holds product j of column n at [n][j] (j = 0..3), 4 N + [n][j - 4] (j = 4..7), 8 N + [n] (j = 8); j < 6: U[q][j]; j = 6..8: U[4 + q / 2][3 (q % 2) + j - 6].  tap9[3 r + s] = the tap index of kernel
// position (dy, dx) = (r - 1, s - 1) in the GEMM panel.  One thread per (c, n).

__global__ __launch_bounds__(256) void lwg_winograd4_panel_kernel(const float* __restrict__ wp, float* __restrict__ U, int Cin, int N, LwgWinoTaps taps) {
    const int n = blockIdx.x * 64 + (threadIdx.x & 63), c = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (n >= N || c >= Cin) return;
    double g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int k = ((c >> 5) * 9 + taps.t[3 * r + s]) * 32 + (c & 31);
            g[r][s] = (double)wp[((size_t)(k >> 2) * N + n) * 4 + (k & 3)];
        }
    const double G[6][3] = {{1.0 / 4, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6}, {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    double t[6][3];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int s = 0; s < 3; ++s) t[i][s] = G[i][0] * g[0][s] + G[i][1] * g[1][s] + G[i][2] * g[2][s];
    const int s8 = c >> 3, kk = (c & 7) >> 1, kh = c & 1;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
        float* dst = U + ((((size_t)qq * (Cin >> 3) + s8) * 4 + kk) * 2 + kh) * 9 * (size_t)N;
        float o[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int xi = j < 6 ? qq : 4 + (qq >> 1), nu = j < 6 ? j : 3 * (qq & 1) + (j - 6);
            o[j] = (float)(t[xi][0] * G[nu][0] + t[xi][1] * G[nu][1] + t[xi][2] * G[nu][2]);
        }
        *reinterpret_cast<floatx4*>(dst + 4 * n) = floatx4{o[0], o[1], o[2], o[3]};
        *reinterpret_cast<floatx4*>(dst + 4 * (size_t)N + 4 * n) = floatx4{o[4], o[5], o[6], o[7]};
        dst[8 * (size_t)N + n] = o[8];
    }
}

// every registered panel of a training step in one launch (the weights change every step; conv_winograd.hip: lwg_winograd_panels_kernel): workgroup b
// serves descriptor d = the last one with first_block <= b (binary search), block lb of its ceil(N / 64) x ceil(Cin / 4) grid.  Bitwise the values of
// the single launch: the kernel above is left to the compiler's contraction (its code is unchanged), which evaluates every three-term sum
// a0 b0 + a1 b1 + a2 b2 as fma(a2, b2, fma(a1, b1, a0 * b0)) - one rounded product, two fused steps, in this order (terms with a zero coefficient
// add an exact zero wherever the compiler places them); this copy writes that order out and forbids any other contraction.
__device__ __forceinline__ double w4_panel_sum3(double a0, double b0, double a1, double b1, double a2, double b2) {
#pragma clang fp contract(off)
    const double p = a0 * b0;
    return __builtin_fma(a2, b2, __builtin_fma(a1, b1, p));
}
__device__ __forceinline__ void lwg_winograd4_panels_pair(const float* __restrict__ wp, float* __restrict__ U, int Cin, int N, const int* t9, int c, int n) {
    double g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int k = ((c >> 5) * 9 + t9[3 * r + s]) * 32 + (c & 31);
            g[r][s] = (double)wp[((size_t)(k >> 2) * N + n) * 4 + (k & 3)];
        }
    const double G[6][3] = {{1.0 / 4, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6}, {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    double t[6][3];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int s = 0; s < 3; ++s) t[i][s] = w4_panel_sum3(G[i][0], g[0][s], G[i][1], g[1][s], G[i][2], g[2][s]);
    const int s8 = c >> 3, kk = (c & 7) >> 1, kh = c & 1;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
        float* dst = U + ((((size_t)qq * (Cin >> 3) + s8) * 4 + kk) * 2 + kh) * 9 * (size_t)N;
        float o[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int xi = j < 6 ? qq : 4 + (qq >> 1), nu = j < 6 ? j : 3 * (qq & 1) + (j - 6);
            o[j] = (float)w4_panel_sum3(t[xi][0], G[nu][0], t[xi][1], G[nu][1], t[xi][2], G[nu][2]);
        }
        *reinterpret_cast<floatx4*>(dst + 4 * n) = floatx4{o[0], o[1], o[2], o[3]};
        *reinterpret_cast<floatx4*>(dst + 4 * (size_t)N + 4 * n) = floatx4{o[4], o[5], o[6], o[7]};
        dst[8 * (size_t)N + n] = o[8];
    }
}
__global__ __launch_bounds__(256) void lwg_winograd4_panels_kernel(const LwgWinoDesc* __restrict__ descs, int ndesc) {
    int lo = 0, hi = ndesc - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const LwgWinoDesc* d = descs + lo;
    const int N = d->N, Cin = d->Cin, nbx = (N + 63) >> 6;
    const int lb = (int)blockIdx.x - d->first_block;
    const int n = (lb % nbx) * 64 + (threadIdx.x & 63), c = (lb / nbx) * 4 + (threadIdx.x >> 6);
    if (n < N && c < Cin) lwg_winograd4_panels_pair(d->wpanel, d->upk, Cin, N, d->tap9, c, n);
}

extern "C" int lwg_winograd4_panels_f32(const LwgWinoDesc* descs_dev, int ndesc, int total_blocks, lwg_stream_t stream_) {
    if (!descs_dev || ndesc < 1 || total_blocks < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lwg_winograd4_panels_kernel, dim3((unsigned)total_blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream_), descs_dev, ndesc);
    return (int)hipGetLastError();
}

extern "C" int lwg_winograd4_panel_f32(const float* wpanel, float* upk, int Cin, int N, const int* tap9, lwg_stream_t stream_) {
    LwgWinoTaps taps;
    if (!cw_panel_args_ok(wpanel, upk, Cin, N, tap9, taps)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lwg_winograd4_panel_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)((Cin + 3) / 4)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream_), wpanel, upk, Cin, N, taps);
    return (int)hipGetLastError();
}

// args: lwg_conv_wino.h's fp32 contract (lwg_conv2d_winograd_f32's launch description) with args->w = the F(4x4, 3x3) fragment panel of
// lwg_winograd4_panel_f32, 144 Cin N bytes; an output image is one buffer of the store path, with 256 bytes of slack for the second channel group
template <int EPI, bool SM>
static int lwg_wino4_go(const LwgConvArgs& a, dim3 grid, size_t lds, hipStream_t stream) {
    return a.C1 > 0 ? cw_launch<lwg_conv_winograd4_kernel<EPI, true, SM>>(grid, SM ? 256 : W4_THREADS, lds, stream, a)
                    : cw_launch<lwg_conv_winograd4_kernel<EPI, false, SM>>(grid, SM ? 256 : W4_THREADS, lds, stream, a);
}

extern "C" int lwg_conv2d_winograd4_f32(const LwgConvArgs* pa, lwg_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!pa || !cw_contract_ok(*pa, 144ull, 256ll)) return (int)hipErrorInvalidValue;
    const LwgConvArgs& a = *pa;
    const size_t lds = (size_t)(W4_BIAS_OFF + 64) * 4;
    const int cus = lwg_device_cus();
    long long total = cw_total_blocks(a.B, a.H, a.W, a.N, 4 * W4_PBX, 4 * W4_PBY, W4_NB);
    // small launches (the 8-wave blocks would leave half the chip or more without a workgroup): the 4-wave form, 32 channels per block (SPADE: gamma | beta
    // of 16 channels) - bitwise the same result (see the kernel), so the choice may depend on the batch
    const bool sm = LWG_W4_SMALL && 2 * total <= cus;
    if (sm) total *= 2;
    const dim3 grid = cw_persistent_grid(total, cus);
    if (a.epi == LWG_EPI_SPADE) return sm ? lwg_wino4_go<LWG_EPI_SPADE, true>(a, grid, lds, stream) : lwg_wino4_go<LWG_EPI_SPADE, false>(a, grid, lds, stream);
    if (a.epi == LWG_EPI_RESIDUAL) return sm ? lwg_wino4_go<LWG_EPI_RESIDUAL, true>(a, grid, lds, stream) : lwg_wino4_go<LWG_EPI_RESIDUAL, false>(a, grid, lds, stream);
    return sm ? lwg_wino4_go<LWG_EPI_NONE, true>(a, grid, lds, stream) : lwg_wino4_go<LWG_EPI_NONE, false>(a, grid, lds, stream);
}

// The split-K launch of a training step (include/lwg_hip.h; lwg_conv_wino.h: cw4_split_plan): ws = NULL, or a launch the plan runs whole - the
// entry point above.
static Cw4Split lwg_wino4_split_plan(const LwgConvArgs& a) {
    const bool mask = a.epi == LWG_EPI_RESIDUAL && a.act == LWG_ACT_RELU_MASK;
    return cw4_split_plan(cw_total_blocks(a.B, a.H, a.W, a.N, 4 * W4_PBX, 4 * W4_PBY, 32), (a.C0 + a.C1) / W4_KS, lwg_device_cus(),
                          LWG_W4_SMALL && (a.epi == LWG_EPI_NONE || mask), cw4_slab_image_ok(a.H, a.W, a.N));
}
extern "C" size_t lwg_conv2d_winograd4_ws_floats(const LwgConvArgs* pa) {
    if (!pa || !cw_contract_ok(*pa, 144ull, 256ll)) return 0;
    return cw4_slab_offset(lwg_wino4_split_plan(*pa).slices, pa->M, pa->N);
}
// *blocks = 32 x 16-pixel blocks of the launch (times the K slices when with_ws and the split plan applies), *slices = K slices (0 = whole), *nbv =
// output channels per block (64 | 32), *workgroups = workgroups launched.  Returns 0, or 1 when the launch does not meet the contract.
extern "C" int lwg_conv2d_winograd4_plan(const LwgConvArgs* pa, int with_ws, long long* blocks, int* slices, int* nbv, int* workgroups) {
    if (!pa || !cw_contract_ok(*pa, 144ull, 256ll)) return (int)hipErrorInvalidValue;
    const LwgConvArgs& a = *pa;
    const int sl = with_ws ? lwg_wino4_split_plan(a).slices : 0;
    const int cus = lwg_device_cus();
    const long long b64 = cw_total_blocks(a.B, a.H, a.W, a.N, 4 * W4_PBX, 4 * W4_PBY, W4_NB);
    const int v = sl > 1 || (LWG_W4_SMALL && 2 * b64 <= cus) ? 32 : W4_NB;
    const long long nb = b64 * (W4_NB / v) * (sl > 1 ? sl : 1);
    if (blocks) *blocks = nb;
    if (slices) *slices = sl > 1 ? sl : 0;
    if (nbv) *nbv = v;
    if (workgroups) *workgroups = (int)(sl > 1 ? nb : (nb < cus ? nb : cus));
    return 0;
}
extern "C" int lwg_conv2d_winograd4_f32_ws(const LwgConvArgs* pa, float* ws, lwg_stream_t stream_) {
    if (!pa || !cw_contract_ok(*pa, 144ull, 256ll)) return (int)hipErrorInvalidValue;
    const LwgConvArgs& a = *pa;
    const Cw4Split sp = ws ? lwg_wino4_split_plan(a) : Cw4Split{0, 0};
    if (sp.slices < 2) return lwg_conv2d_winograd4_f32(pa, stream_);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    LwgConvArgs part = a;                                    // raw sums into the slabs: dense (M, N) rows, no bias / residual / activation
    part.y = ws;
    part.YC = a.N;
    part.ycoff = 0;
    part.bias = nullptr;
    part.epi = LWG_EPI_NONE;
    part.act = LWG_ACT_NONE;
    part.res = nullptr;
    part.cshift = sp.sps;
    const size_t lds = (size_t)(W4_BIAS_OFF + 64) * 4;
    const dim3 grid((unsigned)cw_total_blocks(a.B, a.H, a.W, a.N, 4 * W4_PBX, 4 * W4_PBY, 32), 1u, (unsigned)sp.slices);
    const int e = a.C1 > 0 ? cw_launch<lwg_conv_winograd4_split_kernel<true>>(grid, 256, lds, stream, part)
                           : cw_launch<lwg_conv_winograd4_split_kernel<false>>(grid, 256, lds, stream, part);
    return e != (int)hipSuccess ? e : (int)lwg_splitk_finish_launch(a, ws, sp.slices, stream);
}

// The list-driven launch (include/lwg_hip.h): the same contract, LWG_EPI_NONE / LWG_EPI_SPADE and one input only; the grid is sized from the launch's
// total as above (the lists' counts are read by the kernel, never by the host).  Launches of the 4-wave form run the plain entry point.
static bool lwg_wino4_list_ok(const LwgConvArgs* pa) {
    return pa && cw_contract_ok(*pa, 144ull, 256ll) && pa->C1 == 0 && (pa->epi == LWG_EPI_NONE || pa->epi == LWG_EPI_SPADE) &&
           cw_contract_calib_ok(*pa) && cw_total_blocks(pa->B, pa->H, pa->W, pa->N, 4 * W4_PBX, 4 * W4_PBY, W4_NB) < (1ll << 30);
}
extern "C" int lwg_conv2d_winograd4_list_applies(const LwgConvArgs* pa) {
    if (!lwg_wino4_list_ok(pa)) return 0;
    return !(LWG_W4_SMALL && 2 * cw_total_blocks(pa->B, pa->H, pa->W, pa->N, 4 * W4_PBX, 4 * W4_PBY, W4_NB) <= lwg_device_cus());
}
// G = void: pl = the block lists of lwg_spade_skip_lists_f32, one kernel.  G = Cw4F | Cw4Q: pl->heavy / light / counts = the SUB-TILE lists of that
// geometry (lwg_spade_skip_fine_lists_f32 / _q8_lists_f32), the list kernel and its nothing-is-light companion; the same contract, the same
// launch-size rule (lwg_conv2d_winograd4_list_applies) and the same result at every granularity
template <typename G>
static int lwg_wino4_lists_go(const LwgConvArgs* pa, const LwgConvLists* pl, lwg_stream_t stream_) {
    if (!lwg_wino4_list_ok(pa) || !pl || !pl->heavy || !pl->light || !pl->counts || !pl->cal) return (int)hipErrorInvalidValue;
    if (!lwg_conv2d_winograd4_list_applies(pa)) return lwg_conv2d_winograd4_f32(pa, stream_);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const LwgConvArgs& a = *pa;
    const size_t lds = (size_t)(w4_bias_off<G> + 64) * 4, ldsp = (size_t)(W4_BIAS_OFF + 64) * 4;
    const dim3 grid = cw_persistent_grid(cw_total_blocks(a.B, a.H, a.W, a.N, 4 * W4_PBX, 4 * W4_PBY, W4_NB), lwg_device_cus());
    if constexpr (std::is_void<G>::value) {
        return a.epi == LWG_EPI_SPADE ? cw_launch_lists<lwg_conv_winograd4_list_kernel<LWG_EPI_SPADE>>(grid, W4_THREADS, lds, stream, a, *pl)
                                      : cw_launch_lists<lwg_conv_winograd4_list_kernel<LWG_EPI_NONE>>(grid, W4_THREADS, lds, stream, a, *pl);
    } else {
        const int e = a.epi == LWG_EPI_SPADE ? cw_launch_lists<lwg_conv_winograd4_sub_kernel<LWG_EPI_SPADE, G>>(grid, W4_THREADS, lds, stream, a, *pl)
                                             : cw_launch_lists<lwg_conv_winograd4_sub_kernel<LWG_EPI_NONE, G>>(grid, W4_THREADS, lds, stream, a, *pl);
        if (e != 0) return e;
        return a.epi == LWG_EPI_SPADE ? cw_launch_lists<lwg_conv_winograd4_sub_plain_kernel<LWG_EPI_SPADE, G>>(grid, W4_THREADS, ldsp, stream, a, *pl)
                                      : cw_launch_lists<lwg_conv_winograd4_sub_plain_kernel<LWG_EPI_NONE, G>>(grid, W4_THREADS, ldsp, stream, a, *pl);
    }
}
extern "C" int lwg_conv2d_winograd4_list_f32(const LwgConvArgs* pa, const LwgConvLists* pl, lwg_stream_t stream_) { return lwg_wino4_lists_go<void>(pa, pl, stream_); }
extern "C" int lwg_conv2d_winograd4_fine_f32(const LwgConvArgs* pa, const LwgConvLists* pl, lwg_stream_t stream_) { return lwg_wino4_lists_go<Cw4F>(pa, pl, stream_); }
extern "C" int lwg_conv2d_winograd4_q8_f32(const LwgConvArgs* pa, const LwgConvLists* pl, lwg_stream_t stream_) { return lwg_wino4_lists_go<Cw4Q>(pa, pl, stream_); }
