// Fused F(2x2, 3x3) Winograd form of the 3x3 / stride 1 / pad 1 convolution on bf16 NHWC activations, v_mfma_f32_32x32x16_bf16
// (ops.conv_precision("bf16_winograd"); entry point lwg_conv2d_winograd_bf16).  The bf16 sibling of conv_winograd.hip:
//   y = act(bias + sum x * w [+ res]) as U = G w G^T (host panel, fp64 -> bf16), V = B^T d B per 4x4 input patch d (patches overlap by two
//   pixels), M_{xi,nu} = sum_c V_{xi,nu} U_{xi,nu} - sixteen GEMMs over Cin - and Y = A^T M A: 4 multiplies per output instead of 9.
// Rounding points (the test bounds depend on them): the halo is read as bf16; B^T d B is evaluated in fp32 (B^T d first, then (.) B) and rounded
// ONCE (RNE) to bf16; U is rounded once from fp64 on the host; the MFMA accumulation, A^T M A, the bias and the epilogue arithmetic are fp32; one
// rounding to bf16 at the store.
// Workgroup: 512 threads = 8 waves; block = 8 x 8 patches (16 x 16 output pixels) x 64 output channels.  Wave w owns the FOUR products
// (xi = w % 4, nu = 0..3) for all 64 patches x the 32 output channels of column tile w / 4: 4 x 2 accumulator tiles of 32 x 32 = 128 registers, the
// nu half of A^T M A is register-local and half of the products' volume crosses waves in the epilogue (as in conv_winograd.hip).
// MFMA orientation: D^T - the U fragment is the row operand (rows = output channels), the V fragment the column operand (columns = patches): a
// lane owns one patch and 4 consecutive channels per 8-channel group.
// A K stage is 32 input channels = two MFMA k-steps (the option of the issue's list chosen here: "a K stage of >= 32 channels"; the compiler is
// free to use packed fp32 adds in the transform - the four channels of a thread are independent lanes of the same expressions):
//   * U fragments: a lane loads its 16 bytes of a (k-step, product) fragment straight from the panel [Cin/16][16][N][16] (1 KB contiguous per
//     wave and load) into ONE register set of 8 fragments; a k-step's four fragments are re-requested for the next stage right behind their last
//     MFMA, so they land under the other k-step's MFMAs and the next stage's transform.  The weights never touch LDS;
//   * the raw 18 x 18 x 32 halo goes global -> registers (requested two stages ahead) -> raw (64 bytes per pixel; padding pixels carry an
//     out-of-range buffer offset: the hardware returns zeros, no branches);
//   * the input transform of stage s + 1 (a thread = one patch x 4 channels: sixteen 8-byte reads, 32 adds per channel, sixteen 8-byte writes)
//     is issued in front of the MFMAs of stage s and writes the OTHER of two V buffers; the two waves of a SIMD overlap one's transform with
//     the other's MFMAs as far as the two barriers per stage (raw is single-buffered: 2 V buffers + 2 raw buffers exceed the 160 KB) allow.
// LDS images, laid out so that every 16-byte fragment read and 8-byte transform access covers the banks once per lane group (by construction):
//   raw  [pixel 18 hy + hx][64 B], the two pixels of a 128-byte pair swapped when (hx >> 2) & 1: the four patches of a 32-lane half (hx apart
//        by 2) then cover the 64 banks once;
//   V    [product 16][patch 64][64 B], the 16-byte k-octet o (channels 8 o ..) at slot o ^ ((patch >> 2) & 3).
// Budget (the reason the mode is opt-in): per stage and wave 16 MFMAs (512 matrix cycles) against 16 V reads (1 per MFMA: inside the 2-per-gap
// LDS budget), 8 KB of U from L2 (64 B / clk / CU with both waves of the SIMDs busy: TWICE the row-renaming kernel's 32, and at the L2's rate -
// F(2x2, 3x3) has sixteen weight matrices and a block of 64 patches re-uses a fragment twice) and a transform of 4 (patch, channel) per thread.
// Measured (MI355X, 1024^2 layer shapes at frame batch 20, profiles/bf16wino_layers.txt): SLOWER than lwg_conv2d_nhwc_bf16_hr on every
// shape - 1.12x (skip convolutions) to 1.65x (Cin = 64: two stages per block) its time, 0.21-0.37 PFLOP/s executed against 0.73-1.23; the clip
// 670 against 899 frames/s.  The limit is the stream and the transform above, not the matrix pipe; the layer rule (ops.BF16_WINO_MIN_CIN)
// excludes nothing because no shape wins.
// Registers: 256 VGPRs, 3-4 spilled (a thread's three halo LDS destinations: stored in the set-up, re-loaded in a block's prologue - no scratch
// access inside the K loop in any instantiation).
// Epilogue: every wave folds its four products over nu in registers (M A: two values per (xi, patch, channel)); the four xi of a (patch, channel)
// live in four waves -> one exchange through LDS ([xi][j][patch][64 + 4] fp32); a thread then owns one patch x 8 consecutive output columns:
// A^T (.) over xi, + bias (+ residual | SPADE) + activation, one 16-byte bf16 store per pixel (SPADE: the 8 columns are gamma | beta of FOUR
// channels - the panel interleaves them in blocks of 4 - one 8-byte store).
// Persistent workgroups in the XCD-aware order: min(blocks, CUs) workgroups; workgroup blockIdx.x takes the ids r, r + gridDim.x, ... with
// r = lwg_xcd_remap(blockIdx.x, gridDim.x), so in every pass each XCD (workgroups are dealt round-robin over the eight) works on a CONTIGUOUS
// range of ids; id = column block * tiles + tile: neighbouring tiles (shared halo rows) and one column block of the panel (32 Cin x 64 bytes)
// per XCD L2.  A block's arithmetic does not depend on which workgroup runs it.
// Batch invariance: a block's arithmetic depends on its own image only (per-image buffer descriptors: any batch in one launch); every output
// element is accumulated over the stages and k-steps in the same order whatever B; there is one form and no split-K.
#include "lwg_common.h"
#include "lwg_conv_wino.h"

typedef __bf16 wb_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int wb_uintx4 __attribute__((ext_vector_type(4)));
typedef unsigned int wb_uintx2 __attribute__((ext_vector_type(2)));

#define WB_THREADS 512
#define WB_KS 32                                   // input channels per stage
#define WB_HALO 18
#define WB_HALO_PIX (WB_HALO * WB_HALO)
#define WB_RAW_BYTES (WB_HALO_PIX * 64)            // [pixel][32 bf16]
#define WB_V_BYTES (16 * 64 * 64)                  // [product][patch][32 bf16]
#define WB_LOOP_BYTES (WB_RAW_BYTES + 2 * WB_V_BYTES)
#define WB_MS_ROW 68                               // floats per (xi, j, patch) row of the exchange buffer
#define WB_MS_BYTES (8 * 64 * WB_MS_ROW * 4)
#define WB_LDS_BYTES (WB_LOOP_BYTES > WB_MS_BYTES ? WB_LOOP_BYTES : WB_MS_BYTES)
#define WB_HALO_LOADS 3                            // 18 * 18 pixels * 4 sixteen-byte pieces = 1296 <= 3 * 512

__device__ __forceinline__ unsigned wb_pack2(float lo, float hi) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float wb_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float wb_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

template <int EPI, bool TWO>
__global__ __launch_bounds__(WB_THREADS, 1) void lwg_conv_winograd_bf16_kernel(const LwgConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char wb_smem[];
    char* const raw = wb_smem;
    char* const Vs = wb_smem + WB_RAW_BYTES;               // [2][WB_V_BYTES]
    float* const Ms = reinterpret_cast<float*>(wb_smem);   // the epilogue's exchange buffer (after the K loop)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xi = wid & 3, nt = wid >> 2;
    const int khalf = lane >> 5, l31 = lane & 31;
    const int H = a.H, W = a.W, N = a.N, Cin = a.C0 + a.C1;
    const int nst = Cin / WB_KS;                           // even (host: Cin % 64 == 0)
    const CwGrid g = cw_grid(a.B, H, W, N, 16, 16, 64);    // (lwg_conv_wino.h: the grid, the halo offsets, the image descriptors, the contract)
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, (int)(32u * (unsigned)Cin * (unsigned)N), 0x00020000);

    // ---- thread roles that do not depend on the block
    // halo piece q of this thread: pixel (tid + 512 q) >> 2, 16-byte piece (tid + 512 q) & 3
    unsigned hdst[WB_HALO_LOADS];
#pragma unroll
    for (int q = 0; q < WB_HALO_LOADS; ++q) {
        const int i = tid + WB_THREADS * q;
        const int pix = i >> 2, px = pix % WB_HALO;
        hdst[q] = ((unsigned)(pix * 64) ^ (unsigned)(((px >> 2) & 1) << 6)) + (unsigned)(i & 3) * 16u;
    }
    const bool hlast = tid + WB_THREADS * (WB_HALO_LOADS - 1) < 4 * WB_HALO_PIX;   // the last piece exists for this thread (the others for all)
    // transform: patch tp, channel quad tq of the stage
    const int tp = tid >> 3, tq = tid & 7;
    const int tpy = tp >> 3, tpx = tp & 7;
    const unsigned vdst = (unsigned)(tp * 64 + ((((tq >> 1) ^ ((tp >> 2) & 3))) << 4) + (tq & 1) * 8);
    // fragment reads: patch tile pt, k-octet c = 2 ks + khalf of patch p = 32 pt + l31 -> byte offset inside a product's plane
    unsigned vsrc[2][2];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int p = pt * 32 + l31;
            vsrc[pt][ks] = (unsigned)(p * 64 + (((2 * ks + khalf) ^ ((p >> 2) & 3)) << 4));
        }

    for (int blk = lwg_xcd_remap(blockIdx.x, gridDim.x); blk < g.total; blk += gridDim.x) {
        const int cb = blk / g.tiles;
        const int t = blk - cb * g.tiles, b = cw_image(g, t);
        int x0, y0;
        cw_corner(g, t - b * g.bx * g.by, 16, 16, x0, y0);
        const int n0 = cw_n0(cb, 64);
        const __amdgpu_buffer_rsrc_t rx0 = cw_image_rsrc(a.x0, b, H, W, a.C0, 2u);
        const __amdgpu_buffer_rsrc_t rx1 = TWO ? cw_image_rsrc(a.x1, b, H, W, a.C1, 2u) : rx0;
        int hlin[WB_HALO_LOADS];                           // pixel index inside the image, -1 = padding / no piece
#pragma unroll
        for (int q = 0; q < WB_HALO_LOADS; ++q) hlin[q] = cw_halo_pixel(tid + WB_THREADS * q, WB_HALO, 4 * WB_HALO_PIX, 2, x0, y0, H, W);
        const unsigned uvoff = (unsigned)((n0 + nt * 32 + l31) * 32 + khalf * 16);

        wb_uintx4 hreg[WB_HALO_LOADS];
        auto load_halo = [&](int s) {
            const int cc = s * WB_KS;
            const bool use1 = cw_stage_second(cc, a.C0, TWO);
            const unsigned soff = cw_stage_soff(cc, a.C0, TWO, 2);
#pragma unroll
            for (int q = 0; q < WB_HALO_LOADS; ++q) {
                const unsigned voff = cw_halo_pixel_voff(hlin[q], tid + WB_THREADS * q, 2, use1 ? a.C1 : a.C0, 2);
                hreg[q] = __builtin_bit_cast(wb_uintx4, use1 ? __builtin_amdgcn_raw_buffer_load_b128(rx1, (int)voff, (int)soff, 0)
                                                             : __builtin_amdgcn_raw_buffer_load_b128(rx0, (int)voff, (int)soff, 0));
            }
        };
        auto store_raw = [&]() {
#pragma unroll
            for (int q = 0; q < WB_HALO_LOADS; ++q)
                if (q + 1 < WB_HALO_LOADS || hlast) *reinterpret_cast<wb_uintx4*>(raw + hdst[q]) = hreg[q];
        };
        // V = B^T d B of this thread's (patch, 4 channels): raw -> Vbuf
        auto transform = [&](char* Vbuf) {
            // rows first (t_c = B^T d[.][c] per patch column c), then V[.][nu] from the columns as they arrive: at most three columns are live
            float tc[4][4][4];                                 // [patch column c][xi][channel]
            auto column = [&](int c) {
                float d[4][4];                                 // [patch row r][channel]
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int hy = 2 * tpy + r, hx = 2 * tpx + c;
                    const unsigned off = ((unsigned)((hy * WB_HALO + hx) * 64) ^ (unsigned)(((hx >> 2) & 1) << 6)) + (unsigned)tq * 8u;
                    const wb_uintx2 v = *reinterpret_cast<const wb_uintx2*>(raw + off);
                    d[r][0] = wb_lo(v[0]); d[r][1] = wb_hi(v[0]); d[r][2] = wb_lo(v[1]); d[r][3] = wb_hi(v[1]);
                }
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    tc[c][0][ch] = d[0][ch] - d[2][ch];
                    tc[c][1][ch] = d[1][ch] + d[2][ch];
                    tc[c][2][ch] = d[2][ch] - d[1][ch];
                    tc[c][3][ch] = d[1][ch] - d[3][ch];
                }
            };
            auto emit = [&](int nu, int ca, int cb2, bool add) {   // V[.][nu] = t_ca +- t_cb2
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    float v[4];
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) v[ch] = add ? tc[ca][x][ch] + tc[cb2][x][ch] : tc[ca][x][ch] - tc[cb2][x][ch];
                    wb_uintx2 pk;
                    pk[0] = wb_pack2(v[0], v[1]);
                    pk[1] = wb_pack2(v[2], v[3]);
                    *reinterpret_cast<wb_uintx2*>(Vbuf + (x * 4 + nu) * 4096 + vdst) = pk;
                }
            };
            column(0); column(2);
            emit(0, 0, 2, false);
            column(1);
            emit(1, 1, 2, true);
            emit(2, 2, 1, false);
            column(3);
            emit(3, 1, 3, false);
        };
        wb_bf16x8 uq[2][4];                                    // [k-step][nu]
        auto load_u = [&](int s, int ks) {
#pragma unroll
            for (int nu = 0; nu < 4; ++nu) {
                const unsigned soff = (unsigned)(((s * 2 + ks) * 16 + xi * 4 + nu)) * (unsigned)N * 32u;
                uq[ks][nu] = __builtin_bit_cast(wb_bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ru, (int)uvoff, (int)soff, 0));
            }
        };

        floatx16 acc[4][2];
#pragma unroll
        for (int nu = 0; nu < 4; ++nu)
#pragma unroll
            for (int pt = 0; pt < 2; ++pt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[nu][pt][r] = 0.f;

        // ---- prologue: stage 0 -> V[0], stage 1 -> raw
        load_halo(0);
        load_u(0, 0);
        load_u(0, 1);
        store_raw();
        __syncthreads();
        transform(Vs);
        load_halo(1);                                          // nst >= 2
        __syncthreads();
        store_raw();
        __syncthreads();

        for (int s = 0; s < nst; ++s) {
            // here: V[s & 1] holds stage s, raw holds stage s + 1 (if any), uq holds / awaits stage s
            const char* Vcur = Vs + (s & 1) * WB_V_BYTES;
            const bool more1 = s + 1 < nst, more2 = s + 2 < nst;
            if (more2) load_halo(s + 2);
            if (more1) transform(Vs + ((s + 1) & 1) * WB_V_BYTES);
            const int sn = more1 ? s + 1 : s;                  // (last stage: a harmless re-load of its own fragments, no branch between the MFMAs)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int nu = 0; nu < 4; ++nu) {
                    const char* vp = Vcur + (xi * 4 + nu) * 4096;
                    const wb_bf16x8 f0 = *reinterpret_cast<const wb_bf16x8*>(vp + vsrc[0][ks]);
                    const wb_bf16x8 f1 = *reinterpret_cast<const wb_bf16x8*>(vp + vsrc[1][ks]);
                    acc[nu][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(uq[ks][nu], f0, acc[nu][0], 0, 0, 0);
                    acc[nu][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(uq[ks][nu], f1, acc[nu][1], 0, 0, 0);
                }
                load_u(sn, ks);
            }
            __syncthreads();                                   // every wave has left raw and V[s & 1]; V[(s + 1) & 1] is written
            if (more2) store_raw();
            __syncthreads();
        }

        // ---- epilogue: fold over nu (M A), exchange over xi, A^T (.), bias / residual / SPADE, activation, store
        // acc[nu][pt][4 g + c] = patch 32 pt + l31, channel 32 nt + 8 g + 4 khalf + c
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                floatx4 t0, t1;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int r = 4 * g + c;
                    t0[c] = (acc[0][pt][r] + acc[1][pt][r]) + acc[2][pt][r];
                    t1[c] = (acc[1][pt][r] - acc[2][pt][r]) - acc[3][pt][r];
                }
                const int chn = nt * 32 + 8 * g + 4 * khalf;
                *reinterpret_cast<floatx4*>(Ms + ((xi * 2 + 0) * 64 + pt * 32 + l31) * WB_MS_ROW + chn) = t0;
                *reinterpret_cast<floatx4*>(Ms + ((xi * 2 + 1) * 64 + pt * 32 + l31) * WB_MS_ROW + chn) = t1;
            }
        __syncthreads();
        {
            const int ep = tid >> 3, c8 = tid & 7;             // patch, group of 8 output columns
            const int epy = ep >> 3, epx = ep & 7;
            __bf16* const yb = reinterpret_cast<__bf16*>(a.y);
            const __bf16* const resb = reinterpret_cast<const __bf16*>(a.res);
            const __bf16* const xnb = reinterpret_cast<const __bf16*>(a.xn);
            float bs[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) bs[c] = a.bias ? a.bias[n0 + 8 * c8 + c] : 0.f;
            float mu[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
            const int sch = (n0 >> 1) + 4 * c8;                // SPADE: first of this thread's four output channels
            if constexpr (EPI == LWG_EPI_SPADE) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    mu[c] = a.mean[(size_t)b * a.YC + sch + c];
                    rs[c] = a.rstd[(size_t)b * a.YC + sch + c];
                }
            }
            lwg_act_dispatch(a.act, [&](auto actc) {
                constexpr int EA = decltype(actc)::value;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float T[4][8];
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        const float* mp = Ms + ((x * 2 + j) * 64 + ep) * WB_MS_ROW + 8 * c8;
                        const floatx4 lo = *reinterpret_cast<const floatx4*>(mp), hi = *reinterpret_cast<const floatx4*>(mp + 4);
#pragma unroll
                        for (int c = 0; c < 4; ++c) { T[x][c] = lo[c]; T[x][4 + c] = hi[c]; }
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int oy = y0 + 2 * epy + i, ox = x0 + 2 * epx + j;
                        if (oy >= H || ox >= W) continue;
                        const size_t opix = ((size_t)b * H + oy) * W + ox;
                        float yv[8];
#pragma unroll
                        for (int c = 0; c < 8; ++c)
                            yv[c] = (i == 0 ? (T[0][c] + T[1][c]) + T[2][c] : (T[1][c] - T[2][c]) - T[3][c]) + bs[c];
                        if constexpr (EPI == LWG_EPI_SPADE) {
                            const wb_uintx2 xv = *reinterpret_cast<const wb_uintx2*>(xnb + opix * a.YC + sch);
                            const float xf[4] = {wb_lo(xv[0]), wb_hi(xv[0]), wb_lo(xv[1]), wb_hi(xv[1])};
                            float o[4];
#pragma unroll
                            for (int c = 0; c < 4; ++c) o[c] = lwg_act_c<EA>((xf[c] - mu[c]) * rs[c] * (1.f + yv[c]) + yv[4 + c], a.act);
                            wb_uintx2 pk;
                            pk[0] = wb_pack2(o[0], o[1]);
                            pk[1] = wb_pack2(o[2], o[3]);
                            *reinterpret_cast<wb_uintx2*>(yb + opix * a.YC + sch) = pk;
                        } else {
                            const size_t oidx = opix * a.YC + a.ycoff + n0 + 8 * c8;
                            if constexpr (EPI == LWG_EPI_RESIDUAL) {
                                const wb_uintx4 rv = *reinterpret_cast<const wb_uintx4*>(resb + oidx);
#pragma unroll
                                for (int c = 0; c < 4; ++c) { yv[2 * c] += wb_lo(rv[c]); yv[2 * c + 1] += wb_hi(rv[c]); }
                            }
                            wb_uintx4 pk;
#pragma unroll
                            for (int c = 0; c < 4; ++c) pk[c] = wb_pack2(lwg_act_c<EA>(yv[2 * c], a.act), lwg_act_c<EA>(yv[2 * c + 1], a.act));
                            *reinterpret_cast<wb_uintx4*>(yb + oidx) = pk;
                        }
                    }
                }
            });
        }
        __syncthreads();                                       // the exchange buffer is the next block's raw / V
    }
}

template <int EPI>
static int wb_launch_epi(const LwgConvArgs& a, hipStream_t stream) {
    const long long total = cw_total_blocks(a.B, a.H, a.W, a.N, 16, 16, 64), cus = lwg_device_cus();
    const dim3 grid((unsigned)(total < cus ? total : cus));
    return a.C1 > 0 ? cw_launch<lwg_conv_winograd_bf16_kernel<EPI, true>>(grid, WB_THREADS, WB_LDS_BYTES, stream, a)
                    : cw_launch<lwg_conv_winograd_bf16_kernel<EPI, false>>(grid, WB_THREADS, WB_LDS_BYTES, stream, a);
}

// Contract: include/lwg_hip.h, cwb_contract_ok (lwg_conv_wino.h).  Everything outside it is refused here, before any launch.
extern "C" int lwg_conv2d_winograd_bf16(const LwgConvArgs* pa, lwg_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!pa || !cwb_contract_ok(*pa)) return (int)hipErrorInvalidValue;
    if (pa->epi == LWG_EPI_SPADE) return wb_launch_epi<LWG_EPI_SPADE>(*pa, stream);
    if (pa->epi == LWG_EPI_RESIDUAL) return wb_launch_epi<LWG_EPI_RESIDUAL>(*pa, stream);
    return wb_launch_epi<LWG_EPI_NONE>(*pa, stream);
}
