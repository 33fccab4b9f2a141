// Weight gradient of the NHWC fp32 implicit-GEMM convolution with bf16 OPERANDS on the CDNA4 matrix cores (v_mfma_f32_32x32x16_bf16), fp32
// accumulation.  Opt-in (ops.WGRAD_PRECISION = "bf16"); bf16-operand grade, not the direct kernel's bits, deterministic.
//
// GEMM view as in csrc/conv_wgrad.hip:  dW[K, N] = A[M, K]^T * dY[M, N], the reduction runs over the M = B*OH*OW output positions; A is the
// forward pass's implicit operand, K in the forward panel's order (32-channel chunk major, tap minor).  x and dy stay fp32 in memory: both are
// gathered with raw buffer loads (hardware zero fill for the halo, ragged rows and the end of the range), rounded to bf16 in registers (plain
// casts: round to nearest even, the compiler's packed convert - what tensor.bfloat16() does) and exist as bf16 only in LDS.
//   * Workgroup = 4 waves, output tile 128 (k) x BN (n), BN = 128 (wave tile 64 x 64 = 2 x 2 MFMA tiles) or 64 (64 x 32) for the launches whose
//     last 128 columns would be half empty.  The M range of the workgroup is walked in chunks of 64 rows = 4 MFMA reduction steps.
//   * The operand layout.  Both MFMA operands want, per lane, 8 consecutive reduction indices of ONE channel, the memory rows are [m][channel].
//     The transpose happens in registers while staging: a thread loads one channel quad of 8 consecutive rows (8 loads of 16 bytes), packs the 8
//     values of each of its 4 channels along m and writes them to a [channel][m] bf16 image - one ds_write_b128 per channel; 8 adjacent lanes
//     write the 128 contiguous bytes of one channel row.  A fragment is then ONE ds_read_b128.  Channel rows are 144 bytes apart (64 rows + 8 of
//     padding): the 16 lanes of a ds_read_b128 group start on 16 different multiples of 4 banks (36 r mod 64, r = the 16 residues) - conflict
//     free.  Wave w gathers the w-th 32-k group of the tile, so tap and source tensor are wave-uniform (descriptor in SGPRs).
//   * Two LDS stages: the loads of chunk i + 1 are issued before the MFMAs of chunk i, their conversion and LDS writes follow them; one
//     barrier per chunk.
//   * The reduction is split over gridDim.y workgroups; the direct kernel's slabs, reduction, split plan and tile width: lwg_wgrad_slab.h.
//   * Bias gradient: the workgroups of k-tile 0 add up the fp32 dY values they load, BEFORE rounding.
#include <type_traits>

#include "lwg_common.h"
#include "lwg_conv_direct.h"
#include "lwg_wgrad_slab.h"

#define WGB_OOB 0xC0000000u
#define WGB_BR 64                                        // rows of a chunk
#define WGB_PITCH 72                                     // bf16 elements between the channel rows of an LDS image (144 bytes)

typedef __bf16 wgb_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 wgb_bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ floatx4 wgb_buf_load(const float* base, unsigned bytes, unsigned voff) {
    __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)bytes, 0x00020000);
    return __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, 0, 0));
}

// a: the FORWARD geometry (x0 / x1, taps, stride, OH / OW / M, N, YC, ycoff; dy dense: omul 1, YH == OH, YW == OW); a.y is unused.
// dy_: gradient of the forward output.  part: the slabs.
template <int BN>
__global__ __launch_bounds__(256, 2) void lwg_conv_wgrad_bf16_kernel(const LwgConvArgs a, const float* __restrict__ dy_, int Ktot,
                                                                    int chunks_per_split, float* __restrict__ part, int want_bias) {
    constexpr int BK = 128, BR = WGB_BR, P = WGB_PITCH;
    constexpr int NT = BN / 64;                          // 32-column MFMA tiles per wave
    constexpr int YR = BN / 16;                          // dY rows per thread and chunk: 8 (one row octet), or 4 (half an octet) for BN = 64
    constexpr int XIMG = BK * P, YIMG = BN * P;          // bf16 elements of one operand, one stage
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __bf16* Xs = reinterpret_cast<__bf16*>(smem_raw);    // [2][BK][P]
    __bf16* Ys = Xs + 2 * XIMG;                          // [2][BN][P]
    int* taptab = reinterpret_cast<int*>(Ys + 2 * YIMG); // packed dy | dx << 16

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, khalf = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = wid >> 1, wn = wid & 1;
    const int tiles_n = (a.N + BN - 1) / BN;
    const int tile_k = blockIdx.x / tiles_n, tile_n = blockIdx.x % tiles_n;
    const int k_base = tile_k * BK, n_base = tile_n * BN;
    if (tid < a.ntaps) taptab[tid] = (a.dy[tid] & 0xffff) | (a.dx[tid] << 16);
    __syncthreads();

    // ---- this thread's slice of the gather: rows moct * 8 .. + 7 of the chunk; channel quad kq of the wave's 32-k group; dY quad yq ----
    const int moct = tid & 7, kq = (tid >> 3) & 7;
    const int yq = BN == 128 ? tid >> 3 : (tid >> 3) & 15;           // column quad of the tile
    const int yrow0 = BN == 128 ? 0 : (tid >> 7) * 4;                // first dY row of the thread within its octet
    const int k0 = k_base + wid * 32;                                // first k of the wave's group (Ktot % 32 == 0: groups are whole)
    const bool gok = k0 < Ktot;
    const int G = gok ? k0 >> 5 : 0;                                 // group id = cchunk * ntaps + tap
    const int cchunk = G / a.ntaps, tap = G - cchunk * a.ntaps;
    const bool use1 = cchunk * 32 >= a.C0;                           // wave-uniform: a 32-channel chunk never straddles x0 | x1
    const float* xsrc = use1 ? a.x1 : a.x0;
    const int xcs = use1 ? a.C1 : a.C0;
    const unsigned xbytes = (unsigned)a.B * a.H * a.W * xcs * 4u;
    const unsigned ybytes = (unsigned)a.B * a.YH * a.YW * a.YC * 4u;
    const unsigned xpix = (unsigned)xcs * 4u;
    const unsigned xlane = (unsigned)(cchunk * 32 - (use1 ? a.C0 : 0) + kq * 4) * 4u;
    const unsigned ypix = (unsigned)a.YC * 4u;
    const unsigned ylane = (unsigned)(a.ycoff + n_base + yq * 4) * 4u;
    const bool yok = n_base + yq * 4 < a.N;
    const int tdy = (int)(short)(taptab[tap] & 0xffff), tdx = taptab[tap] >> 16;

    const int nchunks_total = (a.M + BR - 1) / BR;
    const int c_begin = blockIdx.y * chunks_per_split;
    const int c_end = min(nchunks_total, c_begin + chunks_per_split);

    // the thread's first GEMM row of the chunk being loaded: (image, oy, ox), advanced without divisions
    int rm = c_begin * BR + moct * 8;
    int rb, roy, rox;
    {
        const int mm = rm < a.M ? rm : 0;
        const int HW = a.OH * a.OW;
        rb = mm / HW;
        const int rem = mm - rb * HW;
        roy = rem / a.OW;
        rox = rem - roy * a.OW;
    }
    floatx4 rx[8], ry[YR];
    const bool do_bias = want_bias != 0 && tile_k == 0;
    floatx4 cs = {0.f, 0.f, 0.f, 0.f};
    auto gload = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int iy = roy * a.stride + tdy, ix = rox * a.stride + tdx;
            const bool ok = gok && rm + j < a.M && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const unsigned off = (unsigned)((rb * a.H + iy) * a.W + ix) * xpix + xlane;
            rx[j] = wgb_buf_load(xsrc, xbytes, ok ? off : WGB_OOB);
            if (++rox == a.OW) {
                rox = 0;
                if (++roy == a.OH) { roy = 0; ++rb; }
            }
        }
#pragma unroll
        for (int j = 0; j < YR; ++j) {
            const int row = rm + yrow0 + j;
            ry[j] = wgb_buf_load(dy_, ybytes, yok && row < a.M ? (unsigned)row * ypix + ylane : WGB_OOB);
        }
        rm += BR;                                        // the row state stands 8 rows on: 56 more to the next chunk's first row
        rox += BR - 8;
        while (rox >= a.OW) {
            rox -= a.OW;
            if (++roy == a.OH) { roy = 0; ++rb; }
        }
    };
    // round to bf16, pack along m, write the [channel][m] images of stage buf
    auto tstore = [&](int buf) __attribute__((always_inline)) {
        __bf16* xb = Xs + buf * XIMG + ((wid * 8 + kq) * 4) * P + moct * 8;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            wgb_bf16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (__bf16)rx[j][c];
            *reinterpret_cast<wgb_bf16x8*>(xb + c * P) = v;
        }
        __bf16* yb = Ys + buf * YIMG + (yq * 4) * P + moct * 8 + yrow0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if constexpr (YR == 8) {
                wgb_bf16x8 v;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (__bf16)ry[j][c];
                *reinterpret_cast<wgb_bf16x8*>(yb + c * P) = v;
            } else {
                wgb_bf16x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (__bf16)ry[j][c];
                *reinterpret_cast<wgb_bf16x4*>(yb + c * P) = v;
            }
        }
        if (do_bias) {
#pragma unroll
            for (int j = 0; j < YR; ++j) cs += ry[j];
        }
    };

    floatx16 acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragments of reduction step s: lane (r, h) reads rows 16 s + 8 h .. + 7 of channel r of the operand tile - one ds_read_b128
    const __bf16* fx = Xs + (wk * 64 + l31) * P + khalf * 8;
    const __bf16* fy = Ys + (wn * (BN / 2) + l31) * P + khalf * 8;
    auto mfma_chunk = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < BR / 16; ++s) {
            wgb_bf16x8 fa[2], fb[NT];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const wgb_bf16x8*>(fx + buf * XIMG + i * 32 * P + s * 16);
#pragma unroll
            for (int j = 0; j < NT; ++j) fb[j] = *reinterpret_cast<const wgb_bf16x8*>(fy + buf * YIMG + j * 32 * P + s * 16);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
    };

    if (c_begin < c_end) {
        gload();
        tstore(0);
        __syncthreads();
        // the chunk loop is unrolled by two so the LDS stage is a compile-time constant (base register + immediate)
        auto chunk = [&](auto cur_c, bool next) __attribute__((always_inline)) {
            constexpr int CUR = decltype(cur_c)::value;
            if (next) gload();                           // chunk i + 1's loads in flight during chunk i's MFMAs
            mfma_chunk(CUR);
            if (next) tstore(CUR ^ 1);                   // stage CUR ^ 1 was last read before the previous barrier
            __syncthreads();
        };
        using k0c = std::integral_constant<int, 0>;
        using k1c = std::integral_constant<int, 1>;
        int c = c_begin;
        for (; c + 2 <= c_end; c += 2) {
            chunk(k0c{}, true);
            chunk(k1c{}, c + 2 < c_end);
        }
        if (c < c_end) chunk(k0c{}, false);
    }
    // ---- partial tile -> slab blockIdx.y.  Lane owns column n = lane & 31, rows k = (r & 3) + 8 (r >> 2) + 4 khalf ----
    float* slab = lwg_wgrad_slab(part, blockIdx.y, Ktot, a.N);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k_base + wk * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
            if (k >= Ktot) continue;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = n_base + wn * (BN / 2) + j * 32 + l31;
                if (n < a.N) slab[(size_t)k * a.N + n] = acc[i][j][r];
            }
        }
    if (do_bias) {   // the threads' partial column sums through LDS, added in a fixed order (deterministic)
        constexpr int PARTS = 256 * 4 / BN;              // partial sums per column: 8, or 16 for BN = 64
        float* red = reinterpret_cast<float*>(smem_raw); // [PARTS][BN]; every LDS read of the chunk loop lies before its last barrier
        *reinterpret_cast<floatx4*>(red + ((BN == 128 ? 0 : (tid >> 7) * 8) + moct) * BN + yq * 4) = cs;
        __syncthreads();
        if (tid < BN && n_base + tid < a.N) {
            float t = red[tid];
#pragma unroll
            for (int r = 1; r < PARTS; ++r) t += red[r * BN + tid];
            slab[(size_t)Ktot * a.N + n_base + tid] = t;
        }
    }
}

// The contract of lwg_conv2d_wgrad_bf16_f32 (include/lwg_hip.h); host only, touches no device.
static bool wgb_contract_ok(const LwgConvArgs& a) {
    if (!a.x0 || a.B <= 0 || a.H <= 0 || a.W <= 0 || a.OH <= 0 || a.OW <= 0 || a.C0 <= 0 || (a.C0 % 32) != 0 || a.C1 < 0 || (a.C1 % 32) != 0 ||
        (a.C1 > 0 && !a.x1) || a.N <= 0 || (a.N % 64) != 0 || a.ntaps < 1 || a.ntaps > LWG_MAX_TAPS || a.stride < 1 || a.omul != 1 || a.ooy != 0 ||
        a.oox != 0 || a.YH != a.OH || a.YW != a.OW || (long long)a.M != (long long)a.B * a.OH * a.OW || a.xdt != LWG_DT_F32 || a.ydt != LWG_DT_F32 ||
        a.ycoff < 0 || (a.ycoff & 3) || (a.YC & 3) || a.ycoff + a.N > a.YC)
        return false;
    return cd_inputs_fit(a, 4ull) && lwg_buf_fits((unsigned long long)a.B * a.YH * a.YW * (unsigned long long)a.YC * 4ull);
}

// a function of the launch shape and the CU count only
static LwgSplitPlan wgb_splits(const LwgConvArgs& a, int cus) {
    const int Ktot = a.ntaps * (a.C0 + a.C1);
    return lwg_wgrad_split_plan(lwg_wgrad_tiles(Ktot, a.N), (a.M + WGB_BR - 1) / WGB_BR, 2 * cus, (long long)lwg_wgrad_slab_floats(Ktot, a.N) * 4, 48ll << 20);
}

extern "C" size_t lwg_conv2d_wgrad_bf16_ws_floats(const LwgConvArgs* pa) {
    if (!pa || !wgb_contract_ok(*pa)) return 0;
    return (size_t)wgb_splits(*pa, lwg_device_cus()).splits * lwg_wgrad_slab_floats(pa->ntaps * (pa->C0 + pa->C1), pa->N);
}

extern "C" int lwg_conv2d_wgrad_bf16_f32(const LwgConvArgs* pa, const float* dy, float* ws, float* dw, int D0, int D1, int KH, int KW,
                                         int transposed, const int* kidx, int cin, int nout, float* db, lwg_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    LwgUnpackMap u;
    if (!pa || !dy || !ws || !dw || !wgb_contract_ok(*pa) || !lwg_wgrad_unpack_map_make(pa, D0, D1, KH, KW, transposed, kidx, cin, nout, &u))
        return (int)hipErrorInvalidValue;
    const LwgConvArgs& a = *pa;
    const int Ktot = a.ntaps * (a.C0 + a.C1), bn = lwg_wgrad_bn(a.N);
    const LwgSplitPlan plan = wgb_splits(a, lwg_device_cus());
    const dim3 grid(lwg_wgrad_tiles(Ktot, a.N), plan.splits);
    const size_t lds = (size_t)2 * (128 + bn) * WGB_PITCH * 2 + LWG_MAX_TAPS * sizeof(int);
    const hipError_t e = bn == 64 ? lwg_launch_lds<lwg_conv_wgrad_bf16_kernel<64>>(grid, dim3(256), lds, stream, a, dy, Ktot, plan.cps, ws, db ? 1 : 0)
                                  : lwg_launch_lds<lwg_conv_wgrad_bf16_kernel<128>>(grid, dim3(256), lds, stream, a, dy, Ktot, plan.cps, ws, db ? 1 : 0);
    if (e != hipSuccess) return (int)e;
    lwg_wgrad_reduce_unpack(ws, plan.splits, u, dw, db, stream);
    return (int)hipGetLastError();
}
