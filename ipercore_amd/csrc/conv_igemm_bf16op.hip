// NHWC implicit-GEMM convolution, fp32 in / fp32 out, with ONE bf16 product per multiply ("bf16 operands"): both fp32 operands are rounded to bf16
// (round to nearest even, the compiler's packed convert = tensor.bfloat16()) in registers on their way to LDS, the products run on
// v_mfma_f32_32x32x16_bf16 and accumulate in fp32; bias, activation, residual / ReLU mask stay fp32 (lwg_conv_epilogue.h as it is).  The opt-in
// "bf16_operands" mode of ops.conv_precision / trainers.TrainOpts.conv_precision; tests/convbf16op_emu.py is the definition.
//
// Same GEMM view, K order (32-channel chunk major, tap minor), gather machinery and D^T convention (weights as the row operand) as conv_igemm.hip;
// the weights are read from THAT kernel's fp32 panel w[k/4][n][k%4] - no panel of its own, nothing for a panel cache or a captured graph to refresh.
//
// Structure:
//   * 4 waves; tiles 128 x 128 (64 x 64 per wave), 128 x 64 (N % 128 != 0: four waves stacked in M) or 64 x 64 (launches that do not fill 256 CUs);
//   * a K-step is 32 channels of one tap = two MFMA k-steps of 16; a STAGE is two K-steps (64 k): ONE barrier per 4 MFMA k-steps, i.e. per 16
//     MFMAs per wave on the 128 x 128 tile (512 matrix-pipe cycles at 32 cycles per MFMA).  An odd K-step count leaves the last stage half empty: its
//     second half is neither loaded nor multiplied (a uniform branch);
//   * the loads of stage u + 1 (fp32, raw buffer loads; a padding tap gets the out-of-range offset of lwg_conv_direct.h and reads zeros) are issued
//     before the MFMAs of stage u, rounded and stored to the other LDS buffer after them;
//   * LDS image, both operands: [k-octet][row][8 bf16] - one ds_read_b128 is one MFMA operand (lane l: row l & 31, k-octet 2 h + (l >> 5) of MFMA
//     k-step h).  32 consecutive lanes read 512 contiguous bytes, so each of ds_read_b128's 16-lane groups covers 16 distinct 16-byte slots of the
//     256-byte bank row: conflict-free with no swizzle.  PADDING RULE: an A k-octet row is (BM + 2) slots - a 16-lane ds_write_b64 group writes
//     4 k-octets x 2 rows (8 channel quads x 2 pixels), and (BM + 2) * 16 = 32 (mod 128) puts those four 32-byte runs on four different quarters of
//     the 32 banks a store sees.  B rows are unpadded: lane pairs hold the two quads of one k-octet, 16 lanes write 128 contiguous bytes.
// What bounds it (128 x 128 tile, per MFMA): the operands arrive as fp32 - (128 + 128) rows x 32 k x 4 B = 32 KB per K-step and workgroup for 32
//   MFMAs = 1 KB per MFMA from L2 (the fp32 kernel: the same bytes for 16x the matrix-pipe time), against 0.25 KB for a bf16-storage kernel: like
//   the bf16 weight gradient this kernel is bound by its fp32 operand stream, not by the matrix pipe.  LDS: 8 ds_read_b128 per 8 MFMAs per wave = 1
//   read per MFMA (64 x 64 tile: 4 per 2 = 2 per MFMA), below the 2-per-gap issue rate that the LDS array sustains.  Barriers: ntaps * Cin / 64 + 2
//   per workgroup (one per stage, the tap table's, the prologue's).
// Split-K (the _ws form): blockIdx.y = slice of whole 32-channel chunks, dense [slice][M][N] slabs, added in slice order by lwg_splitk_finish_launch
//   (conv_igemm.hip) with bias / activation / ReLU mask: deterministic, no float atomics.  lwg_bf16op_split_plan below is the plan.
// The result is a function of the launch description alone: tile form, slice plan and summation order depend on nothing else.

#include "lwg_common.h"
#include "lwg_conv_args.h"
#include "lwg_conv_direct.h"
#include "lwg_conv_epilogue.h"

typedef __bf16 obf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int ouintx2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ floatx4 lwg_obuf_load(const void* base, unsigned bytes, unsigned voff, unsigned soff) {
    __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
    return __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}

// four fp32 -> four bf16 (round to nearest even), element 0 in the low half of word 0
__device__ __forceinline__ ouintx2 lwg_pk4_bf16(const floatx4 v) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    bf16x2_t lo, hi;
    lo[0] = (__bf16)v[0];
    lo[1] = (__bf16)v[1];
    hi[0] = (__bf16)v[2];
    hi[1] = (__bf16)v[3];
    return ouintx2{__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
}

// split_chunks > 0: blockIdx.y = K slice of split_chunks 32-channel chunks (all taps), raw sums to slabs[slice][M][N]; 0: the whole K range, epilogue
template <int WAVES_M, int WAVES_N, int TM, int TN, int EPI>
__global__ __launch_bounds__(256, 2) void lwg_conv_igemm_bf16op_kernel(const LwgConvArgs a, const int split_chunks, float* __restrict__ slabs) {
    constexpr unsigned OOB = (unsigned)LWG_BUF_RANGE;         // at or beyond any buffer's size (cd_contract_ok): the load returns zeros
    constexpr int BM = WAVES_M * TM * 32, BN = WAVES_N * TN * 32;
    constexpr int A_ROW = (BM + 2) * 16, B_ROW = BN * 16;     // bytes per k-octet row (padding rule: header)
    constexpr int A_STEP = 4 * A_ROW, B_STEP = 4 * B_ROW;     // a K-step = 32 k = 4 octets
    constexpr int A_STAGE = 2 * A_STEP, B_STAGE = 2 * B_STEP; // a stage = 2 K-steps
    constexpr int PA = BM / 32;                               // float4 loads per thread and K-step: A is BM rows x 8 quads, B is 8 quads x BN columns
    constexpr int PB = BN / 32;
    static_assert(WAVES_M * WAVES_N == 4, "4 waves per workgroup");

    extern __shared__ __attribute__((aligned(16))) char smem_o[];
    char* As = smem_o;
    char* Bs = smem_o + 2 * A_STAGE;
    int* taptab = reinterpret_cast<int*>(smem_o + 2 * A_STAGE + 2 * B_STAGE);  // [3][LWG_MAX_TAPS]: tap byte offset in x0, in x1, packed dy | dx

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WAVES_N, wn = wid % WAVES_N;
    const int tiles_n = a.N / BN;
    const int lid = lwg_xcd_remap(blockIdx.x, gridDim.x);
    const int tile_n = lid % tiles_n, tile_m = lid / tiles_n;
    const int m_base = tile_m * BM, n_base = tile_n * BN;

    // ---- per-thread gather coordinates: channel quad kq of the rows mrow + 32 p
    const int kq = tid & 7, mrow = tid >> 3;
    const int HW = a.OH * a.OW;
    const int Cin = a.C0 + a.C1;
    int pixlin[PA];
    unsigned long long vmask[PA];      // bit tap = the tap's sample lies inside the image (and the row is < M)
    {
        int piy[PA], pix[PA];
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const int m = m_base + mrow + 32 * p;
            const bool ok = m < a.M;
            const int mm = ok ? m : 0;
            const int b = mm / HW, rem = mm - b * HW;
            const int oy = rem / a.OW, ox = rem - oy * a.OW;
            piy[p] = ok ? oy * a.stride : -1000;
            pix[p] = ox * a.stride;
            pixlin[p] = (b * a.H + oy * a.stride) * a.W + ox * a.stride;
            vmask[p] = 0ull;
        }
        if (tid < a.ntaps) {
            const int dy = a.dy[tid], dx = a.dx[tid];
            taptab[tid] = (dy * a.W + dx) * a.C0 * 4;
            taptab[LWG_MAX_TAPS + tid] = (dy * a.W + dx) * a.C1 * 4;
            taptab[2 * LWG_MAX_TAPS + tid] = (dy & 0xffff) | (dx << 16);
        }
        __syncthreads();
        for (int tp = 0; tp < a.ntaps; ++tp) {
            const int packed = taptab[2 * LWG_MAX_TAPS + tp];
            const int dy = (int)(short)(packed & 0xffff), dx = packed >> 16;
#pragma unroll
            for (int p = 0; p < PA; ++p) {
                const int iy = piy[p] + dy, ix = pix[p] + dx;
                const bool ok = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                vmask[p] |= (unsigned long long)ok << tp;
            }
        }
    }

    const unsigned bytes0 = (unsigned)a.B * a.H * a.W * a.C0 * 4u;
    const unsigned bytes1 = (unsigned)a.B * a.H * a.W * a.C1 * 4u;
    const unsigned wbytes = (unsigned)a.ntaps * (unsigned)Cin * (unsigned)a.N * 4u;
    const int cc_first = split_chunks > 0 ? (int)blockIdx.y * split_chunks * 32 : 0;
    const int nsteps = (split_chunks > 0 ? (min(Cin - cc_first, split_chunks * 32) >> 5) : (Cin >> 5)) * a.ntaps;     // K-steps of 32
    const int nstages = (nsteps + 1) >> 1;

    // ---- loader state: the K-step whose loads are issued next (chunk major, tap minor)
    int ld_tap = 0, ld_cc = cc_first, ld_use1 = 0;
    unsigned ld_soffA = 0;
    unsigned ld_soffB = (unsigned)((cc_first >> 5) * a.ntaps) * (unsigned)a.N * 128u;      // a K-step of the panel: 8 quads x N x 16 bytes
    const float* ld_src = a.x0;
    unsigned ld_bytes = bytes0;
    unsigned pixb[PA], vbase[PA], wvoff[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p) {
        // item idx: lane pairs = the two quads of one k-octet of one column, so that a pair's two 8-byte stores fill one 16-byte LDS slot
        const int idx = tid + 256 * p;
        const int r = idx >> 1, n = r % BN, kqb = 2 * (r / BN) + (idx & 1);
        wvoff[p] = ((unsigned)kqb * a.N + n_base + n) * 16u;
    }
    auto source = [&]() {
        ld_use1 = ld_cc >= a.C0;
        const int cs = ld_use1 ? a.C1 : a.C0;
        ld_src = ld_use1 ? a.x1 : a.x0;
        ld_bytes = ld_use1 ? bytes1 : bytes0;
        ld_soffA = (unsigned)(ld_cc - (ld_use1 ? a.C0 : 0)) * 4u;
#pragma unroll
        for (int p = 0; p < PA; ++p) pixb[p] = ((unsigned)pixlin[p] * (unsigned)cs + (unsigned)kq * 4u) * 4u;
    };
    auto tap_rows = [&]() {
        const int toff = taptab[ld_use1 * LWG_MAX_TAPS + ld_tap];
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            const bool ok = (vmask[p] >> ld_tap) & 1ull;
            vbase[p] = ok ? pixb[p] + (unsigned)toff : OOB;
        }
    };
    auto advance = [&]() {
        ld_soffB += (unsigned)a.N * 128u;
        if (++ld_tap == a.ntaps) {
            ld_tap = 0;
            ld_cc += 32;
            ld_soffA += 128u;
            if (ld_cc == a.C0 && a.C1 > 0) source();
        }
        tap_rows();
    };

    floatx4 ra0[PA], rb0[PB], ra1[PA], rb1[PB];               // the two K-steps of the stage in flight
    auto gload = [&](floatx4 (&ra)[PA], floatx4 (&rb)[PB]) {
#pragma unroll
        for (int p = 0; p < PA; ++p) ra[p] = lwg_obuf_load(ld_src, ld_bytes, vbase[p], ld_soffA);
#pragma unroll
        for (int p = 0; p < PB; ++p) rb[p] = lwg_obuf_load(a.w, wbytes, wvoff[p], ld_soffB);
    };
    // the loads of stage u (K-steps 2u, 2u + 1); leaves the loader at K-step 2u + 2
    auto gload_stage = [&](int u) {
        gload(ra0, rb0);
        advance();
        if (2 * u + 1 < nsteps) {
            gload(ra1, rb1);
            advance();
        }
    };
    const int st_a = (kq >> 1) * A_ROW + mrow * 16 + (kq & 1) * 8;      // + 512 p
    const int st_b = tid * 8;                                           // + 2048 p: items are (octet, column, half)-linear
    auto lstore = [&](char* Ab, char* Bb, const floatx4 (&ra)[PA], const floatx4 (&rb)[PB]) {
#pragma unroll
        for (int p = 0; p < PA; ++p) *reinterpret_cast<ouintx2*>(Ab + st_a + 512 * p) = lwg_pk4_bf16(ra[p]);
#pragma unroll
        for (int p = 0; p < PB; ++p) *reinterpret_cast<ouintx2*>(Bb + st_b + 2048 * p) = lwg_pk4_bf16(rb[p]);
    };
    auto lstore_stage = [&](int u) {
        char* Ab = As + (u & 1) * A_STAGE;
        char* Bb = Bs + (u & 1) * B_STAGE;
        lstore(Ab, Bb, ra0, rb0);
        if (2 * u + 1 < nsteps) lstore(Ab + A_STEP, Bb + B_STEP, ra1, rb1);
    };

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int khalf = lane >> 5;
    const char* fr_a = As + khalf * A_ROW + (wm * TM * 32 + (lane & 31)) * 16;
    const char* fr_b = Bs + khalf * B_ROW + (wn * TN * 32 + (lane & 31)) * 16;
    // one K-step from LDS: two MFMA k-steps of TM x TN MFMAs, k-octets (2 h + khalf)
    auto kstep = [&](const char* pa, const char* pb) {
        obf16x8 fa[2][TM], fb[2][TN];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[h][i] = *reinterpret_cast<const obf16x8*>(pa + 2 * h * A_ROW + i * 512);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[h][j] = *reinterpret_cast<const obf16x8*>(pb + 2 * h * B_ROW + j * 512);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[h][j], fa[h][i], acc[i][j], 0, 0, 0);
    };

    source();
    tap_rows();
    gload_stage(0);
    lstore_stage(0);
    __syncthreads();
    for (int u = 0; u < nstages; ++u) {
        const bool next = u + 1 < nstages;
        if (next) gload_stage(u + 1);
        __builtin_amdgcn_sched_barrier(0);                    // the loads are issued before the MFMAs of this stage
        const char* pa = fr_a + (u & 1) * A_STAGE;
        const char* pb = fr_b + (u & 1) * B_STAGE;
        kstep(pa, pb);
        if (2 * u + 1 < nsteps) kstep(pa + A_STEP, pb + B_STEP);
        if (next) lstore_stage(u + 1);
        __syncthreads();
    }

    if (EPI == LWG_EPI_NONE && split_chunks > 0) {
        lwg_conv_epilogue_slab<TM, TN>(slabs + (size_t)blockIdx.y * a.M * a.N, a.M, a.N, acc, m_base, n_base, wm, wn, lane);
        return;
    }
    lwg_conv_epilogue<TM, TN, EPI>(a, acc, m_base, n_base, wm, wn, lane);
}

// ---- host side ----
// The tile form of a launch: 0 = 64 x 64 (fewer 128 x 128 tiles than the chip has CUs: four times the workgroups), 1 = 128 x 64 (N % 128 != 0),
// 2 = 128 x 128
static int lwg_bf16op_tile(const LwgConvArgs& a) {
    const long tiles128 = (long)((a.M + 127) / 128) * ((a.N + 127) / 128);
    if (tiles128 < 256) return 0;
    return a.N % 128 == 0 ? 2 : 1;
}

// Split-K plan (0 = run whole), from the rules of conv_igemm.hip's lwg_conv_split_plan: only launches on 64 x 64 tiles with fewer than 512 of
// them; plain epilogue or the ReLU mask (what the finishing kernel finishes); slices of whole 32-channel chunks with at least 8 K-steps each; aim
// at ~1024 workgroups, at most 8 slices.
static int lwg_bf16op_split_plan(const LwgConvArgs& a, int* chunks_per_slice) {
    const int Cin = a.C0 + a.C1;
    const bool mask = a.epi == LWG_EPI_RESIDUAL && a.act == LWG_ACT_RELU_MASK;
    if (a.M <= 0 || a.N <= 0 || a.N % 64 != 0 || a.ntaps < 1 || Cin <= 0 || Cin % 32 != 0 || (a.epi != LWG_EPI_NONE && !mask)) return 0;
    if (lwg_bf16op_tile(a) != 0) return 0;
    const long tiles = (long)((a.M + 63) / 64) * (a.N / 64);
    const int chunks = Cin / 32;
    if (tiles >= 512 || chunks < 2) return 0;
    int want = (int)((1024 + tiles - 1) / tiles);
    if (want > 8) want = 8;
    int cps = (chunks + want - 1) / want;
    while (cps * a.ntaps < 8 && cps < chunks) ++cps;
    const int slices = (chunks + cps - 1) / cps;
    if (slices < 2) return 0;
    *chunks_per_slice = cps;
    return slices;
}

template <int WAVES_M, int WAVES_N, int TM, int TN, int EPI>
static hipError_t launch_bf16op_cfg(const LwgConvArgs& a, hipStream_t stream, int slices, int cps, float* ws) {
    constexpr int BM = WAVES_M * TM * 32, BN = WAVES_N * TN * 32;
    constexpr size_t lds = (size_t)2 * 8 * ((BM + 2) * 16 + BN * 16) + 3 * LWG_MAX_TAPS * sizeof(int);
    const int tiles_m = (a.M + BM - 1) / BM, tiles_n = a.N / BN;
    return lwg_launch_lds<lwg_conv_igemm_bf16op_kernel<WAVES_M, WAVES_N, TM, TN, EPI>>(dim3(tiles_m * tiles_n, slices > 1 ? slices : 1), dim3(256), lds, stream, a,
                                                                                       slices > 1 ? cps : 0, ws);
}

template <int EPI>
static hipError_t launch_bf16op(const LwgConvArgs& a, hipStream_t stream) {
    const int tile = lwg_bf16op_tile(a);
    if (tile == 0) return launch_bf16op_cfg<2, 2, 1, 1, EPI>(a, stream, 0, 0, nullptr);
    if (tile == 2) return launch_bf16op_cfg<2, 2, 2, 2, EPI>(a, stream, 0, 0, nullptr);
    return launch_bf16op_cfg<4, 1, 1, 2, EPI>(a, stream, 0, 0, nullptr);
}

extern "C" size_t lwg_conv2d_bf16op_ws_floats(const LwgConvArgs* pa) {
    if (!pa || pa->M <= 0 || pa->N <= 0) return 0;
    int cps = 0;
    return (size_t)lwg_bf16op_split_plan(*pa, &cps) * (size_t)pa->M * (size_t)pa->N;
}

// ws: NULL, or lwg_conv2d_bf16op_ws_floats(args) floats - the launches the plan splits then run split-K through it.
extern "C" int lwg_conv2d_nhwc_f32_bf16op_ws(const LwgConvArgs* pa, float* ws, lwg_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!pa) return (int)hipErrorInvalidValue;
    const LwgConvArgs& a = *pa;
    // inputs beyond the 32-bit buffer-offset range: the same launch in batch slices (a workspace is sized for the whole launch: refused)
    if (const int e = cd_sliced(a, [&](const LwgConvArgs& s) { return ws ? 1 : lwg_conv2d_nhwc_f32_bf16op_ws(&s, nullptr, stream_); }); e >= 0) return e;
    // fp32 in, fp32 NHWC out; Cin % 32 == 0, a second input on 32 channels; the fp32 panel of 4 bytes per (k, n)
    if (!cd_contract_ok(a, CdEngine{LWG_DT_F32, LWG_DT_F32, 32, 32, 4, 4ull})) return (int)hipErrorInvalidValue;
    // plain or residual epilogue (the ReLU mask with the residual only)
    if (a.epi == LWG_EPI_SPADE || !cd_epilogue_ok(a, 128, false) || (a.act == LWG_ACT_RELU_MASK && a.epi != LWG_EPI_RESIDUAL)) return (int)hipErrorInvalidValue;
    int cps = 0;
    const int slices = ws ? lwg_bf16op_split_plan(a, &cps) : 0;
    if (slices > 1) {       // always the 64 x 64 form (the plan): slabs, then bias / activation / ReLU mask in the finishing kernel
        if (hipError_t e = launch_bf16op_cfg<2, 2, 1, 1, LWG_EPI_NONE>(a, stream, slices, cps, ws); e != hipSuccess) return (int)e;
        return (int)lwg_splitk_finish_launch(a, ws, slices, stream);
    }
    if (a.epi == LWG_EPI_RESIDUAL) return (int)launch_bf16op<LWG_EPI_RESIDUAL>(a, stream);
    return (int)launch_bf16op<LWG_EPI_NONE>(a, stream);
}

extern "C" int lwg_conv2d_nhwc_f32_bf16op(const LwgConvArgs* pa, lwg_stream_t stream_) { return lwg_conv2d_nhwc_f32_bf16op_ws(pa, nullptr, stream_); }
