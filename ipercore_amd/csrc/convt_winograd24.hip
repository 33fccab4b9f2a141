// nn.ConvTranspose2d(kernel 4, stride 2, padding 1) in fp32 as a fused F(2x4, 2x2) Winograd convolution on v_mfma_f32_32x32x2_f32 - the successor of
// convt_winograd.hip's F(2x2, 2x2) form with the same block footprint, staging and store paths - lwg_convt_wino.h.
//   Output parity (py, px) of the layer is a 2 x 2-tap convolution of the input: y[2i + py][2j + px] = sum_{r,q in {0,1}} x[i + py - 1 + r][j + px - 1 + q]
//   g_p[r][q].  Along rows F(2, 2) as in convt_winograd.hip (3 products for 2 outputs: row forms R0 = r0 - r1, R1 = r1, R2 = r2 - r1, R3 = r2,
//   R4 = r3 - r2 of the four staged rows; parity 0 uses R0 R1 R2, parity 1 -R2 R3 R4, the sign lives in the panel).  Along columns F(4, 2) with the
//   points {0, 1, -1, 1/2, inf} (5 products for 4 outputs), its data transform scaled to small integers (the factors live in the fp64 panel):
//     B^T = [[1,-2,-1,2,0], [0,-1,1,2,0], [0,1,-3,2,0], [0,-1,0,1,0], [0,1,-2,-1,2]],  A^T = [[1,1,1,1,0], [0,1,-1,1/2,0], [0,1,1,1/4,0], [0,1,-1,1/8,1]]
//   on the windows c0..c4 (parity 0) and c1..c5 (parity 1) of the six staged columns; parity 0's last row equals parity 1's first, so the two
//   parities need 9 column forms C0..C8 (parity px uses C(4 px + nu), nu = 0..4): 45 transformed values per (patch, input channel) serve 60
//   products per patch of 2 x 4 input pixels (convt_winograd.hip: 72).
// Workgroup: 512 threads = 8 waves; block = 8 x 4 patches (16 x 16 input pixels -> 32 x 32 output pixels) x 32 output channels.  Wave w has parity
// p = w % 4 and half h = w / 4: h = 0 owns the products (xi, nu), nu = 0..2 (9 accumulator tiles of 32 x 32, rows = output channels, columns =
// the block's 32 patches), h = 1 owns nu = 3, 4 (6 tiles); waves p and p + 4 share SIMD p: 15 products per k-pair and SIMD (F(2x2, 2x2): 18).
// The output transform over xi is register-local; the column transform has a partial sum in each half: h = 1 writes its partials into the epilogue's
// exchange buffer, h = 0 adds its own, the bias and the activation in place - then the shared store phase (lwg_convt_wino.h).
// A K stage is 8 input channels = four k-pairs; per k-pair a lane loads its weights (h = 0: two 16-byte loads and one 4-byte load, h = 1: one 16-byte
// and two 4-byte loads) from the panel Upk[4][Cin/8][4][2][15 N] (contiguous per load instruction; two k-pairs ahead, four register sets) and reads its
// V fragments (4 bytes each) from LDS.  The raw 18 x 18 x 8 halo goes global -> registers (three stages ahead) -> raw[s % 2]; each (patch, channel) is
// transformed by two threads - h = 0 threads rows 0..2 into R0..R2, h = 1 threads rows 2, 3 into R3, R4, nine column forms each - from raw[(s + 1) % 2]
// into Vs[(s + 1) % 2] beside the MFMAs of k-pairs 0 and 1; one barrier per stage, in the middle of k-pair 3.
// Rounding: the data transform multiplies by 2 and 3 only, the output transform by powers of two; panel entries are formed in fp64 and rounded once.
// fp32-grade, NOT the bits of the direct kernel or of convt_winograd.hip.
#include <hip/hip_runtime.h>
#include "lwg_common.h"
#include "lwg_convt_wino.h"       // the block footprint, the block walk, the halo staging, the store phase and the launch (shared with convt_winograd.hip)

#define NPATCH 32        // 8 x 4 patches of 2 x 4 input pixels per block
#define VSTR NPATCH
#define NFORM 45                             // [row form 0..4][column form 0..8]
#define VS_FLOATS (NFORM * KS * VSTR)        // [form][k][patch]
#define WSB() __builtin_amdgcn_sched_barrier(0)
// Who transforms what (profiles/f24_transform_balance.txt: the three layers at 32 / 8 / 4 frames, best of 5 x 10 launches, A/B twice, bitwise equal):
// h = 1 threads on rows 0..2 (R0..R2, 27 values) and h = 0 threads on rows 2, 3 (R3, R4, 18 values) 2.089 ms per pass; the heavier share on the
// waves with 9 MFMAs per k-pair (CTW24_TSWAP = 1, the product) 2.043 ms; the column transforms one row form per TWO MFMA slots over k-pairs 1 and 2
// (CTW24_TSPREAD = 1) 2.068 ms, with the swap 2.043 ms (not kept: no gain over the swap alone).  The F(2x2, 2x2) kernel: 2.305 ms.
#ifndef CTW24_TSWAP
#define CTW24_TSWAP 1
#endif
#ifndef CTW24_TSPREAD
#define CTW24_TSPREAD 0
#endif

// lab instrumentation (compiled out of the product): tools/up4ts24.py on a -DLWG_CTW24_TS build - every wave of a workgroup's SECOND block
// (steady state) writes its hardware id (SIMD id in bits 5:4) and four s_memtime stamps into args->res: [wg][wave][8] 64-bit words
#ifdef LWG_CTW24_TS
#define CTS24(i, v) do { if (lab_bi == 1 && lane == 0) reinterpret_cast<unsigned long long*>(const_cast<float*>(a.res))[((size_t)blockIdx.x * 8 + wid) * 8 + (i)] = (v); } while (0)
#else
#define CTS24(i, v) do { } while (0)
#endif

namespace {

// Where output pixel (ly, lx) of the block lies in row ly of the exchange buffer (rows of 32 pixel slots x 36 floats; the bank quad of slot s is
// 9 s mod 16).  A ds_write_b128 of the epilogue: eight consecutive lanes are patches etx = 0..3 of two patch rows ety = 2 m, 2 m + 1 - pixels
// lx = 8 etx + r (r fixed), ly = 4 ety + const: slots 4 r + etx and (4 r + etx) ^ 4, eight distinct bank quads.  The channel-quad-plane reader's 16-lane
// groups of 32 consecutive pixels land on sixteen distinct slots mod 16 (tests/test_convt_winograd24_cpu.py enumerates both).
__device__ __forceinline__ int ctw24_slot(int ly, int lx) {
    return ((lx & 7) * 4 + (lx >> 3)) ^ (((ly >> 2) & 1) << 2);
}

// the nine column forms of six staged columns (B^T above on c0..c4 and c1..c5; C4 is shared)
__device__ __forceinline__ void ctw24_cols(const float (&c)[6], float (&v)[9]) {
    const float d12 = c[2] - c[1], d23 = c[3] - c[2], d34 = c[4] - c[3];
    const float e13 = c[3] - c[1], e24 = c[4] - c[2];
    v[0] = (c[0] - c[2]) + 2.f * e13;
    v[1] = d12 + 2.f * c[3];
    v[2] = 2.f * d23 - d12;
    v[3] = e13;
    v[4] = 2.f * e24 - e13;
    v[5] = d23 + 2.f * c[4];
    v[6] = 2.f * d34 - d23;
    v[7] = e24;
    v[8] = 2.f * (c[5] - c[3]) - e24;
}

}  // namespace

__global__ __launch_bounds__(WG_THREADS, 1) void lwg_convt_winograd24_kernel(const LwgConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int Cin = a.C0, N = a.N;
    float* const raw0 = smem;                                // [2][RAW], then [2][VS] (45 planes of [k][patch])
    const int tid = threadIdx.x, lane = tid & 63;
    int blk = blockIdx.x;
    const int nst = Cin / KS;                                // even (host: Cin % 16 == 0)
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, (int)(240u * (unsigned)Cin * (unsigned)N), 0x00020000);
    const int par = wid & 3, py = par >> 1, px = par & 1;    // this wave's output parity
    const int hh = wid >> 2;                                 // ... and its half of the column products (0: nu = 0..2, 1: nu = 3, 4)
    floatx16 acc[9];                                         // h = 0: [3 xi + nu]; h = 1: [2 xi + nu - 3]
    // the workgroup's walk over its blocks and the per-block state (lwg_convt_wino.h; the XCD-aware order always on) and this lane's column
    // of the panel: the 16-byte part(s), the 4-byte part(s)
    CtwBlock<true> bk(a, tid, DUMP_OFF);
    unsigned uvoff, uvoffc;
    auto setup = [&](int id) {
        bk.setup(a, tid, id);
        // element (parity, stage, k-pair, k-half) = 15 N floats: [N][4] products 0-3, [N][4] products 4-7, [N] product 8 (h = 0), [N][4] products
        // 9-12, [N] product 13, [N] product 14 (h = 1)
        const unsigned kh = (unsigned)(lane >> 5) * 15u * (unsigned)N, n = (unsigned)(bk.n0 + (lane & 31));
        uvoff = (kh + (hh ? 9u * N : 0u) + 4u * n) * 4u;
        uvoffc = (kh + (hh ? 13u : 8u) * N + n) * 4u;
    };
    setup(blk);
    floatx4 rreg[2];
    floatx4 ufr[4][3];                                       // [register set = k-pair][16-byte parts | last part]: loaded TWO k-pairs ahead
    const unsigned ukk = (unsigned)N * 120u;                 // bytes between two k-pairs: [2][15 N] floats
    const unsigned upar = (unsigned)par * (unsigned)nst * 4u * ukk;
    const unsigned ubo = (unsigned)N * 16u;                  // h = 0: bytes from products 0-3 to products 4-7
    auto uld1 = [&](int st, int kk, int j, int h) -> floatx4 {      // (h: compile-time in the K loop)
        const unsigned so = upar + (unsigned)(st * 4 + kk) * ukk;
        floatx4 r;
        if (h == 0) {
            if (j < 2) return ctw_buf_load(ru, uvoff, so + (j ? ubo : 0u));
            r[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ru, (int)uvoffc, (int)so, 0));
            r[1] = r[2] = r[3] = 0.f;
            return r;
        }
        if (j == 0) return ctw_buf_load(ru, uvoff, so);
        r[0] = r[1] = r[2] = r[3] = 0.f;
        if (j == 1) {                                        // (two 4-byte loads: see DESIGN.md 3.12c on __builtin_amdgcn_raw_buffer_load_b64)
            r[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ru, (int)uvoffc, (int)so, 0));
            r[1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ru, (int)uvoffc, (int)(so + 4u * (unsigned)N), 0));
        }
        return r;
    };
    // transform threads: (patch, channel) = tid % 256; with CTW24_TSWAP h = 0 threads rows 0..2 of the 4-row patch -> row forms 0..2, h = 1 threads rows 2, 3 -> 3, 4
    const int patch = tid & 31, tc = (tid >> 5) & 7;
    const int pty = patch >> 2, ptx = patch & 3;
    unsigned dbs[2];                                         // this thread's first staged row inside raw[u] (float index into smem)
    unsigned vbs[2];                                         // ... its first row form's values inside Vs[u]
    unsigned fbs[2];                                         // this lane's fragments inside Vs[u]: form (2 py + xi, 4 px + 3 h + nu'), k-half, patch
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        dbs[u] = (unsigned)(u * RAW_FLOATS + tc * PLANE + (2 * pty + ((hh ^ CTW24_TSWAP) ? 0 : 2)) * HALO + 4 * ptx) >> 1;
        asm volatile("" : "+v"(dbs[u]));
        dbs[u] <<= 1;
        vbs[u] = (unsigned)(2 * RAW_FLOATS + u * VS_FLOATS + ((hh ^ CTW24_TSWAP) ? 0 : 27) * KS * VSTR + tc * VSTR + patch);
        asm volatile("" : "+v"(vbs[u]));
        fbs[u] = (unsigned)(2 * RAW_FLOATS + u * VS_FLOATS + (18 * py + 4 * px + 3 * hh) * KS * VSTR + (lane >> 5) * VSTR + (lane & 31));
        asm volatile("" : "+v"(fbs[u]));
    }
    float fb[2][9];                                          // [register set = k-pair % 2][product]

    // the K loop of one block for the waves of half HV (compile-time: 9 or 6 products, 2 or 3 staged rows / row forms per transform thread)
    auto kloop = [&](auto HC) {
        constexpr int HV = decltype(HC)::value;
        constexpr int NP = HV ? 6 : 9;                       // products per k-pair
        constexpr int NU = HV ? 2 : 3;                       // column products per row product
        constexpr int TV = HV ^ CTW24_TSWAP;                 // the transform role of this wave's threads (1: rows 0..2 -> R0..R2, 0: rows 2, 3 -> R3, R4)
        constexpr int NR = TV ? 3 : 2;                       // staged rows read / row forms written per transform thread
        auto fragread = [&](int buf, int kk) {
#pragma unroll
            for (int q = 0; q < NP; ++q) fb[kk & 1][q] = smem[fbs[buf] + ((9 * (q / NU) + q % NU) * KS + 2 * kk) * VSTR];
        };
        auto rowforms = [&](const float (&dd)[3][6], float (&t)[3][6]) {
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                if (TV) {
                    t[0][j] = dd[0][j] - dd[1][j];
                    t[1][j] = dd[1][j];
                    t[2][j] = dd[2][j] - dd[1][j];
                } else {
                    t[0][j] = dd[0][j];
                    t[1][j] = dd[1][j] - dd[0][j];
                }
            }
        };
        auto tstore = [&](int buf, int i, const float (&t)[3][6]) {
            float v[9];
            ctw24_cols(t[i], v);
            float* dst = smem + vbs[buf] + (9 * i) * KS * VSTR;
#pragma unroll
            for (int f = 0; f < 9; ++f) dst[f * KS * VSTR] = v[f];
        };
        auto ddread = [&](int buf, int i, float (&dd)[3][6]) {
#pragma unroll
            for (int j = 0; j < 6; ++j) dd[i][j] = smem[dbs[buf] + i * HALO + j];
        };
        auto iteration = [&](int s, auto SET, auto NXT) {
            constexpr int set = decltype(SET)::value;        // s % 2
            constexpr bool nxt = decltype(NXT)::value != 0;  // the last stage has no next one to prepare (peeled: no branches in the loop)
            const int s3 = s + 3 < nst ? s + 3 : nst - 1;    // past the end: a harmless re-load of the last stage (its halo store lands in a dead buffer)
            float dd[3][6], t[3][6];
            auto mf = [&](int kk, int q) {
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ufr[kk][q >> 2][q & 3], fb[kk & 1][q], acc[q], 0, 0, 0);
                WSB();
            };
            auto uldn = [&](int kk) {
                constexpr int NJ = HV ? 2 : 3;
                if (kk < 2) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) ufr[kk + 2][j] = uld1(s, kk + 2, j, HV);
                } else if (nxt) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) ufr[kk - 2][j] = uld1(s + 1, kk - 2, j, HV);
                }
                WSB();
            };
            // k-pair 0: next weights, next fragments; the halo of stage s + 2 -> raw[s % 2], the loads of stage s + 3; this thread's staged rows of
            // stage s + 1, one row per MFMA slot
            uldn(0);
            fragread(set, 1);
            WSB();
            mf(0, 0);
            if (nxt) { bk.rst1(raw0, set, 0, rreg[0]); rreg[0] = bk.rld1(s3, 0); }
            WSB();
            mf(0, 1);
            if (nxt) { bk.rst1(raw0, set, 1, rreg[1]); rreg[1] = bk.rld1(s3, 1); }
            WSB();
#pragma unroll
            for (int q = 2; q < NP; ++q) {
                mf(0, q);
                if (nxt && q - 2 < NR) ddread(set ^ 1, q - 2, dd);
                WSB();
            }
            if (nxt) rowforms(dd, t);
            WSB();
            // k-pair 1: the transform of stage s + 1 into Vs[(s + 1) % 2], one row form per MFMA slot
            uldn(1);
            fragread(set, 2);
            WSB();
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                mf(1, q);
                if (nxt && !CTW24_TSPREAD && q < NR) tstore(set ^ 1, q, t);
                if (nxt && CTW24_TSPREAD && q % 2 == 0 && q / 2 < (NR + 1) / 2) tstore(set ^ 1, q / 2, t);
                WSB();
            }
            // k-pair 2
            uldn(2);
            fragread(set, 3);
            WSB();
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                mf(2, q);
                if (nxt && CTW24_TSPREAD && q % 2 == 0 && (NR + 1) / 2 + q / 2 < NR) tstore(set ^ 1, (NR + 1) / 2 + q / 2, t);
                WSB();
            }
            // k-pair 3: the barrier in its middle, then the next stage's first fragments
            uldn(3);
#pragma unroll
            for (int q = 0; q < NP / 2; ++q) mf(3, q);
            __syncthreads();
            if (nxt) fragread(set ^ 1, 0);
            WSB();
#pragma unroll
            for (int q = NP / 2; q < NP; ++q) mf(3, q);
        };
        {   // stage 0's transform (raw[0] is staged and visible)
            float dd[3][6], t[3][6];
#pragma unroll
            for (int i = 0; i < NR; ++i) ddread(0, i, dd);
            rowforms(dd, t);
#pragma unroll
            for (int i = 0; i < NR; ++i) tstore(0, i, t);
        }
        __syncthreads();
        fragread(0, 0);
#pragma unroll
        for (int q = 0; q < NP; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
        int s = 0;
        for (; s + 2 < nst; s += 2) {
            iteration(s, IntT<0>(), IntT<1>());
            iteration(s + 1, IntT<1>(), IntT<1>());
        }
        iteration(s, IntT<0>(), IntT<0 + 1>());
        iteration(s + 1, IntT<1>(), IntT<0>());
    };

    floatx4 r0[2], r1[2];
    float bq;
    auto issue_loads = [&]() {
        bq = a.bias ? a.bias[bk.n0 + (tid & 31)] : 0.f;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            r0[q] = bk.rld1(0, q);
            r1[q] = bk.rld1(1, q);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            ufr[0][j] = uld1(0, 0, j, hh);
            ufr[1][j] = uld1(0, 1, j, hh);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) rreg[q] = bk.rld1(nst > 2 ? 2 : 1, q);
    };
    issue_loads();
#ifdef LWG_CTW24_TS
    int lab_bi = 0;
#endif
    for (;;) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        bk.rst1(raw0, 0, q, r0[q]);
        bk.rst1(raw0, 1, q, r1[q]);
    }
    if (tid < 32) smem[BIAS_OFF + tid] = bq;
    __syncthreads();
    CTS24(0, (unsigned long long)__builtin_amdgcn_s_getreg(63492));      // HW_ID (all 32 bits)
    CTS24(1, __builtin_readcyclecounter());
    if (hh == 0) kloop(IntT<0>()); else kloop(IntT<1>());
    CTS24(2, __builtin_readcyclecounter());
    const int eb = bk.b, ex0 = bk.x0, ey0 = bk.y0, en0 = bk.n0;          // this block's coordinates (the state moves on to the next block below)
    // epilogue: per output row ia of the patch the xi sums S[nu] = M[ia][nu] + M[ia + 1][nu]; the column transform A^T S is split - h = 1 writes
    // (S3, S3 / 2, S3 / 4, S3 / 8 + S4) into the exchange buffer, h = 0 adds (S0 + S1 + S2, S1 - S2, S1 + S2, S1 - S2), the bias, the activation.
    // Lane: patch lane % 32 (ety = patch / 4, etx = patch % 4), per register group g the four channels 8 g + 4 (lane / 32) ..
    int tide = tid;                                          // (an empty asm per block: the epilogue's address arithmetic stays out of the K loop)
    asm volatile("" : "+v"(tide));
    const int lanee = tide & 63;
    const int ety = (lanee & 31) >> 2, etx = lanee & 3;
    const int chl = 4 * (lanee >> 5);
    auto opix = [&](int ia, int ib) -> float* {               // pixel (ia, ib) of this lane's patch in the exchange buffer, its channel quad of group 0
        const int ly = 4 * ety + 2 * ia + py, lx = 8 * etx + 2 * ib + px;
        return smem + (ly * 32 + ctw24_slot(ly, lx)) * OROW + chl;
    };
    __syncthreads();                                         // every wave has read its last fragments: the loop's LDS is free
    if (hh == 1) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int ia = 0; ia < 2; ++ia) {
                floatx4 o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int r = 4 * g + k;
                    const float s3 = acc[2 * ia][r] + acc[2 * ia + 2][r], s4 = acc[2 * ia + 1][r] + acc[2 * ia + 3][r];
                    o[0][k] = s3;
                    o[1][k] = 0.5f * s3;
                    o[2][k] = 0.25f * s3;
                    o[3][k] = __builtin_fmaf(0.125f, s3, s4);
                }
#pragma unroll
                for (int ib = 0; ib < 4; ++ib) *reinterpret_cast<floatx4*>(opix(ia, ib) + 8 * g) = o[ib];
            }
    }
    __syncthreads();
    CTS24(3, __builtin_readcyclecounter());
    if (hh == 0) {
        lwg_act_dispatch(a.act, [&](auto ACTC) {             // (the activation resolved once per block: lwg_common.h)
        constexpr int EA = decltype(ACTC)::value;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const floatx4 bv = *reinterpret_cast<const floatx4*>(smem + BIAS_OFF + 8 * g + chl);
#pragma unroll
            for (int ia = 0; ia < 2; ++ia) {
                floatx4 o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int r = 4 * g + k;
                    const float s0 = acc[3 * ia][r] + acc[3 * ia + 3][r], s1 = acc[3 * ia + 1][r] + acc[3 * ia + 4][r];
                    const float s2 = acc[3 * ia + 2][r] + acc[3 * ia + 5][r];
                    o[0][k] = (s0 + s1) + s2;
                    o[1][k] = s1 - s2;
                    o[2][k] = s1 + s2;
                    o[3][k] = s1 - s2;
                }
#pragma unroll
                for (int ib = 0; ib < 4; ++ib) {
                    floatx4* dst = reinterpret_cast<floatx4*>(opix(ia, ib) + 8 * g);
                    const floatx4 pv = *dst;
                    floatx4 y;
#pragma unroll
                    for (int k = 0; k < 4; ++k) y[k] = lwg_act_c<EA>((o[ib][k] + pv[k]) + bv[k], a.act);
                    *dst = y;
                }
            }
        }
        });
    }
    // the next block of this workgroup: its first loads go out here and land under the stores below (as convt_winograd.hip)
    const int nblk = blk + (int)gridDim.x;
    const bool more = bk.has_block(nblk);
    setup(more ? nblk : blk);
    issue_loads();
    __syncthreads();
    // the block's outputs: exchange buffer -> global memory (lwg_convt_wino.h; default cache policy)
    ctw_store_block<0>(a, smem, tide, eb, ex0, ey0, en0, [](int ly, int lx) { return ctw24_slot(ly, lx); });
    CTS24(4, __builtin_readcyclecounter());
    if (!more) break;
#ifdef LWG_CTW24_TS
    ++lab_bi;
#endif
    blk = nblk;
    __syncthreads();                                         // every thread has read its outputs from the exchange buffer: raw[0] / raw[1] may be written
    }
}

// args: as lwg_conv_transpose4_winograd_f32 (Cin % 16 == 0, N % 32 == 0, ydt LWG_DT_F32 or LWG_DT_F32_Q4, ycoff / YC channel slices, ReLU / tanh /
// none), EXCEPT args->w = the F(2x4, 2x2) panel Upk[4][Cin/8][4][2][15 N] (ops._wwino_t24): per (parity 2 py + px, stage s, k-pair kk, k-half kh)
// [N][4] products 0-3, [N][4] products 4-7, [N] product 8, [N][4] products 9-12, [N] product 13, [N] product 14; product 3 xi + nu (nu < 3) / 9 + 2 xi + nu - 3
// (nu >= 3) of column n = sgn * (G_y g G_x^T)[xi][nu] with g[r][q] = w[c][n][3 - py - 2 r][3 - px - 2 q] of input channel c = 8 s + 2 kk + kh,
// G_y = [[1,0],[1,1],[0,1]], G_x = [[1,0],[1/2,1/2],[-1/6,1/6],[-8/3,-4/3],[0,1/2]] and sgn = (py == 1 && xi == 0 ? -1 : 1).
extern "C" int lwg_conv_transpose4_winograd24_f32(const LwgConvArgs* pa, lwg_stream_t stream) {
    static unsigned long long done = 0;
    return ctw_launch(lwg_convt_winograd24_kernel, pa, stream, 240ull, 0x7fffffffull, (size_t)(BIAS_OFF + 32) * 4, done);
}
