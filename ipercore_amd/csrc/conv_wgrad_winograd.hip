// Weight gradient of the 3x3 / stride 1 / pad 1 NHWC fp32 convolution in F(2x2, 3x3) Winograd form on the CDNA4 matrix cores
// (v_mfma_f32_32x32x2_f32): 16 products per 2x2 output tile and (input channel, output channel) pair where the direct form
// (csrc/conv_wgrad.hip) spends 36.  Opt-in (ops.WGRAD_PRECISION = "winograd"); fp32-grade, not the direct kernel's bits.
//
//   V_t = B^T d_t B        d_t: the 4 x 4 input patch of tile t (2 x 2 outputs) with its 1-pixel halo, zero outside the image
//   Z_t = A dy_t A^T       dy_t: the tile's 2 x 2 output gradients, zero beyond a ragged edge
//   dU[xi, nu][c][n] = sum_t V_t[xi, nu][c] Z_t[xi, nu][n]        16 GEMMs, the reduction runs over all tiles of all images
//   dw[n][c] = G^T dU[., .][c][n] G                               (3 x 3)
//   B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]], A^T = [[1,1,1,0],[0,1,-1,-1]], G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]
//
//   * Workgroup = 8 waves, a 64 (c) x 64 (n) block of all 16 positions (xi, nu); wave w owns positions 2w and 2w + 1, each 2 x 2 MFMA
//     tiles (128 accumulator registers).  The tile range of the workgroup is walked in chunks of 8 tiles = 4 MFMA reduction steps.
//   * Neither V nor Z exists in memory: wave w gathers tile w of the chunk - lane = channel, the 16 patch pixels and the 4 dy pixels as
//     20 raw buffer loads of 256 contiguous bytes (hardware zero fill for the halo, ragged tiles and the end of the range) -, transforms
//     in registers and writes V[16][8][64] | Z[16][8][64] to LDS.  Two LDS stages: the loads of chunk i + 1 are issued before the MFMAs
//     of chunk i, their transforms and LDS writes follow them; one barrier per chunk.
//   * The reduction is split over gridDim.y workgroups; each writes its partial dU block to a workspace slab [16][Cin][N] and
//     lwg_wgw_reduce_kernel adds the slabs in slab order (deterministic - no float atomics), applies G^T . G and writes nn.Conv2d's
//     (nout, cin, 3, 3) layout.
#include <type_traits>

#include "lwg_common.h"
#include "lwg_conv_direct.h"
#include "lwg_wgrad_slab.h"

#define WGW_OOB 0xC0000000u
#define WGW_CT 8                                         // tiles per chunk
#define WGW_PLANE (WGW_CT * 64)                          // floats of one position of one operand
#define WGW_STAGE (2 * 16 * WGW_PLANE)                   // floats of one stage: V | Z

__device__ __forceinline__ float wgw_buf_load(const float* base, unsigned bytes, unsigned voff) {
    __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)bytes, 0x00020000);
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, 0, 0));
}

// a: the FORWARD geometry (x0 / x1, C0 / C1, B, H, W, N, YC, ycoff); dy_: gradient of the forward output (B, H, W, YC).
// part: [gridDim.y][16][C0 + C1][N] partial sums.  TH x TW tiles per image, T tiles in all, chunks_per_split chunks per workgroup.
__global__ __launch_bounds__(512) void lwg_conv_wgrad_winograd_kernel(const LwgConvArgs a, const float* __restrict__ dy_, int TH, int TW, int T,
                                                                     int chunks_per_split, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [2][V | Z][16][8][64]
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, khalf = lane >> 5;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nblocks = a.N >> 6;
    const int c_base = (blockIdx.x / nblocks) * 64, n_base = (blockIdx.x % nblocks) * 64;
    const int Ctot = a.C0 + a.C1;

    // ---- the gather: this wave's tile of the chunk, this lane's channel of the block (workgroup-uniform source: C0 % 64 == 0) ----
    const bool use1 = c_base >= a.C0;
    const float* xsrc = use1 ? a.x1 : a.x0;
    const int xcs = use1 ? a.C1 : a.C0;
    const unsigned xbytes = (unsigned)a.B * a.H * a.W * xcs * 4u;
    const unsigned ybytes = (unsigned)a.B * a.H * a.W * a.YC * 4u;
    const unsigned xlane = (unsigned)((use1 ? c_base - a.C0 : c_base) + lane) * 4u;
    const unsigned ylane = (unsigned)(a.ycoff + n_base + lane) * 4u;
    const unsigned xpix = (unsigned)xcs * 4u, ypix = (unsigned)a.YC * 4u;

    const int nchunks_total = (T + WGW_CT - 1) / WGW_CT;
    const int c_begin = blockIdx.y * chunks_per_split;
    const int c_end = min(nchunks_total, c_begin + chunks_per_split);
    const int t_end = min(T, c_end * WGW_CT);

    int tcur = c_begin * WGW_CT + wid;                   // the tile this wave loads next: (image tb, tile row tty, tile column ttx)
    int tb, tty, ttx;
    {
        const int tt = tcur < T ? tcur : 0;
        tb = tt / (TH * TW);
        const int rem = tt - tb * TH * TW;
        tty = rem / TW;
        ttx = rem - tty * TW;
    }
    float rx[16], ry[4];
    auto gload = [&]() {
        const bool tv = tcur < t_end;
        const int iy0 = 2 * tty - 1, ix0 = 2 * ttx - 1;
        const int prow = tb * a.H;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int iy = iy0 + i, ix = ix0 + j;
                const bool ok = tv && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                const unsigned off = (unsigned)((prow + iy) * a.W + ix) * xpix + xlane;
                rx[i * 4 + j] = wgw_buf_load(xsrc, xbytes, ok ? off : WGW_OOB);
            }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int oy = iy0 + 1 + i, ox = ix0 + 1 + j;
                const bool ok = tv && oy < a.H && ox < a.W;
                const unsigned off = (unsigned)((prow + oy) * a.W + ox) * ypix + ylane;
                ry[i * 2 + j] = wgw_buf_load(dy_, ybytes, ok ? off : WGW_OOB);
            }
        tcur += WGW_CT;                                  // advance to the next chunk's tile without divisions
        ttx += WGW_CT;
        while (ttx >= TW) {
            ttx -= TW;
            if (++tty == TH) { tty = 0; ++tb; }
        }
    };
    // V = B^T d B and Z = A dy A^T of the loaded tile -> stage buf, row wid of every position
    auto tstore = [&](int buf) {
        float* vs = smem + buf * WGW_STAGE + wid * 64 + lane;
        float* zs = vs + 16 * WGW_PLANE;
        float t[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                    // columns: t = B^T d
            t[0 * 4 + j] = rx[0 * 4 + j] - rx[2 * 4 + j];
            t[1 * 4 + j] = rx[1 * 4 + j] + rx[2 * 4 + j];
            t[2 * 4 + j] = rx[2 * 4 + j] - rx[1 * 4 + j];
            t[3 * 4 + j] = rx[1 * 4 + j] - rx[3 * 4 + j];
        }
#pragma unroll
        for (int x = 0; x < 4; ++x) {                    // rows: V = t B
            vs[(x * 4 + 0) * WGW_PLANE] = t[x * 4 + 0] - t[x * 4 + 2];
            vs[(x * 4 + 1) * WGW_PLANE] = t[x * 4 + 1] + t[x * 4 + 2];
            vs[(x * 4 + 2) * WGW_PLANE] = t[x * 4 + 2] - t[x * 4 + 1];
            vs[(x * 4 + 3) * WGW_PLANE] = t[x * 4 + 1] - t[x * 4 + 3];
        }
        const float u[4][2] = {{ry[0], ry[1]}, {ry[0] + ry[2], ry[1] + ry[3]}, {ry[0] - ry[2], ry[1] - ry[3]}, {-ry[2], -ry[3]}};   // A dy
#pragma unroll
        for (int x = 0; x < 4; ++x) {                    // Z = u A^T
            zs[(x * 4 + 0) * WGW_PLANE] = u[x][0];
            zs[(x * 4 + 1) * WGW_PLANE] = u[x][0] + u[x][1];
            zs[(x * 4 + 2) * WGW_PLANE] = u[x][0] - u[x][1];
            zs[(x * 4 + 3) * WGW_PLANE] = -u[x][1];
        }
    };

    floatx16 acc[2][2][2];                               // [position of the wave][32 channels][32 columns]
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[q][i][j][r] = 0.f;

    // fragments of reduction step s: lanes 0-31 tile 2s of the chunk, lanes 32-63 tile 2s + 1; one ds_read_b32 per 32 x 32 operand tile
    const float* fv = smem + (2 * wid) * WGW_PLANE + khalf * 64 + l31;
    auto mfma_chunk = [&](int buf) {
#pragma unroll
        for (int s = 0; s < WGW_CT / 2; ++s)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float* v = fv + buf * WGW_STAGE + q * WGW_PLANE + 2 * s * 64;
                const float* z = v + 16 * WGW_PLANE;
                const float fa0 = v[0], fa1 = v[32], fb0 = z[0], fb1 = z[32];
                acc[q][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0, fb0, acc[q][0][0], 0, 0, 0);
                acc[q][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0, fb1, acc[q][0][1], 0, 0, 0);
                acc[q][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1, fb0, acc[q][1][0], 0, 0, 0);
                acc[q][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1, fb1, acc[q][1][1], 0, 0, 0);
            }
    };

    if (c_begin < c_end) {
        gload();
        tstore(0);
        __syncthreads();
        // the chunk loop is unrolled by two so the LDS stage is a compile-time constant (base register + immediate)
        auto chunk = [&](auto cur_c, bool next) {
            constexpr int CUR = decltype(cur_c)::value;
            if (next) gload();                           // chunk i + 1's loads in flight during chunk i's MFMAs
            mfma_chunk(CUR);
            if (next) tstore(CUR ^ 1);                   // stage CUR ^ 1 was last read before the previous barrier
            __syncthreads();
        };
        using k0 = std::integral_constant<int, 0>;
        using k1 = std::integral_constant<int, 1>;
        int c = c_begin;
        for (; c + 2 <= c_end; c += 2) {
            chunk(k0{}, true);
            chunk(k1{}, c + 2 < c_end);
        }
        if (c < c_end) chunk(k0{}, false);
    }
    // ---- partial dU -> workspace slab blockIdx.y.  Lane owns column n = lane & 31, rows c = (r & 3) + 8 (r >> 2) + 4 khalf ----
    float* slab = part + (size_t)blockIdx.y * 16 * Ctot * a.N;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        float* sp = slab + ((size_t)(2 * wid + q) * Ctot + c_base) * a.N + n_base + l31;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cc = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
#pragma unroll
                for (int j = 0; j < 2; ++j) sp[(size_t)cc * a.N + j * 32] = acc[q][i][j][r];
            }
    }
}

// dw[n][c][3][3] = G^T (sum over the slabs, in slab order, of dU[16][c][n]) G for c < cin, n < nout.  G lanes share an element - lane g adds
// slabs g, g + G, ... - and a fixed-order LDS pass adds the G partial sums (the association depends only on (nsplit, G): deterministic), as
// lwg_slab_reduce_unpack4g_kernel does: the slab volume is 16/9 of the direct kernel's.
template <int G>
__global__ __launch_bounds__(256) void lwg_wgw_reduce_kernel(const float* __restrict__ part, int nsplit, size_t slab, int Ctot, int Npad, int cin, int nout,
                                                             float* __restrict__ dw) {
    constexpr int EPB = 256 / G;
    __shared__ float sh[G > 1 ? 16 : 1][256];
    const int e = threadIdx.x % EPB, g = threadIdx.x / EPB;
    const size_t i = (size_t)blockIdx.x * EPB + e;
    const bool live = i < (size_t)cin * nout;
    const int n = live ? (int)(i % nout) : 0, c = live ? (int)(i / nout) : 0;
    const float* src = part + (size_t)c * Npad + n;
    const size_t plane = (size_t)Ctot * Npad;
    float u[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) u[p] = 0.f;
    if (live)
        for (int k = g; k < nsplit; k += G) {
            const float* s = src + (size_t)k * slab;
#pragma unroll
            for (int p = 0; p < 16; ++p) u[p] += s[p * plane];
        }
    if (G > 1) {
#pragma unroll
        for (int p = 0; p < 16; ++p) sh[p][threadIdx.x] = u[p];
        __syncthreads();
        if (g != 0) return;
#pragma unroll
        for (int j = 1; j < G; ++j)
#pragma unroll
            for (int p = 0; p < 16; ++p) u[p] += sh[p][j * EPB + e];
    }
    if (!live) return;
    float m[3][4];                                        // G^T dU
#pragma unroll
    for (int nu = 0; nu < 4; ++nu) {
        const float h = 0.5f * (u[4 + nu] + u[8 + nu]);
        m[0][nu] = u[nu] + h;
        m[1][nu] = 0.5f * (u[4 + nu] - u[8 + nu]);
        m[2][nu] = h + u[12 + nu];
    }
    float* o = dw + ((size_t)n * cin + c) * 9;
#pragma unroll
    for (int k = 0; k < 3; ++k) {                         // (G^T dU) G
        const float h = 0.5f * (m[k][1] + m[k][2]);
        o[3 * k + 0] = m[k][0] + h;
        o[3 * k + 1] = 0.5f * (m[k][1] - m[k][2]);
        o[3 * k + 2] = h + m[k][3];
    }
}

// The contract of lwg_conv2d_wgrad_winograd_f32 (include/lwg_hip.h); host only, touches no device.
static bool wgw_contract_ok(const LwgConvArgs& a) {
    if (!a.x0 || a.B <= 0 || a.H <= 0 || a.W <= 0 || a.C0 <= 0 || (a.C0 % 64) != 0 || a.C1 < 0 || (a.C1 % 64) != 0 || (a.C1 > 0 && !a.x1) || a.N <= 0 ||
        (a.N % 64) != 0 || a.ntaps != 9 || a.stride != 1 || a.omul != 1 || a.ooy != 0 || a.oox != 0 || a.OH != a.H || a.OW != a.W || a.YH != a.H ||
        a.YW != a.W || (long long)a.M != (long long)a.B * a.H * a.W || a.xdt != LWG_DT_F32 || a.ydt != LWG_DT_F32 || a.ycoff < 0 || a.ycoff + a.N > a.YC)
        return false;
    for (int t = 0; t < 9; ++t)
        if (a.dy[t] != t / 3 - 1 || a.dx[t] != t % 3 - 1) return false;
    const unsigned long long pix = (unsigned long long)a.B * a.H * a.W;
    if (pix * (unsigned long long)(a.C0 > a.C1 ? a.C0 : a.C1) * 4ull >= (unsigned long long)WGW_OOB) return false;
    if (pix * (unsigned long long)a.YC * 4ull >= (unsigned long long)WGW_OOB) return false;
    return true;
}

static int wgw_tiles(const LwgConvArgs& a) { return a.B * ((a.H + 1) / 2) * ((a.W + 1) / 2); }

// a function of the launch shape and the CU count only (lwg_wgrad_slab.h: the plan)
static LwgSplitPlan wgw_splits(const LwgConvArgs& a, int cus) {
    return lwg_wgrad_split_plan(((a.C0 + a.C1) / 64) * (a.N / 64), (wgw_tiles(a) + WGW_CT - 1) / WGW_CT, cus, 64ll * (a.C0 + a.C1) * a.N, 64ll << 20);
}

extern "C" size_t lwg_conv2d_wgrad_winograd_ws_floats(const LwgConvArgs* pa) {
    if (!pa || !wgw_contract_ok(*pa)) return 0;
    return (size_t)wgw_splits(*pa, lwg_device_cus()).splits * 16 * (size_t)(pa->C0 + pa->C1) * pa->N;
}

extern "C" int lwg_conv2d_wgrad_winograd_f32(const LwgConvArgs* pa, const float* dy, float* ws, float* dw, int cin, int nout, lwg_stream_t stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!pa || !dy || !ws || !dw || !wgw_contract_ok(*pa) || cin < 1 || nout < 1 || cin > pa->C0 + pa->C1 || nout > pa->N) return (int)hipErrorInvalidValue;
    const LwgConvArgs& a = *pa;
    const int Ctot = a.C0 + a.C1;
    const int TH = (a.H + 1) / 2, TW = (a.W + 1) / 2, T = wgw_tiles(a);
    const LwgSplitPlan plan = wgw_splits(a, lwg_device_cus());
    const int splits = plan.splits;
    const size_t lds = (size_t)2 * WGW_STAGE * sizeof(float);
    if (hipError_t e = lwg_launch_lds<lwg_conv_wgrad_winograd_kernel>(dim3((Ctot / 64) * (a.N / 64), splits), dim3(512), lds, stream, a, dy, TH, TW, T, plan.cps, ws); e != hipSuccess) return (int)e;
    const size_t slab = (size_t)16 * Ctot * a.N, total = (size_t)cin * nout;
    if (total < 65536 && splits >= 32)
        hipLaunchKernelGGL(lwg_wgw_reduce_kernel<16>, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, stream, ws, splits, slab, Ctot, a.N, cin, nout, dw);
    else if (total < 262144 && splits >= 8)
        hipLaunchKernelGGL(lwg_wgw_reduce_kernel<4>, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, stream, ws, splits, slab, Ctot, a.N, cin, nout, dw);
    else
        hipLaunchKernelGGL(lwg_wgw_reduce_kernel<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ws, splits, slab, Ctot, a.N, cin, nout, dw);
    return (int)hipGetLastError();
}
