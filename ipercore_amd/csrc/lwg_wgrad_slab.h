// What the weight-gradient family shares - conv_wgrad.hip (direct, fp32 MFMA), conv_wgrad_bf16.hip (bf16 operands), conv_wgrad_winograd.hip (F(2x2, 3x3);
// the split plan only) and the panel kernels of train_ops.hip (the K order and the parameter layouts): the slab format, the split plan and the tile width.
//
// The slab format.  A weight-gradient launch splits its reduction (the M = B OH OW output positions) over gridDim.y workgroups per output tile; split s
// writes its partial sums to slab s of a workspace [splits][Ktot + 1][N], and one reduction launch adds the slabs IN SLAB ORDER (deterministic - no float
// atomics) straight into the parameter tensor's own layout.  Row k < Ktot = ntaps * cin_pad is K in the forward panel's order (lwg_korder_k: 32-channel chunk
// major and tap minor, or tap * cin_pad + c for the small-Cin first layers); row Ktot is the bias gradient (the column sums of dY that the workgroups of
// k-tile 0 add up from the quads they stage anyway - no separate pass over dY).  The parameter tensor is (D0, D1, KH, KW): nn.Conv2d's (N, Cin, KH, KW), or
// (Cin-of-the-GEMM, N, KH, KW) for transposed = 1; tap t lands at kernel position kidx[t], positions no tap maps to stay untouched (the four parity launches
// of a transposed convolution fill one tensor), cin <= cin_pad and nout <= n_pad drop the zero-extended channels.
//
// The split plan (lwg_wgrad_split_plan).  splits = workgroups / blocks fills the engine's workgroup budget with the launch's output tiles in ONE wave (no
// ragged second one); capped so that the slabs - each written once and read once more by the reduction - stay under cap_bytes; at most nchunks / 4, so every
// workgroup walks at least four chunks of rows; at least 1.  cps = chunks per workgroup, and the splits that would get no chunk are dropped (128 chunks over
// 14 splits: 10 each -> 13 workgroups have work).  The function that sizes the workspace and the launcher take splits AND cps from the one returned value.
//   engine     workgroups   cap     chunk      slab bytes
//   direct     512          48 MB   32 rows    (Ktot + 1) N 4      (512 = the 256 CUs at 2 workgroups each)
//   bf16       2 cus        48 MB   64 rows    (Ktot + 1) N 4
//   Winograd   cus          64 MB   8 tiles    64 Ctot N           (its own [16][Ctot][N] slab and G^T . G reduction stay in its file; 128 KB of LDS: 1 per CU)
//
// Part 1 is plain C++ that a host compiler can include: tests/test_wgrad_slab_cpu.py compiles these very functions with signed-overflow traps and holds them
// to a numpy restatement.  Part 2 (hipcc only) is the reduction's entry.  The kernels' MFMA accumulator-to-slab epilogues (part 2 says why), gathers,
// raw-buffer-load helpers and out-of-range markers stay in their files.
#pragma once
#include <stddef.h>
#include "lwg_conv_args.h"
#ifdef __HIPCC__
#include "lwg_common.h"
#define LWG_SLAB_FN __host__ __device__ __forceinline__
#else
#define LWG_SLAB_FN static inline
#endif

// ---- part 1: host-compilable ----
struct LwgSplitPlan { int splits, cps; };
LWG_SLAB_FN LwgSplitPlan lwg_wgrad_split_plan(int blocks, int nchunks, int workgroups, long long slab_bytes, long long cap_bytes) {
    int splits = workgroups / blocks;
    if ((long long)splits * slab_bytes > cap_bytes) splits = (int)(cap_bytes / slab_bytes);
    if (splits > nchunks / 4) splits = nchunks / 4;
    if (splits < 1) splits = 1;
    const int cps = (nchunks + splits - 1) / splits;
    return LwgSplitPlan{(nchunks + cps - 1) / cps, cps};
}

// Columns of the output tile (the tile is 128 rows of K): 64 when the last 128 columns would be half empty - the N = 64 layers (last up-sampling layer, first
// discriminator / encoder layers), where a 128-column tile spends half of its MFMAs on columns that do not exist (33 - 53 TFLOP/s on those launches)
LWG_SLAB_FN int lwg_wgrad_bn(int N) { return (N % 128 != 0 && N % 128 <= 64) ? 64 : 128; }
LWG_SLAB_FN int lwg_wgrad_tiles(int Ktot, int N) { return ((Ktot + 127) / 128) * ((N + lwg_wgrad_bn(N) - 1) / lwg_wgrad_bn(N)); }
LWG_SLAB_FN size_t lwg_wgrad_slab_floats(int Ktot, int N) { return (size_t)(Ktot + 1) * N; }
LWG_SLAB_FN float* lwg_wgrad_slab(float* part, unsigned split, int Ktot, int N) { return part + (size_t)split * (Ktot + 1) * N; }     // (the kernels' association)

// row of (tap, c) in the forward panel's K order; its inverse; offset of element (c, n) of kernel position 0 in the (D0, D1, KH, KW) parameter tensor
LWG_SLAB_FN int lwg_korder_k(int ntaps, int cin_pad, int tap, int c) { return (cin_pad & 31) == 0 ? ((c >> 5) * ntaps + tap) * 32 + (c & 31) : tap * cin_pad + c; }
LWG_SLAB_FN void lwg_korder_decode(int k, int ntaps, int cin_pad, int& tap, int& c) {
    if ((cin_pad & 31) == 0) {
        const int chunk = k / (ntaps * 32), rem = k - chunk * ntaps * 32;
        tap = rem >> 5;
        c = chunk * 32 + (rem & 31);
    } else {
        tap = k / cin_pad;
        c = k - tap * cin_pad;
    }
}
LWG_SLAB_FN size_t lwg_param_offset(int transposed, int D1, int KHW, int c, int n) { return ((size_t)(transposed ? c : n) * D1 + (transposed ? n : c)) * KHW; }

// One reduction launch's view of the slabs and of the parameter tensor
struct LwgUnpackMap { int D1, KHW, transposed, ntaps, cin, cin_pad, nout, n_pad, kidx[LWG_MAX_TAPS]; };
LWG_SLAB_FN int lwg_unpack_k(const LwgUnpackMap& u, int tap, int c) { return lwg_korder_k(u.ntaps, u.cin_pad, tap, c); }
LWG_SLAB_FN int lwg_unpack_bias_row(const LwgUnpackMap& u) { return u.ntaps * u.cin_pad; }
LWG_SLAB_FN size_t lwg_unpack_dst(const LwgUnpackMap& u, int tap, int c, int n) { return lwg_param_offset(u.transposed, u.D1, u.KHW, c, n) + u.kidx[tap]; }
LWG_SLAB_FN size_t lwg_unpack_slab_floats(const LwgUnpackMap& u) { return lwg_wgrad_slab_floats(lwg_unpack_bias_row(u), u.n_pad); }
LWG_SLAB_FN size_t lwg_unpack_weights(const LwgUnpackMap& u) { return (size_t)u.ntaps * u.cin * u.nout; }

// element i of the output (tap, c, n; n fastest) -> its slab offset (src) and parameter-tensor offset (dst).  Elements [weights, weights + nout) are the bias
// gradient (the bias row, returned with bias = true and dst = n) when the launch carries one.
LWG_SLAB_FN void lwg_unpack_map(const LwgUnpackMap& u, size_t i, size_t& src, size_t& dst, bool& bias) {
    const int n = (int)(i % u.nout), r = (int)(i / u.nout);
    bias = r >= u.ntaps * u.cin;
    if (bias) {
        src = (size_t)lwg_unpack_bias_row(u) * u.n_pad + n;
        dst = (size_t)n;
        return;
    }
    const int c = r % u.cin, tap = r / u.cin;
    src = (size_t)lwg_unpack_k(u, tap, c) * u.n_pad + n;
    dst = lwg_unpack_dst(u, tap, c, n);
}
// the same for quad i4 of the output (nout % 4 == 0): FOUR consecutive n of one (tap, c) - 16 contiguous bytes at src; lane j of the quad lands at
// lwg_unpack_dst(u, tap, c, n + j), or at db[n + j] for a quad of the bias row
// (two entry points on purpose: unpack4g selects n and r for its idle lanes and calls _at - one select on i4 instead changes its device code, 32 -> 28 VGPRs)
struct LwgUnpackQuad { int n, c, tap; bool bias; size_t src; };
LWG_SLAB_FN LwgUnpackQuad lwg_unpack_quad_at(const LwgUnpackMap& u, int n, int r) {      // quad n / 4 of output row r = (tap, c)
    LwgUnpackQuad q;
    q.n = n, q.bias = r >= u.ntaps * u.cin, q.c = r % u.cin, q.tap = q.bias ? 0 : r / u.cin;
    q.src = (size_t)(q.bias ? lwg_unpack_bias_row(u) : lwg_unpack_k(u, q.tap, q.c)) * u.n_pad + n;
    return q;
}
LWG_SLAB_FN LwgUnpackQuad lwg_unpack_quad(const LwgUnpackMap& u, size_t i4) {
    const int nq = u.nout >> 2;
    return lwg_unpack_quad_at(u, (int)(i4 % nq) * 4, (int)(i4 / nq));
}

// The argument checks of the un-packing entry points: false for an invalid (dw geometry, kidx, cin, nout); else *u is filled
static inline bool lwg_wgrad_unpack_map_make(const LwgConvArgs* pa, int D0, int D1, int KH, int KW, int transposed, const int* kidx, int cin, int nout,
                                             LwgUnpackMap* u) {
    if (!pa || !kidx || cin < 1 || nout < 1 || cin > pa->C0 + pa->C1 || nout > pa->N) return false;
    if ((transposed ? cin : nout) > D0 || (transposed ? nout : cin) > D1 || pa->ntaps < 1 || pa->ntaps > LWG_MAX_TAPS) return false;
    u->D1 = D1; u->KHW = KH * KW; u->transposed = transposed; u->ntaps = pa->ntaps; u->cin = cin; u->cin_pad = pa->C0 + pa->C1;
    u->nout = nout; u->n_pad = pa->N;
    for (int i = 0; i < pa->ntaps; ++i) {
        if (kidx[i] < 0 || kidx[i] >= KH * KW) return false;
        u->kidx[i] = kidx[i];
    }
    return true;
}

// ---- part 2: the reduction (hipcc only).  The MFMA accumulator-to-slab epilogue stays spelled out in the two slab-writing kernels: through a shared
// function their 128-column forms came out with other register numbers in the K loop (profiles/wgrad_slab_isa_vs_parent.txt) ----
#ifdef __HIPCC__
// dw (and db, when not NULL) from `splits` slabs in ws, added in slab order (conv_wgrad.hip)
void lwg_wgrad_reduce_unpack(const float* ws, int splits, const LwgUnpackMap& u, float* dw, float* db, hipStream_t stream);
#endif  // __HIPCC__
