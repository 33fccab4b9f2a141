// What the host side of the direct (implicit-GEMM) convolution family shares - conv_igemm.hip, conv_igemm_split.hip, conv_igemm_bf16.hip, up4_head_bf16.hip,
// the head of bf16_ops.hip and conv_wgrad.hip: the range of a raw buffer, the fit and slicing rules that follow from it, the shape / dtype contract of the
// three generic engines, the epilogue's pointer rules and its dispatch, and the launch of a kernel with more than 64 KB of dynamic LDS.  The kernels, their
// gathers and their out-of-range markers stay in their files.
//   Part 1 is plain C++ that a host compiler can include: tests/test_direct_conv_contracts_cpu.py compiles these very functions with signed-overflow traps
// and holds them to a restatement; its decision table drives every clause through the library.  Part 2 (hipcc only) dispatches and launches.
#pragma once
#include <stddef.h>
#include "lwg_conv_args.h"

// ---- part 1: host-compilable ----
// The kernels address a tensor as ONE raw buffer with 32-bit byte offsets, and give an access that must not happen (a padding tap) the offset 0xC0000000:
// the hardware returns zeros for it as long as it lies at or beyond the buffer's size.  So a tensor fits a buffer iff it is smaller than that.
constexpr unsigned long long LWG_BUF_RANGE = 0xC0000000ull;
static inline bool lwg_buf_fits(unsigned long long bytes) { return bytes < LWG_BUF_RANGE; }
// the gathered inputs (B, H, W, C0 | C1) of ebytes-byte elements; the weight panel of bytes_per_kn bytes per (k, n) of the ntaps Cin x N GEMM operand
static inline bool cd_inputs_fit(const LwgConvArgs& a, unsigned long long ebytes) {
    return lwg_buf_fits((unsigned long long)a.B * a.H * a.W * (unsigned long long)(a.C0 > a.C1 ? a.C0 : a.C1) * ebytes);
}
static inline bool cd_panel_fits(const LwgConvArgs& a, unsigned long long bytes_per_kn) {
    return lwg_buf_fits((unsigned long long)a.ntaps * (unsigned long long)(a.C0 + a.C1) * (unsigned long long)a.N * bytes_per_kn);
}

// ---- batch slicing.  A frame batch whose input exceeds the range is not the caller's problem: the entry points cut the launch along the batch dimension
// into slices that fit and re-base every per-frame pointer (frames are independent rows of the implicit GEMM, so the values are those of the single launch
// bit for bit).  Frames per slice of B frames of `per` bytes; 0 = the batch fits as it is; -1 = a single frame does not fit (contract violation)
static inline int lwg_slice_frames(int B, unsigned long long per) {
    if (per == 0ull || lwg_buf_fits((unsigned long long)B * per)) return 0;
    const unsigned long long n = (LWG_BUF_RANGE - 1ull) / per;
    return n >= 1ull ? (int)n : -1;
}
static inline int lwg_conv_slice_frames(const LwgConvArgs& a) {
    return lwg_slice_frames(a.B, (unsigned long long)a.H * a.W * (unsigned long long)(a.C0 > a.C1 ? a.C0 : a.C1) * (a.xdt == LWG_DT_BF16 ? 2ull : 4ull));
}
static inline LwgConvArgs lwg_conv_slice(const LwgConvArgs& a, int b0, int nb) {
    LwgConvArgs s = a;
    const size_t xs = a.xdt == LWG_DT_BF16 ? 2 : 4, ys = a.ydt == LWG_DT_BF16 ? 2 : 4;
    const size_t xpix = (size_t)a.H * a.W, ypix = (size_t)a.YH * a.YW;
    auto adv = [](const float* p, size_t bytes) { return p ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(p) + bytes) : p; };
    s.x0 = adv(a.x0, (size_t)b0 * xpix * a.C0 * xs);
    s.x1 = adv(a.x1, (size_t)b0 * xpix * a.C1 * xs);
    s.y = const_cast<float*>(adv(a.y, (size_t)b0 * ypix * a.YC * ys));
    s.res = adv(a.res, (size_t)b0 * ypix * a.YC * ys);
    s.xn = adv(a.xn, (size_t)b0 * ypix * a.YC * ys);
    s.mean = adv(a.mean, (size_t)b0 * a.YC * 4);
    s.rstd = adv(a.rstd, (size_t)b0 * a.YC * 4);
    s.B = nb;
    s.M = nb * a.OH * a.OW;
    return s;
}
// The preamble of a sliced entry point, before its field checks: -1 when the launch fits and the entry point should go on as usual; else the batch ran as
// one(slice) per slice and this is the result (0, or the first failure; 1 = hipErrorInvalidValue for a frame that does not fit or M != B OH OW).
template <class F>
static inline int cd_sliced(const LwgConvArgs& a, F&& one) {
    const int nbs = lwg_conv_slice_frames(a);
    if (nbs == 0) return -1;
    if (nbs < 0 || a.M != a.B * a.OH * a.OW) return 1;
    for (int b0 = 0; b0 < a.B; b0 += nbs)
        if (const int e = one(lwg_conv_slice(a, b0, a.B - b0 < nbs ? a.B - b0 : nbs)); e != 0) return e;
    return 0;
}

// ---- the contracts.  What every entry point asks of a launch description: the operands, rows, whole 64-column tiles, the output slice on y_align channels
static inline bool cd_basics_ok(const LwgConvArgs& a, int y_align) {
    return a.x0 && a.w && a.y && a.M > 0 && a.N % 64 == 0 && a.YC % y_align == 0 && a.ycoff % y_align == 0;
}
// ... and the generic engines (lwg_conv2d_nhwc_f32[_ws], _f32_split, _bf16; _bf16_hr's 3 x 3 and 2 x 2 forms): any taps, element types xdt -> ydt, Cin a
// multiple of cin_mult - with a second input C0 of c0_mult -, the inputs and the panel of panel_bytes per (k, n) within the buffer range
struct CdEngine { int xdt, ydt, cin_mult, c0_mult, y_align; unsigned long long panel_bytes; };
static inline bool cd_contract_ok(const LwgConvArgs& a, const CdEngine& g) {
    return cd_basics_ok(a, g.y_align) && a.ntaps >= 1 && a.ntaps <= LWG_MAX_TAPS && a.xdt == g.xdt && a.ydt == g.ydt && (a.C0 + a.C1) % g.cin_mult == 0 &&
           (a.C1 == 0 || (a.C0 % g.c0_mult == 0 && a.x1)) && cd_inputs_fit(a, g.xdt == LWG_DT_BF16 ? 2ull : 4ull) && cd_panel_fits(a, g.panel_bytes);
}
// The epilogue's operands.  SPADE: the tensor to modulate and its statistics, gamma | beta stacked (N = 2 YC, N a multiple of spade_n), and - the bf16
// engines only (ycoff0) - the whole output; RESIDUAL: res; no other code but NONE.
static inline bool cd_epilogue_ok(const LwgConvArgs& a, int spade_n, bool ycoff0) {
    if (a.epi == LWG_EPI_SPADE) return a.xn && a.mean && a.rstd && a.bias && a.N % spade_n == 0 && a.YC * 2 == a.N && !(ycoff0 && a.ycoff != 0);
    return a.epi == LWG_EPI_NONE || (a.epi == LWG_EPI_RESIDUAL && a.res);
}

// ---- part 2: dispatch and launch ----
#ifdef __HIPCC__
#include "lwg_common.h"

// launch(IntC<epilogue>()) for a valid epilogue (a generic lambda: the epilogue is a template argument of the kernels), else hipErrorInvalidValue
template <class F>
static inline int cd_epi_dispatch(const LwgConvArgs& a, int spade_n, bool ycoff0, F&& launch) {
    if (!cd_epilogue_ok(a, spade_n, ycoff0)) return (int)hipErrorInvalidValue;
    if (a.epi == LWG_EPI_SPADE) return (int)launch(IntC<LWG_EPI_SPADE>());
    if (a.epi == LWG_EPI_RESIDUAL) return (int)launch(IntC<LWG_EPI_RESIDUAL>());
    return (int)launch(IntC<LWG_EPI_NONE>());
}

// More than 64 KB of dynamic LDS is an opt-in per kernel and per device (lwg_allow_dynamic_lds): once per device for this KERNEL, then the launch
template <auto KERNEL, class... Args>
static inline hipError_t lwg_launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args&... args) {
    static unsigned long long done = 0ull;
    if (hipError_t e = lwg_allow_dynamic_lds(reinterpret_cast<const void*>(KERNEL), lds, done); e != hipSuccess) return e;
    hipLaunchKernelGGL(KERNEL, grid, block, lds, stream, args...);
    return hipGetLastError();
}
#endif  // __HIPCC__
