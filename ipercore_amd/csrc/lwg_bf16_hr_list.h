// The id arithmetic of the list-driven form of lwg_conv_bf16_hr2_kernel (conv_igemm_bf16.hip: lwg_conv2d_nhwc_bf16_hr_list).
// The kernel's 8-row x 16-column pixel block IS the 16 x 8 sub-tile of lwg_conv_wino.h (Cw4F::SX x Cw4F::SY), so the launch reads the sub-tile lists of
// lwg_spade_skip_fine_lists_f32 as they are: one workgroup per (in-image sub-tile, column tile of 128), the heavy entries first in dispatch order.
// Plain integer arithmetic that a host compiler can include: tests/test_spade_skip_bf16_cpu.py compiles these very functions with signed-overflow
// traps; the kernel goes through them.
#pragma once
#include "lwg_conv_wino.h"

#define HRL_BN 128                           // output columns of a workgroup (WAVES_M = 1: four waves of 32 columns, TM = 4 row tiles each)
#define HRL_TM 4
enum { HRL_EXIT = 0, HRL_HEAVY = 1, HRL_LIGHT = 2 };

// the launch's workgroups: the host's number - every in-image sub-tile once per column tile, whatever the lists say (the counts stay on the device)
CW_FN long long hrl_grid(int B, int OH, int OW, int tiles_n) { return (long long)Cw4F::in_image_total(B, OH, OW) * tiles_n; }
// workgroup lid (after lwg_xcd_remap) -> entry e and column tile
CW_FN void hrl_entry(int lid, int tiles_n, int& e, int& tile_n) { e = lid / tiles_n, tile_n = lid - e * tiles_n; }
// the counts as the kernel takes them: never more entries than the launch has workgroups for, whatever the memory holds
CW_FN void hrl_counts(int c0, int c1, int total, int& nh, int& nl) {
    nh = c0 < 0 ? 0 : c0 > total ? total : c0;
    nl = c1 < 0 ? 0 : c1 > total - nh ? total - nh : c1;
}
// entry e: heavy[idx], light[idx] or nothing to do
CW_FN int hrl_kind(int e, int nh, int nl, int& idx) {
    if (e < nh) { idx = e; return HRL_HEAVY; }
    if (e - nh < nl) { idx = e - nh; return HRL_LIGHT; }
    idx = -1;
    return HRL_EXIT;
}
// sub-tile id u -> image and corner; false: no sub-tile of this launch (an id outside the grid or a sub-tile outside the image - neither is ever listed)
CW_FN bool hrl_locate(int u, int B, int H, int W, int& b, int& x0, int& y0) {
    const CwGrid g = cw_grid(B, H, W, CW_NB, 32, 16, CW_NB);
    b = x0 = y0 = 0;
    if (u < 0 || u >= g.tiles * Cw4F::NS) return false;
    Cw4F::corner(g, u, b, x0, y0);
    return Cw4F::in_image(x0, y0, H, W);
}
// every sub-tile heavy (counts[0] = the total): the plain kernel's tile order - entry e = (image, block row, block column) row-major
CW_FN void hrl_plain_corner(int e, int H, int W, int& b, int& x0, int& y0) {
    const int tx = (W + Cw4F::SX - 1) / Cw4F::SX, ty = (H + Cw4F::SY - 1) / Cw4F::SY;
    const int r = e / tx;
    x0 = (e - r * tx) * Cw4F::SX, y0 = (r % ty) * Cw4F::SY, b = r / ty;
}
// ---- a lane's place in the workgroup's accumulator tile (the row-renaming kernel's D^T layout with WAVES_M = 1): row tile i of HRL_TM is the image-row
// pair (i, i + HRL_TM) of the sub-tile; lane -> pixel (py, px) inside the sub-tile
CW_FN void hrl_lane_pixel(int lane, int i, int& py, int& px) { py = i + HRL_TM * ((lane >> 4) & 1), px = lane & 15; }
// accumulator register r (0..15) of half-wave khalf holds column 8 (r / 4) + 4 khalf + r % 4 of the wave's 32-column tile
CW_FN int hrl_acc_column(int khalf, int r) { return 8 * (r >> 2) + 4 * khalf + (r & 3); }
// The fp32 accumulator frame (1, H, W, N) of the gamma | beta convolution (lwg_conv2d_nhwc_bf16_hr_acc writes it, the light SPADE workgroups read it):
// per pixel the N columns in the kernel's panel order, each 32-column tile stored [khalf][r] - a lane's 16 accumulators of a pixel are 64 consecutive
// bytes, four 16-byte accesses.  -> the float offset of register 0 of (pixel (oy, ox), first column ncol of the wave's tile, khalf)
CW_FN size_t hrl_acc_offset(int oy, int ox, int W, int N, int ncol, int khalf) { return ((size_t)oy * W + ox) * (size_t)N + (size_t)(ncol + 16 * khalf); }
// The bf16 calibration frame (1, H, W, YC) of an LWG_EPI_NONE launch is in the output's own layout: a lane copies channels ycoff + ncol + 16 khalf .. + 15
// of its pixel, two 16-byte accesses.  -> the element offset of the first
CW_FN size_t hrl_copy_offset(int oy, int ox, int W, int YC, int col, int khalf) { return ((size_t)oy * W + ox) * (size_t)YC + (size_t)(col + 16 * khalf); }

// ---- the host contract (shapes only: no pointer is looked at).  3 x 3 / stride 1 / pad 1 on one bf16 input, bf16 output on the same grid, taps the
// ascending 3 x 3 grid, N a multiple of HRL_BN (every SPADE launch of the shipped generators: `shared` N = 128, gamma | beta N = 2 C, C in {64, 128,
// 256}), LWG_EPI_NONE or LWG_EPI_SPADE.  The input is addressed per IMAGE (one buffer descriptor each): one image below the 3 GiB marker, any batch.
CW_FN bool hrl_contract_ok(const LwgConvArgs& a) {
    if (a.B <= 0 || a.H <= 0 || a.W <= 0 || a.C0 <= 0 || a.C1 != 0 || (a.C0 % 64) != 0 || a.N <= 0 || (a.N % HRL_BN) != 0 || a.xdt != LWG_DT_BF16 ||
        a.ydt != LWG_DT_BF16 || a.ntaps != 9 || a.stride != 1 || a.omul != 1 || a.ooy != 0 || a.oox != 0 || a.OH != a.H || a.OW != a.W || a.YH != a.H ||
        a.YW != a.W || (long long)a.M != (long long)a.B * a.H * a.W || (a.YC & 7) != 0 || (a.ycoff & 7) != 0 || a.ycoff < 0)
        return false;
    for (int t = 0; t < 9; ++t)
        if (a.dy[t] != t / 3 - 1 || a.dx[t] != t % 3 - 1) return false;
    if ((unsigned long long)a.H * a.W * (unsigned long long)a.C0 * 2ull >= (unsigned long long)CW_OOB ||
        9ull * (unsigned long long)(a.C0 / 64) * (unsigned long long)a.N * 128ull >= (unsigned long long)CW_OOB)
        return false;
    if (cw_total_blocks(a.B, a.H, a.W, CW_NB, 32, 16, CW_NB) * Cw4F::NS >= (1ll << 30) || (long long)a.H * a.W >= (1ll << 30) ||
        (long long)((a.W + Cw4F::SX - 1) / Cw4F::SX) * ((a.H + Cw4F::SY - 1) / Cw4F::SY) * a.B * (a.N / HRL_BN) >= 0x7fffffffll)
        return false;
    if (a.epi == LWG_EPI_SPADE) return a.YC * 2 == a.N && a.ycoff == 0;
    return a.epi == LWG_EPI_NONE && a.ycoff + a.N <= a.YC;
}
