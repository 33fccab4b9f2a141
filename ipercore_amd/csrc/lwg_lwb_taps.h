// The bilinear taps of a warped source at one pixel and the "has an in-image tap" predicate - shared by lwg_lwb_attention_x (lwb_attn_x.hip), which
// gathers by them, and the SPADE skip classifier (spade_skip.hip), which must call a pixel background exactly where the attention kernel does.
#pragma once
#include "lwg_common.h"

// grid_sample, align_corners=False: pixel = ((g + 1) * size - 1) / 2; the four bilinear weights and the top-left tap (clamped before the int
// conversion so wild flows cannot overflow; out-of-range taps read zeros)
__device__ __forceinline__ void lwb_taps_of(const float2 t, int w, int h, float (&wt)[4], int& tx0, int& ty0) {
    const float ix = ((t.x + 1.f) * (float)w - 1.f) * 0.5f, iy = ((t.y + 1.f) * (float)h - 1.f) * 0.5f;
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const float wx1 = ix - fx0, wy1 = iy - fy0, wx0 = (fx0 + 1.f) - ix, wy0 = (fy0 + 1.f) - iy;
    tx0 = (int)fminf(fmaxf(fx0, -2.f), (float)w + 1.f);
    ty0 = (int)fminf(fmaxf(fy0, -2.f), (float)h + 1.f);
    wt[0] = wy0 * wx0; wt[1] = wy0 * wx1; wt[2] = wy1 * wx0; wt[3] = wy1 * wx1;
}
// does the 2 x 2 tap square at (tx0, ty0) touch the (h, w) image?
__device__ __forceinline__ bool lwb_tap_in_image(int tx0, int ty0, int w, int h) { return tx0 >= -1 && tx0 < w && ty0 >= -1 && ty0 < h; }
