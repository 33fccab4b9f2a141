// From a flow value to four bilinear taps - the Liquid Warping Block family's definition of
//   grid_sample coordinates (align_corners=False), floor, clamp to [-2, size + 1], the four weights      lwb_taps_of
//   zero padding outside the image, per tap and for the 2 x 2 square                                      lwb_tap / lwb_tap_in_image
//   flow resize S x S -> h x w (align_corners=True): indices and weights, the four-texel blend             lwb_resize_of / lwb_flow_at
//   linear pixel -> (frame, row, column)                                                                  lwb_pixel_of
// lwg_lwb_attention_x (lwb_attn_x.hip) gathers by them and the SPADE skip classifier (spade_skip.hip) must call a pixel background exactly where
// that kernel does.  The kernels of lwb_attn.hip and bf16_ops.hip, which also resize the flow field per pixel, use the decode, the per-tap
// predicate and (the fusion kernels) lwb_resize_of, and keep lwb_taps_of's and the blend's expressions as their own text (the
// bits of their resize depend on it).
// No device builtins: the header also compiles as plain host C++ - tests/test_lwb_taps_cpu.py runs it under overflow traps against the fp32
// torch evaluation of the same expressions and holds the kernels' copies to this text.
#pragma once
#ifdef __HIPCC__
#include "lwg_common.h"
#define LWB_FN __host__ __device__ __forceinline__
#else
#include <math.h>
#include <stddef.h>
struct float2 { float x, y; };
#define LWB_FN static inline
#endif

// grid_sample, align_corners=False: pixel = ((g + 1) * size - 1) / 2; the four bilinear weights and the top-left tap (clamped before the int
// conversion so wild flows cannot overflow; out-of-range taps read zeros)
LWB_FN void lwb_taps_of(const float2 t, int w, int h, float (&wt)[4], int& tx0, int& ty0) {
    const float ix = ((t.x + 1.f) * (float)w - 1.f) * 0.5f, iy = ((t.y + 1.f) * (float)h - 1.f) * 0.5f;
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const float wx1 = ix - fx0, wy1 = iy - fy0, wx0 = (fx0 + 1.f) - ix, wy0 = (fy0 + 1.f) - iy;
    tx0 = (int)fminf(fmaxf(fx0, -2.f), (float)w + 1.f);
    ty0 = (int)fminf(fmaxf(fy0, -2.f), (float)h + 1.f);
    wt[0] = wy0 * wx0; wt[1] = wy0 * wx1; wt[2] = wy1 * wx0; wt[3] = wy1 * wx1;
}
// does the 2 x 2 tap square at (tx0, ty0) touch the (h, w) image?
LWB_FN bool lwb_tap_in_image(int tx0, int ty0, int w, int h) { return tx0 >= -1 && tx0 < w && ty0 >= -1 && ty0 < h; }
// tap t in 0..3 (row-major 2 x 2) of the square at (tx0, ty0): its pixel, and whether it lies inside the (h, w) map (zero padding otherwise);
// its weight is wt[t]
LWB_FN bool lwb_tap(int t, int tx0, int ty0, int w, int h, int& tx, int& ty) {
    ty = ty0 + (t >> 1); tx = tx0 + (t & 1);
    return ty >= 0 && ty < h && tx >= 0 && tx < w;
}

// per pixel: flow resize S x S -> h x w, bilinear, align_corners=True (ATen area_pixel_compute_source_index)
struct LwbResize {
    int y0, x0, y1, x1;
    float ly0, ly1, lx0, lx1;
    bool same;              // the field is stored at (h, w): no resize
};
LWB_FN LwbResize lwb_resize_of(int y, int x, int h, int w, int S) {
    LwbResize r;
    const float sc_y = h > 1 ? (float)(S - 1) / (float)(h - 1) : 0.f;
    const float sc_x = w > 1 ? (float)(S - 1) / (float)(w - 1) : 0.f;
    const float sy = sc_y * (float)y, sx = sc_x * (float)x;
    r.y0 = (int)sy; r.x0 = (int)sx;
    r.y1 = r.y0 + (r.y0 < S - 1 ? 1 : 0); r.x1 = r.x0 + (r.x0 < S - 1 ? 1 : 0);
    r.ly1 = sy - (float)r.y0; r.lx1 = sx - (float)r.x0;
    r.ly0 = 1.f - r.ly1; r.lx0 = 1.f - r.lx1;
    r.same = (h == S) && (w == S);
    return r;
}
// the flow value of pixel (y, x): the direct load when the field is already (h, w), the four-texel blend otherwise; Tp: the (S,S,2) field of this
// frame and source.  The reference text of the blend: the kernels spell it out themselves (the compiler contracts a blend that arrives through a
// function differently) and tests/test_lwb_taps_cpu.py holds their text to this one.
LWB_FN float2 lwb_flow_at(const float2* __restrict__ Tp, const LwbResize& r, int y, int x, int S) {
    float2 g;
    if (r.same) {
        g = Tp[(size_t)y * S + x];
    } else {
        const float2 t00 = Tp[(size_t)r.y0 * S + r.x0], t01 = Tp[(size_t)r.y0 * S + r.x1];
        const float2 t10 = Tp[(size_t)r.y1 * S + r.x0], t11 = Tp[(size_t)r.y1 * S + r.x1];
        g.x = r.ly0 * (r.lx0 * t00.x + r.lx1 * t01.x) + r.ly1 * (r.lx0 * t10.x + r.lx1 * t11.x);
        g.y = r.ly0 * (r.lx0 * t00.y + r.lx1 * t01.y) + r.ly1 * (r.lx0 * t10.y + r.lx1 * t11.y);
    }
    return g;
}

// linear pixel gp of a (B,h,w) batch -> (b, y, x)
LWB_FN void lwb_pixel_of(long gp, int h, int w, int& b, int& y, int& x) {
    const int hw = h * w;
    b = (int)(gp / hw);
    const int rem = (int)(gp - (long)b * hw);
    y = rem / w; x = rem - y * w;
}
