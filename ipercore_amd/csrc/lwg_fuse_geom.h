// The comparison canvas of the output stage - the only statement of its layout in C (tests/fusecanvas_emu.py is the definition):
//   source panel: which source lands where, at which size (fuse_source, tools/utils/multimedia/video.py:297-357)     lwg_fuse_panel_cells
//   one canvas row [panel | pad | ref | pad | out0 | pad | out1 ...] (merge_multi_outs / merge_src_out, :173-213)    lwg_fuse_geom_of
//   canvas byte offset within a row -> (region, byte offset within that region's row)                               lwg_fuse_locate
//   pixel of a panel cell -> the 2 x 2 block of source pixels whose mean it is (cv2.resize at factors 1, 2, 4)      lwg_fuse_tap0
// lwg_fuse_sources_u8 and lwg_fuse_canvas_u8 (fuse_canvas.hip) and the two host helpers lwg_fuse_panel_width / lwg_fuse_canvas_width call
// these and hold no layout arithmetic of their own.  No device builtins: the header also compiles as plain host C++ -
// tests/test_fuse_video_cpu.py walks every canvas byte of its grid through it under overflow traps.
#pragma once
#ifdef __HIPCC__
#include "lwg_common.h"
#define LWG_FUSE_FN __host__ __device__ __forceinline__
#else
#define LWG_FUSE_FN static inline
#endif

#define LWG_FUSE_MAX_OUTS 4
#define LWG_FUSE_MAX_CELLS 4
// regions of a canvas row; out k is LWG_FUSE_OUT0 + k
#define LWG_FUSE_PANEL 0
#define LWG_FUSE_PAD 1
#define LWG_FUSE_REF 2
#define LWG_FUSE_OUT0 3

// one square of the source panel: source index (-1: black), top row, left column, side
struct LwgFuseCell { int src, top, left, size; };

// (ns, S) -> the cells and the panel width Wp (the panel is S rows high); 0: arguments the rules refuse.  The reference's code decides, quirks
// included: ns = 7 is padded to eight paths but goes to fuse_four_images (sources 0..3); for ns >= 8 fuse_eight_images hands four paths to
// fuse_two_images, which reads two (sources 0, 1, 4, 5 in ONE column of quarter-size cells).
LWG_FUSE_FN int lwg_fuse_panel_cells(int ns, int S, LwgFuseCell (&cells)[LWG_FUSE_MAX_CELLS], int& ncells) {
    ncells = 0;
    if (ns < 1 || S < 1) return 0;
    if (ns == 1) {
        cells[0] = LwgFuseCell{0, 0, 0, S};
        ncells = 1;
        return S;
    }
    if (ns <= 7) {
        if (S & 1) return 0;
        const int s = S / 2;
        cells[0] = LwgFuseCell{0, 0, 0, s};
        cells[1] = LwgFuseCell{1, s, 0, s};
        ncells = 2;
        if (ns == 2) return s;
        cells[2] = LwgFuseCell{2, 0, s, s};
        cells[3] = LwgFuseCell{ns == 3 ? -1 : 3, s, s, s};
        ncells = 4;
        return S;
    }
    if (S & 3) return 0;
    const int q = S / 4;
    cells[0] = LwgFuseCell{0, 0, 0, q};
    cells[1] = LwgFuseCell{1, q, 0, q};
    cells[2] = LwgFuseCell{4, 2 * q, 0, q};
    cells[3] = LwgFuseCell{5, 3 * q, 0, q};
    ncells = 4;
    return q;
}

// is Wp a panel width of an S-row panel (S, S / 2 for even S, S / 4 for S % 4 == 0)?
LWG_FUSE_FN bool lwg_fuse_panel_width_ok(int Wp, int S) {
    return S >= 1 && (Wp == S || (!(S & 1) && Wp == S / 2) || (!(S & 3) && Wp == S / 4));
}

// cv2.resize(INTER_LINEAR) of uint8 at the integer factors f = S / size in {1, 2, 4}: half-pixel centres put both taps of a pass at weight 1/2
// (11-bit coefficients 1024 | 1024), and the vertical pass's >>4 ... >>16 ... +2 >>2 comes to (a + b + c + d + 2) >> 2 over source rows and
// columns f i + f / 2 - 1 and f i + f / 2 (f = 1: the pixel itself, four times).  -> the first of the two rows / columns, and the step to the second
LWG_FUSE_FN int lwg_fuse_tap0(int i, int f, int& step) {
    step = f > 1 ? 1 : 0;
    return f * i + (f > 1 ? f / 2 - 1 : 0);
}

struct LwgFuseGeom {
    int S, Wp, pad, has_ref, n_out;
    int Wc;                  // canvas width in pixels
    int slot3;               // 3 (S + pad): bytes of one [pad | image] slot in a row
    int row3;                // 3 Wc: bytes of a canvas row
};

// -> false for sizes the rules refuse (or a canvas frame / fp32 frame / reference frame of 2^31 bytes or more)
LWG_FUSE_FN bool lwg_fuse_geom_of(int S, int Wp, int pad, int has_ref, int n_out, LwgFuseGeom& g) {
    if (!lwg_fuse_panel_width_ok(Wp, S) || pad < 0 || n_out < 1 || n_out > LWG_FUSE_MAX_OUTS) return false;
    const long long wc = (long long)Wp + (long long)((has_ref ? 1 : 0) + n_out) * ((long long)S + pad);
    const long long lim = (1ll << 31) - 1;           // (by division: sizes near INT_MAX must be refused without overflowing on the way)
    if (wc > lim / 3 / S || S > lim / 12 / S) return false;
    g.S = S; g.Wp = Wp; g.pad = pad; g.has_ref = has_ref ? 1 : 0; g.n_out = n_out;
    g.Wc = (int)wc;
    g.slot3 = 3 * (S + pad);
    g.row3 = 3 * g.Wc;
    return true;
}

// first byte, within a canvas row, of slot j's image (j = 0 is the reference when there is one, the outs follow)
LWG_FUSE_FN int lwg_fuse_slot_image3(const LwgFuseGeom& g, int j) { return 3 * g.Wp + j * g.slot3 + 3 * g.pad; }

// byte xb in [0, row3) of a canvas row -> its region and the byte offset within that region's own row (panel: 3 Wp bytes; pad: 3 pad; ref and
// outs: 3 S, pixel off / 3, channel off % 3)
LWG_FUSE_FN void lwg_fuse_locate(const LwgFuseGeom& g, int xb, int& region, int& off) {
    if (xb < 3 * g.Wp) {
        region = LWG_FUSE_PANEL; off = xb;
        return;
    }
    const int r = xb - 3 * g.Wp, j = r / g.slot3, q = r - j * g.slot3;
    if (q < 3 * g.pad) {
        region = LWG_FUSE_PAD; off = q;
        return;
    }
    off = q - 3 * g.pad;
    region = g.has_ref ? (j == 0 ? LWG_FUSE_REF : LWG_FUSE_OUT0 + j - 1) : LWG_FUSE_OUT0 + j;
}
