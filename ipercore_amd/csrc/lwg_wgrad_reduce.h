// The slab reduction of a weight gradient fused with its un-packing (conv_wgrad.hip), as the other weight-gradient files reach it:
// conv_wgrad_bf16.hip writes the direct kernel's slabs ([split][Ktot + 1][N], K in the forward panel's order, row Ktot = the bias gradient)
// and hands them to the SAME reduction kernels - one definition of "slab order" and of the parameter layouts.
#pragma once
#include "lwg_common.h"

struct LwgUnpackMap {
    int D1, KHW, transposed, ntaps, cin, cin_pad, nout, n_pad;
    int kidx[LWG_MAX_TAPS];
};

// The argument checks of lwg_conv2d_wgrad_unpacked_f32 (host only): false for an invalid (dw geometry, kidx, cin, nout); else *u is filled.
bool lwg_wgrad_unpack_map_make(const LwgConvArgs* pa, int D0, int D1, int KH, int KW, int transposed, const int* kidx, int cin, int nout, LwgUnpackMap* u);
// dw (and db, when not NULL) from `splits` slabs in ws, added in slab order: the reduction launch of lwg_conv2d_wgrad_unpacked_f32.
void lwg_wgrad_reduce_unpack(const float* ws, int splits, const LwgUnpackMap& u, float* dw, float* db, hipStream_t stream);
