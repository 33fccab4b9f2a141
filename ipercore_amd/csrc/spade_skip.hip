// The tile lists of lwg_conv2d_winograd4_list_f32 (conv_winograd4.hip) from a frame batch's resized flows.
// The renderer marks the pixels outside the body with flow -2: no tap of any source falls into the image there, and lwg_lwb_attention_x leaves the SAME
// vector (bv) at every such pixel of every frame.  A 3x3 convolution block whose whole input window is such pixels computes what the same block of an
// all-background frame computes - the list-driven convolution copies that instead.  Here: (1) per (frame, 32 x 16 block) one mark - does any pixel of the
// block's window (the block grown by d pixels, clipped to the image) have an in-image tap of any source, by the attention kernel's own predicate
// (lwg_lwb_taps.h); (2) one workgroup turns the marks into the heavy and the light tile ids in ascending order (a fixed-order scan, every list slot
// written by one thread) and their counts - all in device memory, read by the convolution kernel only.
#include <hip/hip_runtime.h>
#include "lwg_common.h"
#include "lwg_conv_wino.h"
#include "lwg_lwb_taps.h"

#define SK_EX 32             // the F(4x4, 3x3) kernel's block: 32 x 16 output pixels
#define SK_EY 16

// one workgroup per tile (cw_grid's numbering: b * bx * by + ty * bx + tx)
__global__ __launch_bounds__(256) void lwg_spade_skip_mark_kernel(const float2* __restrict__ T, int B, int ns, int h, int w, int d, int* __restrict__ marks) {
    const CwGrid g = cw_grid(B, h, w, CW_NB, SK_EX, SK_EY, CW_NB);
    const int t = blockIdx.x, b = cw_image(g, t);
    int x0, y0;
    cw_corner(g, t - b * g.bx * g.by, SK_EX, SK_EY, x0, y0);
    const CwWindow win = cw_block_window(x0, y0, SK_EX, SK_EY, d, h, w);
    const int ww = win.x1 - win.x0, n = ww * (win.y1 - win.y0);
    bool mine = false;
    for (int s = 0; s < ns; ++s) {
        const float2* Ts = T + ((size_t)b * ns + s) * h * w;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int yy = i / ww, y = win.y0 + yy, x = win.x0 + (i - yy * ww);
            float wt[4];
            int tx0, ty0;
            lwb_taps_of(Ts[(size_t)y * w + x], w, h, wt, tx0, ty0);
            mine |= lwb_tap_in_image(tx0, ty0, w, h);
        }
    }
    const int any = __syncthreads_or(mine ? 1 : 0);
    if (threadIdx.x == 0) marks[t] = any ? 1 : 0;
}

// ONE workgroup: thread i owns the marks [i per, (i + 1) per); counts per thread, an inclusive scan over the 1024 threads in LDS, then every thread writes
// its tiles behind the heavy / light tiles of the threads before it - both lists ascending
__global__ __launch_bounds__(1024) void lwg_spade_skip_scan_kernel(const int* __restrict__ marks, int n, int* __restrict__ heavy, int* __restrict__ light,
                                                                   int* __restrict__ counts) {
    __shared__ int part[1024];
    const int tid = threadIdx.x, per = (n + 1023) / 1024;
    const int i0 = tid * per < n ? tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    int c = 0;
    for (int i = i0; i < i1; ++i) c += marks[i] != 0;
    part[tid] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int hv = part[tid] - c;                                   // heavy tiles before i0
    for (int i = i0; i < i1; ++i) {
        if (marks[i] != 0) heavy[hv++] = i;
        else light[i - hv] = i;
    }
    if (tid == 1023) {
        counts[0] = part[1023];
        counts[1] = n - part[1023];
    }
}

// The sub-tile classifier (lwg_conv_wino.h: CW4F_SX x CW4F_SY sub-tiles, CW4F_NS per block): one workgroup per block evaluates every pixel of the
// block's window ONCE and notes which sub-tile windows hold it - the block's window is the union of its sub-tiles' windows, so the block's mark (their
// OR) comes out of the same pass.  fmarks[CW4F_NS t + s]: 1 heavy, 0 light, 2 wholly outside the image (neither list).
__global__ __launch_bounds__(256) void lwg_spade_skip_mark_fine_kernel(const float2* __restrict__ T, int B, int ns, int h, int w, int d, int* __restrict__ marks,
                                                                       int* __restrict__ fmarks) {
    const CwGrid g = cw_grid(B, h, w, CW_NB, SK_EX, SK_EY, CW_NB);
    const int t = blockIdx.x, b = cw_image(g, t);
    int x0, y0;
    cw_corner(g, t - b * g.bx * g.by, SK_EX, SK_EY, x0, y0);
    const CwWindow win = cw_block_window(x0, y0, SK_EX, SK_EY, d, h, w);
    const int ww = win.x1 - win.x0, n = ww * (win.y1 - win.y0);
    unsigned mine = 0;                                        // bit s: sub-tile s, bit CW4F_NS: the block
    for (int s = 0; s < ns; ++s) {
        const float2* Ts = T + ((size_t)b * ns + s) * h * w;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int yy = i / ww, y = win.y0 + yy, x = win.x0 + (i - yy * ww);
            float wt[4];
            int tx0, ty0;
            lwb_taps_of(Ts[(size_t)y * w + x], w, h, wt, tx0, ty0);
            if (lwb_tap_in_image(tx0, ty0, w, h)) mine |= (1u << CW4F_NS) | cw4f_reached(x, y, x0, y0, d);
        }
    }
    unsigned all = 0;
    for (int s = 0; s <= CW4F_NS; ++s) all |= __syncthreads_or((int)((mine >> s) & 1u)) ? 1u << s : 0u;
    if (threadIdx.x < CW4F_NS) {
        const int s = threadIdx.x;
        const bool in = cw4f_in_image(x0 + (s % CW4F_NSX) * CW4F_SX, y0 + (s / CW4F_NSX) * CW4F_SY, h, w);
        fmarks[CW4F_NS * t + s] = in ? (int)((all >> s) & 1u) : 2;
    } else if (threadIdx.x == CW4F_NS) {
        marks[t] = (int)((all >> CW4F_NS) & 1u);
    }
}

// Two workgroups, one per mark array (blockIdx.x = 0: the blocks, 1: the sub-tiles): the scan above for marks of three classes - both counts scanned
// over the 1024 threads, every list slot written by one thread, both lists ascending.  A thread's marks are a multiple of four and read 16 bytes at a
// time where the array is so aligned (the sub-tiles' 150 marks per thread at 256^2 x 300 frames, one by one: 110 us of load latency per launch)
struct SkScanJob { const int* marks; int n; int* heavy; int* light; int* counts; };
template <typename F>
__device__ __forceinline__ void sk_for_marks(const int* __restrict__ marks, int i0, int i1, bool vec, F f) {
    int i = i0;
    if (vec)
        for (; i + 4 <= i1; i += 4) {
            const int4 m = *reinterpret_cast<const int4*>(marks + i);
            f(i, m.x), f(i + 1, m.y), f(i + 2, m.z), f(i + 3, m.w);
        }
    for (; i < i1; ++i) f(i, marks[i]);
}
__device__ __forceinline__ void sk_scan_job(const SkScanJob j) {
    __shared__ int ph[1024], pl[1024];
    const int tid = threadIdx.x, n = j.n, per = ((n + 1023) / 1024 + 3) & ~3;
    const int i0 = tid * per < n ? tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    const bool vec = (reinterpret_cast<size_t>(j.marks) & 15) == 0;
    int ch = 0, cl = 0;
    sk_for_marks(j.marks, i0, i1, vec, [&](int, int m) { ch += m == 1, cl += m == 0; });
    ph[tid] = ch, pl[tid] = cl;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int vh = tid >= off ? ph[tid - off] : 0, vl = tid >= off ? pl[tid - off] : 0;
        __syncthreads();
        ph[tid] += vh, pl[tid] += vl;
        __syncthreads();
    }
    int hv = ph[tid] - ch, lt = pl[tid] - cl;                 // heavy / light entries before i0
    sk_for_marks(j.marks, i0, i1, vec, [&](int i, int m) {
        if (m == 1) j.heavy[hv++] = i;
        else if (m == 0) j.light[lt++] = i;
    });
    if (tid == 1023) {
        j.counts[0] = ph[1023];
        j.counts[1] = pl[1023];
    }
}
__global__ __launch_bounds__(1024) void lwg_spade_skip_scan2_kernel(SkScanJob j0, SkScanJob j1) {
    const SkScanJob j = blockIdx.x == 0 ? j0 : j1;
    sk_scan_job(j);
}
// ... three of them: the blocks, the 16 x 8 and the 8 x 8 sub-tiles
__global__ __launch_bounds__(1024) void lwg_spade_skip_scan3_kernel(SkScanJob j0, SkScanJob j1, SkScanJob j2) {
    const SkScanJob j = blockIdx.x == 0 ? j0 : blockIdx.x == 1 ? j1 : j2;
    sk_scan_job(j);
}

// The classifier at 8 x 8 sub-tiles (lwg_conv_wino.h: CW4Q_*): the pass of lwg_spade_skip_mark_fine_kernel with eight window bits per pixel; the 16 x 8
// marks are the ORs of their two halves (cw4q_marks16), the block's mark the OR of all - every granularity from ONE evaluation of each window pixel.
// qmarks[CW4Q_NS t + s] as fmarks: 1 heavy, 0 light, 2 wholly outside the image.
__global__ __launch_bounds__(256) void lwg_spade_skip_mark_q8_kernel(const float2* __restrict__ T, int B, int ns, int h, int w, int d, int* __restrict__ marks,
                                                                     int* __restrict__ fmarks, int* __restrict__ qmarks) {
    const CwGrid g = cw_grid(B, h, w, CW_NB, SK_EX, SK_EY, CW_NB);
    const int t = blockIdx.x, b = cw_image(g, t);
    int x0, y0;
    cw_corner(g, t - b * g.bx * g.by, SK_EX, SK_EY, x0, y0);
    const CwWindow win = cw_block_window(x0, y0, SK_EX, SK_EY, d, h, w);
    const int ww = win.x1 - win.x0, n = ww * (win.y1 - win.y0);
    unsigned mine = 0;                                        // bit s: 8 x 8 sub-tile s, bit CW4Q_NS: the block
    for (int s = 0; s < ns; ++s) {
        const float2* Ts = T + ((size_t)b * ns + s) * h * w;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int yy = i / ww, y = win.y0 + yy, x = win.x0 + (i - yy * ww);
            float wt[4];
            int tx0, ty0;
            lwb_taps_of(Ts[(size_t)y * w + x], w, h, wt, tx0, ty0);
            if (lwb_tap_in_image(tx0, ty0, w, h)) mine |= (1u << CW4Q_NS) | cw4q_reached(x, y, x0, y0, d);
        }
    }
    unsigned all = 0;
    for (int s = 0; s <= CW4Q_NS; ++s) all |= __syncthreads_or((int)((mine >> s) & 1u)) ? 1u << s : 0u;
    const int s = threadIdx.x;
    if (s < CW4Q_NS) {
        const bool in = cw4q_in_image(x0 + (s % CW4Q_NSX) * CW4Q_SX, y0 + (s / CW4Q_NSX) * CW4Q_SY, h, w);
        qmarks[CW4Q_NS * t + s] = in ? (int)((all >> s) & 1u) : 2;
    } else if (s < CW4Q_NS + CW4F_NS) {
        const int f = s - CW4Q_NS;
        const bool in = cw4f_in_image(x0 + (f % CW4F_NSX) * CW4F_SX, y0 + (f / CW4F_NSX) * CW4F_SY, h, w);
        fmarks[CW4F_NS * t + f] = in ? (int)((cw4q_marks16(all) >> f) & 1u) : 2;
    } else if (s == CW4Q_NS + CW4F_NS) {
        marks[t] = (int)((all >> CW4Q_NS) & 1u);
    }
}

extern "C" int lwg_spade_skip_fine_lists_f32(const float* T, int B, int ns, int h, int w, int d, int* marks, int* heavy, int* light, int* counts,
                                             int* fmarks, int* fheavy, int* flight, int* fcounts, lwg_stream_t stream_) {
    if (!T || !marks || !heavy || !light || !counts || !fmarks || !fheavy || !flight || !fcounts || B <= 0 || ns <= 0 || h <= 0 || w <= 0 || d < 0 || d > 64)
        return (int)hipErrorInvalidValue;
    const long long tiles = cw_total_blocks(B, h, w, CW_NB, SK_EX, SK_EY, CW_NB);
    if (tiles * CW4F_NS >= (1ll << 30) || (long long)h * w >= (1ll << 30)) return (int)hipErrorInvalidValue;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(lwg_spade_skip_mark_fine_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, reinterpret_cast<const float2*>(T), B, ns, h, w, d, marks, fmarks);
    hipLaunchKernelGGL(lwg_spade_skip_scan2_kernel, dim3(2), dim3(1024), 0, stream, SkScanJob{marks, (int)tiles, heavy, light, counts},
                       SkScanJob{fmarks, (int)tiles * CW4F_NS, fheavy, flight, fcounts});
    return (int)hipGetLastError();
}

extern "C" int lwg_spade_skip_lists_f32(const float* T, int B, int ns, int h, int w, int d, int* marks, int* heavy, int* light, int* counts,
                                        lwg_stream_t stream_) {
    if (!T || !marks || !heavy || !light || !counts || B <= 0 || ns <= 0 || h <= 0 || w <= 0 || d < 0 || d > 64) return (int)hipErrorInvalidValue;
    const long long tiles = cw_total_blocks(B, h, w, CW_NB, SK_EX, SK_EY, CW_NB);
    if (tiles >= (1ll << 30) || (long long)h * w >= (1ll << 30)) return (int)hipErrorInvalidValue;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(lwg_spade_skip_mark_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, reinterpret_cast<const float2*>(T), B, ns, h, w, d, marks);
    hipLaunchKernelGGL(lwg_spade_skip_scan_kernel, dim3(1), dim3(1024), 0, stream, marks, (int)tiles, heavy, light, counts);
    return (int)hipGetLastError();
}

// The block lists, the 16 x 8 lists (both as lwg_spade_skip_fine_lists_f32 leaves them) AND the 8 x 8 lists (qmarks, qheavy, qlight: 8 * B * tiles ints
// each, qcounts: 2 ints) in the same two launches
extern "C" int lwg_spade_skip_q8_lists_f32(const float* T, int B, int ns, int h, int w, int d, int* marks, int* heavy, int* light, int* counts,
                                           int* fmarks, int* fheavy, int* flight, int* fcounts, int* qmarks, int* qheavy, int* qlight, int* qcounts,
                                           lwg_stream_t stream_) {
    if (!T || !marks || !heavy || !light || !counts || !fmarks || !fheavy || !flight || !fcounts || !qmarks || !qheavy || !qlight || !qcounts || B <= 0 ||
        ns <= 0 || h <= 0 || w <= 0 || d < 0 || d > 64)
        return (int)hipErrorInvalidValue;
    const long long tiles = cw_total_blocks(B, h, w, CW_NB, SK_EX, SK_EY, CW_NB);
    if (tiles * CW4Q_NS >= (1ll << 30) || (long long)h * w >= (1ll << 30)) return (int)hipErrorInvalidValue;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(lwg_spade_skip_mark_q8_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, reinterpret_cast<const float2*>(T), B, ns, h, w, d, marks, fmarks,
                       qmarks);
    hipLaunchKernelGGL(lwg_spade_skip_scan3_kernel, dim3(3), dim3(1024), 0, stream, SkScanJob{marks, (int)tiles, heavy, light, counts},
                       SkScanJob{fmarks, (int)tiles * CW4F_NS, fheavy, flight, fcounts}, SkScanJob{qmarks, (int)tiles * CW4Q_NS, qheavy, qlight, qcounts});
    return (int)hipGetLastError();
}
