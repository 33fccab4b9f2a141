// The tile lists of lwg_conv2d_winograd4_list_f32 / _fine_f32 / _q8_f32 (conv_winograd4.hip) from a frame batch's resized flows.
// The renderer marks the pixels outside the body with flow -2: no tap of any source falls into the image there, and lwg_lwb_attention_x leaves the SAME
// vector (bv) at every such pixel of every frame.  A 3x3 convolution block whose whole input window is such pixels computes what the same block of an
// all-background frame computes - the list-driven convolution copies that instead.  Here: (1) per (frame, 32 x 16 block) one mark - does any pixel of the
// block's window (the block grown by d pixels, clipped to the image) have an in-image tap of any source, by the attention kernel's own predicate
// (lwg_lwb_taps.h) - and, from the same pass, one mark per sub-tile of the block (lwg_conv_wino.h: Cw4F 16 x 8, Cw4Q 8 x 8) down to the granularity the
// entry point asks for; (2) one workgroup per granularity turns its marks into the heavy and the light ids in ascending order (a fixed-order scan, every
// list slot written by one thread) and their counts - all in device memory, read by the convolution kernel only.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "lwg_common.h"
#include "lwg_conv_wino.h"
#include "lwg_lwb_taps.h"

#define SK_EX 32             // the F(4x4, 3x3) kernel's block: 32 x 16 output pixels
#define SK_EY 16

// sub-tile s of the block at (x0, y0): 1 heavy (bit s of m), 0 light, 2 wholly outside the image (neither list)
template <typename G>
__device__ __forceinline__ void sk_write_sub(int* __restrict__ out, int t, int s, unsigned m, int x0, int y0, int h, int w) {
    const bool in = G::in_image(x0 + (s % G::NSX) * G::SX, y0 + (s / G::NSX) * G::SY, h, w);
    out[G::NS * t + s] = in ? (int)((m >> s) & 1u) : 2;
}
// The classifier, G = the finest granularity it writes (void: blocks only, Cw4F: and fmarks, Cw4Q: and fmarks, qmarks).  One workgroup per block (cw_grid's
// numbering: b * bx * by + ty * bx + tx) evaluates every pixel of the block's window ONCE and notes which of G's sub-tile windows hold it (G::reached) - the
// block's window is the union of its sub-tiles' windows, so the block's mark (their OR) comes out of the same pass; the 16 x 8 marks under Cw4Q are the ORs
// of their two halves (cw4_marks16_of8): every granularity from one evaluation of each window pixel.
template <typename G>
__global__ __launch_bounds__(256) void lwg_spade_skip_mark_kernel(const float2* __restrict__ T, int B, int ns, int h, int w, int d, int* __restrict__ marks,
                                                                  int* __restrict__ fmarks, int* __restrict__ qmarks) {
    constexpr bool SUB = !std::is_void<G>::value, Q8 = std::is_same<G, Cw4Q>::value;
    using GS = std::conditional_t<SUB, G, Cw4F>;             // (names G's members where SUB is false and nothing uses them)
    constexpr int NS = SUB ? GS::NS : 0;
    const CwGrid g = cw_grid(B, h, w, CW_NB, SK_EX, SK_EY, CW_NB);
    const int t = blockIdx.x, b = cw_image(g, t);
    int x0, y0;
    cw_corner(g, t - b * g.bx * g.by, SK_EX, SK_EY, x0, y0);
    const CwWindow win = cw_block_window(x0, y0, SK_EX, SK_EY, d, h, w);
    const int ww = win.x1 - win.x0, n = ww * (win.y1 - win.y0);
    unsigned mine = 0;                                        // bit s: sub-tile s of G, bit NS: the block
    for (int s = 0; s < ns; ++s) {
        const float2* Ts = T + ((size_t)b * ns + s) * h * w;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int yy = i / ww, y = win.y0 + yy, x = win.x0 + (i - yy * ww);
            float wt[4];
            int tx0, ty0;
            lwb_taps_of(Ts[(size_t)y * w + x], w, h, wt, tx0, ty0);
            if (lwb_tap_in_image(tx0, ty0, w, h)) mine |= (1u << NS) | (SUB ? GS::reached(x, y, x0, y0, d) : 0u);
        }
    }
    unsigned all = 0;
    for (int s = 0; s <= NS; ++s) all |= __syncthreads_or((int)((mine >> s) & 1u)) ? 1u << s : 0u;
    // the write-out, one thread per mark: the finest sub-tiles, then each coarser level from the finer one, then the block
    int s = threadIdx.x;
    unsigned m = all;
    if constexpr (Q8) {
        if (s < Cw4Q::NS) return sk_write_sub<Cw4Q>(qmarks, t, s, m, x0, y0, h, w);
        s -= Cw4Q::NS, m = cw4_marks16_of8(m);
    }
    if constexpr (SUB) {
        if (s < Cw4F::NS) return sk_write_sub<Cw4F>(fmarks, t, s, m, x0, y0, h, w);
        s -= Cw4F::NS;
    }
    if (s == 0) marks[t] = (int)((all >> NS) & 1u);
}

// The scan: one workgroup per mark array (blockIdx.x = 0: the blocks, 1: the 16 x 8, 2: the 8 x 8 sub-tiles).  Thread i owns the marks [i per,
// (i + 1) per); the heavy and the light counts per thread, an inclusive scan of both over the 1024 threads in LDS, then every thread writes its ids
// behind those of the threads before it - every list slot written by one thread, both lists ascending.  A thread's marks are a multiple of four and
// read 16 bytes at a time where the array is so aligned (the sub-tiles' 150 marks per thread at 256^2 x 300 frames, one by one: 110 us of load
// latency per launch)
struct SkScanJob { int* marks; int n; int* heavy; int* light; int* counts; };
struct SkScanJobs { SkScanJob j[3]; };
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
__global__ __launch_bounds__(1024) void lwg_spade_skip_scan_kernel(SkScanJobs js) {
    __shared__ int ph[1024], pl[1024];
    const SkScanJob j = blockIdx.x == 0 ? js.j[0] : blockIdx.x == 1 ? js.j[1] : js.j[2];
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
        if (m == 1) j.heavy[hv] = i;
        if (m == 0) j.light[lt] = i;
        hv += m == 1, lt += m == 0;                           // (counters as sums: as an if / else pair they become an indexed pair in scratch memory)
    });
    if (tid == 1023) {
        j.counts[0] = ph[1023];
        j.counts[1] = pl[1023];
    }
}

// The two launches of every entry point; js.j[0 .. levels): the blocks, the 16 x 8, the 8 x 8 sub-tiles (levels = 1 + what G adds; n is filled in here)
template <typename G>
static int sk_lists(const float* T, int B, int ns, int h, int w, int d, SkScanJobs js, lwg_stream_t stream_) {
    constexpr int levels = std::is_void<G>::value ? 1 : std::is_same<G, Cw4F>::value ? 2 : 3;
    constexpr int per[3] = {1, Cw4F::NS, Cw4Q::NS};
    for (int i = 0; i < levels; ++i)
        if (!js.j[i].marks || !js.j[i].heavy || !js.j[i].light || !js.j[i].counts) return (int)hipErrorInvalidValue;
    if (!T || B <= 0 || ns <= 0 || h <= 0 || w <= 0 || d < 0 || d > 64) return (int)hipErrorInvalidValue;
    const long long tiles = cw_total_blocks(B, h, w, CW_NB, SK_EX, SK_EY, CW_NB);
    if (tiles * per[levels - 1] >= (1ll << 30) || (long long)h * w >= (1ll << 30)) return (int)hipErrorInvalidValue;
    for (int i = 0; i < levels; ++i) js.j[i].n = (int)tiles * per[i];
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(lwg_spade_skip_mark_kernel<G>, dim3((unsigned)tiles), dim3(256), 0, stream, reinterpret_cast<const float2*>(T), B, ns, h, w, d,
                       js.j[0].marks, js.j[1].marks, js.j[2].marks);
    hipLaunchKernelGGL(lwg_spade_skip_scan_kernel, dim3(levels), dim3(1024), 0, stream, js);
    return (int)hipGetLastError();
}

extern "C" int lwg_spade_skip_lists_f32(const float* T, int B, int ns, int h, int w, int d, int* marks, int* heavy, int* light, int* counts,
                                        lwg_stream_t stream_) {
    return sk_lists<void>(T, B, ns, h, w, d, SkScanJobs{{{marks, 0, heavy, light, counts}, {}, {}}}, stream_);
}
extern "C" int lwg_spade_skip_fine_lists_f32(const float* T, int B, int ns, int h, int w, int d, int* marks, int* heavy, int* light, int* counts,
                                             int* fmarks, int* fheavy, int* flight, int* fcounts, lwg_stream_t stream_) {
    return sk_lists<Cw4F>(T, B, ns, h, w, d, SkScanJobs{{{marks, 0, heavy, light, counts}, {fmarks, 0, fheavy, flight, fcounts}, {}}}, stream_);
}
// The block lists, the 16 x 8 lists (both as lwg_spade_skip_fine_lists_f32 leaves them) AND the 8 x 8 lists (qmarks, qheavy, qlight: 8 * B * tiles ints
// each, qcounts: 2 ints) in the same two launches
extern "C" int lwg_spade_skip_q8_lists_f32(const float* T, int B, int ns, int h, int w, int d, int* marks, int* heavy, int* light, int* counts,
                                           int* fmarks, int* fheavy, int* flight, int* fcounts, int* qmarks, int* qheavy, int* qlight, int* qcounts,
                                           lwg_stream_t stream_) {
    return sk_lists<Cw4Q>(T, B, ns, h, w, d,
                          SkScanJobs{{{marks, 0, heavy, light, counts}, {fmarks, 0, fheavy, flight, fcounts}, {qmarks, 0, qheavy, qlight, qcounts}}}, stream_);
}
