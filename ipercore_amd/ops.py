"""Thin tensor-level wrappers over the C ABI (include/lwg_hip.h).

PyTorch-ROCm is plumbing here: it owns device memory and the stream; every compute call goes through
``liblwg_hip.so``.  All wrappers require contiguous CUDA tensors and raise otherwise - there is no eager /
CPU fallback on the product path.
"""
import collections
import ctypes
import functools

import torch

from . import _lib
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_RELU_MASK, ACT_SIGMOID, ACT_TANH, EPI_NONE, EPI_RESIDUAL, EPI_SPADE  # noqa: F401

EYE_DIST = 2.7320508075688776   # 1/tan(30 deg) + 1 (reference renders/nmr.py:225)


def _ptr(t, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("ipercore_amd ops need CUDA (HIP) tensors: the MI355X path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return t.data_ptr()


# "fp32": native fp32 MFMA.  "bf16": the engine keeps every activation tensor in bf16 and the convs with Cin % 64 == 0 run on the bf16
# MFMA kernel (dispatch is by tensor dtype: ops.conv2d on bf16 tensors; this flag tells the generator what to allocate).  "split": the same convs run on the bf16x6 kernel - both operands split EXACTLY into three bf16 parts,
# six bf16 MFMAs per fp32 product, fp32 accumulation: fp32-level accuracy at 0.375 of the native matrix-pipe time.  "winograd": the 3x3 / stride 1
# convolutions with Cin % 32 == 0 - one input or a skip concatenation (both channel counts % 8 == 0), plain / residual / SPADE (gamma | beta stacked)
# epilogue, fp32 NHWC output - run as fused F(2x2, 3x3) Winograd convolutions on the fp32 matrix pipe (csrc/conv_winograd.hip: 16 multiplies per
# 2x2 outputs instead of 36; fp32-grade, not bitwise the direct result); everything else exactly as "fp32" (same kernels, same head).
# "bf16_winograd": "bf16" with the eligible 3x3 / stride 1 launches (_bf16_wino_eligible) on the fused bf16 F(2x2, 3x3) Winograd kernel
# (csrc/conv_winograd_bf16.hip: 4 multiplies per output instead of 9; V and U rounded once to bf16 - 1.2-1.9x the direct bf16 kernel's error, not its
# bits); every other bf16 launch exactly as in "bf16".
# "bf16_operands" (opt-in, the training step's: trainers.TrainOpts.conv_precision): fp32 tensors, ONE bf16 product per multiply - the launches
# _bf16op_use takes (fp32 in and out, Cin % 32 == 0, N % 64 == 0, plain or residual epilogue, any taps / stride / parity form) round both fp32
# operands to bf16 in the kernel, multiply on the bf16 matrix pipe and accumulate in fp32 (csrc/conv_igemm_bf16op.hip, the fp32 panel as it is;
# DESIGN.md 3.10d; tests/convbf16op_emu.py is the definition): bf16-operand grade, deterministic; every other launch exactly as "fp32".
CONV_PRECISION = "fp32"


class conv_precision(object):
    """Context manager: ``with ops.conv_precision("bf16"): ...``.  "winograd2x2" = "winograd" with the F(4x4, 3x3) kernel off (every eligible layer on
    the F(2x2, 3x3) kernel - rounds 5 / 6's engine): the latency engine of single-frame callers (a one-frame launch of the F(4x4, 3x3) kernel is 32
    workgroups on a 64^2 layer: 3.6 against 2.4 ms per frame at frame batch 1), 20 % slower on frame batches.  Each engine is batch-invariant in itself."""

    def __init__(self, mode):
        assert mode in ("fp32", "bf16", "bf16_winograd", "split", "winograd", "winograd2x2", "bf16_operands")
        self.mode = mode

    def __enter__(self):
        global CONV_PRECISION, _MODE_WINO4
        self.prev = CONV_PRECISION, _MODE_WINO4
        CONV_PRECISION, _MODE_WINO4 = ("winograd", False) if self.mode == "winograd2x2" else (self.mode, True)

    def __exit__(self, *exc):
        global CONV_PRECISION, _MODE_WINO4
        CONV_PRECISION, _MODE_WINO4 = self.prev


_MODE_WINO4 = True      # the mode's say on the F(4x4, 3x3) kernel (False inside "winograd2x2"): set on every enter, never the lab switch WINO4


# bench.py installs a callable(begin, M, spec, epi, info) to bracket conv entry-point calls with HIP events; info (the closing call only, else
# None) = {"kernels": launches behind the call (lwg_conv_slice_count: batch slices), "kind": which kernel family ran ("direct", "winograd",
# "split", "bf16", "bf16_winograd", "bf16op", "up4")} - launch / executed-flop accounting only
CONV_HOOK = None


def _stream():
    return torch.cuda.current_stream().cuda_stream


class ConvSpec:
    """Host description of one packed convolution (weights already in the kernel's layout)."""
    __slots__ = ("w", "bias", "N", "Cin", "ntaps", "dy", "dx", "stride", "cshift", "omul", "ooy", "oox", "algo_kn", "_panels")

    def __init__(self, w, bias, N, Cin, taps, stride=1, omul=1, ooy=0, oox=0, algo_kn=None):
        self.w, self.bias, self.N, self.Cin = w, bias, int(N), int(Cin)
        # un-padded K*N of the convolution this panel implements: 2*M*algo_kn = its algorithmic flops
        self.algo_kn = int(algo_kn) if algo_kn is not None else len(taps) * int(Cin) * int(N)
        self.ntaps = len(taps)
        self.dy = [int(t[0]) for t in taps]
        self.dx = [int(t[1]) for t in taps]
        self.stride, self.omul, self.ooy, self.oox = stride, omul, ooy, oox
        self._panels = {}       # kernel-specific panels derived from w (and bias): read and written by _derived only
        self.cshift = 0
        if self.Cin % 32 != 0:
            q = self.Cin // 4
            assert q in (1, 2, 4), "small-Cin path handles Cin in {4, 8, 16}"
            self.cshift = q.bit_length() - 1


def _derived(specs, key, build, bias=False):
    """The panel ``build()`` derives from one spec's fp32 GEMM panel, or from those of the four parity specs of a transposed convolution, built
    once and kept on the (first) spec under ``key`` = (panel kind, whatever else selects a variant).  An entry records every tensor it was built
    from - ``w`` of each spec, and the spec's ``bias`` where the entry hands a bias back (bias=True) - and is valid only while each of them IS
    still the spec's current tensor (packing.spec_to to another device, a replaced weight); otherwise it is rebuilt.
    The one thing this rule does not see is an in-place write to ``spec.w``: the trainer's persistent GEMM panels are refreshed in place
    (PanelCache.refresh), which is sound because training specs are rebuilt by packing.pack_conv* on every step."""
    specs = specs if isinstance(specs, (list, tuple)) else (specs,)
    src = [s.w for s in specs] + ([specs[0].bias] if bias else [])
    hit = specs[0]._panels.get(key)
    if hit is None or len(hit[0]) != len(src) or any(a is not b for a, b in zip(hit[0], src)):
        hit = specs[0]._panels[key] = (src, build())
    return hit[1]


def _tap_order9(spec):
    """The 3x3 tap order of a spec: position 3 * (dy + 1) + (dx + 1) -> tap index in the GEMM panel."""
    order = [0] * 9
    for t in range(spec.ntaps):
        order[3 * (spec.dy[t] + 1) + spec.dx[t] + 1] = t
    return order


def _spade_columns(N, blk, device):
    """SPADE panels: for every column of a panel that interleaves gamma | beta in blocks of ``blk``, the column of the GEMM panel (blocks of 32)
    that holds it."""
    j = torch.arange(N, device=device)
    ch, beta = blk * (j // (2 * blk)) + j % blk, (j % (2 * blk)) // blk
    return 64 * (ch // 32) + (ch % 32) + 32 * beta


def _w16v2(spec):
    """The bf16 panel of lwg_conv2d_nhwc_bf16, built once per spec from the fp32 panel [K/4][N][4] (K order: 32-channel chunk major,
    tap minor): [ntaps*Cin/64][N][64] with k = ((c/64)*ntaps + tap)*64 + c%64, the eight 16-byte k-octets of row n stored at slot
    octet ^ ((n >> 1) & 7) (include/lwg_hip.h)."""
    def build():
        K4, N, _ = spec.w.shape
        cin, nt = spec.Cin, spec.ntaps
        assert cin % 64 == 0 and K4 * 4 == nt * cin, (cin, nt, K4)
        wk = spec.w.permute(0, 2, 1).reshape(cin // 64, 2, nt, 32, N)             # [c64][half][tap][c%32][n]
        wk = wk.permute(0, 2, 1, 3, 4).reshape(cin // 64 * nt, 64, N)              # [kstep][k%64][n]
        rows = wk.permute(0, 2, 1).reshape(cin // 64 * nt, N, 8, 8)                # [kstep][n][octet][8]
        n = torch.arange(N, device=spec.w.device)
        slot = torch.arange(8, device=spec.w.device)
        src = slot[None, :] ^ ((n[:, None] >> 1) & 7)                              # octet stored at slot s of row n
        rows = torch.gather(rows, 2, src[None, :, :, None].expand(rows.shape[0], N, 8, 8))
        return rows.reshape(cin // 64 * nt, N, 64).contiguous().to(torch.bfloat16)
    return _derived(spec, "w16v2", build)


def _hr_eligible(spec, x0, y, out_hw):
    """lwg_conv2d_nhwc_bf16_hr applies to the 3x3 / 2x2-tap stride-1 launches on a shared input / output grid."""
    if not BF16_HR or spec.stride != 1 or spec.ntaps not in (9, 4) or spec.N % 64 != 0 or spec.Cin % 64 != 0:
        return False
    if any(abs(d) > 1 for d in spec.dy) or any(abs(d) > 1 for d in spec.dx):
        return False
    OH, OW = ((y.shape[1], y.shape[2]) if spec.omul == 1 else (y.shape[1] // spec.omul, y.shape[2] // spec.omul)) if out_hw is None else out_hw
    return (OH, OW) == (x0.shape[1], x0.shape[2])


def _hr_tap_order(spec):
    """Tap permutation of the register-streamed panel: ascending in (dy, dx) - the row-renaming kernel wants an NDY x NDX grid in
    row-major order (a transposed convolution's parity launches list their taps descending)."""
    return sorted(range(spec.ntaps), key=lambda t: (spec.dy[t], spec.dx[t]))


def _w16hr(spec, spade):
    """(panel, bias) of lwg_conv2d_nhwc_bf16_hr: [ntaps*Cin/64][4][N][16] bf16, k = ((c/64)*ntaps + tap)*64 + c%64 split as
    ks*16 + e; for the SPADE epilogue the gamma | beta columns (and the bias) are re-interleaved from blocks of 32 to blocks of 16
    (include/lwg_hip.h).  Built once per (spec, spade)."""
    def build():
        K4, N, _ = spec.w.shape
        cin, nt = spec.Cin, spec.ntaps
        wk = spec.w.permute(0, 2, 1).reshape(cin // 64, 2, nt, 32, N).permute(0, 2, 1, 3, 4).reshape(cin // 64, nt, 64, N)    # [chunk][tap][k%64][n]
        wk = wk[:, _hr_tap_order(spec)].reshape(cin // 64 * nt, 64, N)                                                          # taps ascending in (dy, dx)
        bias = spec.bias
        if spade:
            old = _spade_columns(N, 16, spec.w.device)
            wk = wk[:, :, old]
            bias = None if bias is None else bias[old].contiguous()
        return wk.reshape(cin // 64 * nt, 4, 16, N).permute(0, 1, 3, 2).contiguous().to(torch.bfloat16), bias
    return _derived(spec, ("w16hr", bool(spade)), build, bias=True)


BF16_WINO_MIN_CIN = 64  # "bf16_winograd": layers with fewer input channels stay on the direct kernel (a rule on the LAYER, never on the batch)
_WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def _bf16_wino_eligible(spec, x0, y, x1, epi, act, out_hw, ycoff=0):
    """Launches of the "bf16_winograd" mode that run lwg_conv2d_winograd_bf16: the 3x3 subset of what _hr_eligible takes (stride 1, pad 1,
    Cin % 64 == 0, N % 64 == 0, output grid = input grid) with a plain / residual / SPADE epilogue and Cin >= BF16_WINO_MIN_CIN - tested here
    directly, so the lab switch BF16_HR does not reach this mode.  Never a rule on the batch."""
    if spec.ntaps != 9 or spec.stride != 1 or spec.omul != 1 or spec.N % 64 != 0 or spec.Cin % 64 != 0 or spec.Cin < BF16_WINO_MIN_CIN:
        return False
    if (y.shape[1], y.shape[2]) != (x0.shape[1], x0.shape[2]) or (out_hw is not None and tuple(out_hw) != (x0.shape[1], x0.shape[2])):
        return False
    if sorted(zip(spec.dy, spec.dx)) != _WINO_TAPS or epi not in (EPI_NONE, EPI_RESIDUAL, EPI_SPADE):
        return False
    if act not in (ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID) or y.dtype != torch.bfloat16:
        return False
    if x1 is not None and (x1.dtype != torch.bfloat16 or x0.shape[3] % 64 != 0):
        return False
    if epi == EPI_SPADE:
        return y.shape[3] * 2 == spec.N and ycoff == 0
    return y.shape[3] % 8 == 0 and ycoff % 8 == 0 and ycoff + spec.N <= y.shape[3]


def wwino16_index(ks, p, n, e, N):
    """Element index of (k-step ks, product p = 4 xi + nu, output column n, channel e of the k-step) in lwg_conv2d_winograd_bf16's panel
    Upk[Cin/16][16][N][16] (include/lwg_hip.h): the value there is bf16((G w G^T)[xi][nu]) of input channel 16 ks + e and column n."""
    return ((ks * 16 + p) * N + n) * 16 + e


def wwino16_spade_column(j):
    """SPADE launches: (output channel, is_beta) of panel column j - gamma | beta interleaved in blocks of 4."""
    return 4 * (j // 8) + j % 4, (j % 8) // 4


def _wwino16(spec, spade):
    """(panel, bias) of lwg_conv2d_winograd_bf16, built once per (spec, spade) from the fp32 GEMM panel with torch ops on whatever device spec.w
    is on: U = G w G^T per (input channel, output column) in fp64, rounded ONCE to bf16, stored Upk[Cin/16][16][N][16] (wwino16_index); for the
    SPADE epilogue the gamma | beta columns (and the bias) go from the GEMM panel's blocks of 32 to blocks of 4 (wwino16_spade_column)."""
    def build():
        K4, N, _ = spec.w.shape
        cin, nt = spec.Cin, spec.ntaps
        assert nt == 9 and cin % 64 == 0 and N % 64 == 0 and K4 * 4 == nt * cin, (cin, nt, K4, N)
        dev = spec.w.device
        # fp32 GEMM panel [K/4][N][4], k = ((c / 32) * 9 + tap) * 32 + c % 32  ->  w[tap][c][n]
        wk = spec.w.permute(0, 2, 1).reshape(cin // 32, nt, 32, N).permute(1, 0, 2, 3).reshape(nt, cin, N)
        w33 = wk[_tap_order9(spec)].reshape(3, 3, cin, N).to(torch.float64)                        # [r][s][c][n], tap (dy, dx) = (r - 1, s - 1)
        G = torch.tensor(_WINO_G, dtype=torch.float64, device=dev)
        U = torch.einsum("ar,rscn,bs->abcn", G, w33, G)                                            # [xi][nu][c][n]
        bias = spec.bias
        if spade:
            old = _spade_columns(N, 4, dev)
            U = U[:, :, :, old]
            bias = None if bias is None else bias[old].contiguous()
        return U.reshape(16, cin // 16, 16, N).permute(1, 0, 3, 2).contiguous().to(torch.bfloat16), bias   # [ks][p][n][e]
    return _derived(spec, ("wwino16", bool(spade)), build, bias=True)


BF16_HR = True          # lab switch: False routes every bf16 convolution to lwg_conv2d_nhwc_bf16 (LDS-DMA kernels)
BF16_PW = True          # lab switch: the pointwise (1x1, C -> C) launches on the register-resident-weights kernel
BF16_C8 = True          # lab switch: the fp32-input first layer on the bf16 MFMA kernel (False: fp32 MFMA kernel, bf16 output)


def _pw_eligible(spec, x0, y, x1, epi, out_hw):
    """The 1x1 / stride-1 / C -> C launches (the attention blocks' query projections) go to lwg_conv2d_nhwc_bf16_hr with ntaps = 1."""
    if not BF16_PW or spec.ntaps != 1 or spec.stride != 1 or spec.omul != 1 or x1 is not None or epi != EPI_NONE:
        return False
    if spec.dy[0] != 0 or spec.dx[0] != 0 or spec.N != spec.Cin or spec.N not in (64, 128, 256):
        return False
    OH, OW = (y.shape[1], y.shape[2]) if out_hw is None else out_hw
    return (OH, OW) == (x0.shape[1], x0.shape[2])


def _w16c8(spec):
    """bf16 panel of lwg_conv2d_nhwc_c8_bf16: [ceil(ntaps/2)][N][16], k = tap*8 + c (the small-Cin K order of the fp32 panel)."""
    def build():
        K4, N, _ = spec.w.shape
        nks = (spec.ntaps + 1) // 2
        wk = spec.w.permute(0, 2, 1).reshape(K4 * 4, N)
        if wk.shape[0] < nks * 16:
            wk = torch.cat([wk, wk.new_zeros(nks * 16 - wk.shape[0], N)], dim=0)
        return wk[:nks * 16].reshape(nks, 16, N).permute(0, 2, 1).contiguous().to(torch.bfloat16)
    return _derived(spec, "w16c8", build)


def _w16x3(spec):
    """The three-plane bf16 panel [3][K/8][N][8] of a spec: w = hi + mid + lo exactly (round-to-nearest residual splits)."""
    def build():
        K4, N, _ = spec.w.shape
        wk = spec.w.permute(0, 2, 1).reshape(K4 * 4, N)
        hi = wk.to(torch.bfloat16)
        r1 = wk - hi.float()
        mid = r1.to(torch.bfloat16)
        lo = (r1 - mid.float()).to(torch.bfloat16)
        return torch.stack([hi, mid, lo]).view(3, K4 // 2, 8, N).permute(0, 1, 3, 2).contiguous()
    return _derived(spec, "w16x3", build)


def _bf16op_use(spec, x0, y, x1=None, epi=EPI_NONE, act=ACT_NONE, q4=False, ycoff=0):
    """Launches of the "bf16_operands" mode that run lwg_conv2d_nhwc_f32_bf16op[_ws] - the single place for the rule, a rule on the layer and
    launch description (never on the batch or the data): fp32 NHWC in and out (no channel-quad planes), Cin % 32 == 0 - a second input on
    32 channels -, N % 64 == 0, a plain or residual epilogue (the ReLU mask with the residual only), the output slice on 4 channels.  Any taps,
    stride and parity form (omul / ooy / oox).  Everything else - the small-Cin first layers, SPADE, q4 - keeps the "fp32" route.
    One class of launches is excluded on speed, and not here (a conv2d call does not know its siblings): ``_bf16op_use_parity4``, the
    small parity groups of a ``conv_transpose2d`` call.  The per-shape table is profiles/conv_bf16op_layers.txt."""
    if q4 or x0.dtype != torch.float32 or y.dtype != torch.float32 or spec.Cin % 32 != 0 or spec.N % 64 != 0:
        return False
    if x1 is not None and (x1.dtype != torch.float32 or x0.shape[3] % 32 != 0):
        return False
    if epi not in (EPI_NONE, EPI_RESIDUAL) or (act == ACT_RELU_MASK and epi != EPI_RESIDUAL):
        return False
    return y.shape[-1] % 4 == 0 and ycoff % 4 == 0


def _bf16op_use_parity4(specs, x, y, act=ACT_NONE, splitk=False, out_hw=None, q4=False):
    """``_bf16op_use`` for the four parity launches of ONE ``conv_transpose2d`` call (a transposed convolution's forward, a 4x4 / stride-2 convolution's
    data gradient) - the one class of launches the mode leaves on the "fp32" route for speed, by a rule on the launch description: a group that the
    "fp32" mode runs as ONE grid (lwg_conv_transpose4_is_one_grid: a parity has fewer than 300 tiles of 128 x 128) AND whose parity launches the
    library's plan would split over K (lwg_conv2d_bf16op_ws_floats > 0; training callers, splitk=True).  There the mode would make eight kernels -
    four slab launches, four finishing kernels - against one grid: measured 1.07 - 1.41 of the one-grid form's time on all seven such groups of the
    512^2 step (82 - 108 us against 59 - 95), while every other parity group gains (0.42 - 0.75; profiles/conv_bf16op_parity_groups_before_rule.txt,
    DESIGN.md 3.10d)."""
    s0 = specs[0]
    if not _bf16op_use(s0, x, y, None, EPI_NONE, act, q4):
        return False
    if not (splitk and _up4_f32_ok(x, specs, y)):               # conv_transpose2d's own condition for asking about the one-grid form
        return True
    hw = None if out_hw is None else tuple(out_hw(s0))
    key = (tuple(x.shape), tuple(y.shape), s0.N, hw)            # the two library answers are functions of B, OH, OW, Cin, N, ntaps = 4: asked once
    use = _PARITY4_PLAN.get(key)
    if use is None:
        a = conv_args(x, s0, y, act=act, out_hw=hw)
        use = _PARITY4_PLAN[key] = not (_lib.lib().lwg_conv_transpose4_is_one_grid(a) and _lib.lib().lwg_conv2d_bf16op_ws_floats(a))
    return use


_PARITY4_PLAN = {}


_WINO_TAPS = sorted((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))


def _wino_eligible(spec, x0, y, x1, epi, act, out_hw, q4, ycoff=0):
    """Launches lwg_conv2d_winograd_f32 takes: 3x3 / stride 1 / pad 1, fp32, Cin % 32 == 0 (one input or a skip concatenation with both channel
    counts % 8 == 0), plain / residual / SPADE (gamma | beta stacked, N = 2 C) epilogue, dense output."""
    if q4 or x0.dtype != torch.float32 or y.dtype != torch.float32 or epi not in (EPI_NONE, EPI_RESIDUAL, EPI_SPADE) or \
            (act == ACT_RELU_MASK and epi != EPI_RESIDUAL):
        return False
    if x1 is not None and (x1.dtype != torch.float32 or x0.shape[3] % 8 != 0 or x1.shape[3] % 8 != 0):
        return False
    if spec.ntaps != 9 or spec.stride != 1 or spec.omul != 1 or spec.Cin % 32 != 0 or spec.N % 64 != 0:
        return False
    if epi == EPI_SPADE and (y.shape[3] * 2 != spec.N or ycoff != 0):
        return False
    if sorted(zip(spec.dy, spec.dx)) != _WINO_TAPS:
        return False
    hw = (y.shape[1], y.shape[2]) if out_hw is None else tuple(out_hw)
    return hw == (x0.shape[1], x0.shape[2]) == (y.shape[1], y.shape[2])


WINO_MIN_GRID = 128     # workgroups (64 patches x 32 channels, times the K slices) below which a splitk=True caller gets the direct split-K form instead
WINO_SPLITK = True      # lab switch: False = training launches never split the Winograd kernel's K loop


def _wino_plan(a, spec, y, splitk):
    """How an eligible launch runs in the "winograd" mode: 0 = the Winograd kernel whole, n > 0 = split over K through a workspace of n floats
    (lwg_conv2d_winograd_f32_ws), None = not on the Winograd kernel.  Only a training launch (splitk=True) asks: one whose Winograd grid would leave
    most of the 256 CUs idle - a 28 x 28 x 512 VGG19 layer is 64 workgroups of 64 K stages each, 79 us whole against the direct kernel's split-K
    51 us - runs its K loop in slices when that fills the chip, and stays on the direct split-K kernel when even the slices do not
    (profiles/r05_g_winograd_small_launches.txt).  The synthesis path never asks (splitk=False: batch invariance)."""
    if not splitk:
        return 0
    # the kernel's own plan (lwg_conv2d_winograd_plan) - not a host copy of its tile geometry
    blocks, slices, nbv = ctypes.c_longlong(0), ctypes.c_int(0), ctypes.c_int(0)
    if _lib.lib().lwg_conv2d_winograd_plan(a, 1 if WINO_SPLITK else 0, ctypes.byref(blocks), ctypes.byref(slices), ctypes.byref(nbv), None) != 0:
        return None
    units32 = blocks.value * (nbv.value // 32)              # 64-patch x 32-channel units of work, times the K slices
    return slices.value * a.M * spec.N if units32 >= WINO_MIN_GRID else None


def _wwino(spec):
    """The transformed-weight fragment panel of lwg_conv2d_winograd_f32, built once per spec from the fp32 GEMM panel by ONE launch
    (lwg_winograd_panel_f32): U = G w G^T per (input, output) channel pair in fp64, rounded once, stored [16][Cin/8][2][N][4] - element
    (p, s, kh, n, kk) = U[p // 4][p % 4] of input channel 8 s + 2 kk + kh."""
    def build():
        cin, N, tap9 = _wino_panel_source(spec)
        if PANEL_CACHE is not None:                          # a training step: panels of registered weights are refreshed once per step
            U = PANEL_CACHE.winograd(spec, list(tap9))
            if U is not None:
                return U
        U = torch.empty(16, cin // 8, 2, N, 4, device=spec.w.device, dtype=torch.float32)
        _lib.check(_lib.lib().lwg_winograd_panel_f32(_ptr(spec.w), _ptr(U), cin, N, tap9, _stream()), "lwg_winograd_panel_f32")
        return U
    return _derived(spec, "wwino", build)


def _wino_panel_source(spec):
    """(Cin, N, the tap order as the C array) of a 3x3 spec whose fp32 GEMM panel a panel-building launch may read."""
    K4, N, _ = spec.w.shape
    cin, nt = spec.Cin, spec.ntaps
    assert nt == 9 and cin % 32 == 0 and K4 * 4 == nt * cin, (cin, nt, K4)
    if not spec.w.is_cuda:
        raise RuntimeError("ipercore_amd ops need CUDA (HIP) tensors: the MI355X path has no CPU fallback")
    return cin, N, (ctypes.c_int * 9)(*_tap_order9(spec))


WINO4 = True            # lab switch: in the "winograd" mode the synthesis path's eligible launches with Cin >= WINO4_MIN_CIN run the F(4x4, 3x3) kernel
WINO4_MIN_CIN = 64      # below it the F(2x2, 3x3) kernel stays (a block's K loop must pay for the 28-plane exchange of the F(4x4, 3x3) epilogue)


# The training step's Winograd tiles (trainers.TrainOpts.conv_tiles).  "2x2": every training launch (splitk=True) of the "winograd" mode keeps the
# F(2x2, 3x3) kernel and its split plan, or the direct split-K kernel.  "4x4": the eligible ones with Cin >= WINO4_MIN_CIN that _wino4_plan takes run
# the F(4x4, 3x3) kernel, whole or split over K (lwg_conv2d_winograd4_f32_ws); every other launch exactly as "2x2".  The synthesis
# path (splitk=False) does not read it.
TRAIN_CONV_TILES = "2x2"


class train_conv_tiles(object):
    """Context manager: ``with ops.train_conv_tiles("4x4"): ...`` (trainers.TrainOpts.conv_tiles)."""

    def __init__(self, mode):
        assert mode in ("2x2", "4x4")
        self.mode = mode

    def __enter__(self):
        global TRAIN_CONV_TILES
        self.prev = TRAIN_CONV_TILES
        TRAIN_CONV_TILES = self.mode

    def __exit__(self, *exc):
        global TRAIN_CONV_TILES
        TRAIN_CONV_TILES = self.prev


def _wino4_use(spec, splitk):
    """Which launches of the "winograd" mode run lwg_conv2d_winograd4_f32 (F(4x4, 3x3): 2.25 multiplies per output instead of 4): a rule on the LAYER
    (its Cin), never on the batch - a frame's result must not depend on how many frames share its launch.  Training launches (splitk=True) keep the
    F(2x2, 3x3) kernel and its split plan unless the step runs with ``train_conv_tiles("4x4")`` - then ``_wino4_plan`` has the last word."""
    return WINO4 and _MODE_WINO4 and spec.Cin >= WINO4_MIN_CIN and (not splitk or TRAIN_CONV_TILES == "4x4")


# Which of the library's F(4x4) forms a training launch takes - each only where it was FASTER than the parent's choice on the launch shapes of the
# 512^2 personalization step (tools/train_conv_tiles_ab.py, profiles/train_conv_tiles_layers.txt; DESIGN.md 3.12g has the table):
#  * whole, where the library plans no split and the launch is more than 128 units of 32 x 16 pixels x 32 channels (0.66 - 0.97 of the F(2x2) time
#    on every such shape of the step, 224 units and up; the one measured below that, 32 units, lost: 1.57);
#  * split over K, where every slice keeps at least 128 input channels (0.85 - 0.97 on the four such shapes: Cin 256 in two slices, 512 in four;
#    slices of 64 channels pay the block's prologue and 28-plane epilogue for too little: 0.96 - 1.70, most of them losses).
WINO4_TRAIN_MIN_GRID = 129      # units (times the K slices) a training launch needs for F(4x4)
WINO4_TRAIN_MIN_SLICE_CIN = 128 # input channels per K slice a split launch needs
WINO4_TRAIN_WHOLE = True        # lab switch: False = the training launches the library would run whole stay with the parent's choice
WINO4_TRAIN_SPLITK = True       # lab switch: False = ... and so do the ones it would split over K


def _wino4_plan(a):
    """How a training launch (splitk=True) that ``_wino4_use`` admits runs: 0 = the F(4x4, 3x3) kernel whole, n > 0 = split over K through a
    workspace of n floats (lwg_conv2d_winograd4_f32_ws), None = not on F(4x4) - the launch then falls through to ``_wino_plan`` exactly as with
    ``train_conv_tiles("2x2")``.  The tile geometry and the split plan are the library's (lwg_conv2d_winograd4_plan); the thresholds above say
    which of its answers the step takes."""
    blocks, slices, nbv = ctypes.c_longlong(0), ctypes.c_int(0), ctypes.c_int(0)
    if _lib.lib().lwg_conv2d_winograd4_plan(a, 1, ctypes.byref(blocks), ctypes.byref(slices), ctypes.byref(nbv), None) != 0:
        return None
    if not (WINO4_TRAIN_SPLITK if slices.value else WINO4_TRAIN_WHOLE) or blocks.value * (nbv.value // 32) < WINO4_TRAIN_MIN_GRID:
        return None
    if slices.value and a.C0 + a.C1 < WINO4_TRAIN_MIN_SLICE_CIN * slices.value:
        return None
    return slices.value * a.M * a.N


def _wwino4(spec):
    """The fragment panel of lwg_conv2d_winograd4_f32, built once per spec from the fp32 GEMM panel by ONE launch (lwg_winograd4_panel_f32):
    U = G w G^T (6 x 6) per (input, output) channel pair in fp64, rounded once, stored [4][Cin/8][4][2][9 N] (include/lwg_hip.h)."""
    def build():
        cin, N, tap9 = _wino_panel_source(spec)
        if PANEL_CACHE is not None:                          # a training step: panels of registered weights are refreshed once per step
            U = PANEL_CACHE.winograd4(spec, list(tap9))
            if U is not None:
                return U
        U = torch.empty(4, cin // 8, 4, 2, 9 * N, device=spec.w.device, dtype=torch.float32)
        _lib.check(_lib.lib().lwg_winograd4_panel_f32(_ptr(spec.w), _ptr(U), cin, N, tap9, _stream()), "lwg_winograd4_panel_f32")
        return U
    return _derived(spec, "wwino4", build)


SPADE_SKIP = True       # switch: the SPADE convolutions of the attention sites ("winograd" mode, fp32, F(4x4, 3x3) launches of the 8-wave form) run
                        # list-driven - blocks whose input window is all background are filled from a calibration frame
SPADE_SKIP_D = (1, 5)   # pixels a block's window reaches beyond the block: the `shared` convolution, the gamma | beta convolution behind it
SPADE_SKIP_BF16 = False # ... and, with SPADE_SKIP, the 3 x 3 SPADE launches of the "bf16" mode (lwg_conv2d_nhwc_bf16_hr_list).  OFF by default: on BASELINE
                        # configs[3]'s batch the eighteen launches gain 6.8 %, the generator pass as a whole loses 0.7 % (DESIGN.md 3.12f has the A/B)
SPADE_SKIP_D_BF16 = (1, 2)      # ... in the "bf16" mode (lwg_conv2d_nhwc_bf16_hr_list): the direct kernel has no Winograd patches - an
                                # output pixel depends on its own 3 x 3 window, and the second convolution reads one pixel further


SPADE_SKIP_FINE = True  # ... at the granularity of 16 x 8 sub-tiles (four per block) where ``spade_skip_fine_apply`` says so; False: block lists everywhere

SPADE_SKIP_Q8 = True    # ... and at 8 x 8 sub-tiles (eight per block, lwg_conv2d_winograd4_q8_f32) where ``spade_skip_q8_apply`` says so:
SPADE_SKIP_Q8_MIN = 640         # ... launches of at least this many (in-image block, column block) entries - the smallest measured, still a gain
                                #  - ...
SPADE_SKIP_Q8_MAX_HW = 64 * 64  # ... on feature maps of at most this many pixels: at 128^2 and 256^2 the body is a small part of the frame, the launch
                                # is mostly light entries, and twice as many of half the size cost more than the smaller heavy share returns

_LISTS_APPLY = {}


class SkipLists(tuple):
    """``spade_skip_lists``'s result: the block-level (heavy, light, counts), and as ``.fine`` the sub-tile-level triple from the same launches; as
    ``.fine8`` the 8 x 8 triple where a launch on these frames can take it (``spade_skip_q8_lists_apply``), else None."""
    fine = None
    fine8 = None


def spade_skip_fine_apply(x0):
    """Does a list-driven launch on this input take the sub-tile lists?  A rule on the configuration only (switch, feature size)."""
    return SPADE_SKIP_FINE


def spade_skip_q8_apply(x0, ncb):
    """Does a list-driven launch on this input with ncb column blocks take the 8 x 8 lists?  A rule on the configuration and the launch's size only."""
    B, H, W = x0.shape[:3]
    return SPADE_SKIP_FINE and SPADE_SKIP_Q8 and H * W <= SPADE_SKIP_Q8_MAX_HW and B * ((H + 15) // 16) * ((W + 31) // 32) * ncb >= SPADE_SKIP_Q8_MIN


def spade_skip_q8_lists_apply(tiles, h, w):
    """Are the 8 x 8 lists built for a frame batch of this many blocks at h x w?  Where a launch of up to eight column blocks (N <= 512) could take them."""
    return SPADE_SKIP_FINE and SPADE_SKIP_Q8 and CONV_PRECISION == "winograd" and h * w <= SPADE_SKIP_Q8_MAX_HW and tiles * 8 >= SPADE_SKIP_Q8_MIN


def spade_skip_lists(flow, d):
    """The heavy / light tile lists of one frame batch for ``conv2d(..., lists=)`` from its resized flows (B, ns, h, w, 2): two launches, everything
    stays in device memory (lwg_spade_skip_fine_lists_f32).  Returns (heavy, light, counts) int32 tensors of the 32 x 16 blocks - a ``SkipLists``,
    whose ``.fine`` holds the same triple for the 16 x 8 sub-tiles and ``.fine8`` the one for the 8 x 8 sub-tiles (lwg_spade_skip_q8_lists_f32, the same
    two launches) where ``spade_skip_q8_lists_apply`` says so."""
    B, ns, h, w, two = flow.shape
    assert two == 2 and flow.dtype == torch.float32
    tiles = B * ((h + 15) // 16) * ((w + 31) // 32)
    q8 = spade_skip_q8_lists_apply(tiles, h, w)
    # one buffer: per level (marks, heavy, light) of `per` entries per block, the finest level first (every marks array 16-byte aligned), then the
    # levels' counts - blocks, 16 x 8, 8 x 8
    per = ([8] if q8 else []) + [4, 1]
    n = 3 * sum(per) * tiles
    buf = torch.empty(n + 8, device=flow.device, dtype=torch.int32)
    levels, off = [], 0
    for p in per:
        levels.insert(0, [buf[off + i * p * tiles:off + (i + 1) * p * tiles] for i in range(3)])
        off += 3 * p * tiles
    for i, lv in enumerate(levels):
        lv.append(buf[n + 2 * i:n + 2 * i + 2])
    name = "lwg_spade_skip_q8_lists_f32" if q8 else "lwg_spade_skip_fine_lists_f32"
    _lib.check(getattr(_lib.lib(), name)(_ptr(flow), B, ns, h, w, int(d), *[_ptr(t, torch.int32) for lv in levels for t in lv], _stream()), name)
    out = SkipLists(levels[0][1:])
    out.fine = tuple(levels[1][1:])
    out.fine8 = tuple(levels[2][1:]) if q8 else None
    return out


def conv2d_lists_apply(x0, spec, y, epi=EPI_NONE, act=ACT_NONE, xn=None, mean=None, rstd=None):
    """Would ``conv2d`` run this launch list-driven if it were given lists?  A rule on the configuration (precision mode, switches, layer) and the
    launch's size (lwg_conv2d_winograd4_list_applies: the 8-wave form) - never on the tensors' content.  bf16 tensors in the "bf16" mode: the 3 x 3
    launches of lwg_conv2d_nhwc_bf16_hr that lwg_conv2d_nhwc_bf16_hr_list_applies takes (one input, N % 128 == 0, LWG_EPI_NONE / LWG_EPI_SPADE; any
    batch); never in "bf16_winograd", whose 3 x 3 layers run another kernel."""
    if x0.dtype == torch.bfloat16 or y.dtype == torch.bfloat16:
        if not SPADE_SKIP or not SPADE_SKIP_BF16 or CONV_PRECISION != "bf16" or not x0.is_cuda or x0.dtype != y.dtype or not _hr_eligible(spec, x0, y, None):
            return False
        key = ("bf16", x0.shape, y.shape, spec.Cin, spec.N, spec.ntaps, epi, act)
        if key not in _LISTS_APPLY:
            _LISTS_APPLY[key] = bool(_lib.lib().lwg_conv2d_nhwc_bf16_hr_list_applies(_hr_args(conv_args(x0, spec, y, None, epi, act, None, xn, mean, rstd), spec, epi)))
        return _LISTS_APPLY[key]
    if not SPADE_SKIP or CONV_PRECISION != "winograd" or not x0.is_cuda or x0.dtype != torch.float32 or not _wino4_use(spec, False) or \
            not _wino_eligible(spec, x0, y, None, epi, act, None, False):
        return False
    key = (x0.shape, y.shape, spec.Cin, spec.N, epi, act)          # the C rule reads the launch's sizes only: asked once per shape
    if key not in _LISTS_APPLY:
        a = conv_args(x0, spec, y, None, epi, act, None, xn, mean, rstd)
        a.w = _ptr(_wwino4(spec))
        _LISTS_APPLY[key] = bool(_lib.lib().lwg_conv2d_winograd4_list_applies(a))
    return _LISTS_APPLY[key]


def conv_args(x0, spec, y, x1=None, epi=EPI_NONE, act=ACT_NONE, res=None, xn=None, mean=None, rstd=None,
              out_hw=None, ycoff=0, q4=False):
    """Fill the C-ABI argument block of one conv launch (see ``conv2d``).  q4: y is (B, YC/4, YH, YW, 4) - channel-quad planes
    (LWG_DT_F32_Q4), fp32 launches without a fused residual / SPADE epilogue only."""
    B, H, W, C0 = x0.shape
    C1 = 0 if x1 is None else x1.shape[3]
    assert C0 + C1 == spec.Cin, (C0, C1, spec.Cin)
    if q4:
        YB, YCq, YH, YW, four = y.shape
        assert four == 4 and y.dtype == torch.float32 and x0.dtype == torch.float32 and epi == EPI_NONE and y.is_contiguous()
        YC = 4 * YCq
    else:
        YB, YH, YW, YC = y.shape
    if out_hw is None:
        OH, OW = (YH, YW) if spec.omul == 1 else (YH // spec.omul, YW // spec.omul)
    else:
        OH, OW = out_hw
    a = _lib.LwgConvArgs()
    xdt, ydt = x0.dtype, y.dtype
    a.xdt = _lib.DT_BF16 if xdt == torch.bfloat16 else _lib.DT_F32
    a.ydt = _lib.DT_F32_Q4 if q4 else (_lib.DT_BF16 if ydt == torch.bfloat16 else _lib.DT_F32)
    a.x0, a.x1 = _ptr(x0, xdt), _ptr(x1, xdt)
    a.C0, a.C1 = C0, C1
    a.B, a.H, a.W = B, H, W
    a.OH, a.OW, a.M = OH, OW, B * OH * OW
    a.stride, a.ntaps, a.cshift = spec.stride, spec.ntaps, spec.cshift
    a.w, a.N, a.bias = _ptr(spec.w), spec.N, _ptr(spec.bias)
    a.y, a.YH, a.YW, a.YC, a.ycoff = _ptr(y, ydt), YH, YW, YC, ycoff
    a.omul, a.ooy, a.oox = spec.omul, spec.ooy, spec.oox
    a.epi, a.act = epi, act
    a.res, a.xn, a.mean, a.rstd = _ptr(res, ydt), _ptr(xn, ydt), _ptr(mean), _ptr(rstd)
    a.dy[:spec.ntaps], a.dx[:spec.ntaps] = spec.dy, spec.dx
    return a


def _hr_args(a, spec, epi):
    """The launch description as lwg_conv2d_nhwc_bf16_hr (and its list / accumulator forms) takes it: the register-streamed panel, its bias and
    its tap order."""
    panel, bias = _w16hr(spec, epi == EPI_SPADE)
    a.w, a.bias = _ptr(panel, torch.bfloat16), _ptr(bias)
    for i, t in enumerate(_hr_tap_order(spec)):                      # the panel's tap order
        a.dy[i], a.dx[i] = spec.dy[t], spec.dx[t]
    return a


def conv2d_acc_frame(x0, spec, spade=True):
    """The fp32 ACCUMULATORS of the bf16 3 x 3 convolution of x0 (B, H, W, Cin) as lwg_conv2d_nhwc_bf16_hr_acc leaves them - no bias, no activation,
    no rounding, columns in the kernel's own order (spade: the gamma | beta panel): the calibration frame of a list-driven EPI_SPADE launch,
    (B, H, W, N) fp32.  A cold path: not announced to CONV_HOOK."""
    B, H, W, _ = x0.shape
    y = torch.empty(B, H, W, spec.N, device=x0.device, dtype=torch.float32)
    a = conv_args(x0, spec, y)
    a.ydt = _lib.DT_F32
    _hr_args(a, spec, EPI_SPADE if spade else EPI_NONE)
    _lib.check(_lib.lib().lwg_conv2d_nhwc_bf16_hr_acc(a, _stream()), "lwg_conv2d_nhwc_bf16_hr_acc")
    return y


def _hook_end(a, spec, epi, kind, slices=True, extra=0):
    """Closing hook call: how many kernel launches the entry point made (the C rule: lwg_conv_slice_count; extra: a split launch's finishing
    kernel) and which kernel family ran."""
    n = (max(1, int(_lib.lib().lwg_conv_slice_count(a))) if slices else 1) + extra
    CONV_HOOK(False, a.M, spec, epi, {"kernels": n, "kind": kind})


# What ONE conv launch runs - decided once (conv2d_route, conv_transpose2d_route) and read by whoever needs the answer; a value, no behaviour.
# kind: what CONV_HOOK is told; entry: the library function (None: the four parity conv2d calls of a transposed convolution); form: "plain"
# entry(a, stream), "ws" entry(a, workspace of nws floats, stream) or "lists" entry(a, LwgConvLists, stream); sliced / extra: as _hook_end takes
# them (sliced=False: per-image buffer descriptors, one launch at any batch size); panel: the builder ("_wwino", ... - looked up on the module
# at the launch) of the derived panel the entry reads, None = the fp32 GEMM panel.
ConvRoute = collections.namedtuple("ConvRoute", "kind entry form nws sliced extra panel")


@functools.lru_cache(maxsize=None)
def _route(kind, entry, panel=None, nws=0, sliced=True, extra=0, lists=False):
    """The record of a launch: split over K through a workspace (nws > 0: the ``_ws`` entry, ``extra`` finishing kernels), list-driven, or plain."""
    if nws:
        return ConvRoute(kind, entry + "_ws", "ws", nws, sliced, extra, panel)
    return ConvRoute(kind, entry, "lists" if lists else "plain", 0, sliced, 0, panel)


def conv2d_route(x0, spec, y, x1=None, epi=EPI_NONE, act=ACT_NONE, res=None, xn=None, mean=None, rstd=None,
                 out_hw=None, ycoff=0, splitk=False, q4=False, lists=None, a=None):
    """The ``ConvRoute`` of the ``conv2d`` call with these arguments (a: its filled argument block, where the caller has one) under the current
    modes and switches.  Raises conv2d's ValueErrors; asks the library's host planners (training launches, splitk=True, only) and launches nothing."""
    mode, xdt, ydt, f32, bf = CONV_PRECISION, x0.dtype, y.dtype, torch.float32, torch.bfloat16
    if q4 and (splitk or mode not in ("fp32", "winograd", "bf16_operands") or xdt != f32):
        raise ValueError("channel-quad-plane outputs: fp32 activations on the fp32 MFMA path, no split-K")
    w4 = mode == "winograd" and _wino4_use(spec, splitk)
    hr = xdt == bf and _hr_eligible(spec, x0, y, out_hw)
    if lists is not None and not (w4 and xdt == f32 and ydt == f32) and not (hr and ydt == bf and mode == "bf16" and x1 is None and spec.ntaps == 9):
        raise ValueError("lists: the F(4x4, 3x3) launches of the \"winograd\" mode and the 3 x 3 launches of the \"bf16\" mode only (conv2d_lists_apply)")
    if xdt == bf:
        # bf16 activation storage (BASELINE configs[3]): bf16 in, bf16 out, bf16 MFMA operands, fp32 accumulation
        if ydt != bf or spec.Cin % 64 != 0:
            raise ValueError("bf16 convolutions need bf16 outputs and Cin % 64 == 0")
        if mode == "bf16_winograd" and _bf16_wino_eligible(spec, x0, y, x1, epi, act, out_hw, ycoff):
            return _route("bf16_winograd", "lwg_conv2d_winograd_bf16", "_wwino16", sliced=False)
        if hr or _pw_eligible(spec, x0, y, x1, epi, out_hw):
            if lists is not None:                       # the sub-tile lists and the calibration frame: ONE kernel, never sliced
                return _route("bf16", "lwg_conv2d_nhwc_bf16_hr_list", "_w16hr", sliced=False, lists=True)
            return _route("bf16", "lwg_conv2d_nhwc_bf16_hr", "_w16hr")
        return _route("bf16", "lwg_conv2d_nhwc_bf16", "_w16v2")
    if ydt == bf:
        # the first layer of a network in bf16 mode: fp32 image-like input (Cin < 32), bf16 output
        if BF16_C8 and spec.Cin == 8 and spec.N == 64 and spec.ntaps <= 10 and x1 is None and epi == EPI_NONE and spec.omul == 1:
            return _route("direct", "lwg_conv2d_nhwc_c8_bf16", "_w16c8")
        return _route("direct", "lwg_conv2d_nhwc_f32")
    if splitk and a is None:                            # only the planners of the training launches read the argument block
        a = conv_args(x0, spec, y, x1, epi, act, res, xn, mean, rstd, out_hw, ycoff, q4)
    if mode == "winograd" and _wino_eligible(spec, x0, y, x1, epi, act, out_hw, q4, ycoff):
        # F(4x4) where _wino4_use admits the launch and, a training launch, _wino4_plan takes it; else F(2x2) by _wino_plan; else the direct kernels
        n4 = None if not w4 else _wino4_plan(a) if splitk else 0
        if n4 is not None and lists is not None:        # the granularity -> its entry point: a plain 4-tuple is block lists with their calibration frame
            name = "lwg_conv2d_winograd4_list_f32"
            if len(lists) == 2 and isinstance(lists[0], SkipLists) and lists[0].fine is not None and spade_skip_fine_apply(x0):
                q8 = lists[0].fine8 is not None and spade_skip_q8_apply(x0, spec.N // 64)
                name = "lwg_conv2d_winograd4_q8_f32" if q8 else "lwg_conv2d_winograd4_fine_f32"
            return _route("winograd4", name, "_wwino4", sliced=False, lists=True)
        if n4 is not None:                              # n4 > 0: a training launch (train_conv_tiles("4x4")) split over K
            return _route("winograd4", "lwg_conv2d_winograd4_f32", "_wwino4", nws=n4, sliced=False, extra=1)
        n = _wino_plan(a, spec, y, splitk)
        if n is not None:
            return _route("winograd", "lwg_conv2d_winograd_f32", "_wwino", nws=n, sliced=False, extra=1)
    # (``lists`` is not read below: a launch the guard let through on _wino4_use alone, but which _wino_eligible or the plans refuse, runs
    # without its lists, silently - as it always has)
    if mode == "bf16_operands" and _bf16op_use(spec, x0, y, x1, epi, act, q4, ycoff):       # the fp32 panel as it is: rounded in the kernel
        return _route("bf16op", "lwg_conv2d_nhwc_f32_bf16op", nws=_lib.lib().lwg_conv2d_bf16op_ws_floats(a) if splitk else 0, extra=1)
    if mode == "split" and spec.Cin % 32 == 0:
        return _route("split", "lwg_conv2d_nhwc_f32_split", "_w16x3")
    return _route("direct", "lwg_conv2d_nhwc_f32", nws=_lib.lib().lwg_conv2d_ws_floats(a) if splitk else 0)   # > 0: a small-M / large-K launch, split-K


def _conv_lists(entry, lists, x0, spec, y, epi):
    """The LwgConvLists of a list-driven entry point out of conv2d's ``lists``: the 4-tuple, or the triple of the entry's granularity + cal."""
    hr = entry == "lwg_conv2d_nhwc_bf16_hr_list"        # its 8 x 16 pixel block is one 16 x 8 sub-tile
    if len(lists) == 2 and isinstance(lists[0], SkipLists):     # entry -> the SkipLists triple it reads (None: the block lists themselves)
        attr = {"lwg_conv2d_winograd4_list_f32": None, "lwg_conv2d_winograd4_fine_f32": "fine", "lwg_conv2d_winograd4_q8_f32": "fine8", "lwg_conv2d_nhwc_bf16_hr_list": "fine"}[entry]
        lists = tuple(lists[0] if attr is None else getattr(lists[0], attr)) + (lists[1],)
    if hr:
        nsub = x0.shape[0] * ((x0.shape[1] + 7) // 8) * ((x0.shape[2] + 15) // 16)
        if min(lists[0].numel(), lists[1].numel()) < nsub or lists[2].numel() < 2 or \
                lists[3].numel() != x0.shape[1] * x0.shape[2] * (spec.N if epi == EPI_SPADE else y.shape[3]):
            raise ValueError("lists: the sub-tile lists of this frame batch and ONE calibration frame at its feature size")
    return _lib.LwgConvLists(*[_ptr(t, torch.int32) for t in lists[:3]], _ptr(lists[3], torch.bfloat16 if hr and epi != EPI_SPADE else torch.float32))


def conv2d(x0, spec, y, x1=None, epi=EPI_NONE, act=ACT_NONE, res=None, xn=None, mean=None, rstd=None,
           out_hw=None, ycoff=0, splitk=False, q4=False, lists=None):
    """y <- conv(cat[x0, x1]) per ``spec``; x*: (B,H,W,C) NHWC; y: (B,YH,YW,YC) NHWC (written in place).
    lists: (heavy, light, counts, cal) - ``spade_skip_lists`` and the calibration frame - for a launch ``conv2d_lists_apply`` accepted; or
    (SkipLists, cal): the sub-tile lists where ``spade_skip_fine_apply`` says so, else the block lists.  bf16 ("bf16" mode): always the sub-tile
    triple (``SkipLists.fine``, or given as the 4-tuple); cal = the bf16 output frame of the all-background input, for EPI_SPADE the fp32
    accumulator frame of ``conv2d_acc_frame``.
    splitk: let the library split small-M / large-K launches over K (the training step's one-sample launches).  Off on the
    synthesis path: a frame's result must not depend on how many frames share its launch (batch invariance is a parity check).
    q4: y is (B, YC/4, YH, YW, 4), channel-quad planes (the fp32 MFMA path only: what ``head_compose(..., q4=True)`` reads)."""
    a = conv_args(x0, spec, y, x1, epi, act, res, xn, mean, rstd, out_hw, ycoff, q4)
    # the guards are the route's (it raises before it asks or decides anything): a refused call has announced nothing to the hook
    kind, entry, form, nws, sliced, extra, panel = conv2d_route(x0, spec, y, x1, epi, act, res, xn, mean, rstd, out_hw, ycoff, splitk, q4, lists, a)
    if CONV_HOOK is not None:
        CONV_HOOK(True, a.M, spec, epi, None)
    if panel == "_w16hr":
        _hr_args(a, spec, epi)
    elif panel == "_wwino16":
        w, bias = _wwino16(spec, epi == EPI_SPADE)
        a.w, a.bias = _ptr(w, torch.bfloat16), _ptr(bias)
        a.dy[:9], a.dx[:9] = zip(*_WINO_TAPS)                         # the panel's tap order
    elif panel is not None:
        a.w = _ptr(globals()[panel](spec), torch.float32 if panel in ("_wwino", "_wwino4") else torch.bfloat16)    # (_w16v2, _w16c8, _w16x3: bf16)
    if form == "ws":
        ws = torch.empty(nws, device=x0.device, dtype=torch.float32)
        rc = getattr(_lib.lib(), entry)(a, _ptr(ws), _stream())
    elif form == "lists":
        ld = _conv_lists(entry, lists, x0, spec, y, epi)
        rc = getattr(_lib.lib(), entry)(a, ctypes.byref(ld), _stream())
    else:
        rc = getattr(_lib.lib(), entry)(a, _stream())
    _lib.check(rc, entry)
    if CONV_HOOK is not None:
        _hook_end(a, spec, epi, kind, sliced, extra)
    return y


WINO_UP4 = True         # lab switch: in the "winograd" mode the fp32 transposed convolutions of the synthesis path run lwg_conv_transpose4_winograd_f32
F32_UP4 = True          # lab switch: fp32 transposed convolutions through lwg_conv_transpose4_nhwc_f32 (False: four conv2d calls)
BF16_UP4 = True         # lab switch: the four parity launches of a bf16 transposed convolution fused into one (Cin <= 128)


def _parity_specs_ok(specs):
    """The four parity specs of ONE ConvTranspose2d(4, 2, 1) in order (packing.pack_conv_transpose): parity p's taps are parity 0's shifted by p."""
    s0 = specs[0]
    return (len(specs) == 4 and all(s.ntaps == 4 and s.omul == 2 and s.stride == 1 and (s.ooy, s.oox) == (i >> 1, i & 1) and s.N == s0.N and s.Cin == s0.Cin
                                    and [(dy - (i >> 1), dx - (i & 1)) for dy, dx in zip(s.dy, s.dx)] == list(zip(s0.dy, s0.dx)) for i, s in enumerate(specs)))


def _up4_f32_ok(x, specs, y):
    """The fp32 transposed convolutions lwg_conv_transpose4_nhwc_f32 can take as ONE grid - where lwg_conv_transpose4_is_one_grid then agrees."""
    return (F32_UP4 and x.is_cuda and x.dtype == torch.float32 and y.dtype == torch.float32 and specs[0].Cin % 32 == 0 and _parity_specs_ok(specs))


def _wwino_t(specs):
    """The transformed-weight panel of lwg_conv_transpose4_winograd_f32 from the four parity GEMM panels, built once per layer (a weight transform at
    load time, like the packing itself): Upk[4][Cin/8][4][2][9 N] - per (parity 2 py + px, s, kk, kh) [N][4] products 0-3, [N][4] products 4-7, [N] product 8 -, product 3 xi + nu of column n = sgn (G g G^T)[xi][nu] for input
    channel 8 s + 2 kk + kh - g the parity's 2 x 2 sub-kernel in input-offset order, G = [[1,0],[1,1],[0,1]], formed in fp64 and rounded once; the
    sign (-1 where a parity-1 row / column takes the form the parity-0 one already holds negated) is documented in include/lwg_hip.h."""
    def build():
        Cin, N = specs[0].Cin, specs[0].N
        G = torch.tensor([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], dtype=torch.float64, device=specs[0].w.device)
        parts = []
        for par, g in enumerate(_parity_subkernels(specs)):
            u = torch.einsum("ar,rqcn,bq->abcn", G, g, G)                          # (3, 3, Cin, N)
            if par >> 1:
                u[0] = -u[0]
            if par & 1:
                u[:, 0] = -u[:, 0]
            parts.append(u.reshape(9, Cin, N))
        U9 = torch.stack(parts).float()                                              # (4, 9, Cin, N)
        # per (parity, input channel): 9 N floats - [N][4] products 0-3, [N][4] products 4-7, [N] product 8 (every load of the kernel reads contiguous memory)
        U = torch.cat([U9[:, 0:4].permute(0, 2, 3, 1).reshape(4, Cin, 4 * N), U9[:, 4:8].permute(0, 2, 3, 1).reshape(4, Cin, 4 * N), U9[:, 8]], dim=2)
        return U.view(4, Cin // 8, 4, 2, 9 * N).contiguous()                         # c = 8 s + 2 kk + kh
    return _derived(specs, "wwino_t", build)


def _parity_subkernels(specs):
    """The four parity GEMM panels of a ConvTranspose2d(4, 2, 1) as fp64 2 x 2 sub-kernels in input-offset order: per parity 2 py + px a tensor
    g (2, 2, Cin, N), g[r][q] the weight that multiplies x[i + py - 1 + r][j + px - 1 + q]."""
    Cin, N = specs[0].Cin, specs[0].N
    out = []
    for par, sp in enumerate(specs):
        py, px = par >> 1, par & 1
        W = sp.w.double().permute(0, 2, 1).reshape(4 * Cin, N)                  # rows k = ((c / 32) 4 + tap) 32 + c % 32
        W = W.view(Cin // 32, 4, 32, N).permute(1, 0, 2, 3).reshape(4, Cin, N)  # [tap][c][n]
        g = torch.zeros(2, 2, Cin, N, dtype=torch.float64, device=W.device)
        for t, (dy, dx) in enumerate(zip(sp.dy, sp.dx)):
            g[dy - (py - 1), dx - (px - 1)] = W[t]
        out.append(g)
    return out


# F(4, 2) along the columns of the F(2x4, 2x2) kernel (csrc/convt_winograd24.hip): the points {0, 1, -1, 1/2, inf}, the scale factors of its data
# transform moved here so that the kernel's B^T has the entries 0, +-1, +-2, -3 only (tools/convt_tile_study.py)
_G_X24 = ((1.0, 0.0), (0.5, 0.5), (-1.0 / 6.0, 1.0 / 6.0), (-8.0 / 3.0, -4.0 / 3.0), (0.0, 0.5))


def _wwino_t24(specs):
    """The transformed-weight panel of lwg_conv_transpose4_winograd24_f32 from the four parity GEMM panels, built once per layer:
    Upk[4][Cin/8][4][2][15 N] - per (parity 2 py + px, s, kk, kh) [N][4] products 0-3, [N][4] products 4-7, [N] product 8, [N][4] products 9-12,
    [N] product 13, [N] product 14 (every load of the kernel reads contiguous memory).  Product 3 xi + nu (nu < 3) / 9 + 2 xi + nu - 3 (nu >= 3) of column n =
    sgn (G_y g G_x^T)[xi][nu] for input channel 8 s + 2 kk + kh, g the parity's 2 x 2 sub-kernel in input-offset order, G_y = [[1,0],[1,1],[0,1]],
    G_x = _G_X24, sgn = -1 for the parity-1 row form the parity-0 one already holds negated (xi = 0, py = 1); formed in fp64 and rounded once."""
    def build():
        Cin, N = specs[0].Cin, specs[0].N
        Gy = torch.tensor([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], dtype=torch.float64, device=specs[0].w.device)
        Gx = torch.tensor(_G_X24, dtype=torch.float64, device=specs[0].w.device)
        parts = []
        for par, g in enumerate(_parity_subkernels(specs)):
            u = torch.einsum("ar,rqcn,bq->abcn", Gy, g, Gx)                        # (3, 5, Cin, N)
            if par >> 1:
                u[0] = -u[0]
            parts.append(torch.cat([u[:, :3].reshape(9, Cin, N), u[:, 3:].reshape(6, Cin, N)]))
        U15 = torch.stack(parts).float()                                             # (4, 15, Cin, N)
        quad = lambda lo, hi: U15[:, lo:hi].permute(0, 2, 3, 1).reshape(4, Cin, (hi - lo) * N)     # noqa: E731
        U = torch.cat([quad(0, 4), quad(4, 8), U15[:, 8], quad(9, 13), U15[:, 13], U15[:, 14]], dim=2)
        return U.view(4, Cin // 8, 4, 2, 15 * N).contiguous()                        # c = 8 s + 2 kk + kh
    return _derived(specs, "wwino_t24", build)


WINO_UP4_24 = True          # lab switch: the synthesis path's eligible transposed convolutions run the F(2x4, 2x2) kernel (False: F(2x2, 2x2))
# ... for images of at least this many input pixels; smaller launches keep F(2x2, 2x2).  NOT a measured crossover: the bound is set so that the
# shapes tests/gpu_checks.py::check_winograd_up4 pins to lwg_conv_transpose4_winograd_f32's bits (<= 48 x 64 input pixels) keep that kernel, while
# the 512 x 512 decoder's three layers (64^2, 128^2, 256^2 inputs, where both kernels were timed) take the new one.  The 256 x 256 pipeline's
# first layer (32^2) stays on F(2x2, 2x2) untimed against F(2x4, 2x2); tests/test_gpu_convt_winograd24.py runs the new kernel on the small shapes.
WINO_UP4_24_MIN_HW = 64 * 64


def _up4_24(x):
    """Whether a "winograd"-mode transposed convolution of x (B, H, W, Cin) runs lwg_conv_transpose4_winograd24_f32."""
    return WINO_UP4_24 and x.shape[1] * x.shape[2] >= WINO_UP4_24_MIN_HW


class _FusedTransposeSpec(object):
    """What a launch-accounting hook (bench.ConvTimer) sees for the fused transposed convolution: per INPUT pixel 16 taps and 4 N
    outputs; flops = 2 M algo_kn, bytes = M Cin in + 4 M N out + the four panels."""

    def __init__(self, s0, panel):
        self.N, self.Cin, self.ntaps, self.stride, self.omul = 4 * s0.N, s0.Cin, 16, 1, 2
        self.algo_kn, self.w = 4 * s0.algo_kn, panel


def _fused_transpose_launch(a, s0, panel, entry, kind, sliced=True, extra=(), kernels=None):
    """One launch = a whole transposed convolution (16 taps, 4 N output values per input pixel): ``entry(a, *extra, stream)`` of the library on
    ``panel``, bracketed by the accounting hook with ONE pseudo-spec for the layer.  kernels: the closing hook call's launch count where the caller
    knows it (else the C rule of ``_hook_end``; sliced=False: one launch at any batch size)."""
    a.w = _ptr(panel, panel.dtype)
    if CONV_HOOK is not None:
        whole = _FusedTransposeSpec(s0, panel)
        CONV_HOOK(True, a.M, whole, EPI_NONE, None)
    _lib.check(getattr(_lib.lib(), entry)(a, *extra, _stream()), entry)
    if CONV_HOOK is not None:
        if kernels is None:
            _hook_end(a, whole, EPI_NONE, kind, sliced)
        else:
            CONV_HOOK(False, a.M, whole, EPI_NONE, {"kernels": kernels, "kind": kind})


def _w16up(specs):
    """The panel of the fused bf16 transposed convolutions (lwg_conv_transpose4_nhwc_bf16, lwg_up4_head_compose_bf16): the four parity specs'
    register-streamed panels (_w16hr) stacked, [parity][Cin/64 * 4][4][N][16] bf16."""
    return _derived(specs, "w16up", lambda: torch.stack([_w16hr(s, False)[0] for s in specs]).contiguous())


def _w32up(specs):
    """The panel of lwg_conv_transpose4_nhwc_f32: the four parity specs' fp32 GEMM panels, flattened and stacked."""
    return _derived(specs, "w32up", lambda: torch.stack([s.w.reshape(-1) for s in specs]).contiguous())


def _up4_route(x, specs, y, act, splitk, out_hw, q4):
    """(``ConvRoute``, the filled argument block of its ONE launch - None with the four parity calls) of a ``conv_transpose2d`` call."""
    s0, mode, f32 = specs[0], CONV_PRECISION, x.dtype == torch.float32 and y.dtype == torch.float32
    if (BF16_UP4 and BF16_HR and x.dtype == torch.bfloat16 and y.dtype == torch.bfloat16 and len(specs) == 4 and s0.Cin in (64, 128)
            and s0.N % 64 == 0 and all(s.ntaps == 4 and s.omul == 2 and (s.ooy, s.oox) == (i >> 1, i & 1) for i, s in enumerate(specs))):
        return _route("up4", "lwg_conv_transpose4_nhwc_bf16", "_w16up"), conv_args(x, s0, y, act=act)
    if WINO_UP4 and mode == "winograd" and not splitk and out_hw is None and x.is_cuda and f32 and s0.Cin % 32 == 0 and s0.N % 32 == 0 and _parity_specs_ok(specs):
        # the synthesis path in the "winograd" mode: ONE fused Winograd launch (per-image work in a fixed order: a frame does not depend on its batch),
        # F(2x4, 2x2) for images of >= WINO_UP4_24_MIN_HW input pixels.  Training callers (splitk=True) keep the direct forms.
        name, panel = ("lwg_conv_transpose4_winograd24_f32", "_wwino_t24") if _up4_24(x) else ("lwg_conv_transpose4_winograd_f32", "_wwino_t")
        return _route("winograd_up4", name, panel, sliced=False), conv_args(x, s0, y, act=act, q4=q4)
    if _up4_f32_ok(x, specs, y) and (mode in ("fp32", "winograd") or (mode == "bf16_operands" and not _bf16op_use_parity4(specs, x, y, act, splitk, out_hw, q4))):
        # fp32, small launch (a parity is a workgroup per CU or less): ONE grid of four times the workgroups; large launches stay four conv2d calls
        # (the library would issue the same four launches) - the same values bit for bit (same tiles, same K order).  "bf16_operands": a layer
        # the mode refuses (q4 planes, a one-grid group whose parity launches would run split-K) keeps exactly this "fp32" form
        a = conv_args(x, s0, y, act=act, q4=q4)
        if _lib.lib().lwg_conv_transpose4_is_one_grid(a):
            return _route("up4", "lwg_conv_transpose4_nhwc_f32", "_w32up"), a
    return _route("parity4", None), None


def conv_transpose2d_route(x, specs, y, act=ACT_NONE, splitk=False, out_hw=None, q4=False):
    """The ``ConvRoute`` of the ``conv_transpose2d`` call with these arguments: the fused bf16 launch, the F(2x2, 2x2) or F(2x4, 2x2) Winograd launch,
    the one-grid fp32 launch (panel: the builder that takes the four specs), or entry None = four parity ``conv2d`` calls (each with its own route)."""
    return _up4_route(x, specs, y, act, splitk, out_hw, q4)[0]


def conv_transpose2d(x, specs, y, act=ACT_NONE, splitk=False, out_hw=None, q4=False):
    """y (B,2H,2W,N) <- ConvTranspose2d(4, 2, 1) of x (B,H,W,Cin) given its four parity specs (packing.pack_conv_transpose).
    bf16 activations with Cin <= 128: ONE launch (lwg_conv_transpose4_nhwc_bf16: the input block is staged once for the four
    parities); fp32 in the "winograd" mode on the synthesis path (splitk=False): ONE fused F(2x2, 2x2) Winograd launch
    (lwg_conv_transpose4_winograd_f32: 36 products per 4 x 4 input patch instead of 64; fp32-grade, not the direct forms' bits);
    otherwise the one-grid form for small fp32 launches or the four parity launches of ``conv2d``.  ``splitk`` / ``out_hw`` are handed to those four launches (the
    training callers' plan: the one-grid form and the four-launch fall-back then differ only in launch count); ``out_hw`` is a
    callable spec -> (OH, OW) or None.  q4 (fp32 only): y is (B, N/4, 2H, 2W, 4), channel-quad planes (see ``conv2d``)."""
    r, a = _up4_route(x, specs, y, act, splitk, out_hw, q4)
    if r.entry is not None:
        _fused_transpose_launch(a, specs[0], globals()[r.panel](specs), r.entry, r.kind, r.sliced)
        return y
    for s in specs:
        conv2d(x, s, y, act=act, splitk=splitk, out_hw=None if out_hw is None else out_hw(s), q4=q4)
    return y


def instnorm_stats(x, mean, rstd, ws, eps=1e-5, nsplit=None):
    B, H, W, C = x.shape
    HW = H * W
    if nsplit is None:
        nsplit = max(1, min(64, HW // 64))
    assert ws.numel() >= B * C * nsplit * 3
    if x.dtype == torch.bfloat16:
        _lib.check(_lib.lib().lwg_instnorm_stats_nhwc_bf16(_ptr(x, torch.bfloat16), B, HW, C, eps, _ptr(mean), _ptr(rstd), _ptr(ws), nsplit,
                                                            _stream()), "lwg_instnorm_stats_nhwc_bf16")
        return
    _lib.check(_lib.lib().lwg_instnorm_stats_nhwc_f32(_ptr(x), B, HW, C, eps, _ptr(mean), _ptr(rstd), _ptr(ws), nsplit,
                                                       _stream()), "lwg_instnorm_stats_nhwc_f32")


def instnorm_apply(x, mean, rstd, y, act=ACT_NONE, res=None):
    B, H, W, C = x.shape
    _lib.check(_lib.lib().lwg_instnorm_apply_nhwc_f32(_ptr(x), _ptr(mean), _ptr(rstd), _ptr(res), _ptr(y), B, H * W, C, act,
                                                       _stream()), "lwg_instnorm_apply_nhwc_f32")
    return y


def flow_resize(T, h, w):
    """(B,ns,S,S,2) flows -> (B,ns,h,w,2): F.interpolate(bilinear, align_corners=True) of LWB.resize_trans as its own pass."""
    B, ns, S = T.shape[0], T.shape[1], T.shape[2]
    T = T.contiguous()
    out = torch.empty(B, ns, h, w, 2, device=T.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_flow_resize_f32(_ptr(T), B * ns, S, h, w, _ptr(out), _stream()), "lwg_flow_resize_f32")
    return out


def lwb_attention(q, Ks, Vs, bk, bv, T, out, src_batched=False):
    B, h, w, C = q.shape
    ns = T.shape[1]
    S = T.shape[2]
    assert T.shape[0] == B and Ks.shape[0] == (B * ns if src_batched else ns) and tuple(Ks.shape[1:]) == (h, w, C)
    if q.dtype == torch.bfloat16:
        bf = torch.bfloat16
        _lib.check(_lib.lib().lwg_lwb_attention_bf16(_ptr(q, bf), _ptr(Ks, bf), _ptr(Vs, bf), _ptr(bk), _ptr(bv), _ptr(T), _ptr(out, bf), B, ns, h,
                                                      w, C, S, 1 if src_batched else 0, _stream()), "lwg_lwb_attention_bf16")
        return out
    _lib.check(_lib.lib().lwg_lwb_attention_f32(_ptr(q), _ptr(Ks), _ptr(Vs), _ptr(bk), _ptr(bv), _ptr(T), _ptr(out), B, ns, h,
                                                 w, C, S, 1 if src_batched else 0, _stream()), "lwg_lwb_attention_f32")
    return out


def attn_records(h, w, C, dtype=torch.float32):
    """Records per image the statistics form of ``lwb_attention_x`` leaves: one per workgroup = per 8 x 8-pixel tile, or per part of a
    tile on small feature maps (a function of (h, w, C, storage type) only - never of the batch)."""
    n = _lib.lib().lwg_lwb_attention_x_records(int(h), int(w), int(C), 2 if dtype == torch.bfloat16 else 4)
    if n <= 0:
        raise ValueError(f"lwb_attention_x: unsupported (h, w, C, dtype) = {(h, w, C, dtype)}")
    return n


def lwb_attention_x(x, Kq, kappa, Vs, bv, T, out, stats=None, src_batched=False):
    """The attention-form Liquid Warping Block with the query projection folded into the source side (csrc/lwb_attn_x.hip):
    logit_s = (warp_s(Kq) . x + warp_s(kappa)) / sqrt(C), out = sum_s softmax_s(logit) warp_s(Vs) + bv.
    x (B,h,w,C) fp32 | bf16; Kq, Vs (nsrc,h,w,C) in x's dtype; kappa (nsrc,h,w) fp32; T (B,ns,h,w,2) flows ALREADY at (h,w).
    stats: None or a fp32 buffer of >= B * attn_records(h, w, C, dtype) * C * 3 floats receiving the partial InstanceNorm records of x."""
    B, h, w, C = x.shape
    ns = T.shape[1]
    nsrc = B * ns if src_batched else ns
    assert tuple(T.shape) == (B, ns, h, w, 2), (tuple(T.shape), (B, ns, h, w, 2))
    assert tuple(Kq.shape) == (nsrc, h, w, C) and tuple(Vs.shape) == (nsrc, h, w, C) and tuple(kappa.shape) == (nsrc, h, w)
    assert Kq.dtype == x.dtype and Vs.dtype == x.dtype and out.dtype == x.dtype and kappa.dtype == torch.float32
    assert stats is None or stats.numel() >= B * attn_records(h, w, C, x.dtype) * C * 3
    if x.dtype == torch.bfloat16:
        bf = torch.bfloat16
        _lib.check(_lib.lib().lwg_lwb_attention_x_bf16(_ptr(x, bf), _ptr(Kq, bf), _ptr(kappa), _ptr(Vs, bf), _ptr(bv), _ptr(T), _ptr(out, bf),
                                                        _ptr(stats), B, ns, h, w, C, 1 if src_batched else 0, _stream()), "lwg_lwb_attention_x_bf16")
        return out
    _lib.check(_lib.lib().lwg_lwb_attention_x_f32(_ptr(x), _ptr(Kq), _ptr(kappa), _ptr(Vs), _ptr(bv), _ptr(T), _ptr(out), _ptr(stats), B, ns, h, w,
                                                   C, 1 if src_batched else 0, _stream()), "lwg_lwb_attention_x_f32")
    return out


def instnorm_finalize_ws(B, C, nrec):
    """Floats of the record buffer ``instnorm_finalize`` takes: the (B, nrec, C, 3) records + scratch for the segment partials of long lists."""
    return int(_lib.lib().lwg_instnorm_finalize_ws_floats(int(B), int(C), int(nrec)))


def instnorm_finalize(ws, B, C, nrec, mean, rstd, eps=1e-5):
    """(B, nrec, C, 3) records (count, mean, M2) -> mean, rstd (B, C) of nn.InstanceNorm2d (biased variance).  ws: >= instnorm_finalize_ws floats."""
    assert ws.numel() >= instnorm_finalize_ws(B, C, nrec)
    _lib.check(_lib.lib().lwg_instnorm_finalize_f32(_ptr(ws), B, C, nrec, float(eps), _ptr(mean), _ptr(rstd), _stream()), "lwg_instnorm_finalize_f32")


def lwb_fuse(tsf_x, src_x, T, out, gate=None, scale_w=1.0, scale_o=1.0, src_batched=False):
    """out = (tsf_x + gate * scale_w * sum_s warp_s(src_x)) * scale_o - AddLWB / AvgLWB / SoftGateLWB fusion.
    tsf_x (B,h,w,C) fp32 | bf16; src_x, gate, out in tsf_x's dtype; T (B,ns,S,S,2) fp32 flows."""
    B, h, w, C = tsf_x.shape
    ns, S = T.shape[1], T.shape[2]
    assert T.shape[0] == B and src_x.shape[0] == (B * ns if src_batched else ns) and tuple(src_x.shape[1:]) == (h, w, C)
    assert src_x.dtype == tsf_x.dtype and out.dtype == tsf_x.dtype and (gate is None or gate.dtype == tsf_x.dtype)
    assert T.dtype == torch.float32
    if tsf_x.dtype == torch.bfloat16:
        bf = torch.bfloat16
        _lib.check(_lib.lib().lwg_lwb_fuse_bf16(_ptr(tsf_x, bf), _ptr(src_x, bf), _ptr(gate, bf), _ptr(T), _ptr(out, bf), B, ns, h, w, C, S,
                                                1 if src_batched else 0, float(scale_w), float(scale_o), _stream()), "lwg_lwb_fuse_bf16")
        return out
    _lib.check(_lib.lib().lwg_lwb_fuse_f32(_ptr(tsf_x), _ptr(src_x), _ptr(gate), _ptr(T), _ptr(out), B, ns, h, w, C, S,
                                           1 if src_batched else 0, float(scale_w), float(scale_o), _stream()), "lwg_lwb_fuse_f32")
    return out


def lwb_fuse_bwd(src_x, gate, T, dout, src_batched=False, scale_w=1.0, scale_o=1.0):
    """Gradients of ``lwb_fuse`` w.r.t. tsf_x, src_x and gate (the flows are constants) -> (d_tsf, d_src, d_gate | None).
    d_src is summed with fp32 atomics (bilinear scatter): its last bits depend on arrival order."""
    B, h, w, C = dout.shape
    ns, S = T.shape[1], T.shape[2]
    assert T.shape[0] == B and src_x.shape[0] == (B * ns if src_batched else ns) and tuple(src_x.shape[1:]) == (h, w, C)
    assert gate is None or gate.shape == dout.shape
    dout = dout.contiguous()
    d_tsf = torch.empty_like(dout)
    d_src = torch.zeros_like(src_x)
    d_gate = None if gate is None else torch.empty_like(dout)
    _lib.check(_lib.lib().lwg_lwb_fuse_bwd_f32(_ptr(src_x), _ptr(gate), _ptr(T), _ptr(dout), _ptr(d_tsf), _ptr(d_src), _ptr(d_gate), B, ns, h, w, C,
                                               S, 1 if src_batched else 0, float(scale_w), float(scale_o), _stream()), "lwg_lwb_fuse_bwd_f32")
    return d_tsf, d_src, d_gate


def lwb_attention_bwd(q, Ks, Vs, bk, bv, T, dout, src_batched=False):
    """Gradients of ``lwb_attention`` w.r.t. q, Ks, Vs (the flows are constants).  dbv = colsum(dout), dbk = 0."""
    B, h, w, C = q.shape
    ns, S = T.shape[1], T.shape[2]
    dout = dout.contiguous()
    dq = torch.empty_like(q)
    dKs = torch.zeros_like(Ks)
    dVs = torch.zeros_like(Vs)
    _lib.check(_lib.lib().lwg_lwb_attention_bwd_f32(_ptr(q), _ptr(Ks), _ptr(Vs), _ptr(bk), _ptr(bv), _ptr(T), _ptr(dout), _ptr(dq),
                                                     _ptr(dKs), _ptr(dVs), B, ns, h, w, C, S, 1 if src_batched else 0, _stream()),
               "lwg_lwb_attention_bwd_f32")
    return dq, dKs, dVs


def lwb_attention_kv(q, kv, bk, bv, T, out, src_batched=False):
    """``lwb_attention`` with K | V as one tensor kv (nsrc,h,w,2C) (the stacked fk | fv projection of the training step)."""
    B, h, w, C = q.shape
    ns, S = T.shape[1], T.shape[2]
    assert T.shape[0] == B and kv.shape[0] == (B * ns if src_batched else ns) and tuple(kv.shape[1:]) == (h, w, 2 * C)
    _lib.check(_lib.lib().lwg_lwb_attention_kv_f32(_ptr(q), _ptr(kv), _ptr(bk), _ptr(bv), _ptr(T), _ptr(out), B, ns, h, w, C, S,
                                                    1 if src_batched else 0, _stream()), "lwg_lwb_attention_kv_f32")
    return out


def lwb_attention_kv_bwd(q, kv, bk, bv, T, dout, src_batched=False):
    """Gradients of ``lwb_attention_kv`` w.r.t. q and kv -> (dq, dkv)."""
    B, h, w, C = q.shape
    ns, S = T.shape[1], T.shape[2]
    dout = dout.contiguous()
    dq = torch.empty_like(q)
    dkv = torch.zeros_like(kv)
    _lib.check(_lib.lib().lwg_lwb_attention_kv_bwd_f32(_ptr(q), _ptr(kv), _ptr(bk), _ptr(bv), _ptr(T), _ptr(dout), _ptr(dq), _ptr(dkv),
                                                        B, ns, h, w, C, S, 1 if src_batched else 0, _stream()), "lwg_lwb_attention_kv_bwd_f32")
    return dq, dkv


def project_faces(verts, cam, faces, want_faces_v=True, want_f2pts=True):
    B, nv, _ = verts.shape
    nf = faces.shape[0]
    fv = torch.empty(B, nf, 3, 3, device=verts.device, dtype=torch.float32) if want_faces_v else None
    f2 = torch.empty(B, nf, 3, 2, device=verts.device, dtype=torch.float32) if want_f2pts else None
    cam = cam.contiguous()
    _lib.check(_lib.lib().lwg_project_faces_f32(_ptr(verts), _ptr(cam), _ptr(faces, torch.int32), B, nv, nf, EYE_DIST, _ptr(fv),
                                                 _ptr(f2), _stream()), "lwg_project_faces_f32")
    return fv, f2


def rasterize_fim_wim(faces_v, image_size, near=0.1, far=100.0):
    B, nf = faces_v.shape[0], faces_v.shape[1]
    S = int(image_size)
    dev = faces_v.device
    fim = torch.empty(B, S, S, device=dev, dtype=torch.int32)
    wim = torch.empty(B, S, S, 3, device=dev, dtype=torch.float32)
    ws = torch.empty(_lib.lib().lwg_rasterize_ws_bytes(B, nf, S), device=dev, dtype=torch.uint8)
    _lib.check(_lib.lib().lwg_rasterize_fim_wim_f32(_ptr(faces_v), B, nf, S, near, far, _ptr(fim, torch.int32), _ptr(wim),
                                                     ws.data_ptr(), _stream()), "lwg_rasterize_fim_wim_f32")
    return fim, wim


def texture_sample(fim, wim, faces_v, textures, eps=1e-3, background_color=(0.0, 0.0, 0.0)):
    """rgb (B,S,S,3) from the index / weight maps, faces_v (B,nf,3,3) and per-face textures (B|1,nf,T,T,T,3)."""
    B, S = fim.shape[0], fim.shape[1]
    nf, T = faces_v.shape[1], textures.shape[2]
    assert textures.shape[0] in (1, B) and textures.shape[1] == nf
    rgb = torch.empty(B, S, S, 3, device=fim.device, dtype=torch.float32)
    bg = (ctypes.c_float * 3)(*[float(c) for c in background_color])
    _lib.check(_lib.lib().lwg_texture_sample_f32(_ptr(fim, torch.int32), _ptr(wim), _ptr(faces_v.contiguous()), _ptr(textures.contiguous()), B, nf,
                                                 S, T, 1 if textures.shape[0] == B and B > 1 else (1 if textures.shape[0] == B else 0),
                                                 float(eps), bg, _ptr(rgb), _stream()), "lwg_texture_sample_f32")
    return rgb


def flow_compose(fim, wim, map_fn, f_uvs2img, uv_img4, src_f2pts, want_cond=False, want_tuv=False):
    B, S, _ = fim.shape
    nf = f_uvs2img.shape[0]
    ns = src_f2pts.shape[0]
    dev = fim.device
    tsf = torch.empty(B, S, S, 8, device=dev, dtype=torch.float32)
    Tst = torch.empty(B, ns, S, S, 2, device=dev, dtype=torch.float32)
    cond = torch.empty(B, 3, S, S, device=dev, dtype=torch.float32) if want_cond else None
    tuv = torch.empty(B, S, S, 2, device=dev, dtype=torch.float32) if want_tuv else None
    Hu, Wu = uv_img4.shape[0], uv_img4.shape[1]
    _lib.check(_lib.lib().lwg_flow_compose_f32(_ptr(fim, torch.int32), _ptr(wim), B, S, _ptr(map_fn), nf, _ptr(f_uvs2img),
                                                _ptr(uv_img4), Hu, Wu, _ptr(src_f2pts), ns, _ptr(tsf), _ptr(Tst), _ptr(cond),
                                                _ptr(tuv), _stream()), "lwg_flow_compose_f32")
    return tsf, Tst, cond, tuv


def bc_transform(f2pts, fim, wim):
    B, S, _ = fim.shape
    nf = f2pts.shape[1]
    T = torch.empty(B, S, S, 2, device=fim.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_bc_transform_f32(_ptr(f2pts), _ptr(fim, torch.int32), _ptr(wim), B, S, nf, _ptr(T), _stream()),
               "lwg_bc_transform_f32")
    return T


def encode_fim(fim, map_fn):
    B, S, _ = fim.shape
    D = map_fn.shape[1]
    out = torch.empty(B, D, S, S, device=fim.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_encode_fim_f32(_ptr(fim, torch.int32), _ptr(map_fn), B, S, map_fn.shape[0] - 1, D, _ptr(out),
                                              _stream()), "lwg_encode_fim_f32")
    return out


def head_compose(x, wpk, bg, want_pred=True, want_mask=True, want_img=False, q4=False):
    """q4: x is (B, C/4, S, S, 4) fp32, channel-quad planes (a convolution launched with q4=True wrote it)."""
    if q4:
        B, Cq, S, _, four = x.shape
        C = 4 * Cq
        assert four == 4 and x.dtype == torch.float32 and x.is_contiguous()
    else:
        B, S, _, C = x.shape
    dev = x.device
    pred = torch.empty(B, 3, S, S, device=dev, dtype=torch.float32) if want_pred else None
    mask = torch.empty(B, 1, S, S, device=dev, dtype=torch.float32) if want_mask else None
    img = torch.empty(B, 3, S, S, device=dev, dtype=torch.float32) if want_img else None
    bstride = 0
    if bg is not None and bg.shape[0] != 1:
        assert bg.shape[0] == B
        bstride = 3 * S * S
    if x.dtype == torch.bfloat16:                    # wpk: packing.pack_head_bf16
        _lib.check(_lib.lib().lwg_head_compose_bf16(_ptr(x, torch.bfloat16), _ptr(wpk, torch.bfloat16), _ptr(bg), bstride, B, S, C, _ptr(pred),
                                                     _ptr(mask), _ptr(img), _stream()), "lwg_head_compose_bf16")
        return pred, mask, img
    if q4:
        _lib.check(_lib.lib().lwg_head_compose_q4_f32(_ptr(x), _ptr(wpk), _ptr(bg), bstride, B, S, C, _ptr(pred), _ptr(mask), _ptr(img),
                                                       _stream()), "lwg_head_compose_q4_f32")
        return pred, mask, img
    _lib.check(_lib.lib().lwg_head_compose_f32(_ptr(x), _ptr(wpk), _ptr(bg), bstride, B, S, C, _ptr(pred), _ptr(mask), _ptr(img),
                                                _stream()), "lwg_head_compose_f32")
    return pred, mask, img


BF16_UP4_HEAD = True    # lab switch: False = the bf16 engine's last up-sampling layer and its output head as two launches (rounds 2-5)


def up4_head_eligible(x, specs, act):
    """The fused last stage of the bf16 engine (lwg_up4_head_compose_bf16): ConvTranspose2d(128 -> 64, 4, 2, 1) + ReLU on a bf16 input."""
    s0 = specs[0]
    return (BF16_UP4_HEAD and BF16_UP4 and BF16_HR and x.is_cuda and x.dtype == torch.bfloat16 and len(specs) == 4 and s0.Cin == 128 and s0.N == 64
            and act == ACT_RELU and s0.bias is not None
            and all(s.ntaps == 4 and s.omul == 2 and (s.ooy, s.oox) == (i >> 1, i & 1) for i, s in enumerate(specs)))


def up4_head_compose_bf16(x, specs, head16, bg, want_pred=True, want_mask=True, want_img=False):
    """BASELINE configs[3]'s last stage as ONE launch (csrc/up4_head_bf16.hip): x (B,H,W,128) bf16 -> ReLU(ConvTranspose2d(4, 2, 1)) (B,2H,2W,64), never
    written -> the 5x5 regressors + tanh / sigmoid + compositing -> (pred, mask, img) fp32 NCHW at (2H, 2W), as ``head_compose`` returns them.
    specs: the layer's four parity specs (packing.pack_conv_transpose); head16: packing.pack_head_bf16's panel."""
    B, H, W, _ = x.shape
    s0 = specs[0]
    dev = x.device
    S2h, S2w = 2 * H, 2 * W
    pred = torch.empty(B, 3, S2h, S2w, device=dev, dtype=torch.float32) if want_pred else None
    mask = torch.empty(B, 1, S2h, S2w, device=dev, dtype=torch.float32) if want_mask else None
    img = torch.empty(B, 3, S2h, S2w, device=dev, dtype=torch.float32) if want_img else None
    bstride = 0
    if bg is not None and bg.shape[0] != 1:
        assert bg.shape[0] == B
        bstride = 3 * S2h * S2w
    # the layer's output does not exist: a zero-batch tensor gives the launch description its geometry
    a = conv_args(x, s0, torch.empty(0, S2h, S2w, s0.N, device=dev, dtype=torch.bfloat16), act=ACT_RELU, out_hw=(H, W))
    # accounted as the transposed convolution it contains (16 taps, 4 N outputs per input pixel) + nothing for the head (as before)
    per = H * W * 256
    _fused_transpose_launch(a, s0, _w16up(specs), "lwg_up4_head_compose_bf16", "up4_head",
                            extra=(_ptr(head16, torch.bfloat16), _ptr(bg), bstride, _ptr(pred), _ptr(mask), _ptr(img)),
                            kernels=max(1, -(-B // max(1, (0xC0000000 - 1) // per))))
    return pred, mask, img


def thin_conv(x, wpk, ks):
    """Stride-1 ks x ks convolution (pad ks // 2, no bias) with <= 4 outputs: x (B,S,S,C) NHWC, wpk (ks*ks, C, 4) -> (B,S,S,4)
    pre-activation (csrc/head.hip lwg_thin_conv_f32)."""
    B, S, S2, C = x.shape
    assert S == S2 and tuple(wpk.shape) == (ks * ks, C, 4), (x.shape, wpk.shape, ks)
    y = torch.empty(B, S, S, 4, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_thin_conv_f32(_ptr(x), _ptr(wpk), B, S, C, ks, _ptr(y), _stream()), "lwg_thin_conv_f32")
    return y


def nchw_to_nhwc(x, c_pad=None):
    B, C = x.shape[0], x.shape[1]
    H, W = x.shape[2], x.shape[3]
    Cp = C if c_pad is None else c_pad
    y = torch.empty(B, H, W, Cp, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_nchw_to_nhwc_f32(_ptr(x), _ptr(y), B, C, Cp, H * W, _stream()), "lwg_nchw_to_nhwc_f32")
    return y


def nhwc_to_nchw(x, channels=None):
    B, H, W, Cs = x.shape
    C = Cs if channels is None else channels
    y = torch.empty(B, C, H, W, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_nhwc_to_nchw_f32(_ptr(x), _ptr(y), B, C, Cs, H * W, _stream()), "lwg_nhwc_to_nchw_f32")
    return y


def smpl_lbs(model, pose, beta, cam, offsets=None, links=None):
    """model: dict of device buffers (v_template, shapedirs, posedirs, J_regressor, parents int32, lbs_weights)."""
    B = pose.shape[0]
    nv = model["v_template"].shape[0]
    nj = model["J_regressor"].shape[0]
    dev = pose.device
    assert pose.shape[1] == 3 * nj, (pose.shape, nj)
    verts = torch.empty(B, nv, 3, device=dev, dtype=torch.float32)
    j3d = torch.empty(B, nj, 3, device=dev, dtype=torch.float32)
    j2d = torch.empty(B, nj, 2, device=dev, dtype=torch.float32) if cam is not None else None
    ws = torch.empty(_lib.lib().lwg_smpl_lbs_ws_floats(B, nv, nj), device=dev, dtype=torch.float32)
    off_batched = 0
    if offsets is not None:
        off_batched = 1 if offsets.dim() == 3 else 0
        if off_batched:
            assert offsets.shape[0] == B
    nlinks = 0 if links is None else links.shape[0]
    nbeta = beta.shape[1]
    _lib.check(_lib.lib().lwg_smpl_lbs_f32(
        _ptr(pose), pose.shape[1], _ptr(beta), nbeta, nbeta, _ptr(cam), 0 if cam is None else cam.shape[1],
        _ptr(model["v_template"]), _ptr(offsets), off_batched, _ptr(model["shapedirs"]), _ptr(model["posedirs"]),
        _ptr(model["J_regressor"]), _ptr(model["parents"], torch.int32), _ptr(model["lbs_weights"]),
        _ptr(links, torch.int32), nlinks, B, nv, nj, _ptr(verts), _ptr(j3d), _ptr(j2d), _ptr(ws), _stream()),
        "lwg_smpl_lbs_f32")
    return verts, j3d, j2d


# ---------------------------------------------------------------------------------------------- source_setup stage
MORPH_MODES = {"erode": 0, "dilate": 1, "soft_dilate": 2}


def morph(x, ks, mode="erode"):
    """(n,1,H,W) mask -> morphed mask (tools/utils/morphology/morph_ops.py:7-63)."""
    n, c, H, W = x.shape
    assert c == 1
    x = x.contiguous().float()
    out = torch.empty_like(x)
    ws = torch.empty_like(x)
    _lib.check(_lib.lib().lwg_morph_f32(_ptr(x), _ptr(out), n, H, W, int(ks), MORPH_MODES[mode], _ptr(ws), _stream()),
               "lwg_morph_f32")
    return out


def canny_edges(sil, gauss9, sobelx9, low, high):
    """(n,1,H,W) -> thin edges in {0,1} (canny_ops.py:137-212 with hysteresis).  gauss9/sobelx9: 9 python floats."""
    import ctypes
    n, c, H, W = sil.shape
    assert c == 1
    sil = sil.contiguous().float()
    edges = torch.empty_like(sil)
    ws = torch.empty(3 * sil.numel(), device=sil.device, dtype=torch.float32)
    g = (ctypes.c_float * 9)(*[float(v) for v in gauss9])
    s = (ctypes.c_float * 9)(*[float(v) for v in sobelx9])
    _lib.check(_lib.lib().lwg_canny_f32(_ptr(sil), n, H, W, g, s, float(low), float(high), _ptr(edges), _ptr(ws), _stream()),
               "lwg_canny_f32")
    return edges


def boundary_fill(src, confidant, outpad, edges, want_top3=False):
    """flowcomposition.py:268-386 body -> (morph_img (n,3,H,W), edge counts (n,) int32 device, top3 or None)."""
    n, _, H, W = src.shape
    src, confidant, outpad, edges = (t.contiguous().float() for t in (src, confidant, outpad, edges))
    out = torch.empty_like(src)
    top3 = torch.empty(n, 3, H, W, device=src.device, dtype=torch.int32) if want_top3 else None
    ws = torch.empty(n * (H * W + 1), device=src.device, dtype=torch.int32)
    _lib.check(_lib.lib().lwg_boundary_fill_f32(_ptr(src), _ptr(confidant), _ptr(outpad), _ptr(edges), n, H, W, _ptr(out),
                                                 _ptr(top3, torch.int32), _ptr(ws, torch.int32), _stream()),
               "lwg_boundary_fill_f32")
    return out, ws[n * H * W:], top3


def grid_sample(img, grid):
    """F.grid_sample(img (n|1,C,H,W), grid (n,Ho,Wo,2)) bilinear / zeros / align_corners=False."""
    n, Ho, Wo, _ = grid.shape
    nb, C, H, W = img.shape
    assert nb in (1, n)
    img, grid = img.contiguous().float(), grid.contiguous().float()
    out = torch.empty(n, C, Ho, Wo, device=img.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_grid_sample_nchw_f32(_ptr(img), 0 if (nb == 1 and n > 1) else C * H * W, _ptr(grid), n, C, H, W,
                                                    Ho, Wo, _ptr(out), _stream()), "lwg_grid_sample_nchw_f32")
    return out


def uv_merge(src_warp, vis):
    """flowcomposition.py:123-130 for one batch item: (ns,3,H,W), (ns,1,H,W) -> (3,H,W)."""
    ns, _, H, W = src_warp.shape
    out = torch.empty(3, H, W, device=src_warp.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_uv_merge_f32(_ptr(src_warp.contiguous()), _ptr(vis.contiguous()), ns, H, W, _ptr(out), _stream()),
               "lwg_uv_merge_f32")
    return out


def uv_merge_parts(uv_imgs, vis):
    """flowcomposition.py:816-856 (merge_uv_img): (n,3,H,W), (n,1,H,W) -> (1,3,H,W)."""
    n, _, H, W = uv_imgs.shape
    out = torch.empty(1, 3, H, W, device=uv_imgs.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_uv_merge_parts_f32(_ptr(uv_imgs.contiguous()), _ptr(vis.contiguous()), n, H, W, _ptr(out), _stream()),
               "lwg_uv_merge_parts_f32")
    return out


def pack_inputs(a, b, mask, c_pad):
    """cat[a * mask, b] (NCHW) -> NHWC with c_pad channels."""
    n, Ca, H, W = a.shape
    Cb = 0 if b is None else b.shape[1]
    out = torch.empty(n, H, W, c_pad, device=a.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_pack_inputs_f32(_ptr(a.contiguous()), Ca, _ptr(None if b is None else b.contiguous()), Cb,
                                               _ptr(None if mask is None else mask.contiguous()), n, H, W, c_pad, _ptr(out),
                                               _stream()), "lwg_pack_inputs_f32")
    return out


def frames_to_u8(pred, bgr=False):
    """(B,3,S,S) fp32 in [-1,1] -> (B,S,S,3) uint8 with save_cv2_img(normalize=True)'s numerics (cv_utils.py:111-113)."""
    B, C, S, S2 = pred.shape
    assert C == 3 and S == S2
    out = torch.empty(B, S, S, 3, device=pred.device, dtype=torch.uint8)
    if B == 0:               # an empty shard / all-padding chunk (sharding.sharded_synthesize): nothing to launch (a zero-size grid is invalid)
        return out
    _lib.check(_lib.lib().lwg_frames_to_u8(_ptr(pred), B, S, 1 if bgr else 0, _ptr(out, torch.uint8), _stream()), "lwg_frames_to_u8")
    return out


def png_deflate(u8, rows_per_segment=16):
    """(B,H,W,3) uint8 device frames -> (streams (B, capacity) uint8, nbytes (B,) int32): streams[b, :nbytes[b]] is the zlib stream of frame
    b's PNG IDAT chunk (include/lwg_hip.h lwg_png_deflate_u8; ``output.png_from_stream`` wraps it into a file).  Bytes behind nbytes[b] are
    not written."""
    if not u8.is_cuda:
        raise RuntimeError("png_deflate needs a device tensor: there is no CPU fallback")
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
        raise ValueError("png_deflate takes a (B,H,W,3) uint8 tensor")
    B, H, W, _ = u8.shape
    lib = _lib.lib()
    cap = lib.lwg_png_stream_capacity(H, W, int(rows_per_segment))
    nws = lib.lwg_png_deflate_ws_bytes(max(B, 1), H, W, int(rows_per_segment))
    if cap == 0 or nws == 0:
        raise ValueError(f"png_deflate: no encoding for {H} x {W} frames in segments of {rows_per_segment} rows (a segment holds at most 65535 bytes)")
    streams = torch.empty(B, cap, device=u8.device, dtype=torch.uint8)
    nbytes = torch.empty(B, device=u8.device, dtype=torch.int32)
    if B == 0:
        return streams, nbytes
    ws = torch.empty(nws, device=u8.device, dtype=torch.uint8)
    _lib.check(lib.lwg_png_deflate_u8(_ptr(u8.contiguous(), torch.uint8), B, H, W, int(rows_per_segment), _ptr(ws, torch.uint8), _ptr(streams, torch.uint8),
                                      _ptr(nbytes, torch.int32), _stream()), "lwg_png_deflate_u8")
    return streams, nbytes


_JPEG_ENTRIES = {"444": "lwg_jpeg", "420": "lwg_jpeg420"}      # subsampling -> the prefix of its four C entry points


def _jpeg_entries(subsampling):
    try:
        return _JPEG_ENTRIES[subsampling]
    except (KeyError, TypeError):
        raise ValueError("jpeg subsampling must be '444' or '420', not %r" % (subsampling,)) from None


def jpeg_mcu_size(subsampling="444"):
    """Pixels along an MCU's side: 8 at 4:4:4, 16 at 4:2:0 (restart intervals count MCUs of that size)."""
    return 8 if _jpeg_entries(subsampling) == "lwg_jpeg" else 16


def jpeg_max_mcus_per_segment(subsampling="444"):
    """The largest restart interval ``jpeg_scan`` takes (include/lwg_hip.h lwg_jpeg_max_mcus_per_segment, lwg_jpeg420_max_mcus_per_segment)."""
    return int(getattr(_lib.lib(), _jpeg_entries(subsampling) + "_max_mcus_per_segment")())


def _jpeg_frames(u8, quality, mcus_per_segment, subsampling, what, scan):
    """The argument checks in front of the jpeg entry points -> (entry prefix, quantiser bytes, B, H, W, interval)."""
    entry = _jpeg_entries(subsampling)
    if not u8.is_cuda:
        raise RuntimeError(what + " needs a device tensor: there is no CPU fallback")
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
        raise ValueError(what + " takes a (B,H,W,3) uint8 tensor")
    from .output import jpeg_tables
    luma, chroma = jpeg_tables(quality)
    B, H, W, _ = u8.shape
    lib = _lib.lib()
    most = getattr(lib, entry + "_max_mcus_per_segment")()
    side = jpeg_mcu_size(subsampling)
    ri = int(mcus_per_segment) if mcus_per_segment is not None else min((W + side - 1) // side, most)
    cap = getattr(lib, entry + scan + "_capacity")(H, W, ri)
    nws = getattr(lib, entry + scan + "_ws_bytes")(max(B, 1), H, W, ri)
    if cap == 0 or nws == 0:
        raise ValueError(f"{what}: no encoding for {B} frames of {H} x {W} in segments of {ri} MCUs (1 .. {most})")
    return entry, bytes(luma) + bytes(chroma), B, H, W, ri, cap, nws


def jpeg_scan(u8, quality=90, mcus_per_segment=None, subsampling="444", huffman="fixed"):
    """(B,H,W,3) uint8 RGB device frames -> (scans (B, capacity) uint8, nbytes (B,) int32): scans[b, :nbytes[b]] is the entropy-coded scan of
    frame b's baseline JPEG (4:4:4, restart interval ``mcus_per_segment`` MCUs, default min(ceil(W / 8), the largest); include/lwg_hip.h
    lwg_jpeg_scan_u8; ``output.jpeg_from_scan`` wraps it into a file).  capacity is the worst case, several times the raw frame: copy
    prefixes.  Bytes behind nbytes[b] are not written.  ``subsampling="420"``: lwg_jpeg420_scan_u8 - 16 x 16 MCUs of four Y blocks and one
    Cb and Cr block each, the default interval min(ceil(W / 16), the largest); chroma detail is lost (noise-like colour almost entirely).
    ``huffman="optimized"``: lwg_jpeg_scan_opt_u8 / lwg_jpeg420_scan_opt_u8 - every frame is coded with Huffman tables built from its own
    symbol counts; -> (scans, nbytes, tables (B, 4, 272) uint8: per table, in DHT order, 16 counts per length and 256 symbol slots), which
    ``output.jpeg_from_scan(tables=...)`` takes.  The decoded pixels are those of the fixed-table scan."""
    from .output import jpeg_check_huffman
    opt = jpeg_check_huffman(huffman) == "optimized"
    scan = "_scan_opt" if opt else "_scan"
    entry, qtab, B, H, W, ri, cap, nws = _jpeg_frames(u8, quality, mcus_per_segment, subsampling, "jpeg_scan", scan)
    scans = torch.empty(B, cap, device=u8.device, dtype=torch.uint8)
    nbytes = torch.empty(B, device=u8.device, dtype=torch.int32)
    tables = torch.empty(B, 4, 272, device=u8.device, dtype=torch.uint8) if opt else None
    if B:
        ws = torch.empty(nws, device=u8.device, dtype=torch.uint8)
        args = (_ptr(u8.contiguous(), torch.uint8), B, H, W, qtab, ri, _ptr(ws, torch.uint8), _ptr(scans, torch.uint8), _ptr(nbytes, torch.int32))
        if opt:
            args += (_ptr(tables, torch.uint8),)
        _lib.check(getattr(_lib.lib(), entry + scan + "_u8")(*args, _stream()), entry + scan + "_u8")
    return (scans, nbytes, tables) if opt else (scans, nbytes)


def jpeg_symbol_histogram(u8, quality=90, mcus_per_segment=None, subsampling="444"):
    """(B,H,W,3) uint8 RGB device frames -> (B, 4, 256) int32 (the bits of the uint32 counts): how often frame b's scan codes every symbol of
    its DC luminance, AC luminance, DC chrominance and AC chrominance table - the first step of ``jpeg_scan(huffman="optimized")`` alone
    (include/lwg_hip.h lwg_jpeg_hist_u8, lwg_jpeg420_hist_u8; tests/jpeghuff_emu.py ``histogram``)."""
    entry, qtab, B, H, W, ri, _, nws = _jpeg_frames(u8, quality, mcus_per_segment, subsampling, "jpeg_symbol_histogram", "_scan_opt")
    hist = torch.empty(B, 4, 256, device=u8.device, dtype=torch.int32)
    if B:
        ws = torch.empty(nws, device=u8.device, dtype=torch.uint8)
        name = entry + "_hist_u8"
        _lib.check(getattr(_lib.lib(), name)(_ptr(u8.contiguous(), torch.uint8), B, H, W, qtab, ri, _ptr(ws, torch.uint8), _ptr(hist, torch.int32),
                                             _stream()), name)
    return hist


def jpeg_huffman_tables(hist):
    """(B, 4, 256) int32 device counts (read as uint32) -> (tables (B, 4, 272) uint8, codes (B, 544) int32): the second step of
    ``jpeg_scan(huffman="optimized")`` alone (include/lwg_hip.h lwg_jpeg_huff_tables; tests/jpeghuff_emu.py ``table``, ``dht`` and
    ``coder_words``).  Any counts are taken; a DC table's symbols from 16 on have no place in ``codes``."""
    if not hist.is_cuda:
        raise RuntimeError("jpeg_huffman_tables needs a device tensor: there is no CPU fallback")
    if hist.dtype != torch.int32 or hist.dim() != 3 or tuple(hist.shape[1:]) != (4, 256):
        raise ValueError("jpeg_huffman_tables takes a (B,4,256) int32 tensor")
    B = hist.shape[0]
    tables = torch.empty(B, 4, 272, device=hist.device, dtype=torch.uint8)
    codes = torch.empty(B, 544, device=hist.device, dtype=torch.int32)
    if B:
        _lib.check(_lib.lib().lwg_jpeg_huff_tables(_ptr(hist.contiguous(), torch.int32), B, _ptr(tables, torch.uint8), _ptr(codes, torch.int32),
                                                   _stream()), "lwg_jpeg_huff_tables")
    return tables, codes


def png_rows_per_segment(H, W, most=16):
    """The largest of 16, 8, 4, 2, 1 rows (at most ``most``) whose deflate segment of an (H, W) frame ``png_deflate`` takes (a segment holds
    at most 65 535 raw bytes: 16 rows up to W = 1 364, which covers every square frame up to 1024 and not a fused canvas of three 512 panels)."""
    lib = _lib.lib()
    for r in (16, 8, 4, 2, 1):
        if r <= int(most) and lib.lwg_png_stream_capacity(int(H), int(W), r):
            return r
    raise ValueError(f"png_deflate: no encoding for {H} x {W} frames (one row is more than a 65535-byte segment)")


def fuse_source_panel(src_img):
    """(ns,3,S,S) (or (1,ns,3,S,S)) fp32 source images in [-1,1] on the device -> the (S,Wp,3) uint8 RGB source panel of the reference's
    comparison video (fuse_source, tools/utils/multimedia/video.py:297-357; include/lwg_hip.h lwg_fuse_sources_u8).  The panel is what the
    reference's CODE shows, its two quirks included: ns = 7 shows sources 0..3 (padded to eight paths, then handed to fuse_four_images), and
    ns >= 8 shows sources 0, 1, 4, 5 in one quarter-size column (fuse_eight_images hands four paths to fuse_two_images, which reads two)."""
    if not src_img.is_cuda:
        raise RuntimeError("fuse_source_panel needs a device tensor: there is no CPU fallback")
    if src_img.dim() == 5 and src_img.shape[0] == 1:
        src_img = src_img[0]
    if src_img.dim() != 4 or src_img.shape[1] != 3 or src_img.shape[2] != src_img.shape[3] or src_img.dtype != torch.float32:
        raise ValueError("fuse_source_panel takes a (ns,3,S,S) fp32 tensor")
    ns, _, S, _ = src_img.shape
    lib = _lib.lib()
    Wp = lib.lwg_fuse_panel_width(ns, S)
    if Wp == 0:
        raise ValueError(f"fuse_source_panel: no panel for {ns} sources of {S} x {S} (ns >= 1; 2..7 sources need an even size, 8 and more S % 4 == 0)")
    panel = torch.empty(S, Wp, 3, device=src_img.device, dtype=torch.uint8)
    _lib.check(lib.lwg_fuse_sources_u8(_ptr(src_img.contiguous()), ns, S, _ptr(panel, torch.uint8), _stream()), "lwg_fuse_sources_u8")
    return panel


def fuse_canvas(panel, refs, outs, pad=10, pad_val=0):
    """panel (S,Wp,3) uint8 (``fuse_source_panel``), refs (B,S,S,3) uint8 RGB or None, outs: one (B,3,S,S) fp32 tensor or a sequence of 1..4 ->
    the (B,S,Wc,3) uint8 canvas [panel | pad | ref | pad | out0 | pad | out1 ...] of the reference's merge_multi_outs / merge_src_out
    (video.py:173-213; include/lwg_hip.h lwg_fuse_canvas_u8), its out regions ``frames_to_u8``'s bytes.  Device tensors only."""
    if torch.is_tensor(outs):
        outs = (outs,)
    outs = tuple(outs)
    if not 1 <= len(outs) <= 4:
        raise ValueError("fuse_canvas takes 1 .. 4 output tensors")
    for t in (panel, refs) + outs:
        if t is not None and not t.is_cuda:
            raise RuntimeError("fuse_canvas needs device tensors: there is no CPU fallback")
    B, C, S, S2 = outs[0].shape
    if C != 3 or S != S2 or any(tuple(o.shape) != (B, 3, S, S) or o.dtype != torch.float32 for o in outs):
        raise ValueError("fuse_canvas: every output is a (B,3,S,S) fp32 tensor of the same shape")
    if panel.dtype != torch.uint8 or panel.dim() != 3 or panel.shape[0] != S or panel.shape[2] != 3:
        raise ValueError("fuse_canvas: the panel is a (S,Wp,3) uint8 tensor")
    if refs is not None and (refs.dtype != torch.uint8 or tuple(refs.shape) != (B, S, S, 3)):
        raise ValueError("fuse_canvas: the reference frames are a (B,S,S,3) uint8 tensor")
    Wp, pad, pad_val = int(panel.shape[1]), int(pad), int(pad_val)
    if pad < 0 or not 0 <= pad_val <= 255:
        raise ValueError("fuse_canvas: pad >= 0 and 0 <= pad_val <= 255")
    Wc = Wp + ((refs is not None) + len(outs)) * (S + pad)
    canvas = torch.empty(B, S, Wc, 3, device=outs[0].device, dtype=torch.uint8)
    if B == 0:
        return canvas
    outs = tuple(o.contiguous() for o in outs)
    ptrs = (ctypes.c_void_p * len(outs))(*[_ptr(o) for o in outs])
    err = _lib.lib().lwg_fuse_canvas_u8(_ptr(panel.contiguous(), torch.uint8), Wp, None if refs is None else _ptr(refs.contiguous(), torch.uint8), ptrs,
                                        len(outs), B, S, pad, pad_val, _ptr(canvas, torch.uint8), _stream())
    if err == 1:
        raise ValueError(f"fuse_canvas: no canvas for S = {S}, panel width {Wp}, pad {pad}, {len(outs)} outputs (include/lwg_hip.h lwg_fuse_canvas_u8)")
    _lib.check(err, "lwg_fuse_canvas_u8")
    return canvas


# ---------------------------------------------------------------------------------------------- backward of the convs
def conv2d_wgrad(x0, spec, dy, x1=None, out_hw=None, ycoff=0):
    """dW of the conv described by ``spec`` for inputs x0 (x1) and output gradient dy (laid out like the forward y) ->
    (ntaps * Cin, N) fp32 in the forward panel's K order (see packing.unpack_wgrad)."""
    a = conv_args(x0, spec, dy, x1=x1, out_hw=out_hw, ycoff=ycoff)
    Ktot = spec.ntaps * spec.Cin
    dw = torch.empty(Ktot, spec.N, device=x0.device, dtype=torch.float32)
    ws = torch.empty(_lib.lib().lwg_conv2d_wgrad_ws_floats(Ktot, spec.N, a.M), device=x0.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_conv2d_wgrad_nhwc_f32(a, _ptr(dy), _ptr(dw), _ptr(ws), _stream()), "lwg_conv2d_wgrad_nhwc_f32")
    return dw


def conv2d_wgrad_unpacked(x0, spec, dy, dw, transposed, kidx, cin, nout, x1=None, out_hw=None, ycoff=0, db=None):
    """``conv2d_wgrad`` + ``unpack_wgrad`` in one reduction launch: the weight gradient lands at positions kidx of dw (D0,D1,KH,KW).
    db: optional (nout,) tensor that receives the bias gradient (column sums of dy) from the same two launches."""
    a = conv_args(x0, spec, dy, x1=x1, out_hw=out_hw, ycoff=ycoff)
    Ktot = spec.ntaps * spec.Cin
    D0, D1, KH, KW = dw.shape
    assert dw.is_contiguous() and len(kidx) == spec.ntaps
    ws = torch.empty(_lib.lib().lwg_conv2d_wgrad_ws_floats(Ktot, spec.N, a.M), device=x0.device, dtype=torch.float32)
    arr = (ctypes.c_int * spec.ntaps)(*[int(k) for k in kidx])
    if db is not None:
        assert db.is_contiguous() and db.dtype == torch.float32 and db.numel() == nout
    _lib.check(_lib.lib().lwg_conv2d_wgrad_unpacked_f32(a, _ptr(dy), _ptr(ws), _ptr(dw), D0, D1, KH, KW, 1 if transposed else 0, arr, cin, nout,
                                                        None if db is None else _ptr(db), _stream()), "lwg_conv2d_wgrad_unpacked_f32")
    return dw


# "direct": every weight gradient on lwg_conv_wgrad_kernel.  "winograd": the 3x3 / stride 1 / pad 1 launches with both channel counts % 64 == 0
# (_wgrad_wino_use) run lwg_conv2d_wgrad_winograd_f32 - dU = sum V^T Z, dw = G^T dU G: 16 products per 2x2 output tile and channel pair instead of
# 36 (csrc/conv_wgrad_winograd.hip); fp32-grade, not the direct kernel's bits, bias gradient by ops.colsum.  Every other launch exactly as "direct".
# "bf16" (entered through ``wgrad_mode``): the launches with C0 % 32 == 0, C1 % 32 == 0, N % 64 == 0 and a dense dy (_wgrad_bf16_use; any taps and
# stride) run lwg_conv2d_wgrad_bf16_f32 - both fp32 operands rounded to bf16 in the kernel, v_mfma_f32_32x32x16_bf16, fp32 accumulation, the fused
# bias gradient from the fp32 dy (csrc/conv_wgrad_bf16.hip); bf16-operand grade.  Every other launch exactly as "direct".
WGRAD_PRECISION = "direct"


class wgrad_precision(object):
    """Context manager: ``with ops.wgrad_precision("winograd"): ...`` - the two fp32-grade modes, as before the bf16 mode existed (it keeps rejecting
    every other name: tests/test_wgrad_winograd_cpu.py pins that); ``wgrad_mode`` takes all three."""
    MODES = ("direct", "winograd")

    def __init__(self, mode):
        assert mode in self.MODES
        self.mode = mode

    def __enter__(self):
        global WGRAD_PRECISION
        self.prev = WGRAD_PRECISION
        WGRAD_PRECISION = self.mode

    def __exit__(self, *exc):
        global WGRAD_PRECISION
        WGRAD_PRECISION = self.prev


class wgrad_mode(wgrad_precision):
    """The same switch with every value of trainers.TrainOpts.wgrad_precision: ``with ops.wgrad_mode("bf16"): ...`` (nests with ``wgrad_precision``)."""
    MODES = ("direct", "winograd", "bf16")


def launch_modes():
    """Every mode switch a captured step freezes into its kernels: a capture made under one value of this tuple is replayed only under that value
    (trainers.LWGTrainer).  A new switch of this kind belongs HERE - nowhere else is there a list to extend."""
    return CONV_PRECISION, _MODE_WINO4, WGRAD_PRECISION, TRAIN_CONV_TILES


def _wgrad_wino_use(x0, spec, dy, x1=None):
    """Launches lwg_conv2d_wgrad_winograd_f32 takes (its C contract): fp32 device tensors, 3x3 / stride 1 / pad 1 with the taps ascending in (dy, dx),
    C0 % 64 == 0, C1 % 64 == 0, N % 64 == 0, dy dense (B, H, W, N), every tensor < 3 GiB."""
    if not (x0.is_cuda and dy.is_cuda) or x0.dtype != torch.float32 or dy.dtype != torch.float32 or x0.dim() != 4 or dy.dim() != 4:
        return False
    if x1 is not None and (not x1.is_cuda or x1.dtype != torch.float32 or x1.shape[:3] != x0.shape[:3] or x1.shape[3] % 64 != 0):
        return False
    C1 = 0 if x1 is None else x1.shape[3]
    if spec.ntaps != 9 or spec.stride != 1 or spec.omul != 1 or spec.ooy != 0 or spec.oox != 0 or x0.shape[3] % 64 != 0 or spec.N % 64 != 0 or \
            x0.shape[3] + C1 != spec.Cin or list(zip(spec.dy, spec.dx)) != _WINO_TAPS:
        return False
    if tuple(dy.shape) != (x0.shape[0], x0.shape[1], x0.shape[2], spec.N):
        return False
    pix = x0.shape[0] * x0.shape[1] * x0.shape[2]
    return pix * max(x0.shape[3], C1, spec.N) * 4 < 0xC0000000


def conv2d_wgrad_winograd(x0, spec, dy, dw, cin, nout, x1=None):
    """The weight gradient of an eligible 3x3 launch (``_wgrad_wino_use``) in F(2x2, 3x3) Winograd form, written into dw (nout, cin, 3, 3)
    (lwg_conv2d_wgrad_winograd_f32: one fused slab launch + one reduction launch; no bias gradient - ``colsum``)."""
    a = conv_args(x0, spec, dy, x1=x1)
    assert dw.is_contiguous() and tuple(dw.shape) == (nout, cin, 3, 3)
    nws = _lib.lib().lwg_conv2d_wgrad_winograd_ws_floats(a)
    if nws == 0:
        raise ValueError("launch outside lwg_conv2d_wgrad_winograd_f32's contract (ops._wgrad_wino_use)")
    if CONV_HOOK is not None:
        CONV_HOOK(True, a.M, spec, EPI_NONE, None)
    ws = torch.empty(nws, device=x0.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_conv2d_wgrad_winograd_f32(a, _ptr(dy), _ptr(ws), _ptr(dw), cin, nout, _stream()), "lwg_conv2d_wgrad_winograd_f32")
    if CONV_HOOK is not None:
        CONV_HOOK(False, a.M, spec, EPI_NONE, {"kernels": 2, "kind": "wgrad_winograd"})
    return dw


def _wgrad_bf16_shapes_ok(xs, spec, dys, x1s=None):
    """The shape part of lwg_conv2d_wgrad_bf16_f32's contract for x0 / dy / x1 of shapes xs / dys / x1s, launched as ``conv_args`` would (dy is the
    whole output: ycoff 0): C0 % 32 == 0, C1 % 32 == 0, C0 + C1 == spec.Cin, N % 64 == 0, omul 1, dy (B, OH, OW, N) dense, every tensor < 3 GiB."""
    if len(xs) != 4 or len(dys) != 4 or (x1s is not None and (len(x1s) != 4 or tuple(x1s[:3]) != tuple(xs[:3]))):
        return False
    C0, C1 = xs[3], 0 if x1s is None else x1s[3]
    if min(xs) < 1 or min(dys) < 1 or C0 % 32 != 0 or C1 % 32 != 0 or C0 + C1 != spec.Cin or spec.N % 64 != 0 or not 1 <= spec.ntaps <= _lib.LWG_MAX_TAPS or \
            spec.stride < 1 or spec.omul != 1 or spec.ooy != 0 or spec.oox != 0 or dys[0] != xs[0] or dys[3] != spec.N:
        return False
    return xs[0] * xs[1] * xs[2] * max(C0, C1) * 4 < 0xC0000000 and dys[0] * dys[1] * dys[2] * dys[3] * 4 < 0xC0000000


def _wgrad_bf16_use(x0, spec, dy, x1=None):
    """Launches lwg_conv2d_wgrad_bf16_f32 takes (its C contract): fp32 device tensors, C0 % 32 == 0, C1 % 32 == 0, N % 64 == 0, any tap list and stride,
    dy dense (B, OH, OW, N) with omul 1, every tensor < 3 GiB.  The small-Cin first layers (Cin 4 .. 16) and the parity launches of a transposed
    convolution (omul 2) are outside it."""
    ts = (x0, dy) if x1 is None else (x0, dy, x1)
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in ts):
        return False
    return _wgrad_bf16_shapes_ok(tuple(x0.shape), spec, tuple(dy.shape), None if x1 is None else tuple(x1.shape))


def conv2d_wgrad_bf16(x0, spec, dy, dw, transposed, kidx, cin, nout, x1=None, out_hw=None, ycoff=0, db=None):
    """``conv2d_wgrad_unpacked`` with bf16 operands and fp32 accumulation (lwg_conv2d_wgrad_bf16_f32: one slab launch + one reduction launch, the bias
    gradient ``db`` - fp32 column sums of dy - from the same two) for a launch inside ``_wgrad_bf16_use``; bf16-operand grade, deterministic."""
    a = conv_args(x0, spec, dy, x1=x1, out_hw=out_hw, ycoff=ycoff)
    D0, D1, KH, KW = dw.shape
    assert dw.is_contiguous() and len(kidx) == spec.ntaps
    nws = _lib.lib().lwg_conv2d_wgrad_bf16_ws_floats(a)
    if nws == 0:
        raise ValueError("launch outside lwg_conv2d_wgrad_bf16_f32's contract (ops._wgrad_bf16_use)")
    if db is not None:
        assert db.is_contiguous() and db.dtype == torch.float32 and db.numel() == nout
    if CONV_HOOK is not None:
        CONV_HOOK(True, a.M, spec, EPI_NONE, None)
    ws = torch.empty(nws, device=x0.device, dtype=torch.float32)
    arr = (ctypes.c_int * spec.ntaps)(*[int(k) for k in kidx])
    _lib.check(_lib.lib().lwg_conv2d_wgrad_bf16_f32(a, _ptr(dy), _ptr(ws), _ptr(dw), D0, D1, KH, KW, 1 if transposed else 0, arr, cin, nout,
                                                    None if db is None else _ptr(db), _stream()), "lwg_conv2d_wgrad_bf16_f32")
    if CONV_HOOK is not None:
        CONV_HOOK(False, a.M, spec, EPI_NONE, {"kernels": 2, "kind": "wgrad_bf16"})
    return dw


class PanelCache:
    """The panels of a training step, re-packed by ONE launch per step (lwg_pack_panels_f32) instead of one launch per panel.

    While a cache is installed (``ops.PANEL_CACHE``; trainers.LWGTrainer installs its own for the duration of a step) ``pack_panel``
    hands out a persistent output buffer per (weight storage, packing arguments): the first request packs it with a single launch
    and registers it, later requests return the buffer untouched - it was refreshed from the current weights by ``refresh()`` at the
    start of the step (no weight changes between that point and its last use within a step: Adam(G) runs after G's backward,
    Adam(D) at the end).  The weights are held by reference, so a registered address is never recycled."""

    def __init__(self, params=()):
        """params: the tensors whose STORAGE may be cached from (module parameters / flat optimizer buffers).  A weight assembled per
        call (e.g. the concatenated image + mask regressors of the fused head's backward) lives in a temporary: its address
        changes every step, so it is packed by a single launch each time and never registered."""
        self.out, self.rows, self.keep, self.table, self.blocks = {}, [], [], None, 0
        params = list(params)
        self.storages = {p.untyped_storage().data_ptr() for p in params}
        self.training_storages = {p.untyped_storage().data_ptr() for p in params if p.requires_grad}    # (pack_panel sees detached views)
        # Winograd fragment panels derived from registered GEMM panels (ops._wwino): key (panel address, tap order) -> U; the ones whose
        # weights train are re-derived by ONE launch per step behind the GEMM panels' refresh (lwg_winograd_panels_f32)
        self.src_of, self.wino, self.wino_rows, self.wino_table, self.wino_blocks = {}, {}, [], None, 0
        # ... and the F(4x4, 3x3) panels (ops._wwino4; train_conv_tiles("4x4")): one more launch behind that one (lwg_winograd4_panels_f32)
        self.wino4, self.wino4_rows, self.wino4_table, self.wino4_blocks = {}, [], None, 0
        # frozen weights (the loss networks): packed once - but watched: [weight, tensor version at pack time, cache key]; refresh() re-packs a
        # panel whose weight was written since (load_state_dict / an un-freeze after the first step) instead of training against a stale one
        self.frozen = []

    def cacheable(self, w):
        return w.untyped_storage().data_ptr() in self.storages

    def get(self, w, transposed, kidx, cin, cin_pad, nout, n_pad):
        key = (w.data_ptr(), tuple(w.shape), bool(transposed), kidx, cin, cin_pad, nout, n_pad)
        hit = self.out.get(key)
        if hit is not None:
            return hit, False
        if self.table is not None and torch.cuda.is_current_stream_capturing() and w.untyped_storage().data_ptr() in self.training_storages:
            raise RuntimeError("PanelCache: a panel was requested for the first time inside a hipGraph capture (the table upload is "
                               "not capturable): run one eager step before capturing")
        D0, D1, KH, KW = w.shape
        Kp = (len(kidx) * cin_pad + 31) // 32 * 32
        out = torch.empty(Kp // 4, n_pad, 4, device=w.device, dtype=torch.float32)
        self.out[key] = out
        self.src_of[out.data_ptr()] = w
        self.keep.append(w)
        if w.untyped_storage().data_ptr() in self.training_storages:     # a frozen weight (the loss networks) is packed once, by the caller's launch
            self.rows.append((w.data_ptr(), out.data_ptr(), D1, KH * KW, 1 if transposed else 0, len(kidx), cin, cin_pad, nout, n_pad, Kp, kidx))
            self.table = None
        else:
            self.frozen.append([w, w._version, key])
        return out, True

    def _repack_stale_frozen(self):
        """Frozen weights written in place since their panels were packed: single launches, eager only (a captured step cannot see the host check:
        ``invalidate()`` + a re-capture is the route there, and the trainer re-captures when this raises)."""
        stale = [f for f in self.frozen if f[0]._version != f[1]]
        if not stale:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("PanelCache: a frozen weight changed (load_state_dict / un-freeze) - its panels cannot be re-packed inside a hipGraph "
                               "capture: call refresh() eagerly once (or invalidate()) before capturing")
        for f in stale:
            w, _, key = f
            _, _, transposed, kidx, cin, cin_pad, nout, n_pad = key
            out = self.out[key]
            D0, D1, KH, KW = w.shape
            arr = (ctypes.c_int * len(kidx))(*kidx)
            _lib.check(_lib.lib().lwg_pack_panel_f32(_ptr(w), D0, D1, KH, KW, 1 if transposed else 0, arr, len(kidx), cin, cin_pad, nout, n_pad,
                                                     _ptr(out), _stream()), "lwg_pack_panel_f32")
            for (pp, tap9), U in self.wino.items():
                if pp == out.data_ptr():
                    arr9 = (ctypes.c_int * 9)(*tap9)
                    _lib.check(_lib.lib().lwg_winograd_panel_f32(_ptr(out), _ptr(U), cin_pad, out.shape[1], arr9, _stream()), "lwg_winograd_panel_f32")
            for (pp, tap9), U in self.wino4.items():
                if pp == out.data_ptr():
                    arr9 = (ctypes.c_int * 9)(*tap9)
                    _lib.check(_lib.lib().lwg_winograd4_panel_f32(_ptr(out), _ptr(U), cin_pad, out.shape[1], arr9, _stream()), "lwg_winograd4_panel_f32")
            f[1] = w._version

    def invalidate(self):
        """Forget every panel (weights re-allocated or reloaded wholesale): the next requests pack afresh."""
        self.out, self.rows, self.keep, self.table, self.blocks, self.frozen = {}, [], [], None, 0, []
        self.src_of, self.wino, self.wino_rows, self.wino_table, self.wino_blocks = {}, {}, [], None, 0
        self.wino4, self.wino4_rows, self.wino4_table, self.wino4_blocks = {}, [], None, 0

    def refresh(self):
        """Re-pack every registered panel of a weight that trains (requires_grad when the cache was built) from the current weights: one launch
        on the current stream, one more for the Winograd panels derived from them.  Panels of frozen weights are built once and re-packed only
        when the weight's tensor version moved since (an in-place load_state_dict)."""
        self._repack_stale_frozen()
        if not self.rows:
            return
        if self.table is None:
            descs = (_lib.LwgPackDesc * len(self.rows))()
            first = 0
            for d, (wp, op, D1, KHW, tr, nt, cin, cp, nout, npad, Kp, kidx) in zip(descs, self.rows):
                d.w, d.out = wp, op
                d.D1, d.KHW, d.transposed, d.ntaps, d.cin, d.cin_pad, d.nout, d.n_pad, d.Kp, d.first_block = D1, KHW, tr, nt, cin, cp, nout, npad, Kp, first
                for i, k in enumerate(kidx):
                    d.kidx[i] = k
                first += ((Kp // 4) * npad + 255) // 256
            raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8)
            self.table = raw.to(self.keep[0].device)
            self.blocks = first
        _lib.check(_lib.lib().lwg_pack_panels_f32(self.table.data_ptr(), len(self.rows), self.blocks, _stream()), "lwg_pack_panels_f32")
        if self.wino_rows:
            if self.wino_table is None:
                self.wino_table, self.wino_blocks = self._wino_table(self.wino_rows, 16)
            _lib.check(_lib.lib().lwg_winograd_panels_f32(self.wino_table.data_ptr(), len(self.wino_rows), self.wino_blocks, _stream()),
                       "lwg_winograd_panels_f32")
        if self.wino4_rows:
            if self.wino4_table is None:
                self.wino4_table, self.wino4_blocks = self._wino_table(self.wino4_rows, 4)
            _lib.check(_lib.lib().lwg_winograd4_panels_f32(self.wino4_table.data_ptr(), len(self.wino4_rows), self.wino4_blocks, _stream()),
                       "lwg_winograd4_panels_f32")

    def _wino_table(self, rows, cpb):
        """rows of (GEMM panel, fragment panel, Cin, N, tap order) -> (the device table of LwgWinoDesc records, its total blocks); a block = 64
        output columns x cpb input channels (lwg_winograd_panels_f32: 16, lwg_winograd4_panels_f32: 4)."""
        descs = (_lib.LwgWinoDesc * len(rows))()
        first = 0
        for d, (wp, up, cin, N, tap9) in zip(descs, rows):
            d.wpanel, d.upk, d.Cin, d.N, d.first_block = wp, up, cin, N, first
            for i in range(9):
                d.tap9[i] = tap9[i]
            first += ((N + 63) // 64) * ((cin + cpb - 1) // cpb)
        raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8)
        return raw.to(self.keep[0].device), first

    def winograd(self, spec, tap9):
        """The F(2x2, 3x3) fragment panel [16][Cin/8][2][N][4] of a spec whose GEMM panel is registered here, or None (a per-call temporary: single
        launch each time).  First request: allocated, built by a single launch and - when the source weight trains - registered for the per-step
        refresh."""
        return self._fragment_panel(spec, tap9, self.wino, self.wino_rows, "wino_table", lambda N: (16, spec.Cin // 8, 2, N, 4), "lwg_winograd_panel_f32")

    def winograd4(self, spec, tap9):
        """The same for the F(4x4, 3x3) fragment panel [4][Cin/8][4][2][9 N] (ops._wwino4)."""
        return self._fragment_panel(spec, tap9, self.wino4, self.wino4_rows, "wino4_table", lambda N: (4, spec.Cin // 8, 4, 2, 9 * N),
                                    "lwg_winograd4_panel_f32")

    def _fragment_panel(self, spec, tap9, panels, rows, table, shape, single):
        w = self.src_of.get(spec.w.data_ptr())
        if w is None:
            return None
        key = (spec.w.data_ptr(), tuple(tap9))
        U = panels.get(key)
        if U is None:
            trains = w.untyped_storage().data_ptr() in self.training_storages
            if getattr(self, table) is not None and trains and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("PanelCache: a Winograd panel was requested for the first time inside a hipGraph capture: run one eager step first")
            K4, N, _ = spec.w.shape
            U = torch.empty(*shape(N), device=spec.w.device, dtype=torch.float32)
            arr = (ctypes.c_int * 9)(*tap9)
            _lib.check(getattr(_lib.lib(), single)(_ptr(spec.w), _ptr(U), spec.Cin, N, arr, _stream()), single)
            panels[key] = U
            if trains:                                       # frozen weights (the loss networks): built once
                rows.append((spec.w.data_ptr(), U.data_ptr(), spec.Cin, N, tuple(tap9)))
                setattr(self, table, None)
        return U


PANEL_CACHE = None      # a PanelCache while a trainer step runs (trainers.LWGTrainer), else None: every pack_panel call launches
BRANCH_STREAM = None    # a torch.cuda.Stream while a trainer step runs the background network next to the source / transfer streams


def pack_panel(w, transposed, kidx, cin, cin_pad, nout, n_pad):
    """Weight (D0,D1,KH,KW) on the device -> the fp32 GEMM panel [ceil32(ntaps*cin_pad)/4][n_pad][4] in one launch
    (csrc/train_ops.hip lwg_pack_panel_f32; see include/lwg_hip.h for the index convention)."""
    w = w.detach()
    assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
    D0, D1, KH, KW = w.shape
    kidx = tuple(int(k) for k in kidx)
    ntaps = len(kidx)
    Kp = (ntaps * cin_pad + 31) // 32 * 32
    if PANEL_CACHE is not None and PANEL_CACHE.cacheable(w):
        out, fresh = PANEL_CACHE.get(w, transposed, kidx, cin, cin_pad, nout, n_pad)
        if not fresh:
            return out
    else:
        out = torch.empty(Kp // 4, n_pad, 4, device=w.device, dtype=torch.float32)
    arr = (ctypes.c_int * ntaps)(*[int(k) for k in kidx])
    _lib.check(_lib.lib().lwg_pack_panel_f32(_ptr(w), D0, D1, KH, KW, 1 if transposed else 0, arr, ntaps, cin, cin_pad, nout, n_pad,
                                             _ptr(out), _stream()), "lwg_pack_panel_f32")
    return out


def unpack_wgrad(dwk, dw, transposed, kidx, cin, cin_pad, nout):
    """(ntaps*cin_pad, n_pad) weight gradient in kernel K order -> positions kidx of dw (D0,D1,KH,KW), in place."""
    D0, D1, KH, KW = dw.shape
    ntaps = len(kidx)
    assert dwk.is_contiguous() and dw.is_contiguous() and dwk.shape[0] == ntaps * cin_pad
    arr = (ctypes.c_int * ntaps)(*[int(k) for k in kidx])
    _lib.check(_lib.lib().lwg_unpack_wgrad_f32(_ptr(dwk), D0, D1, KH, KW, 1 if transposed else 0, arr, ntaps, cin, cin_pad, nout,
                                               dwk.shape[1], _ptr(dw), _stream()), "lwg_unpack_wgrad_f32")
    return dw


def maxpool2_fwd(x):
    """MaxPool2d(2, 2) on (B,H,W,C) NHWC."""
    B, H, W, C = x.shape
    y = torch.empty(B, H // 2, W // 2, C, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_maxpool2_fwd_nhwc_f32(_ptr(x), _ptr(y), B, H, W, C, _stream()), "lwg_maxpool2_fwd_nhwc_f32")
    return y


def maxpool2_bwd(x, dy):
    B, H, W, C = x.shape
    dx = torch.empty_like(x)
    _lib.check(_lib.lib().lwg_maxpool2_bwd_nhwc_f32(_ptr(x), _ptr(dy.contiguous()), _ptr(dx), B, H, W, C, _stream()), "lwg_maxpool2_bwd_nhwc_f32")
    return dx


def colsum(x2d_or_nhwc):
    """Sum over every dimension but the last (bias gradient)."""
    x = x2d_or_nhwc.contiguous()
    C = x.shape[-1]
    rows = x.numel() // C
    out = torch.empty(C, device=x.device, dtype=torch.float32)
    ws = torch.empty(512 * C, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().lwg_colsum_nhwc_f32(_ptr(x), rows, C, _ptr(out), _ptr(ws), _stream()), "lwg_colsum_nhwc_f32")
    return out


def act_bwd(dy, y, act):
    """dy * act'(y) for ReLU / LeakyReLU(0.2) / tanh / sigmoid outputs y."""
    dy, y = dy.contiguous(), y.contiguous()
    out = torch.empty_like(dy)
    _lib.check(_lib.lib().lwg_act_bwd_f32(_ptr(dy), _ptr(y), dy.numel(), act, _ptr(out), _stream()), "lwg_act_bwd_f32")
    return out


def crop_resize(x, box, out_hw, want_valid=True):
    """(N,C,H,W) fp32 NCHW, box (N,4) int64 device tensor (min_x, max_x, min_y, max_y) -> (crops (N,C,OH,OW), valid (N) fp32): the head crops of
    FaceLoss (faceloss.py:384-406) resized with bilinear / align_corners = True, the boxes never read by the host (lwg_crop_resize_bilinear_f32)."""
    N, C, H, W = x.shape
    OH, OW = out_hw
    x = x.contiguous()
    box = box.contiguous()
    y = x.new_empty(N, C, OH, OW)
    valid = x.new_empty(N) if want_valid else None
    _lib.check(_lib.lib().lwg_crop_resize_bilinear_f32(_ptr(x), _ptr(box, torch.int64), _ptr(y), _ptr(valid), N, C, H, W, OH, OW, _stream()),
               "lwg_crop_resize_bilinear_f32")
    return y, valid


def crop_resize_bwd(dy, box, in_hw):
    """Gradient of ``crop_resize`` with respect to the images: (N,C,OH,OW) -> (N,C,H,W)."""
    N, C, OH, OW = dy.shape
    H, W = in_hw
    dx = dy.new_zeros(N, C, H, W)
    _lib.check(_lib.lib().lwg_crop_resize_bilinear_bwd_f32(_ptr(dy.contiguous()), _ptr(box.contiguous(), torch.int64), _ptr(dx), N, C, H, W, OH, OW,
                                                           _stream()), "lwg_crop_resize_bilinear_bwd_f32")
    return dx


def prelu(x, slope, res=None):
    """(.., C) NHWC fp32, slope (C): res + PReLU(x) in one launch (lwg_prelu_f32; the frozen Sphere20a's activations and residual adds)."""
    x = x.contiguous()
    C = x.shape[-1]
    y = torch.empty_like(x)
    _lib.check(_lib.lib().lwg_prelu_f32(_ptr(x), _ptr(slope.contiguous()), None if res is None else _ptr(res.contiguous()), x.numel() // C, C, _ptr(y),
                                        _stream()), "lwg_prelu_f32")
    return y


def prelu_bwd(x, slope, dy):
    """dx of ``prelu`` (the slopes are frozen; the residual's gradient is dy)."""
    x, dy = x.contiguous(), dy.contiguous()
    C = x.shape[-1]
    dx = torch.empty_like(x)
    _lib.check(_lib.lib().lwg_prelu_bwd_f32(_ptr(x), _ptr(slope.contiguous()), _ptr(dy), x.numel() // C, C, _ptr(dx), _stream()), "lwg_prelu_bwd_f32")
    return dx


def _nsplit(hw):
    return max(1, min(64, hw // 64))


def _elem_ptr(t, off):
    """Device address of element ``off`` of a contiguous fp32 tensor (the beta / dbeta half of a fused gamma | beta tensor)."""
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


def norm_fwd(x, gamma=None, beta=None, act=ACT_NONE, eps=1e-5, gb=None):
    """y = act(InstanceNorm(x) * (1 + gamma) + beta) on NHWC -> (y, mean, rstd).
    gb: (B,H,W,2C) = gamma | beta as ONE tensor (the output of the fused mlp_gamma | mlp_beta convolution) instead of gamma, beta."""
    B, H, W, C = x.shape
    x = x.contiguous()
    mean, rstd = x.new_empty(B, C), x.new_empty(B, C)
    ns = _nsplit(H * W)
    instnorm_stats(x, mean, rstd, x.new_empty(B * C * ns * 3), eps=eps, nsplit=ns)
    y = torch.empty_like(x)
    if gb is not None:
        assert gamma is None and beta is None and gb.is_contiguous() and gb.shape == (B, H, W, 2 * C)
        gp, bp, gs = _ptr(gb), _elem_ptr(gb, C), 2 * C
    else:
        gp, bp, gs = _ptr(None if gamma is None else gamma.contiguous()), _ptr(None if beta is None else beta.contiguous()), 0
    _lib.check(_lib.lib().lwg_norm_fwd_nhwc_f32(_ptr(x), _ptr(mean), _ptr(rstd), gp, bp, gs, B, H * W, C, act, _ptr(y),
                                                 _stream()), "lwg_norm_fwd_nhwc_f32")
    return y, mean, rstd


def _nsplit_bwd(hw, B, C):
    """Splits of the reduction pass of norm_bwd: ~512 workgroups per launch (one training sample is B = 1: the statistics' 64 splits
    leave three quarters of the CUs idle), at least 32 pixels per split."""
    per_image = max(1, 512 // max(1, B * ((C // 4 + 63) // 64)))
    return max(1, min(per_image, hw // 32, 512))


def norm_bwd(dy, y, x, mean, rstd, gamma=None, act=ACT_NONE, gb=None):
    """Backward of norm_fwd -> (dx, dgamma, dbeta); with gb (the fused gamma | beta tensor) -> (dx, dgb (B,H,W,2C), None)."""
    B, H, W, C = x.shape
    dy = dy.contiguous()
    ns = _nsplit_bwd(H * W, B, C)
    dx = torch.empty_like(x)
    ws = x.new_empty(B * (ns + 1) * C * 2)          # the split records + their fold
    if gb is not None:
        dgb = torch.empty_like(gb)
        _lib.check(_lib.lib().lwg_norm_bwd_nhwc_f32(_ptr(dy), _ptr(y), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gb), 2 * C, B, H * W, C, act, ns,
                                                     _ptr(dx), _ptr(dgb), _elem_ptr(dgb, C), _ptr(ws), _stream()), "lwg_norm_bwd_nhwc_f32")
        return dx, dgb, None
    dg = torch.empty_like(x) if gamma is not None else None
    db = torch.empty_like(x) if gamma is not None else None
    _lib.check(_lib.lib().lwg_norm_bwd_nhwc_f32(_ptr(dy), _ptr(y), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), 0, B, H * W, C, act, ns,
                                                 _ptr(dx), _ptr(dg), _ptr(db), _ptr(ws), _stream()), "lwg_norm_bwd_nhwc_f32")
    return dx, dg, db


def adam_step_dev(p, g, m, v, lr, beta1, beta2, eps, t_dev):
    """In-place Adam update with the step count on the device: t_dev (1,) int32 is incremented, then used (graph-capturable)."""
    _lib.check(_lib.lib().lwg_adam_step_dev_f32(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, beta1, beta2, eps, _ptr(t_dev, torch.int32),
                                                _stream()), "lwg_adam_step_dev_f32")


def adam_step(p, g, m, v, lr, beta1, beta2, eps, t):
    """In-place Adam update of the flat fp32 buffers p, m, v with gradient g."""
    _lib.check(_lib.lib().lwg_adam_step_f32(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, beta1, beta2, eps, int(t), _stream()),
               "lwg_adam_step_f32")
