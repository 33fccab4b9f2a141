#!/usr/bin/env python3
"""A/B of the opt-in bf16-operand weight gradient (ops.wgrad_mode("bf16"), csrc/conv_wgrad_bf16.hip) against the direct kernel of the same
tree on the personalization step (BASELINE configs[4], 512 x 512), one process, one GPU:

  1. the weight-gradient launches of one eager step that the mode takes are enumerated by wrapping ops.conv2d_wgrad_unpacked
     (ops._wgrad_bf16_use decides; the transposed convolutions' one-launch adjoint form is among them);
  2. each distinct launch shape is timed with HIP events on seeded operands, lwg_conv2d_wgrad_unpacked_f32 and lwg_conv2d_wgrad_bf16_f32 (both
     with the fused bias gradient where the step has one) alternating A/B/A/B after a warm-up -> <out>/wgrad_bf16_layers.txt;
  3. the whole captured step is timed with TrainOpts.wgrad_precision "direct" and "bf16" in alternating blocks on ONE trainer, for the L1 step
     and for the default-loss step (VGG19 + face) -> <out>/wgrad_bf16_step_ab.txt.

    python tools/wgrad_bf16_ab.py [--size 512] [--reps 20] [--steps 10] [--blocks 3] [--out profiles]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def enumerate_launches(tr):
    """One eager default step -> {key: [launches per step, spec, kidx, dw shape]} of the launches the mode would take; key = (x0 shape, C1, dy H, W,
    N, ntaps, stride, cin, nout, bias)."""
    from ipercore_amd import ops
    seen = {}
    orig = ops.conv2d_wgrad_unpacked

    def spy(x0, spec, dy, dw, transposed, kidx, cin, nout, x1=None, out_hw=None, ycoff=0, db=None):
        if not transposed and out_hw is None and ycoff == 0 and ops._wgrad_bf16_use(x0, spec, dy, x1):
            key = (tuple(x0.shape), 0 if x1 is None else x1.shape[3], dy.shape[1], dy.shape[2], spec.N, spec.ntaps, spec.stride, cin, nout, db is not None)
            seen.setdefault(key, [0, spec, list(kidx), tuple(dw.shape)])[0] += 1
        return orig(x0, spec, dy, dw, transposed, kidx, cin, nout, x1=x1, out_hw=out_hw, ycoff=ycoff, db=db)

    graph = tr.opts.use_graph
    ops.conv2d_wgrad_unpacked, tr.opts.use_graph = spy, False
    try:
        tr.optimize_parameters()
        torch.cuda.synchronize()
    finally:
        ops.conv2d_wgrad_unpacked, tr.opts.use_graph = orig, graph
    return seen


def time_launch(key, spec, kidx, dwshape, reps, dev):
    from ipercore_amd import ops
    (B, H, W, C0), C1, OH, OW, N, _, _, cin, nout, bias = key
    g = torch.Generator(device="cpu").manual_seed(1)
    x0 = torch.randn(B, H, W, C0, generator=g).to(dev)
    x1 = torch.randn(B, H, W, C1, generator=g).to(dev) if C1 else None
    dy = torch.randn(B, OH, OW, N, generator=g).to(dev)
    dwa, dwb = torch.empty(dwshape, device=dev), torch.empty(dwshape, device=dev)
    db = torch.empty(nout, device=dev) if bias else None

    def direct():
        ops.conv2d_wgrad_unpacked(x0, spec, dy, dwa, False, kidx, cin, nout, x1=x1, db=db)

    def bf16():
        ops.conv2d_wgrad_bf16(x0, spec, dy, dwb, False, kidx, cin, nout, x1=x1, db=db)

    for _ in range(3):
        direct()
        bf16()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, acc in ((direct, ta), (bf16, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1) * 1e3)
    rel = float((dwb - dwa).norm() / dwa.norm())
    return statistics.median(ta), statistics.median(tb), min(ta), min(tb), rel


def time_steps(tr, mode, steps):
    tr.opts.wgrad_precision = mode
    tr._graphs = None                        # every block captures the step anew (the eager enumeration step left a graph of the default mode behind)
    for _ in range(2):                       # the first call captures the step
        tr.optimize_parameters()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        tr.optimize_parameters()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    import bench_personalize
    dev = torch.device("cuda", 0)
    os.makedirs(args.out, exist_ok=True)

    def trainer(use_vgg, use_face):
        hold = {}
        bench_personalize.measure(dev, steps=1, warmup=0, size=args.size, use_vgg=use_vgg, use_face=use_face, _keep=hold, _host_probe=False)
        return hold["trainer"]

    tr = trainer(False, False)
    seen = enumerate_launches(tr)
    lines = [f"# tools/wgrad_bf16_ab.py --size {args.size} --reps {args.reps}: the weight-gradient launches of one personalization step (L1) that the bf16 mode takes,",
             "# direct = lwg_conv2d_wgrad_unpacked_f32, bf16 = lwg_conv2d_wgrad_bf16_f32, both with the fused bias gradient where the step has one;",
             "# median us of --reps event-timed launches each, alternating A/B/A/B in one process after a warm-up; ratio = bf16 / direct (< 1: faster);",
             "# relL2 = |bf16 - direct| / |direct| of the two results on the timed operands (randn)",
             f"# {'x B x H x W':>14s} {'C0+C1':>9s} {'dy HxW':>9s} {'N':>5s} taps s {'cin':>4s} {'nout':>4s} bias  n/step  direct_us    bf16_us  ratio   min_d   min_b    relL2"]
    tot_a = tot_b = 0.0
    for key in sorted(seen, key=lambda k: (-k[0][1] * k[0][2], k[5], k[0][3] + k[1], k[4])):
        n, spec, kidx, dwshape = seen[key]
        a, b, ma, mb, rel = time_launch(key, spec, kidx, dwshape, args.reps, dev)
        tot_a, tot_b = tot_a + n * a, tot_b + n * b
        (B, H, W, C0), C1, OH, OW, N, ntaps, stride, cin, nout, bias = key
        lines.append(f"  {f'{B}x{H}x{W}':>14s} {f'{C0}+{C1}':>9s} {f'{OH}x{OW}':>9s} {N:5d} {ntaps:4d} {stride:1d} {cin:4d} {nout:4d} {int(bias):4d} {n:7d} "
                     f"{a:10.1f} {b:10.1f} {b / a:6.2f} {ma:7.1f} {mb:7.1f} {rel:8.2e}")
    lines.append(f"# per step, launches x median: direct {tot_a / 1e3:.3f} ms, bf16 {tot_b / 1e3:.3f} ms, ratio {tot_b / max(tot_a, 1e-9):.3f} over "
                 f"{sum(v[0] for v in seen.values())} launches of {len(seen)} shapes")
    with open(os.path.join(args.out, "wgrad_bf16_layers.txt"), "w") as fp:
        fp.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)

    out = [f"# tools/wgrad_bf16_ab.py --size {args.size} --steps {args.steps} --blocks {args.blocks}: the whole captured personalization step on ONE trainer per loss set,",
           "# TrainOpts.wgrad_precision alternating in blocks (the step is re-captured at each switch, two untimed steps first); ms per step"]
    for name, vgg, face in (("L1", False, False), ("VGG19 + face", True, True)):
        if vgg:
            del tr
            torch.cuda.empty_cache()
            tr = trainer(vgg, face)
        rows = []
        for blk in range(args.blocks):
            for mode in ("direct", "bf16"):
                rows.append((blk, mode, time_steps(tr, mode, args.steps), tr.step_mode))
        tr.opts.wgrad_precision = "direct"
        out.append(f"# losses: {name}")
        for blk, mode, ms, sm in rows:
            out.append(f"  block {blk} {mode:7s} {ms:8.3f} ms   [{sm}]")
        da, ba = [r[2] for r in rows if r[1] == "direct"], [r[2] for r in rows if r[1] == "bf16"]
        md, mb = statistics.median(da), statistics.median(ba)
        out.append(f"# {name}: median direct {md:.3f} ms (min {min(da):.3f}, max {max(da):.3f}), bf16 {mb:.3f} ms (min {min(ba):.3f}, max {max(ba):.3f}), ratio {mb / md:.4f}")
        with open(os.path.join(args.out, "wgrad_bf16_step_ab.txt"), "w") as fp:
            fp.write("\n".join(out) + "\n")
    print("\n".join(out), flush=True)


if __name__ == "__main__":
    main()
