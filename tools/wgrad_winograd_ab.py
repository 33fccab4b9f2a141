#!/usr/bin/env python3
"""A/B of the opt-in F(2x2, 3x3) Winograd weight gradient (ops.wgrad_precision("winograd"), csrc/conv_wgrad_winograd.hip) against the direct
kernel of the same tree on the personalization step (BASELINE configs[4], 512 x 512), one process, one GPU:

  1. the eligible weight-gradient launches of one eager step are enumerated by wrapping ops.conv2d_wgrad_unpacked (ops._wgrad_wino_use decides);
  2. each distinct launch shape is timed with HIP events on seeded operands, lwg_conv2d_wgrad_unpacked_f32 (with its fused bias gradient, what
     the step runs) and lwg_conv2d_wgrad_winograd_f32 + ops.colsum (what the mode runs instead) alternating A/B/A/B after a warm-up
     -> profiles/wgrad_winograd_layers.txt;
  3. the whole captured step is timed with TrainOpts.wgrad_precision "direct" and "winograd" in alternating blocks on ONE trainer
     -> profiles/wgrad_winograd_step_ab.txt.

    python tools/wgrad_winograd_ab.py [--size 512] [--reps 20] [--steps 10] [--blocks 3] [--use-vgg] [--use-face] [--out profiles]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def enumerate_launches(tr):
    """One eager default step -> {(B, H, W, C0, C1, N, cin, nout, bias): launches per step} of the launches the new mode would take."""
    from ipercore_amd import ops
    seen = {}
    orig = ops.conv2d_wgrad_unpacked

    def spy(x0, spec, dy, dw, transposed, kidx, cin, nout, x1=None, out_hw=None, ycoff=0, db=None):
        if not transposed and len(list(kidx)) == 9 and out_hw is None and ycoff == 0 and ops._wgrad_wino_use(x0, spec, dy, x1):
            key = (x0.shape[0], x0.shape[1], x0.shape[2], x0.shape[3], 0 if x1 is None else x1.shape[3], spec.N, cin, nout, db is not None)
            seen[key] = seen.get(key, 0) + 1
        return orig(x0, spec, dy, dw, transposed, kidx, cin, nout, x1=x1, out_hw=out_hw, ycoff=ycoff, db=db)

    graph = tr.opts.use_graph
    ops.conv2d_wgrad_unpacked, tr.opts.use_graph = spy, False
    try:
        tr.optimize_parameters()
        torch.cuda.synchronize()
    finally:
        ops.conv2d_wgrad_unpacked, tr.opts.use_graph = orig, graph
    return seen


def time_launch(key, reps, dev):
    from ipercore_amd import ops
    from ipercore_amd.networks import packing
    B, H, W, C0, C1, N, cin, nout, bias = key
    g = torch.Generator(device="cpu").manual_seed(1)
    w = torch.randn(nout, cin, 3, 3, generator=g) * 0.05
    spec = packing.spec_to(packing.pack_conv(w, None, stride=1, pad=1, cin_pad=C0 + C1, n_pad=N), dev)
    x0 = torch.randn(B, H, W, C0, generator=g).to(dev)
    x1 = torch.randn(B, H, W, C1, generator=g).to(dev) if C1 else None
    dy = torch.randn(B, H, W, N, generator=g).to(dev)
    dwa, dwb = torch.empty(nout, cin, 3, 3, device=dev), torch.empty(nout, cin, 3, 3, device=dev)
    db = torch.empty(nout, device=dev) if bias else None

    def direct():
        ops.conv2d_wgrad_unpacked(x0, spec, dy, dwa, False, range(9), cin, nout, x1=x1, db=db)

    def wino():
        ops.conv2d_wgrad_winograd(x0, spec, dy, dwb, cin, nout, x1=x1)
        if bias:
            ops.colsum(dy)

    for _ in range(3):
        direct()
        wino()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, acc in ((direct, ta), (wino, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ta), statistics.median(tb), min(ta), min(tb)


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
    ap.add_argument("--use-vgg", action="store_true")
    ap.add_argument("--use-face", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    import bench_personalize
    dev = torch.device("cuda", 0)
    hold = {}
    bench_personalize.measure(dev, steps=1, warmup=0, size=args.size, use_vgg=args.use_vgg, use_face=args.use_face, _keep=hold, _host_probe=False)
    tr = hold["trainer"]
    losses = "L1" + (" + VGG19" if args.use_vgg else "") + (" + face" if args.use_face else "")
    os.makedirs(args.out, exist_ok=True)

    seen = enumerate_launches(tr)
    lines = [f"# tools/wgrad_winograd_ab.py --size {args.size} --reps {args.reps}: the eligible weight-gradient launches of one personalization step ({losses}),",
             "# direct = lwg_conv2d_wgrad_unpacked_f32 (fused bias gradient where the step has one), winograd = lwg_conv2d_wgrad_winograd_f32 (+ colsum there);",
             "# median us of --reps event-timed launches each, alternating A/B/A/B in one process after a warm-up; ratio = winograd / direct (< 1: faster)",
             f"# {'B x H x W':>14s} {'C0+C1':>9s} {'N':>5s} {'cin':>4s} {'nout':>4s} bias  n/step  direct_us  winograd_us  ratio   min_d   min_w"]
    tot_a = tot_b = 0.0
    for key in sorted(seen, key=lambda k: (-k[1] * k[2], k[3] + k[4], k[5])):
        a, b, ma, mb = time_launch(key, args.reps, dev)
        n = seen[key]
        tot_a, tot_b = tot_a + n * a, tot_b + n * b
        B, H, W, C0, C1, N, cin, nout, bias = key
        lines.append(f"  {f'{B}x{H}x{W}':>14s} {f'{C0}+{C1}':>9s} {N:5d} {cin:4d} {nout:4d} {int(bias):4d} {n:7d} {a:10.1f} {b:12.1f} {b / a:6.2f} {ma:7.1f} {mb:7.1f}")
    lines.append(f"# per step, launches x median: direct {tot_a / 1e3:.3f} ms, winograd {tot_b / 1e3:.3f} ms, ratio {tot_b / max(tot_a, 1e-9):.3f} over {sum(seen.values())} launches")
    with open(os.path.join(args.out, "wgrad_winograd_layers.txt"), "w") as fp:
        fp.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)

    rows = []
    for blk in range(args.blocks):
        for mode in ("direct", "winograd"):
            rows.append((blk, mode, time_steps(tr, mode, args.steps), tr.step_mode))
    tr.opts.wgrad_precision = "direct"
    out = [f"# tools/wgrad_winograd_ab.py --size {args.size} --steps {args.steps} --blocks {args.blocks}: the whole personalization step ({losses}) on ONE trainer,",
           "# TrainOpts.wgrad_precision alternating in blocks (the step is re-captured at each switch, two untimed steps first); ms per step"]
    for blk, mode, ms, sm in rows:
        out.append(f"  block {blk} {mode:9s} {ms:8.3f} ms   [{sm}]")
    md = statistics.median(r[2] for r in rows if r[1] == "direct")
    mw = statistics.median(r[2] for r in rows if r[1] == "winograd")
    out.append(f"# median: direct {md:.3f} ms, winograd {mw:.3f} ms, ratio {mw / md:.4f}")
    with open(os.path.join(args.out, "wgrad_winograd_step_ab.txt"), "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("\n".join(out), flush=True)


if __name__ == "__main__":
    main()
