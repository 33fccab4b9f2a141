#!/usr/bin/env python3
"""A/B of the opt-in F(4x4, 3x3) Winograd forward / data gradient of the training step (TrainOpts.conv_tiles = "4x4", ops.train_conv_tiles,
csrc/conv_winograd4.hip's split-K form) against the step as it stands ("2x2") on the personalization step (BASELINE configs[4],
512 x 512), one process, one GPU:

  1. the training launches (ops.conv2d, splitk=True) of one eager default step that the mode could take - ops._wino_eligible and
     Cin >= ops.WINO4_MIN_CIN - are enumerated with the kind ops.CONV_HOOK reports for each (what the parent runs: "winograd" whole / split, or
     "direct"): G, D and the frozen loss networks, forward and data gradient;
  2. each distinct launch shape is timed with HIP events on seeded operands three ways, interleaved A/B/C/A/B/C after a warm-up: the parent's
     choice (ops.conv2d under "2x2"), F(4x4) whole (lwg_conv2d_winograd4_f32) and F(4x4) split over K (lwg_conv2d_winograd4_f32_ws, where the
     library's plan splits the launch at all), plus the form ops._wino4_plan picks -> profiles/train_conv_tiles_layers.txt;
  3. the whole captured step is timed with TrainOpts.conv_tiles "2x2" and "4x4" in alternating blocks on ONE trainer per loss set (L1; the default
     set L1 + VGG19 + face) -> profiles/train_conv_tiles_step_ab.txt.

    python tools/train_conv_tiles_ab.py [--size 512] [--reps 20] [--steps 10] [--blocks 3] [--no-layers] [--no-steps] [--lab] [--min-grid G] [--min-slice-cin C] [--out profiles]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def enumerate_launches(tr):
    """One eager default step -> {(B, H, W, C0, C1, N, epi, act, bias): [launches per step, the parent's kind, kernels]}."""
    from ipercore_amd import ops
    seen, cur = {}, []
    orig, prev_hook = ops.conv2d, ops.CONV_HOOK

    def spy(x0, spec, y, x1=None, epi=ops.EPI_NONE, act=ops.ACT_NONE, res=None, xn=None, mean=None, rstd=None, out_hw=None, ycoff=0, splitk=False,
            q4=False, lists=None):
        key = None
        if splitk and x0.is_cuda and ops._wino_eligible(spec, x0, y, x1, epi, act, out_hw, q4, ycoff) and spec.Cin >= ops.WINO4_MIN_CIN:
            key = (x0.shape[0], x0.shape[1], x0.shape[2], x0.shape[3], 0 if x1 is None else x1.shape[3], spec.N, epi, act, spec.bias is not None)
        cur.append(key)
        try:
            return orig(x0, spec, y, x1=x1, epi=epi, act=act, res=res, xn=xn, mean=mean, rstd=rstd, out_hw=out_hw, ycoff=ycoff, splitk=splitk, q4=q4,
                        lists=lists)
        finally:
            cur.pop()

    def hook(begin, M, spec, epi=0, info=None):
        if not begin and cur and cur[-1] is not None:
            e = seen.setdefault(cur[-1], [0, info["kind"], info["kernels"]])
            e[0] += 1

    graph = tr.opts.use_graph
    ops.conv2d, ops.CONV_HOOK, tr.opts.use_graph = spy, hook, False
    try:
        tr.optimize_parameters()
        torch.cuda.synchronize()
    finally:
        ops.conv2d, ops.CONV_HOOK, tr.opts.use_graph = orig, prev_hook, graph
    return seen


def time_launch(key, reps, dev, inner=8):
    """-> {"parent" | "whole" | "split": (median us, min us)} ("split": None where the library's plan does not split the launch), the parent's kind as
    re-derived here, the K slices, and what ops._wino4_plan picks.  Every form is timed as the bare library calls ops.conv2d would make for it (panels,
    workspace and arguments prepared beforehand), `inner` launches back to back per event pair: the kernels of these shapes take 20 - 150 us, less
    than the Python path around them, and a pair of events around one ops.conv2d call times the host."""
    from ipercore_amd import _lib, ops
    from ipercore_amd.networks import packing
    B, H, W, C0, C1, N, epi, act, bias = key
    g = torch.Generator(device="cpu").manual_seed(1)
    w = torch.randn(N, C0 + C1, 3, 3, generator=g) * 0.05
    spec = packing.spec_to(packing.pack_conv(w, torch.randn(N, generator=g) * 0.1 if bias else None, stride=1, pad=1), dev)
    x0 = torch.randn(B, H, W, C0, generator=g).to(dev)
    x1 = torch.randn(B, H, W, C1, generator=g).to(dev) if C1 else None
    res = torch.randn(B, H, W, N, generator=g).to(dev) if epi == ops.EPI_RESIDUAL else None
    y = torch.empty(B, H, W, N, device=dev)
    kw = dict(x1=x1, epi=epi, act=act, res=res)
    L = _lib.lib()
    st = ops._stream()

    def args(panel):
        a = ops.conv_args(x0, spec, y, **kw)
        if panel is not None:
            a.w = ops._ptr(panel)
        return a

    # the parent's choice, as ops.conv2d makes it under train_conv_tiles("2x2")
    with ops.conv_precision("winograd"), ops.train_conv_tiles("2x2"):
        a0 = args(None)
        n2 = ops._wino_plan(a0, spec, y, True)
    if n2 is None:
        nd = L.lwg_conv2d_ws_floats(a0)
        wsd = torch.empty(max(nd, 1), device=dev)
        kind = "direct,1"                    # (the hook does not count the direct kernel's finishing launch)
        parent = (lambda: L.lwg_conv2d_nhwc_f32_ws(a0, wsd.data_ptr(), st)) if nd else (lambda: L.lwg_conv2d_nhwc_f32(a0, st))
    else:
        a2 = args(ops._wwino(spec))
        ws2 = torch.empty(max(n2, 1), device=dev)
        kind = "winograd," + ("2" if n2 else "1")
        parent = (lambda: L.lwg_conv2d_winograd_f32_ws(a2, ws2.data_ptr(), st)) if n2 else (lambda: L.lwg_conv2d_winograd_f32(a2, st))
    a4 = args(ops._wwino4(spec))
    nws = L.lwg_conv2d_winograd4_ws_floats(a4)
    ws4 = torch.empty(max(nws, 1), device=dev)
    fns = {"parent": parent, "whole": lambda: L.lwg_conv2d_winograd4_f32(a4, st)}
    if nws:
        fns["split"] = lambda: L.lwg_conv2d_winograd4_f32_ws(a4, ws4.data_ptr(), st)
    for _ in range(3):
        for k, fn in fns.items():
            _lib.check(fn(), k)
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    out = {k: (statistics.median(v), min(v)) for k, v in t.items()}
    out.setdefault("split", None)
    with ops.train_conv_tiles("4x4"):
        n4 = ops._wino4_plan(args(None)) if ops._wino4_use(spec, True) else None
    return out, kind, int(nws // (a4.M * a4.N)), "parent" if n4 is None else "split" if n4 else "whole"


def time_steps(tr, tiles, steps):
    tr.opts.conv_tiles = tiles
    tr._graphs = None                        # every block captures the step anew (the trainer drops the other mode's fragment panels at the switch)
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


EPI = {0: "none", 1: "res", 2: "spade"}
ACT = {0: "-", 1: "relu", 2: "tanh", 3: "sigm", 4: "lrelu", 5: "mask"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--no-layers", dest="layers", action="store_false")
    ap.add_argument("--no-steps", dest="step_ab", action="store_false")
    ap.add_argument("--min-grid", type=int, default=None, help="lab: ops.WINO4_TRAIN_MIN_GRID for the run")
    ap.add_argument("--min-slice-cin", type=int, default=None, help="lab: ops.WINO4_TRAIN_MIN_SLICE_CIN for the run")
    ap.add_argument("--lab", action="store_true", help="the L1 step A/B besides with the whole-K launches only and with the split launches only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    import bench_personalize
    from ipercore_amd import ops
    dev = torch.device("cuda", 0)
    os.makedirs(args.out, exist_ok=True)
    if args.min_grid is not None:
        ops.WINO4_TRAIN_MIN_GRID = args.min_grid
    if args.min_slice_cin is not None:
        ops.WINO4_TRAIN_MIN_SLICE_CIN = args.min_slice_cin
    trainers = {}
    for name, vgg, face in (("L1", False, False), ("L1 + VGG19 + face", True, True)):
        hold = {}
        bench_personalize.measure(dev, steps=1, warmup=0, size=args.size, use_vgg=vgg, use_face=face, _keep=hold, _host_probe=False)
        trainers[name] = hold["trainer"]

    if args.layers:
        seen = enumerate_launches(trainers["L1 + VGG19 + face"])
        lines = [f"# tools/train_conv_tiles_ab.py --size {args.size} --reps {args.reps}: the training launches (forward and data gradient; G, D, VGG19, Sphere20a) of one",
                 "# personalization step (L1 + VGG19 + face) that are ops._wino_eligible with Cin >= ops.WINO4_MIN_CIN.  parent = what the step runs today (kind / kernels",
                 "# as ops.CONV_HOOK reports them), whole = lwg_conv2d_winograd4_f32, split = lwg_conv2d_winograd4_f32_ws (sl = its K slices; - = the library's plan",
                 "# does not split the launch), plan-> = the form ops._wino4_plan takes under train_conv_tiles(\"4x4\").  Every form as the bare library calls behind",
                 "# ops.conv2d, 8 launches back to back per event pair; median us per launch of --reps such measurements each, interleaved in one process after a",
                 "# warm-up (min in brackets); w/p, s/p = whole / parent, split / parent (< 1: faster)",
                 f"# WINO4_TRAIN_MIN_GRID = {ops.WINO4_TRAIN_MIN_GRID}, WINO4_TRAIN_MIN_SLICE_CIN = {ops.WINO4_TRAIN_MIN_SLICE_CIN}, WINO_MIN_GRID = {ops.WINO_MIN_GRID}",
                 f"# {'B x H x W':>12s} {'C0+C1':>8s} {'N':>4s} {'epi':>5s} {'act':>5s} n/step  parent(kind,k)        parent_us         whole_us   sl         split_us   w/p   s/p  plan->"]
        tot = {"parent": 0.0, "plan": 0.0, "best": 0.0}
        for key in sorted(seen, key=lambda k: (-k[0] * k[1] * k[2], k[3] + k[4], k[5], k[6], k[7])):
            t, kind2, sl, pick = time_launch(key, args.reps, dev)
            n, kind, kern = seen[key]
            assert kind2 == f"{kind},{kern}", (key, kind2, kind, kern)      # the form timed as "parent" is the one the step ran
            B, H, W, C0, C1, N, epi, act, bias = key
            p, wh, sp = t["parent"], t["whole"], t["split"]
            tot["parent"] += n * p[0]
            tot["plan"] += n * t[pick][0]
            tot["best"] += n * min(p[0], wh[0], sp[0] if sp else 1e30)
            fmt = lambda v: f"{v[0]:8.1f} ({v[1]:7.1f})" if v else f"{'-':>8s} {'':9s}"      # noqa: E731
            lines.append(f"  {f'{B}x{H}x{W}':>12s} {f'{C0}+{C1}':>8s} {N:4d} {EPI[epi]:>5s} {ACT[act]:>5s} {n:6d}  {kind2:<14s} {fmt(p)} {fmt(wh)} {sl:4d} {fmt(sp)} "
                         f"{wh[0] / p[0]:5.2f} {(sp[0] / p[0] if sp else float('nan')):5.2f}  {pick:<6s}")
        lines.append(f"# per step, launches x median: parent {tot['parent'] / 1e3:.3f} ms, plan {tot['plan'] / 1e3:.3f} ms, best form per shape {tot['best'] / 1e3:.3f} ms "
                     f"over {sum(v[0] for v in seen.values())} launches of {len(seen)} shapes")
        with open(os.path.join(args.out, "train_conv_tiles_layers.txt"), "w") as fp:
            fp.write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)

    if args.step_ab:
        out = [f"# tools/train_conv_tiles_ab.py --size {args.size} --steps {args.steps} --blocks {args.blocks}: the whole captured personalization step on ONE trainer per loss",
               "# set, TrainOpts.conv_tiles alternating in blocks (the step is re-captured at each switch, two untimed steps first); ms per step",
               f"# WINO4_TRAIN_MIN_GRID = {ops.WINO4_TRAIN_MIN_GRID}, WINO4_TRAIN_MIN_SLICE_CIN = {ops.WINO4_TRAIN_MIN_SLICE_CIN}"]
        runs = [(name, tr, True, True) for name, tr in trainers.items()]
        if args.lab:
            runs += [("L1, whole-K launches only", trainers["L1"], True, False), ("L1, split launches only", trainers["L1"], False, True)]
        for name, tr, whole, split in runs:
            ops.WINO4_TRAIN_WHOLE, ops.WINO4_TRAIN_SPLITK = whole, split
            rows = []
            for blk in range(args.blocks):
                for tiles in ("2x2", "4x4"):
                    rows.append((blk, tiles, time_steps(tr, tiles, args.steps), tr.step_mode))
            tr.opts.conv_tiles = "2x2"
            for blk, tiles, ms, sm in rows:
                out.append(f"  [{name}] block {blk} {tiles} {ms:8.3f} ms   [{sm}]")
            m2 = statistics.median(r[2] for r in rows if r[1] == "2x2")
            m4 = statistics.median(r[2] for r in rows if r[1] == "4x4")
            out.append(f"# [{name}] median: 2x2 {m2:.3f} ms, 4x4 {m4:.3f} ms, ratio {m4 / m2:.4f}")
        ops.WINO4_TRAIN_WHOLE = ops.WINO4_TRAIN_SPLITK = True
        with open(os.path.join(args.out, "train_conv_tiles_step_ab.txt"), "w") as fp:
            fp.write("\n".join(out) + "\n")
        print("\n".join(out), flush=True)


if __name__ == "__main__":
    main()
