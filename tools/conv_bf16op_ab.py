#!/usr/bin/env python3
"""A/B of the opt-in bf16-operand forward / data-gradient convolutions (ops.conv_precision("bf16_operands"), csrc/conv_igemm_bf16op.hip) against
the default mode of the same tree on the personalization step (BASELINE configs[4]), one GPU.  Three parts, each a child process under its own
time limit, chained: the driver stops at the first part that fails.

  layers  every distinct launch of one eager 512^2 step (L1) that the mode takes (ops._bf16op_use decides; forward and data gradient), timed with
          HIP events on seeded operands as the step makes it - an ops.conv2d call, or an ops.conv_transpose2d call with its four parity launches,
          which the default mode may run as one grid -: the route the default mode ("winograd", conv_tiles "2x2") gives that call and the new
          mode, alternating A/B/A/B after a warm-up -> <out>/conv_bf16op_layers.txt;
  step    the whole captured step on ONE trainer per loss set, (conv_precision, wgrad_precision) = ("winograd", "direct"), ("winograd", "bf16"),
          ("bf16_operands", "bf16") alternating in blocks -> <out>/conv_bf16op_step_ab.txt;
  effect  50 steps at S = 64 from one seed in the default mode and in ("bf16_operands", "bf16"): the losses side by side, and the relative L2 of
          every parameter's first-step gradient against the "fp32" mode -> <out>/conv_bf16op_effect.txt.

    python tools/conv_bf16op_ab.py [--part all|layers|step|effect] [--size 512] [--reps 20] [--steps 10] [--blocks 3] [--out profiles]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

MODE = "bf16_operands"
LIMITS = {"layers": 420, "step": 420, "effect": 300}          # seconds per part


def _trainer512(size, use_vgg, use_face):
    import bench_personalize
    hold = {}
    bench_personalize.measure(torch.device("cuda", 0), steps=1, warmup=0, size=size, use_vgg=use_vgg, use_face=use_face, _keep=hold, _host_probe=False)
    return hold["trainer"]


def enumerate_launches(tr):
    """One eager step in the mode -> (singles, groups) of the launches the new kernel takes, as the step makes them:
    singles {key: [calls per step, spec, x1 channels, y shape, out_hw, ycoff]} - ops.conv2d calls, keyed by what defines the launch shape (an output
    slice of a wider tensor, or a bias, does not: such calls share a row); groups {key: [calls per step, specs, out_hw per spec]} -
    ops.conv_transpose2d calls (a transposed convolution's forward, a 4x4 / stride-2 convolution's data gradient), whose four parity launches the
    mode runs as four conv2d calls where the default mode may run ONE grid (lwg_conv_transpose4_nhwc_f32): timed as a whole; excluded: the same
    for the groups that ops._bf16op_use_parity4 leaves on the default's one-grid form."""
    from ipercore_amd import ops
    singles, groups, excluded, orig, orig_t, inside = {}, {}, {}, ops.conv2d, ops.conv_transpose2d, [0]

    def spy(x0, spec, y, x1=None, epi=ops.EPI_NONE, act=ops.ACT_NONE, res=None, xn=None, mean=None, rstd=None, out_hw=None, ycoff=0, splitk=False,
            q4=False, lists=None):
        if not inside[0] and ops.CONV_PRECISION == MODE and ops._bf16op_use(spec, x0, y, x1, epi, act, q4, ycoff):
            OH, OW = (y.shape[1] // spec.omul, y.shape[2] // spec.omul) if out_hw is None else tuple(out_hw)
            key = (tuple(x0.shape), 0 if x1 is None else x1.shape[3], (OH, OW), spec.N, spec.ntaps, spec.stride, spec.omul, epi, act, bool(splitk))
            singles.setdefault(key, [0, spec, tuple(y.shape), None if out_hw is None else tuple(out_hw), ycoff])[0] += 1
        return orig(x0, spec, y, x1=x1, epi=epi, act=act, res=res, xn=xn, mean=mean, rstd=rstd, out_hw=out_hw, ycoff=ycoff, splitk=splitk, q4=q4,
                    lists=lists)

    def spy_t(x, specs, y, act=ops.ACT_NONE, splitk=False, out_hw=None, q4=False):
        elig = ops.CONV_PRECISION == MODE and all(ops._bf16op_use(s, x, y, None, ops.EPI_NONE, act, q4) for s in specs)
        take = elig and ops._bf16op_use_parity4(specs, x, y, act, splitk, out_hw, q4)
        if elig:            # (a group the rule of ops._bf16op_use_parity4 leaves on the one-grid form is listed apart)
            hws = None if out_hw is None else tuple(tuple(out_hw(s)) for s in specs)
            key = (tuple(x.shape), tuple(y.shape), specs[0].N, specs[0].ntaps, act, bool(splitk), hws)
            (groups if take else excluded).setdefault(key, [0, specs])[0] += 1
        inside[0] += take
        try:
            return orig_t(x, specs, y, act=act, splitk=splitk, out_hw=out_hw, q4=q4)
        finally:
            inside[0] -= take

    graph, prec = tr.opts.use_graph, tr.opts.conv_precision
    ops.conv2d, ops.conv_transpose2d, tr.opts.use_graph, tr.opts.conv_precision = spy, spy_t, False, MODE
    try:
        tr.optimize_parameters()
        torch.cuda.synchronize()
    finally:
        ops.conv2d, ops.conv_transpose2d, tr.opts.use_graph, tr.opts.conv_precision = orig, orig_t, graph, prec
    return singles, groups, excluded


def time_ab(run, ya, yb, reps):
    """run(mode, y) in the default mode and in the new one, alternating -> (median a, median b, min a, min b, relL2, default kinds, bf16op launches)."""
    from ipercore_amd import ops
    kinds = {"winograd": [], MODE: []}

    def hook(begin, M, spec_, epi_=0, info=None):
        if not begin:
            kinds[ops.CONV_PRECISION].append((info["kind"], info["kernels"]))

    prev, ops.CONV_HOOK = ops.CONV_HOOK, hook
    try:
        run("winograd", ya)
        run(MODE, yb)
    finally:
        ops.CONV_HOOK = prev
    for _ in range(3):
        run("winograd", ya)
        run(MODE, yb)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for mode, y, acc in (("winograd", ya, ta), (MODE, yb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(mode, y)
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1) * 1e3)
    rel = float((yb - ya).norm() / ya.norm().clamp_min(1e-30))
    kd = kinds["winograd"]
    kind = (kd[0][0] if len(kd) == 1 else f"{len(kd)}x{kd[0][0]}") if kd else "?"
    return statistics.median(ta), statistics.median(tb), min(ta), min(tb), rel, kind, sum(k[1] for k in kinds[MODE])


def time_launch(key, rec, reps, dev):
    from ipercore_amd import ops
    xs, C1, _, N, ntaps, stride, omul, epi, act, splitk = key
    _, spec, ys, out_hw, ycoff = rec
    g = torch.Generator(device="cpu").manual_seed(1)
    x0 = torch.randn(xs, generator=g).to(dev)
    x1 = torch.randn(xs[:3] + (C1,), generator=g).to(dev) if C1 else None
    res = torch.randn(ys, generator=g).to(dev) if epi == ops.EPI_RESIDUAL else None
    ya, yb = torch.zeros(ys, device=dev), torch.zeros(ys, device=dev)

    def run(mode, y):
        with ops.conv_precision(mode):
            ops.conv2d(x0, spec, y, x1=x1, epi=epi, act=act, res=res, out_hw=out_hw, ycoff=ycoff, splitk=splitk)

    return time_ab(run, ya, yb, reps)


def time_group(key, rec, reps, dev, whole=False):
    """whole (the excluded groups): the new mode's side is the four parity launches on the new kernel WITHOUT split-K (splitk=False in the mode) -
    what the rule's alternative, "do not split such groups", would run."""
    from ipercore_amd import ops
    xs, ys, N, ntaps, act, splitk, hws = key
    specs = rec[1]
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(xs, generator=g).to(dev)
    ya, yb = torch.zeros(ys, device=dev), torch.zeros(ys, device=dev)
    cb = None if hws is None else (lambda s: hws[[id(q) for q in specs].index(id(s))])

    def run(mode, y):
        with ops.conv_precision(mode):
            ops.conv_transpose2d(x, specs, y, act=act, splitk=splitk and not (whole and mode == MODE), out_hw=cb)

    return time_ab(run, ya, yb, reps)


def part_layers(args):
    dev = torch.device("cuda", 0)
    tr = _trainer512(args.size, False, False)
    singles, groups, excluded = enumerate_launches(tr)
    lines = [f"# tools/conv_bf16op_ab.py --part layers --size {args.size} --reps {args.reps}: the forward / data-gradient launches of one personalization step (L1)",
             "# that the \"bf16_operands\" mode takes, each timed AS THE STEP MAKES IT: default = the route of the default mode (\"winograd\", conv_tiles \"2x2\") for the",
             "# same call, bf16op = the new mode for it; median us of --reps event-timed calls each, alternating A/B/A/B in one process after a warm-up (a call's",
             "# host time rides along on both sides); ratio = bf16op / default (< 1: faster); kind = the default route's kernel family (CONV_HOOK), nk = the kernels",
             "# behind the bf16op call (split-K adds a finishing kernel per launch); relL2 = |bf16op - default| / |default| on the timed operands (randn: ~2.3e-3).",
             "# Rows are distinct launch shapes: calls that differ only in the output slice (ycoff / YC) or in having a bias share a row (n/step counts them all).",
             "#",
             "# (1) ops.conv2d calls - one launch each (a stride-2 data gradient at an odd size comes here as four calls with om = 2)",
             f"# {'x B x H x W':>13s} {'C0+C1':>8s} {'OHxOW':>9s} {'N':>4s} taps s om epi act sk  n/step  {'kind':>10s} nk default_us  bf16op_us  ratio   min_d   min_b    relL2"]
    tot = {"s": [0.0, 0.0], "g": [0.0, 0.0]}
    lose = []
    for key in sorted(singles, key=lambda k: (-k[0][1] * k[0][2], k[4], k[0][3] + k[1], k[3], k[6], k[7], k[8], k[2])):
        rec = singles[key]
        a, b, ma, mb, rel, kind, nk = time_launch(key, rec, args.reps, dev)
        tot["s"][0] += rec[0] * a
        tot["s"][1] += rec[0] * b
        (B, H, W, C0), C1 = key[0], key[1]
        row = (f"  {f'{B}x{H}x{W}':>13s} {f'{C0}+{C1}':>8s} {f'{key[2][0]}x{key[2][1]}':>9s} {key[3]:4d} {key[4]:4d} {key[5]:1d} {key[6]:2d} {key[7]:3d} {key[8]:3d} "
               f"{int(key[9]):2d} {rec[0]:7d}  {kind:>10s} {nk:2d} {a:10.1f} {b:10.1f} {b / a:6.2f} {ma:7.1f} {mb:7.1f} {rel:8.2e}")
        lines.append(row)
        if b > a:
            lose.append(row)
    ns = sum(v[0] for v in singles.values())
    lines.append(f"# (1) per step, calls x median: default {tot['s'][0] / 1e3:.3f} ms, bf16op {tot['s'][1] / 1e3:.3f} ms, ratio {tot['s'][1] / max(tot['s'][0], 1e-9):.3f} "
                 f"over {ns} calls of {len(singles)} shapes; slower than the default route: {len(lose)} of {len(singles)}")
    lines += ["# LOSES" + r[7:] for r in lose]
    lines += ["#",
              "# (2) ops.conv_transpose2d calls - the four parity launches of a transposed convolution's forward (act 1) or of a 4x4 / stride-2 convolution's data",
              "# gradient, as ONE call: the default mode runs small ones as one grid (kind up4, lwg_conv_transpose4_nhwc_f32) and large ones as four direct launches;",
              "# the new mode always makes four launches (nk: + four finishing kernels where the plan splits).  x = the call's input, y = its output; use = the",
              "# transposed convolution's forward (fwd) or a stride-2 convolution's data gradient (dgrad, called with out_hw).",
              f"# {'x B x H x W':>13s} {'Cin':>5s} {'y HxW':>9s} {'N':>4s} taps act sk   use  n/step  {'kind':>10s} nk default_us  bf16op_us  ratio   min_d   min_b    relL2"]
    glose = []
    for key in sorted(groups, key=lambda k: (-k[0][1] * k[0][2], k[0][3], k[2], k[4])):
        rec = groups[key]
        a, b, ma, mb, rel, kind, nk = time_group(key, rec, args.reps, dev)
        tot["g"][0] += rec[0] * a
        tot["g"][1] += rec[0] * b
        B, H, W, C = key[0]
        row = (f"  {f'{B}x{H}x{W}':>13s} {C:5d} {f'{key[1][1]}x{key[1][2]}':>9s} {key[2]:4d} {key[3]:4d} {key[4]:3d} {int(key[5]):2d} {'fwd' if key[6] is None else 'dgrad':>5s} {rec[0]:7d}  {kind:>10s} {nk:2d} "
               f"{a:10.1f} {b:10.1f} {b / a:6.2f} {ma:7.1f} {mb:7.1f} {rel:8.2e}")
        lines.append(row)
        if b > a:
            glose.append(row)
    ng = sum(v[0] for v in groups.values())
    lines.append(f"# (2) per step, calls x median: default {tot['g'][0] / 1e3:.3f} ms, bf16op {tot['g'][1] / 1e3:.3f} ms, ratio {tot['g'][1] / max(tot['g'][0], 1e-9):.3f} "
                 f"over {ng} calls of {len(groups)} shapes; slower than the default route: {len(glose)} of {len(groups)}")
    lines += ["# LOSES" + r[7:] for r in glose]
    lines += ["#",
              "# (3) ops.conv_transpose2d calls that ops._bf16op_use_parity4 leaves on the default mode's one-grid form (a one-grid group whose parity launches the",
              "# plan would split: eight kernels against one grid lost 1.07 - 1.41, profiles/conv_bf16op_parity_groups_before_rule.txt).  In the mode they run",
              "# what the default runs (column mode_us: the same kernel; the 4 - 5 us on top are the host time of evaluating the rule in an eager call, which a captured",
              "# step does not pay); whole4_us = the rule's alternative, the four parity launches on the",
              "# new kernel without split-K, against the same default",
              f"# {'x B x H x W':>13s} {'Cin':>5s} {'y HxW':>9s} {'N':>4s} taps act sk   use  n/step  {'kind':>10s} default_us    mode_us  ratio   whole4_us  ratio"]
    for key in sorted(excluded, key=lambda k: (-k[0][1] * k[0][2], k[0][3], k[2], k[4])):
        rec = excluded[key]
        a, b, _, _, _, kind, _ = time_group(key, rec, args.reps, dev)
        a2, w, _, _, _, _, _ = time_group(key, rec, args.reps, dev, whole=True)
        tot["g"][0] += rec[0] * a
        tot["g"][1] += rec[0] * b
        B, H, W, C = key[0]
        lines.append(f"  {f'{B}x{H}x{W}':>13s} {C:5d} {f'{key[1][1]}x{key[1][2]}':>9s} {key[2]:4d} {key[3]:4d} {key[4]:3d} {int(key[5]):2d} {'fwd' if key[6] is None else 'dgrad':>5s} {rec[0]:7d}  {kind:>10s} "
                     f"{a:10.1f} {b:10.1f} {b / a:6.2f}  {w:10.1f} {w / a2:6.2f}")
    ng += sum(v[0] for v in excluded.values())
    ta, tb = tot["s"][0] + tot["g"][0], tot["s"][1] + tot["g"][1]
    lines.append(f"# (1) + (2) per step: default {ta / 1e3:.3f} ms, bf16op {tb / 1e3:.3f} ms, ratio {tb / max(ta, 1e-9):.3f} over {ns + ng} calls of "
                 f"{len(singles) + len(groups) + len(excluded)} shapes ((3) included, as the mode runs it); slower: {len(lose) + len(glose)}")
    with open(os.path.join(args.out, "conv_bf16op_layers.txt"), "w") as fp:
        fp.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def time_steps(tr, conv, wgrad, steps):
    tr.opts.conv_precision, tr.opts.wgrad_precision = conv, wgrad
    tr._graphs = None                        # every block captures the step anew
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


PAIRS = (("winograd", "direct"), ("winograd", "bf16"), (MODE, "bf16"))


def part_step(args):
    out = [f"# tools/conv_bf16op_ab.py --part step --size {args.size} --steps {args.steps} --blocks {args.blocks}: the whole captured personalization step on ONE trainer",
           "# per loss set, (TrainOpts.conv_precision, wgrad_precision) alternating in blocks (re-captured at each switch, two untimed steps first); ms per step"]
    for name, vgg, face in (("L1", False, False), ("VGG19 + face", True, True)):
        tr = _trainer512(args.size, vgg, face)
        rows = []
        for blk in range(args.blocks):
            for conv, wgrad in PAIRS:
                rows.append((blk, (conv, wgrad), time_steps(tr, conv, wgrad, args.steps), tr.step_mode))
        out.append(f"# losses: {name}")
        for blk, pair, ms, sm in rows:
            out.append(f"  block {blk} {str(pair):30s} {ms:8.3f} ms   [{sm}]")
        base = None
        for pair in PAIRS:
            v = [r[2] for r in rows if r[1] == pair]
            md = statistics.median(v)
            base = md if base is None else base
            out.append(f"# {name}: {str(pair):30s} median {md:.3f} ms (min {min(v):.3f}, max {max(v):.3f}), ratio to the default {md / base:.4f}")
        with open(os.path.join(args.out, "conv_bf16op_step_ab.txt"), "w") as fp:
            fp.write("\n".join(out) + "\n")
        del tr
        torch.cuda.empty_cache()
    print("\n".join(out), flush=True)


def part_effect(args):
    from ipercore_amd import synthetic
    from ipercore_amd.networks import NetworksFactory, generator_param_shapes
    from ipercore_amd.trainers import LWGTrainer, PatchGlobalDiscriminator, TrainOpts
    from tests import gpu_checks as gc
    dev = "cuda:0"
    S, ns, nf, nres, bgf = 64, 2, [64, 64, 128], 2, [64, 64, 128]
    u = lambda shape, seed, name: torch.tensor(synthetic.uniform_image(shape, seed, name), device=dev)      # noqa: E731
    bg_in, src_in, tsf_in, Tst = gc._training_inputs(S, ns, nf, nres, bgf, False)
    inp = {"input_G_bg": bg_in.to(dev), "input_G_src": src_in.to(dev), "input_G_tsf": tsf_in.to(dev), "Tst": Tst.to(dev),
           "real_src": u((1, ns, 3, S, S), 700, "real_src"), "real_tsf": u((1, 1, 3, S, S), 701, "real_tsf"),
           "real_bg": u((1, 3, S, S), 702, "real_bg"), "body_mask": (u((1, ns + 1, 1, S, S), 703, "mask") > 0).float()}
    sdn = synthetic.fill_state_dict(generator_param_shapes(nf, nres, bgf), seed=7)

    def trainer(conv, wgrad, graph):
        G = NetworksFactory.get_by_name("AttLWB-SPADE", cfg=gc.pu.gen_cfg(nf, nres, bgf), temporal=False)
        G.load_state_dict({k: torch.tensor(v) for k, v in sdn.items()}, strict=True)
        G.to(dev).train()
        torch.manual_seed(0)
        D = PatchGlobalDiscriminator().to(dev)
        opts = TrainOpts.l1_transfer()
        opts.conv_precision, opts.wgrad_precision, opts.use_graph = conv, wgrad, graph
        tr = LWGTrainer(G, D, opts=opts)
        tr.set_input({k: v.clone() for k, v in inp.items()})
        return tr

    def first_grads(conv, wgrad):
        tr = trainer(conv, wgrad, False)
        tr.optimize_parameters()
        torch.cuda.synchronize()
        return {("G." + n): p.grad.detach().clone() for n, p in tr.G.named_parameters() if p.grad is not None} | \
               {("D." + n): p.grad.detach().clone() for n, p in tr.D.named_parameters() if p.grad is not None}

    n = args.effect_steps
    hist = {}
    for pair in (("winograd", "direct"), (MODE, "bf16")):
        tr = trainer(pair[0], pair[1], True)
        hist[pair] = [tuple(float(v) for v in tr.optimize_parameters()) for _ in range(n)]
        torch.cuda.synchronize()
    out = [f"# tools/conv_bf16op_ab.py --part effect: {n} steps at S = 64 (nf {nf}, nres {nres}, L1 loss set) from one seed, the default mode against",
           "# (\"bf16_operands\", \"bf16\"); recorded, not asserted",
           f"# {'step':>4s} {'G default':>12s} {'G bf16':>12s} {'rel':>9s} {'D default':>12s} {'D bf16':>12s} {'rel':>9s}"]
    a, b = hist[("winograd", "direct")], hist[(MODE, "bf16")]
    for i in range(n):
        out.append(f"  {i:4d} {a[i][0]:12.6f} {b[i][0]:12.6f} {abs(b[i][0] - a[i][0]) / max(abs(a[i][0]), 1e-30):9.2e} "
                   f"{a[i][1]:12.6f} {b[i][1]:12.6f} {abs(b[i][1] - a[i][1]) / max(abs(a[i][1]), 1e-30):9.2e}")
    ref = first_grads("fp32", "direct")
    cols = {"winograd/direct": first_grads("winograd", "direct"), "fp32/direct again": first_grads("fp32", "direct"),
            "bf16_operands/direct": first_grads(MODE, "direct"), "bf16_operands/bf16": first_grads(MODE, "bf16")}
    out.append("# relative L2 of every parameter's first-step gradient against the (\"fp32\", \"direct\") mode (\"fp32/direct again\": a second run of the")
    out.append("# reference itself - the noise of the fp32 atomics in the attention / warp backward)")
    out.append(f"# {'parameter':60s} " + " ".join(f"{c:>20s}" for c in cols))
    worst = {c: 0.0 for c in cols}
    for name, g0 in ref.items():
        nz = float(g0.norm())
        if nz == 0.0:
            continue
        vals = {c: float((cols[c][name] - g0).norm()) / nz for c in cols}
        worst = {c: max(worst[c], vals[c]) for c in cols}
        out.append(f"  {name:60s} " + " ".join(f"{vals[c]:20.3e}" for c in cols))
    out.append(f"# {'worst':60s} " + " ".join(f"{worst[c]:20.3e}" for c in cols))
    with open(os.path.join(args.out, "conv_bf16op_effect.txt"), "w") as fp:
        fp.write("\n".join(out) + "\n")
    print("\n".join(out[:8] + ["  ..."] + out[-3:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("all", "layers", "step", "effect"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--effect-steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.part == "all":
        # every part in a process of its own under its own time limit; the first failure (a fault, an abort, a limit) ends the run
        for part in ("layers", "step", "effect"):
            cmd = ["timeout", "-k", "10", str(LIMITS[part]), sys.executable, os.path.abspath(__file__), "--part", part, "--size", str(args.size),
                   "--reps", str(args.reps), "--steps", str(args.steps), "--blocks", str(args.blocks), "--effect-steps", str(args.effect_steps),
                   "--out", args.out]
            rc = subprocess.call(cmd)
            if rc != 0:
                print(f"conv_bf16op_ab: part {part} ended with status {rc}; stopping", flush=True)
                return rc
        return 0
    assert torch.cuda.is_available(), "needs the MI355X"
    {"layers": part_layers, "step": part_step, "effect": part_effect}[args.part](args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
