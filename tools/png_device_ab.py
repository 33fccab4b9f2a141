"""A/B of the output stage's two PNG encoders (output.FrameWriter encoder="host" | "device") on the 300-frame 512 x 512 fp32 clip, in ONE
process, the encoders alternating block by block (the host is shared: a difference is read against the spread of the repeats).

Per encoder and block: end-to-end frames/s (first launch to the last file closed), GPU-side frames/s (to the device synchronise behind the
last submit), host CPU seconds per frame (process time over all threads), mean file bytes.  Then the two launches of ops.png_deflate alone,
by device events, on a batch of the clip's own frames.  The files of both encoders are decoded and compared on a few frames first.
usage: png_device_ab.py [--fb 16] [--blocks 3] [--frames 300] [--size 512] [--out profiles/png_device_ab.txt]"""
import argparse
import os
import shutil
import sys
import tempfile
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ipercore_amd import ops
from ipercore_amd import synthetic as syn
from ipercore_amd.output import FrameWriter

ap = argparse.ArgumentParser()
ap.add_argument("--fb", type=int, default=16, help="frames per launch batch (bench.py's with_output uses 16)")
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_device_ab.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the MI355X"

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


case = syn.build_case(image_size=args.size, n_frames=args.frames, ns=2)
im = syn.make_imitator(case, frame_batch=args.fb)
tgt = im.prepare_sequence(case.tgt_smpls, "smooth")
n = args.frames // args.fb * args.fb


def clip(encoder, keep=None):
    d = tempfile.mkdtemp(prefix="lwg_pngab_")
    try:
        w = FrameWriter(d, prefix="pred_", encoder=encoder)
        torch.cuda.synchronize()
        c0, t0 = time.process_time(), time.perf_counter()
        for s in range(0, n, args.fb):
            tsf8, Tst, _ = im.make_inputs_for_tsf(im.src_info, tgt[s:s + args.fb], "smooth", t=s)
            w.submit(im.forward(tsf8, Tst)[0], s)
        torch.cuda.synchronize()
        tg = time.perf_counter() - t0
        paths = w.close()
        dt, cpu = time.perf_counter() - t0, time.process_time() - c0
        assert len(paths) == n
        size = sum(os.path.getsize(p) for p in paths) / n
        if keep is not None:
            from PIL import Image
            keep[encoder] = [np.asarray(Image.open(paths[t]).convert("RGB")) for t in range(0, n, max(1, n // 5))]
        return {"fps": n / dt, "gpu_fps": n / tg, "cpu_s": cpu / n, "bytes": size, "workers": w.workers}
    finally:
        shutil.rmtree(d, ignore_errors=True)


say(f"png_device_ab: {n} frames {args.size} x {args.size} fp32, frame batch {args.fb}, {args.blocks} alternating blocks per encoder, "
    f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), cpus usable {len(os.sched_getaffinity(0))} (os.cpu_count {os.cpu_count()})")
kept = {}
for enc in ("host", "device"):                 # warm-up of every shape + the equality check of what lands on disk
    clip(enc, kept)
same = all(np.array_equal(a, b) for a, b in zip(kept["host"], kept["device"]))
say(f"decoded pixels of {len(kept['host'])} frames, host files vs device files: {'equal' if same else 'DIFFERENT'}")
assert same
res = {"host": [], "device": []}
for blk in range(args.blocks):
    for enc in ("host", "device"):
        r = clip(enc)
        res[enc].append(r)
        say(f"block {blk} {enc:6s}: {r['fps']:7.1f} frames/s end to end, {r['gpu_fps']:7.1f} GPU side, {1e3 * r['cpu_s']:6.2f} ms host CPU per frame, "
            f"{r['bytes'] / 1024:7.1f} KiB per file, {r['workers']} workers")
for enc in ("host", "device"):
    f = sorted(r["fps"] for r in res[enc])
    g = sorted(r["gpu_fps"] for r in res[enc])
    say(f"{enc:6s}: end to end median {f[len(f) // 2]:7.1f} (min {f[0]:.1f}, max {f[-1]:.1f}) frames/s; GPU side median {g[len(g) // 2]:7.1f}; "
        f"host CPU {1e3 * np.mean([r['cpu_s'] for r in res[enc]]):.2f} ms per frame; file {np.mean([r['bytes'] for r in res[enc]]) / 1024:.1f} KiB")

# the two launches alone, on the clip's own pixels
tsf8, Tst, _ = im.make_inputs_for_tsf(im.src_info, tgt[:args.fb], "smooth", t=0)
u8 = ops.frames_to_u8(im.forward(tsf8, Tst)[0].contiguous())
for _ in range(3):
    ops.png_deflate(u8, FrameWriter.ROWS_PER_SEGMENT)
torch.cuda.synchronize()
reps = 20
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(reps):
    streams, nbytes = ops.png_deflate(u8, FrameWriter.ROWS_PER_SEGMENT)
e1.record()
torch.cuda.synchronize()
us = 1e3 * e0.elapsed_time(e1) / reps
say(f"ops.png_deflate (segment kernel + pack kernel, workspace allocation included), {args.fb} frames per call, {reps} calls back to back: "
    f"{us:.1f} us per batch = {us / args.fb:.1f} us per frame; stream bytes per frame {float(nbytes.float().mean()):.0f} of capacity {streams.shape[1]}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fp:
    fp.write("\n".join(lines) + "\n")
