"""A/B of the output stage's four forms (output.FrameWriter encoder="host" | "device" | "jpeg" | "mjpeg") on the 300-frame 512 x 512 fp32 clip
WITH files, in ONE process, the encoders alternating block by block (the host is shared: a difference is read against the spread of the repeats).

Per encoder and block: end-to-end frames/s (first launch to the last file closed), GPU-side frames/s (to the device synchronise behind the
last submit), host CPU seconds per frame (process time over all threads), bytes per frame on disk.  PSNR of the decoded JPEG files (the AVI's
chunks too) against the uint8 frames the PNG files hold.  Then the two launches of ops.jpeg_scan alone, by device events, on a batch of the
clip's own frames, and - sizes and PSNR only, they do not depend on the clip - the tests' smooth and smooth + noise 512 x 512 frames.
The clip's frames come from seeded random weights: they are noise-like and compress far worse than footage.
usage: jpeg_device_ab.py [--fb 16] [--blocks 3] [--frames 300] [--size 512] [--quality 90] [--ring R] [--out profiles/jpeg_device_ab.txt]"""
import argparse
import io
import os
import shutil
import struct
import sys
import tempfile
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image
from ipercore_amd import ops, output
from ipercore_amd import synthetic as syn
from ipercore_amd.output import FrameWriter

ap = argparse.ArgumentParser()
ap.add_argument("--fb", type=int, default=16, help="frames per launch batch (bench.py's with_output uses 16)")
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--quality", type=int, default=90)
ap.add_argument("--ring", type=int, default=None, help="FrameWriter's ring: batches in flight between the producer and the files (default: the writer's, 4 for PNG and 8 for JPEG)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_device_ab.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the MI355X"
ENCODERS = ("host", "device", "jpeg", "mjpeg")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def avi_frames(data):
    """The 00dc payloads of an AVI file written by output.MjpegAviWriter, by its idx1."""
    movi = data.index(b"movi")
    i = data.rindex(b"idx1")
    n = struct.unpack("<I", data[i + 4:i + 8])[0] // 16
    out = []
    for k in range(n):
        _, _, o, s = struct.unpack("<4sIII", data[i + 8 + 16 * k:i + 24 + 16 * k])
        out.append(data[movi + o + 8:movi + o + 8 + s])
    return out


case = syn.build_case(image_size=args.size, n_frames=args.frames, ns=2)
im = syn.make_imitator(case, frame_batch=args.fb)
tgt = im.prepare_sequence(case.tgt_smpls, "smooth")
n = args.frames // args.fb * args.fb


def clip(encoder, keep=None):
    d = tempfile.mkdtemp(prefix="lwg_jpegab_")
    try:
        w = FrameWriter(d, prefix="pred_", encoder=encoder, quality=args.quality, ring=args.ring)
        torch.cuda.synchronize()
        c0, t0 = time.process_time(), time.perf_counter()
        for s in range(0, n, args.fb):
            tsf8, Tst, _ = im.make_inputs_for_tsf(im.src_info, tgt[s:s + args.fb], "smooth", t=s)
            w.submit(im.forward(tsf8, Tst)[0], s)
        torch.cuda.synchronize()
        tg = time.perf_counter() - t0
        paths = w.close()
        dt, cpu = time.perf_counter() - t0, time.process_time() - c0
        assert len(paths) == (1 if encoder == "mjpeg" else n)
        size = sum(os.path.getsize(p) for p in paths) / n
        if keep is not None:
            pick = range(0, n, max(1, n // 5))
            if encoder == "mjpeg":
                with open(paths[0], "rb") as fp:
                    chunks = avi_frames(fp.read())
                assert len(chunks) == n
                keep[encoder] = [np.asarray(Image.open(io.BytesIO(chunks[t])).convert("RGB")) for t in pick]
            else:
                keep[encoder] = [np.asarray(Image.open(paths[t]).convert("RGB")) for t in pick]
        return {"fps": n / dt, "gpu_fps": n / tg, "cpu_s": cpu / n, "bytes": size, "workers": w.workers}
    finally:
        shutil.rmtree(d, ignore_errors=True)


say(f"jpeg_device_ab: {n} frames {args.size} x {args.size} fp32, frame batch {args.fb}, quality {args.quality}, ring {args.ring or 'default'}, {args.blocks} alternating blocks per encoder, "
    f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), cpus usable {len(os.sched_getaffinity(0))} (os.cpu_count {os.cpu_count()})")
say("the clip's frames come from seeded random weights: noise-like, far less compressible than footage")
kept = {}
for enc in ENCODERS:                           # warm-up of every shape + what lands on disk
    clip(enc, kept)
same = all(np.array_equal(a, b) for a, b in zip(kept["host"], kept["device"]))
say(f"decoded pixels of {len(kept['host'])} frames, host PNG files vs device PNG files: {'equal' if same else 'DIFFERENT'}")
assert same
for enc in ("jpeg", "mjpeg"):
    p = [psnr(a, b) for a, b in zip(kept[enc], kept["host"])]
    say(f"{enc}: PSNR of {len(p)} decoded frames against the PNG files' pixels: min {min(p):.2f} dB, mean {np.mean(p):.2f} dB")
same = all(np.array_equal(a, b) for a, b in zip(kept["jpeg"], kept["mjpeg"]))
say(f"decoded .jpg files vs decoded AVI chunks: {'equal' if same else 'DIFFERENT'}")
assert same
res = {enc: [] for enc in ENCODERS}
for blk in range(args.blocks):
    for enc in ENCODERS:
        r = clip(enc)
        res[enc].append(r)
        say(f"block {blk} {enc:6s}: {r['fps']:7.1f} frames/s end to end, {r['gpu_fps']:7.1f} GPU side, {1e3 * r['cpu_s']:6.2f} ms host CPU per frame, "
            f"{r['bytes'] / 1024:7.1f} KiB per frame, {r['workers']} workers")
for enc in ENCODERS:
    f = sorted(r["fps"] for r in res[enc])
    g = sorted(r["gpu_fps"] for r in res[enc])
    say(f"{enc:6s}: end to end median {f[len(f) // 2]:7.1f} (min {f[0]:.1f}, max {f[-1]:.1f}) frames/s; GPU side median {g[len(g) // 2]:7.1f}; "
        f"host CPU {1e3 * np.mean([r['cpu_s'] for r in res[enc]]):.2f} ms per frame; {np.mean([r['bytes'] for r in res[enc]]) / 1024:.1f} KiB per frame")

# the two launches alone, on the clip's own pixels
tsf8, Tst, _ = im.make_inputs_for_tsf(im.src_info, tgt[:args.fb], "smooth", t=0)
u8 = ops.frames_to_u8(im.forward(tsf8, Tst)[0].contiguous())
for _ in range(3):
    ops.jpeg_scan(u8, args.quality)
torch.cuda.synchronize()
reps = 20
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(reps):
    scans, nbytes = ops.jpeg_scan(u8, args.quality)
e1.record()
torch.cuda.synchronize()
us = 1e3 * e0.elapsed_time(e1) / reps
say(f"ops.jpeg_scan (segment kernel + pack kernel, workspace allocation included), {args.fb} frames per call, {reps} calls back to back: "
    f"{us:.1f} us per batch = {us / args.fb:.1f} us per frame; scan bytes per frame {float(nbytes.float().mean()):.0f} of capacity {scans.shape[1]} "
    f"(raw frame {args.size * args.size * 3})")

# image-like content: the tests' synthetic frames (a horizontal / vertical / diagonal gradient, and the same + uniform noise of +-6 levels)
S = args.size
yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
smooth = np.stack([(255 * xx) // (S - 1), (255 * yy) // (S - 1), (255 * (xx + yy)) // (2 * S - 2)], axis=-1)
noisy = np.clip(smooth + np.random.default_rng(0).integers(-6, 7, smooth.shape), 0, 255)
for name, img in (("smooth", smooth.astype(np.uint8)), ("smooth + noise", noisy.astype(np.uint8))):
    scans, nbytes = ops.jpeg_scan(torch.from_numpy(img[None]).cuda(), args.quality)
    data = output.jpeg_from_scan(scans[0, :int(nbytes[0])].cpu().numpy(), S, S, args.quality, min((S + 7) // 8, ops.jpeg_max_mcus_per_segment()))
    dec = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    streams, nb = ops.png_deflate(torch.from_numpy(img[None]).cuda(), FrameWriter.ROWS_PER_SEGMENT)
    png_dev = len(output.png_from_stream(streams[0, :int(nb[0])].cpu().numpy(), S, S))
    say(f"{name} {S} x {S}: JPEG {len(data)} bytes, PSNR {psnr(dec, img):.2f} dB; device PNG {png_dev} bytes; host PNG {len(output.png_bytes(img))} bytes; raw {img.size}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fp:
    fp.write("\n".join(lines) + "\n")
