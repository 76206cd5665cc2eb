#!/usr/bin/env python
"""Measure the JPEG encoder on one MI355X: resident RGB store -> one JPEG file per frame (FrameStore.jpeg_frames).

For all 3 600 frames of a 360x640 store and 600 frames of a 1080x1920 store (the synthetic video, quality 75, 4:2:0) it reports,
as medians of 3 runs that alternate with the host alternative in the same process after a warm-up of each,

  device   FrameStore.jpeg_frames: wall time, frames/s, host CPU-seconds (time.process_time: all threads of the process), and
           the block-stage and entropy-stage kernel times by HIP events (summed over the chunks)
  pillow   what a user writes today: host_frames (the raw frames over PCIe) + Pillow's encoder on a 16-thread pool

and checks that both give the same bytes.  Rate: the bytes each stage must move, from the sizes alone -- block stage 3 B/pixel
of RGB in + 2 B/coefficient out; entropy stage the coefficients in (twice: a length pass and a write pass) + the scan's bytes
out (three times: the unstuffed stream written, read twice by the stuffing passes) + the slots -- over the stage's kernel
time, against the achievable-HBM figure of the microarchitecture guide.

  python tools/bench_jpeg_encode.py --out profiles/jpeg_encode_measure          # writes .md and .json

No GPU -> error (a CPU timing says nothing about this).
"""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12          # B/s, MI355X_MICROARCH.md (achievable, not the 8 TB/s peak)
CASES = [("360x640", 3600, 360, 640), ("1080x1920", 600, 1080, 1920)]


def pillow_files(store, secs, quality, threads=16, piece=256):
    from PIL import Image

    def enc(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=quality)
        return buf.getvalue()

    out = []
    with ThreadPoolExecutor(threads) as ex:
        for s0 in range(0, len(secs), piece):
            out += list(ex.map(enc, store.host_frames(secs[s0:s0 + piece])))
    return out


def timed(fn):
    import torch
    torch.cuda.synchronize()
    c0, t0 = time.process_time(), time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0, time.process_time() - c0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write OUT.md and OUT.json")
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (a quick look)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_jpeg_encode needs an MI355X")
    from tstar_amd import jpeg_encode as JE
    from tstar_amd.video import synthetic_video
    rows = []
    for name, n, H, W in CASES:
        n = max(8, int(n * args.scale))
        store = synthetic_video(n, H=H, W=W, seed=5)
        secs = list(range(n))
        warm = secs[:min(n, 32)]
        store.jpeg_frames(warm, args.quality)
        pillow_files(store, warm, args.quality)
        dev, pil = [], []
        files = ref = None
        for _ in range(args.runs):
            stats = {}
            files, wall, cpu = timed(lambda: JE.encode_frames((store, secs), args.quality, stats=stats))
            dev.append(dict(wall=wall, cpu=cpu, block_ms=stats["block_ms"], entropy_ms=stats["entropy_ms"], retried=stats["retried"]))
            # the same call without event timing: the events synchronise between the stages
            _, wall_plain, cpu_plain = timed(lambda: store.jpeg_frames(secs, args.quality))
            dev[-1].update(wall_plain=wall_plain, cpu_plain=cpu_plain)
            ref, wall, cpu = timed(lambda: pillow_files(store, secs, args.quality))
            pil.append(dict(wall=wall, cpu=cpu))
        same = files == ref
        med = lambda rs, k: statistics.median(r[k] for r in rs)       # noqa: E731
        p = JE.Plan(W, H, 2, 2)
        scan_bytes = sum(len(f) for f in files) - n * p.header_bytes
        slot = JE._typical_slot(W, H, p)
        block_bytes = n * (3 * W * H + p.coef_bytes)
        entropy_bytes = n * (2 * p.coef_bytes + 8 * p.blocks) + 3 * scan_bytes + n * (slot // 4 * 4 + 4)       # + the zeroed unstuffed buffer
        row = dict(case=name, frames=n, quality=args.quality, same_bytes=bool(same), jpeg_bytes=sum(len(f) for f in files),
                   device_wall_s=med(dev, "wall_plain"), device_cpu_s=med(dev, "cpu_plain"), device_wall_timed_s=med(dev, "wall"),
                   block_ms=med(dev, "block_ms"), entropy_ms=med(dev, "entropy_ms"), retried=dev[-1]["retried"],
                   pillow_wall_s=med(pil, "wall"), pillow_cpu_s=med(pil, "cpu"),
                   block_bytes=block_bytes, entropy_bytes=entropy_bytes)
        row["block_rate"] = block_bytes / (row["block_ms"] * 1e-3)
        row["entropy_rate"] = entropy_bytes / (row["entropy_ms"] * 1e-3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del store
        torch.cuda.empty_cache()
    lines = ["# JPEG encode on one MI355X", "",
             f"`python tools/bench_jpeg_encode.py`: quality {args.quality}, 4:2:0, the synthetic video; medians of {args.runs} runs alternating "
             "with the host alternative (host_frames + Pillow on 16 threads) in one process.", "",
             "| case | frames | same bytes | device wall s | frames/s | device CPU-s | Pillow wall s | Pillow CPU-s | block stage ms | entropy stage ms | retried |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['frames']} | {r['same_bytes']} | {r['device_wall_s']:.3f} | {r['frames'] / r['device_wall_s']:.0f} | "
                     f"{r['device_cpu_s']:.3f} | {r['pillow_wall_s']:.3f} | {r['pillow_cpu_s']:.3f} | {r['block_ms']:.3f} | {r['entropy_ms']:.3f} | {r['retried']} |")
    lines += ["", "Bytes each stage must move (from the sizes alone) over its kernel time, against 6.3 TB/s achievable HBM:", "",
              "| case | block stage GB | GB/s | of achievable | entropy stage GB | GB/s | of achievable |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['case']} | {r['block_bytes'] / 1e9:.3f} | {r['block_rate'] / 1e9:.0f} | {100 * r['block_rate'] / HBM_ACHIEVABLE:.1f} % | "
                     f"{r['entropy_bytes'] / 1e9:.3f} | {r['entropy_rate'] / 1e9:.0f} | {100 * r['entropy_rate'] / HBM_ACHIEVABLE:.1f} % |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out + ".md", "w") as f:
            f.write(text)
        with open(args.out + ".json", "w") as f:
            json.dump(rows, f, indent=1)
    if not all(r["same_bytes"] for r in rows):
        sys.exit("device and Pillow bytes differ")


if __name__ == "__main__":
    main()
