#!/usr/bin/env python
"""Measure the JPEG encoder's optimised Huffman tables (``optimize=True``) on one MI355X, on tools/bench_jpeg_encode.py's two stores:
3 600 frames of 360x640 and 600 frames of 1080x1920 (the synthetic video, quality 75, 4:2:0).

For ``optimize`` off and on, alternated in one process after a warm-up of each, medians of 3 runs:

  bytes per frame; wall seconds and host CPU-seconds of ``encode_frames((store, secs))`` (time.process_time: all threads);
  the block-stage and entropy-stage kernel times by HIP events (the entropy stage of ``optimize=True`` holds the two new stages);
  the histogram kernel and the table kernel ALONE by HIP events (tstar_jpeg_encode_tables, stages 1 and 2, on one chunk's
  coefficients, scaled to all frames);
  Pillow with ``optimize=True`` on a 16-thread pool (host_frames + the encoder), and that both give the same bytes.

The cost of the option is reported as the ratio to the same run's ``optimize=False``.

``--encode-vs TREE`` first runs tools/bench_jpeg_encode.py of another built checkout (the parent commit) and of this one as child
processes, alternated, and reports the marker-free, standard-table encode time of both with the spread of the runs;
``--bench-vs TREE`` does the same with ``bench.py --gpus 1``.

  python tools/measure_jpeg_optimize.py --out profiles/jpeg_optimize_measure [--encode-vs ../parent] [--bench-vs ../parent]

No GPU -> error (a CPU timing says nothing about this).
"""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("360x640", 3600, 360, 640), ("1080x1920", 600, 1080, 1920)]


def pillow_files(store, secs, quality, threads=16, piece=256):
    from PIL import Image

    def enc(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=quality, optimize=True)
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


def stage_ms(store, n, quality, runs):
    """The histogram kernel and the table kernel alone on the coefficients of one chunk -> (ms per frame of each, frames of the chunk)"""
    import torch
    from tstar_amd import _lib
    from tstar_amd import jpeg_encode as JE
    lib = _lib.load()
    _, H, W, _ = store.shape
    one = JE.Plan(W, H, 2, 2, 1, optimize=True)
    m = JE.encode_chunk_size(one.blocks, n)
    enc = JE.DeviceEncoder(W, H, quality, "4:2:0", m, None, store.device, 0, True)
    idx = torch.arange(m, dtype=torch.int32, device=store.device)
    enc.launch(store.frames, idx)
    args = (enc.coef.data_ptr(), m, W, H, 2, 2, 0, enc.slot)
    tail = (enc.specs.data_ptr(), enc.work.data_ptr(), enc.work.numel(), _lib.stream_ptr())
    out = []
    for stage in (1, 2):
        ms = []
        for _ in range(runs + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            _lib.check(lib.tstar_jpeg_encode_tables(*args, stage, *tail), "tstar_jpeg_encode_tables")
            ev[1].record()
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        out.append(statistics.median(ms[1:]) / m)
    return out[0], out[1], m


def children(tree, script, extra, runs, pick):
    """`script` of `tree` and of this checkout as alternated child processes -> {"other": [...], "this": [...]} of pick(stdout, out base)"""
    got = {"other": [], "this": []}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(runs):
            for who, root in (("other", os.path.abspath(tree)), ("this", ROOT)):
                base = os.path.join(tmp, f"{who}{r}")
                p = subprocess.run([sys.executable, os.path.join(root, script)] + [a.replace("@OUT@", base) for a in extra], cwd=root,
                                   capture_output=True, text=True, check=True)
                got[who].append(pick(p.stdout, base))
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write OUT.md and OUT.json")
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (a quick look)")
    ap.add_argument("--encode-vs", default=None, metavar="TREE")
    ap.add_argument("--bench-vs", default=None, metavar="TREE")
    ap.add_argument("--bench-steps", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("measure_jpeg_optimize needs an MI355X")
    from tstar_amd import jpeg_encode as JE
    from tstar_amd.video import synthetic_video
    result = dict(quality=args.quality, runs=args.runs, cases=[])
    if args.encode_vs:
        def pick(_, base):
            with open(base + ".json") as f:
                return {r["case"]: r["device_wall_s"] for r in json.load(f)}
        result["encode_vs"] = children(args.encode_vs, os.path.join("tools", "bench_jpeg_encode.py"),
                                       ["--out", "@OUT@", "--scale", str(args.scale), "--quality", str(args.quality)], args.runs, pick)
    if args.bench_vs:
        def pick_bench(out, _):
            r = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            return {k: r[k] for k in ("value", "unit", "steps", "ms_per_step")}
        result["bench_vs"] = children(args.bench_vs, "bench.py", ["--gpus", "1", "--steps", str(args.bench_steps), "--warmup", "3"], args.runs,
                                      pick_bench)
    for name, n, H, W in CASES:
        n = max(8, int(n * args.scale))
        store = synthetic_video(n, H=H, W=W, seed=5)
        secs = list(range(n))
        warm = secs[:min(n, 32)]
        for opt in (False, True):
            store.jpeg_frames(warm, args.quality, optimize=opt)
        pillow_files(store, warm, args.quality)
        runs = {False: [], True: [], "pillow": []}
        files = {}
        for _ in range(args.runs):
            for opt in (False, True):
                stats = {}
                _, wall_t, _ = timed(lambda: JE.encode_frames((store, secs), args.quality, stats=stats, optimize=opt))
                files[opt], wall, cpu = timed(lambda: JE.encode_frames((store, secs), args.quality, optimize=opt))
                runs[opt].append(dict(wall=wall, cpu=cpu, block_ms=stats["block_ms"], entropy_ms=stats["entropy_ms"], retried=stats["retried"],
                                      table_bytes=stats.get("table_bytes", 0)))
            ref, wall, cpu = timed(lambda: pillow_files(store, secs, args.quality))
            runs["pillow"].append(dict(wall=wall, cpu=cpu))
        med = lambda rs, k: statistics.median(r[k] for r in rs)       # noqa: E731
        hist_ms, table_ms, chunk = stage_ms(store, n, args.quality, args.runs)
        row = dict(case=name, frames=n, same_bytes=bool(files[True] == ref), chunk=chunk,
                   hist_ms=hist_ms * n, table_ms=table_ms * n, pillow_wall_s=med(runs["pillow"], "wall"), pillow_cpu_s=med(runs["pillow"], "cpu"))
        for opt, key in ((False, "std"), (True, "opt")):
            row[key] = dict(bytes_per_frame=sum(len(f) for f in files[opt]) / n, wall_s=med(runs[opt], "wall"), cpu_s=med(runs[opt], "cpu"),
                            block_ms=med(runs[opt], "block_ms"), entropy_ms=med(runs[opt], "entropy_ms"), retried=runs[opt][-1]["retried"],
                            table_bytes_per_frame=runs[opt][-1]["table_bytes"] / n, walls=[r["wall"] for r in runs[opt]])
        row["wall_ratio"] = row["opt"]["wall_s"] / row["std"]["wall_s"]
        row["entropy_ratio"] = row["opt"]["entropy_ms"] / row["std"]["entropy_ms"]
        row["bytes_ratio"] = row["opt"]["bytes_per_frame"] / row["std"]["bytes_per_frame"]
        result["cases"].append(row)
        print(json.dumps(row), flush=True)
        del store
        torch.cuda.empty_cache()
    L = ["# JPEG encode with optimised Huffman tables on one MI355X", "",
         f"`python tools/measure_jpeg_optimize.py`: quality {args.quality}, 4:2:0, the synthetic video; `optimize` off and on alternated in one "
         f"process, medians of {args.runs} runs; Pillow is `host_frames` + `save(optimize=True)` on a 16-thread pool.", "",
         "| case | frames | optimize | bytes / frame | DHT bytes / frame | wall s | CPU-s | block stage ms | entropy stage ms | retried |",
         "|---|---|---|---|---|---|---|---|---|---|"]
    for r in result["cases"]:
        for key in ("std", "opt"):
            d = r[key]
            L.append(f"| {r['case']} | {r['frames']} | {key == 'opt'} | {d['bytes_per_frame']:.0f} | {d['table_bytes_per_frame']:.0f} | {d['wall_s']:.3f} | "
                     f"{d['cpu_s']:.3f} | {d['block_ms']:.3f} | {d['entropy_ms']:.3f} | {d['retried']} |")
    L += ["", "| case | bytes on / off | wall on / off | entropy stage on / off | histogram kernel ms (all frames) | table kernel ms (all frames) | "
          "Pillow optimize wall s | Pillow CPU-s | same bytes as Pillow |", "|---|---|---|---|---|---|---|---|---|"]
    for r in result["cases"]:
        L.append(f"| {r['case']} | {r['bytes_ratio']:.3f} | {r['wall_ratio']:.3f} | {r['entropy_ratio']:.3f} | {r['hist_ms']:.3f} | {r['table_ms']:.3f} | "
                 f"{r['pillow_wall_s']:.3f} | {r['pillow_cpu_s']:.3f} | {r['same_bytes']} |")
    L += ["", "The two kernels alone are timed on one chunk's coefficients (`tstar_jpeg_encode_tables`, stages 1 and 2) and scaled to all frames."]
    if "encode_vs" in result:
        L += ["", "## Standard-table encode: this commit against the other checkout (`tools/bench_jpeg_encode.py`, alternated child processes)", "",
              "| case | other: wall s of each run | this: wall s of each run | median this / other |", "|---|---|---|---|"]
        for name, *_ in CASES:
            o = [r[name] for r in result["encode_vs"]["other"]]
            t = [r[name] for r in result["encode_vs"]["this"]]
            L.append(f"| {name} | {', '.join(f'{v:.3f}' for v in o)} | {', '.join(f'{v:.3f}' for v in t)} | {statistics.median(t) / statistics.median(o):.3f} |")
    if "bench_vs" in result:
        L += ["", "## `bench.py --gpus 1`: this commit against the other checkout (alternated child processes)", ""]
        for who in ("other", "this"):
            rs = result["bench_vs"][who]
            L.append(f"* {who}: {', '.join(format(r['value'], '.1f') for r in rs)} {rs[0]['unit']} "
                     f"({', '.join(format(r['ms_per_step'], '.2f') for r in rs)} ms per step, {rs[0]['steps']} steps)")
    text = "\n".join(L) + "\n"
    print(text)
    if args.out:
        with open(args.out + ".md", "w") as f:
            f.write(text)
        with open(args.out + ".json", "w") as f:
            json.dump(result, f, indent=1)
    if not all(r["same_bytes"] for r in result["cases"]):
        sys.exit("device and Pillow bytes differ")


if __name__ == "__main__":
    main()
